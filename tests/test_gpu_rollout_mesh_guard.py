"""MMPDERollout.mesh_guard: the fold guard in the DMM stage of the step (set up
as test_gpu_rollout_mesh_check.py, B = 2).

Default models, mesh_guard = 0.1 (cylinder: three fed-back steps; Burgers: one):
nothing folds, so predictions and meshes are bitwise a default engine's, alpha
== [1, 1] and guarded_total == [0, 0].  Fold-scaled cylinder DMM (w_o x 64,
branch half x 8; float64 at step 0: lam_b -1.0166 / -1.0265, 10 / 18 folded
nodes, alpha_ref 0.8853 / 0.8768), three fed-back steps: folds > 0 before and
folds_after == 0 at every step, alpha < 1 where float64 says so, engine.mesh is
bitwise DMM.mesh_guarded's, predictions finite, guarded_total the per-step sum,
and every step's prediction is bitwise the API composition on a creator with
mesh_guard = 0.1 (create_graph -> model_b -> interpolate_pred + model(graph_uni):
test_gpu_parity.py compares the unguarded step bit for bit, so this does too).
hipGraph replay with the guard on is bitwise the eager guarded steps, counters
included.  A default engine holds no guard state and a mesh_check-only engine
reports exactly the monitor's keys.
"""
import pytest
import torch

import mesh_guard_cases as G
import test_gpu_rollout_mesh_check as M

pytestmark = pytest.mark.gpu

DELTA = 0.1
MONITOR_KEYS = ["folds", "detmin", "folds_total"]
GUARD_KEYS = MONITOR_KEYS + ["alpha", "lam_min", "folds_after", "detmin_after", "guarded_total"]
SCALE = (64.0, 8.0)


def _engines(kind, dev, scale=None):
    from mmpde_amd.rollout import MMPDERollout

    pde, model, model_b, itp, dmm, gc, B, u0, sd = M._case(kind, dev, scale)
    plain = MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev)
    eng = MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev)
    assert eng.mesh_guard is None and eng.mesh_alpha == 1.0     # the creator's defaults
    eng.mesh_guard = DELTA
    return plain, eng, (pde, model, model_b, itp, dmm, gc, B, u0, sd)


@pytest.mark.parametrize("kind,n_steps", [("cy", 3), ("burgers", 1)])
def test_default_models_keep_their_bits_under_the_guard(dev, kind, n_steps):
    plain, eng, (pde, model, model_b, itp, dmm, gc, B, u0, sd) = _engines(kind, dev)
    assert eng.mesh_report() is None
    u = u0.to(dev)
    for s in range(1, 1 + n_steps):
        want = plain.step(u, s).clone()
        got = eng.step(u, s).clone()
        assert M._eq(got, want), (kind, s, "the guard changed an unfolded step")
        assert M._eq(eng.mesh, plain.mesh), (kind, s, "the guard changed an unfolded mesh")
        rep = eng.mesh_report()
        assert list(rep) == GUARD_KEYS
        assert rep["alpha"] == [1.0, 1.0] and rep["guarded_total"] == [0, 0]
        assert rep["folds"] == [0, 0] and rep["folds_after"] == [0, 0]
        assert all(-0.5 < x < 0.5 for x in rep["lam_min"])     # 1 + lam far above the floor
        # nothing moved: the det after the guard is the det before it
        assert M._eq(eng.mesh_det_after, eng.mesh_det) and M._eq(eng.mesh_detmin_after, eng.mesh_detmin)
        u = got
    # a default engine holds no guard state
    assert plain.mesh_guard is None and plain.mesh_alpha == 1.0
    assert plain.mesh_alpha_b is None and plain.mesh_lam is None and plain.mesh_guarded_total is None
    assert plain.mesh_det_after is None and plain.hess_cache is None and plain.mesh_report() is None


def test_mesh_check_alone_reports_the_monitors_keys(dev):
    plain, eng, (pde, model, model_b, itp, dmm, gc, B, u0, sd) = _engines("cy", dev, SCALE)
    eng.mesh_guard = None
    eng.mesh_check = True
    eng.step(u0.to(dev), 1)
    assert list(eng.mesh_report()) == MONITOR_KEYS
    assert eng.mesh_alpha_b is None and eng.mesh_lam is None


def test_scaled_head_is_guarded_at_every_step(dev):
    plain, eng, (pde, model, model_b, itp, dmm, gc, B, u0, sd) = _engines("cy", dev, SCALE)
    # the same step through the creator's API, with the guard set on the creator
    gc.mesh_guard = DELTA
    try:
        from mmpde_amd.rollout import MMPDERollout
        assert MMPDERollout("cy", model, model_b, itp, dmm, gc, B, dev).mesh_guard == DELTA
        u = u0.to(dev)
        total = torch.zeros(B, dtype=torch.int64)
        for i, s in enumerate(range(1, 4)):
            got = eng.step(u, s).clone()
            mesh, alpha, lam, hess, det, detmin, folds, folds_before = dmm.mesh_guarded(u, eng.xi, floor=DELTA)
            torch.cuda.synchronize()
            assert M._eq(eng.mesh, mesh), (s, "engine.mesh is not DMM.mesh_guarded's")
            assert M._eq(eng.mesh_alpha_b, alpha) and M._eq(eng.mesh_lam, lam) and M._eq(eng.mesh_hess, hess)
            assert M._eq(eng.mesh_det_after, det) and M._eq(eng.mesh_folds, folds_before)
            rep = eng.mesh_report()
            assert list(rep) == GUARD_KEYS
            assert all(f > 0 for f in rep["folds"]), (s, rep)
            assert rep["folds_after"] == [0, 0] and all(d > 0 for d in rep["detmin_after"]), (s, rep)
            assert all(d < 0 for d in rep["detmin"])
            assert bool(torch.isfinite(got).all())
            total += (alpha.cpu() < 1.0).long()
            assert rep["guarded_total"] == total.tolist()
            if i == 0:
                ref = M._hess_ref("cy", sd, u, eng.xi, B)
                h_bar = M.H_BAR * ref.abs().max().item()
                lam_ref = G.lam_min(G.lam_of(ref).reshape(B, -1))
                a_ref = G.alpha_of(lam_ref, 1.0, G.f32(DELTA))
                assert bool((((1 + lam_ref) - G.f32(DELTA)).abs() > G.MARGIN_BARS * h_bar).all())
                assert bool((a_ref < 1).all()), "float64 guards neither trajectory at step 0"
                assert (lam.double().cpu() - lam_ref).abs().max().item() <= G.LAM_BARS * h_bar
                for b in range(B):
                    assert alpha[b].item() < 1.0
                    assert abs(alpha[b].item() - a_ref[b].item()) <= G.alpha_bar(a_ref[b].item(), lam_ref[b].item(), h_bar)
                print(f"step {s}: lam {lam.tolist()} (float64 {lam_ref.tolist()}) alpha {alpha.tolist()} "
                      f"(float64 {a_ref.tolist()}) folds {rep['folds']} -> {rep['folds_after']}")
            # the API composition of the same step
            data = u.reshape(B, 1, -1)
            graph = gc.create_graph(itp, data, data, [s] * B, dev, dmm)
            graph_uni = gc.create_graph(itp, data, data, [s] * B, dev, None)
            pred = gc.interpolate_pred(itp, model_b(graph), graph, data, dev) + model(graph_uni)
            assert M._eq(graph.pos[:, 1:3], eng.mesh), (s, "create_graph's mesh is not the guarded mesh")
            assert M._eq(pred.reshape(-1), got.reshape(-1)), (s, "the API composition differs from the engine")
            u = got
        assert int(total.sum()) > 0
        # the unguarded engine on the same input folds and goes another way
        plain.step(u0.to(dev), 1)
        assert not M._eq(plain.mesh, mesh)
    finally:
        gc.mesh_guard = None


def test_graph_replay_with_the_guard_on(dev):
    plain, eng, (pde, model, model_b, itp, dmm, gc, B, u0, sd) = _engines("cy", dev, SCALE)
    eager = plain
    eager.mesh_guard = DELTA
    u = u0.to(dev)
    # weight images and caches; the kNN table policy's read-back of the first
    # step is consumed by the second (it cannot be queried inside a capture)
    eng.step(u, 1)
    torch.cuda.synchronize()
    eng.step(u, 1)
    eng.enable_graph(u)
    before = eng.mesh_report()
    for s in (1, 2):
        want = eager.step(u, s).clone()
        got = eng.graph_step(u, s).clone()
        torch.cuda.synchronize()
        assert M._eq(got, want), (s, "replay differs from the eager guarded step")
        for name in ("mesh", "mesh_hess", "mesh_det", "mesh_detmin", "mesh_folds", "mesh_alpha_b", "mesh_lam",
                     "mesh_det_after", "mesh_detmin_after", "mesh_folds_after"):
            assert M._eq(getattr(eng, name), getattr(eager, name)), (s, name)
        rep = eng.mesh_report()
        assert sum(rep["folds"]) > 0 and rep["folds_after"] == [0, 0] and all(a < 1 for a in rep["alpha"])
        # the cumulative counters advance on every replay
        assert rep["folds_total"] == [x + y for x, y in zip(before["folds_total"], rep["folds"])]
        assert rep["guarded_total"] == [x + int(a < 1) for x, a in zip(before["guarded_total"], rep["alpha"])]
        before = rep
        u = got


def test_plain_relaxation_in_the_step(dev):
    """mesh_alpha = 0.5 with no guard: the mesh is halfway to the fixed grid, no
    Hessian state is built."""
    plain, eng, (pde, model, model_b, itp, dmm, gc, B, u0, sd) = _engines("cy", dev)
    eng.mesh_guard = None
    eng.mesh_alpha = 0.5
    u = u0.to(dev)
    plain.step(u, 1)
    got = eng.step(u, 1)
    torch.cuda.synchronize()
    want = G.relax32(plain.mesh.cpu(), eng.xi.cpu(), torch.full((B,), 0.5))
    assert M._eq(eng.mesh.cpu(), want) and bool(torch.isfinite(got).all())
    assert eng.hess_cache is None and eng.mesh_report() is None
