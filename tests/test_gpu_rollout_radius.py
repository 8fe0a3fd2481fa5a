"""The rollout engine on connect_edge='radius' (reference mmpde.py
--connect_edge radius, data_creator_2d.py:195,226,257-258): MMPDERollout with
gc.e = "radius" against the oracle.

The oracle's create_graph is kNN-only, so the radius step is composed here
from its parts: create_graph(mesh_override = the engine's mesh) for x / pos,
refcpu.radius_graph(pos[:, 1:3], gc.radius(), B, 32) for the edges of both
graphs, mp_pde_solver on those edges, interpolate_pred.

Bars: the fixed-grid and moved-mesh tables (nbr and deg) and the kNN-30 rows
torch.equal to the oracle's; the step within the ragged-graph bar of
tests/test_radius.py, 2e-4 max|ref| + 1e-7; the binned routing, graph capture
and shards torch.equal to the plain engine; teacher-forced losses 1e-4
relative (tests/test_gpu_eval.py).
"""
import pytest
import torch

from oracle import refcpu

pytestmark = pytest.mark.gpu


def _bar(ref):
    return 2e-4 * ref.abs().max().item() + 1e-7


def _sds(**mods):
    return {k: {n: t.detach().cpu() for n, t in m.state_dict().items()} for k, m in mods.items() if m is not None}


def _case(kind, dev, neighbors=2, B=2, grid=None, moving_mesh=True):
    from mmpde_amd.synth import build_models, burgers_grid_points, fields

    pde, model, model_b, itp, dmm, gc = build_models(kind, grid=grid, moving_mesh=moving_mesh)
    gc.e, gc.n = "radius", neighbors
    if kind == "cy":
        u = fields(pde.ori_grid, B, 30)
        opde = refcpu.PDEConst("cy", pde.grid_size, ori_grid=pde.ori_grid)
    else:
        u = fields(burgers_grid_points(), B, 31).reshape(B, 31, 48, 48)
        opde = refcpu.PDEConst("burgers", pde.grid_size)
    sds = _sds(model=model, model_b=model_b, itp=itp, dmm=dmm)
    for m in (model, model_b, itp, dmm):
        if m is not None:
            m.to(dev)
    return (model, model_b, itp, dmm, gc), u, opde, sds


def _oracle_step(opde, sds, data, s, B, r, mesh=None):
    """The radius step; mesh None: the fixed-grid model alone.  Returns (pred,
    (nbr_u, deg_u), (nbr_m, deg_m) | None, kNN-30 rows | None)."""
    with torch.no_grad():
        gu = refcpu.create_graph(opde, sds.get("itp"), data, data, [s] * B, dmm_sd=None)
        ei_u, nbr_u, deg_u = refcpu.radius_graph(gu.pos[:, 1:3], r, B, 32)
        out_u = refcpu.mp_pde_solver(sds["model"], opde, gu.x, gu.pos, ei_u)
        if mesh is None:
            return out_u, (nbr_u, deg_u), None, None
        gm = refcpu.create_graph(opde, sds["itp"], data, data, [s] * B, dmm_sd=sds["dmm"], mesh_override=mesh)
        ei_m, nbr_m, deg_m = refcpu.radius_graph(gm.pos[:, 1:3], r, B, 32)
        out_b = refcpu.mp_pde_solver(sds["model_b"], opde, gm.x, gm.pos, ei_m)
        ip, idx = refcpu.interpolate_pred(opde, sds["itp"], out_b, gm, data, return_idx=True)
    return ip + out_u, (nbr_u, deg_u), (nbr_m, deg_m), idx


def _check_step(eng, opde, sds, u, s, tag):
    """One engine step from u against the oracle's on the engine's mesh; returns the prediction."""
    B, N = eng.B, eng.N
    data = u.cpu().reshape(B, 1, *u.shape[1:])
    nxt = eng.step(u, s)
    torch.cuda.synchronize()
    ref, (nbr_u, deg_u), (nbr_m, deg_m), idx = _oracle_step(opde, sds, data, s, B, eng.gc.radius(),
                                                           mesh=eng.mesh.cpu())
    assert torch.equal(eng.deg_u.long().cpu(), deg_u) and torch.equal(eng.nbr_u.long().cpu(), nbr_u), (tag, s)
    assert torch.equal(eng.deg_m.long().cpu(), deg_m), (tag, s, "moved-mesh degrees")
    assert torch.equal(eng.nbr_m.long().cpu(), nbr_m), (tag, s, "moved-mesh radius rows")
    assert torch.equal(eng.idx2.long().cpu().reshape(B, N, 30), idx.reshape(B, N, 30)), (tag, s, "kNN-30")
    err = (nxt.cpu().reshape(-1) - ref.reshape(-1)).abs().max().item()
    print(f"{tag} step {s}: max|err| {err:.3e} bar {_bar(ref):.3e} (max|ref| {ref.abs().max().item():.3e}); "
          f"degrees fixed {deg_u.float().mean():.1f} [{int(deg_u.min())}, {int(deg_u.max())}] "
          f"moved {deg_m.float().mean():.1f} [{int(deg_m.min())}, {int(deg_m.max())}]", flush=True)
    assert err <= _bar(ref), (tag, s, err, _bar(ref))
    return nxt


@pytest.mark.parametrize("edge_gemm", ["f16x3", "f32"])
@pytest.mark.parametrize("kind", ["cy", "burgers"])
def test_radius_rollout_lockstep(dev, kind, edge_gemm):
    """Three fed-back steps at B = 2, neighbors = 2.  (An engine that ignores
    connect_edge builds kNN-2 tables here and fails the table comparison.)"""
    from mmpde_amd.rollout import MMPDERollout

    (model, model_b, itp, dmm, gc), u, opde, sds = _case(kind, dev)
    model.edge_gemm = model_b.edge_gemm = edge_gemm
    eng = MMPDERollout(kind, model, model_b, itp, dmm, gc, 2, dev)
    assert eng.nbr_u.shape[1] == 33 and eng.deg_u is not None
    modes = eng.knn_modes()
    assert modes["graph"] == "radius" and set(modes) == {"graph", "query"} | ({"query1"} if kind == "burgers" else set())
    x = u[:, 0].to(dev).contiguous()
    for s in (1, 2, 3):
        x = _check_step(eng, opde, sds, x, s, f"{kind} {edge_gemm}")
    share = eng.knn_table_share()
    assert share is not None and share[0] is None          # no kNN table serves the graph role


def test_radius_rollout_empty_rows(dev):
    """neighbors = 1 on the cylinder mesh: rows of degree 0 in the fixed grid."""
    from mmpde_amd.rollout import MMPDERollout

    (model, model_b, itp, dmm, gc), u, opde, sds = _case("cy", dev, neighbors=1)
    eng = MMPDERollout("cy", model, model_b, itp, dmm, gc, 2, dev)
    assert int(eng.deg_u.min().item()) == 0
    _check_step(eng, opde, sds, u[:, 4].to(dev).contiguous(), 5, "cy neighbors=1")


def test_radius_rollout_without_moving_mesh(dev):
    from mmpde_amd.rollout import MMPDERollout

    (model, _, _, _, gc), u, opde, sds = _case("cy", dev, moving_mesh=False)
    B, s = 2, 5
    eng = MMPDERollout("cy", model, None, None, None, gc, B, dev, moving_mesh=False)
    x = u[:, s - 1].to(dev).contiguous()
    got = eng.step(x, s)
    ref, (nbr_u, deg_u), _, _ = _oracle_step(opde, sds, u[:, s - 1:s], s, B, gc.radius())
    assert torch.equal(eng.deg_u.long().cpu(), deg_u) and torch.equal(eng.nbr_u.long().cpu(), nbr_u)
    err = (got.cpu().reshape(-1) - ref.reshape(-1)).abs().max().item()
    print(f"cy fixed grid only: max|err| {err:.3e} bar {_bar(ref):.3e}")
    assert err <= _bar(ref)
    assert eng.knn_modes() == {}
    keep = got.clone()
    eng.enable_graph(x)
    assert torch.equal(eng.graph_step(x, s), keep)


def _run(eng, u0, binned, steps=3):
    eng.radius_binned = binned
    u, keep = u0, []
    for s in range(4, 4 + steps):
        u = eng.step(u, s)
        torch.cuda.synchronize()
        keep.append((u.clone(), eng.nbr_m.clone(), eng.deg_m.clone(), eng.idx2.clone()))
    return keep


def _same(a, b):
    for s, (x, y) in enumerate(zip(a, b)):
        for name, t, w in zip(("pred", "nbr_m", "deg_m", "idx2"), x, y):
            assert torch.equal(t, w), (s, name)


def test_radius_rollout_large_mesh_binned_and_captured(dev):
    """A 4500-point cylinder mesh: the moved-mesh radius graph goes through the
    step's bins by default, three steps equal the same engine with that off,
    and one graph-captured step equals the eager one."""
    from mmpde_amd import ops
    from mmpde_amd.rollout import MMPDERollout
    from mmpde_amd.synth import generate_cy_mesh

    (model, model_b, itp, dmm, gc), u, _, _ = _case("cy", dev, grid=generate_cy_mesh(n=4500))
    eng = MMPDERollout("cy", model, model_b, itp, dmm, gc, 2, dev)
    assert eng.knn_binned is True and eng.N >= ops.KNN_BINNED_MIN_POINTS
    assert eng.radius_binned is None and eng.knn_modes()["graph"] == "radius-binned"
    u0 = u[:, 3].to(dev).contiguous()
    auto = _run(eng, u0, None)
    on = _run(eng, u0, True)
    assert eng.knn_modes()["graph"] == "radius-binned"
    off = _run(eng, u0, False)
    assert eng.knn_modes() == {"graph": "radius", "query": "binned"}
    _same(on, off)
    _same(auto, on)
    d = on[0][2].float()
    print(f"4500-point mesh: moved degrees mean {d.mean():.1f} [{int(d.min())}, {int(d.max())}]")
    eng.radius_binned = None
    eng.enable_graph(u0)
    g = eng.graph_step(u0, 4)
    torch.cuda.synchronize()
    assert torch.equal(g, on[0][0])
    assert torch.equal(eng.nbr_m, on[0][1]) and torch.equal(eng.deg_m, on[0][2])
    assert torch.equal(eng.idx2, on[0][3])


def test_radius_rollout_small_mesh_forced_through_bins(dev):
    """Burgers 48 x 48 takes the default the measured threshold gives it; forced
    either way (bins built for the graph alone, the kNN-30 queries still on
    their tables) the step is the same."""
    from mmpde_amd import ops
    from mmpde_amd.rollout import MMPDERollout

    (model, model_b, itp, dmm, gc), u, _, _ = _case("burgers", dev)
    eng = MMPDERollout("burgers", model, model_b, itp, dmm, gc, 2, dev)
    want = "radius-binned" if eng.N >= ops.RADIUS_BINNED_MIN_POINTS else "radius"
    assert eng.knn_binned is False and eng.knn_modes()["graph"] == want
    u0 = u[:, 3].to(dev).contiguous()
    off = _run(eng, u0, False, steps=2)
    on = _run(eng, u0, True, steps=2)
    assert eng.knn_modes()["graph"] == "radius-binned" and eng.knn_modes()["query"] != "binned"
    _same(on, off)


@pytest.mark.parametrize("edge_gemm", ["f16x3", "f32"])
def test_radius_rollout_shard_invariance(dev, edge_gemm):
    """An engine at B = 4 equals, trajectory by trajectory, two engines at B = 2."""
    from mmpde_amd.rollout import MMPDERollout

    (model, model_b, itp, dmm, gc), u, _, _ = _case("cy", dev, B=4)
    model.edge_gemm = model_b.edge_gemm = edge_gemm
    u0 = u[:, 3].to(dev).contiguous()
    whole = MMPDERollout("cy", model, model_b, itp, dmm, gc, 4, dev).rollout(u0, 4, 2).clone()
    for lo in (0, 2):
        part = MMPDERollout("cy", model, model_b, itp, dmm, gc, 2, dev).rollout(u0[lo:lo + 2].contiguous(), 4, 2)
        torch.cuda.synchronize()
        diff = (part - whole[lo:lo + 2]).abs().max().item()
        print(f"{edge_gemm} trajectories {lo}..{lo + 1}: max|diff| {diff:.3e}")
        assert torch.equal(part, whole[lo:lo + 2]), (edge_gemm, lo, diff)


def test_radius_teacher_forced_losses(dev):
    """evaluate.test_timestep_losses on steps [3, 4] against the losses of the
    composed oracle step (on the engine's mesh of the same step)."""
    from mmpde_amd import evaluate as EV
    from mmpde_amd.rollout import MMPDERollout

    B, steps = 2, [3, 4]
    (model, model_b, itp, dmm, gc), u, opde, sds = _case("cy", dev, B=B)
    eng = MMPDERollout("cy", model, model_b, itp, dmm, gc, B, dev)
    ud = u.to(dev)
    ref_traj = []
    for s in steps:
        eng.step(ud[:, s - 1].contiguous(), s)              # the mesh of this teacher-forced step
        torch.cuda.synchronize()
        pred, _, _, _ = _oracle_step(opde, sds, u[:, s - 1:s], s, B, gc.radius(), mesh=eng.mesh.cpu())
        d = pred.reshape(B, -1) - u[:, s].reshape(B, -1)
        ref_traj.append((d * d).mean(1))
    ref_traj = torch.stack(ref_traj)
    res = EV.test_timestep_losses(eng, ud, B, steps=steps)
    got = res["per_trajectory"].cpu()
    print("radius per-step", res["per_step"].tolist(), "oracle", ref_traj.mean(1).tolist())
    assert torch.allclose(got, ref_traj, rtol=1e-4, atol=0)
    assert torch.allclose(res["per_step"].cpu(), ref_traj.mean(1), rtol=1e-4, atol=0)
    assert abs(res["mean"].item() - ref_traj.mean().item()) <= 1e-4 * ref_traj.mean().item()


def test_unknown_connect_edge_is_refused(dev):
    from mmpde_amd.rollout import MMPDERollout

    (model, model_b, itp, dmm, gc), _, _, _ = _case("cy", dev)
    gc.e = "delaunay"
    with pytest.raises(ValueError, match="delaunay"):
        MMPDERollout("cy", model, model_b, itp, dmm, gc, 2, dev)
    with pytest.raises(ValueError, match="delaunay"):
        MMPDERollout("cy", model, None, None, None, gc, 2, dev, moving_mesh=False)
