"""MMPDERollout.mesh_check: the fold monitor reports det(dx/dxi) of the DMM
stage without changing the step.

An engine with mesh_check = True gives the predictions and meshes of a default
engine bit for bit (cylinder: three fed-back steps; Burgers, array mode with xi
in 'xy' order: one step); its mesh_det / mesh_detmin / mesh_folds are those of
a stand-alone DMM.mesh_hess on the same u, mesh_report() returns them with the
counts summed over the steps, and the Hessian of step 0 is within 2e-5 of
max|H_ref| of float64 autograd.  The same with a DMM whose head is scaled until
the mesh folds (w_o x 64, the branch half of out_nn.layers.0 x 8: the float64
reference folds 10 / 18 nodes of the two cylinder trajectories at step 0), with
hipGraph replay, and a default engine holds no monitor state at all.
"""
import pytest
import torch

from oracle import refcpu

pytestmark = pytest.mark.gpu

H_BAR = 2e-5


def _eq(a, b):
    """torch.equal on the bits (a rollout on a folded mesh may reach NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _case(kind, dev, scale=None):
    from mmpde_amd.synth import build_models, burgers_grid_points, fields

    pde, model, model_b, itp, dmm, gc = build_models(kind)
    B = 2
    if kind == "cy":
        u0 = fields(pde.ori_grid, B, 30)[:, 0]
    else:
        u0 = fields(burgers_grid_points(), B, 31).reshape(B, 31, 48, 48)[:, 0]
    if scale is not None:
        f_wo, f_wb = scale
        L = dmm.trunk.layers[1].out_features
        with torch.no_grad():
            dmm.out_nn.layers[1].weight.mul_(f_wo)
            dmm.out_nn.layers[0].weight[:, :L].mul_(f_wb)
    sd = {n: t.detach().cpu().double() for n, t in dmm.state_dict().items()}
    for m in (model, model_b, itp, dmm):
        m.to(dev)
    return pde, model, model_b, itp, dmm, gc, B, u0.contiguous(), sd


def _hess_ref(kind, sd, u, xi, B):
    """[B N, 3] float64 through refcpu's autograd on xi.repeat(B, 1)."""
    xi = xi.cpu().double()
    rows = xi.repeat(B, 1).clone().requires_grad_(True)
    kw = dict(ori_grid=xi) if kind == "cy" else {}
    with torch.enable_grad():
        phi = refcpu.dmm_forward(sd, "graph" if kind == "cy" else "array", u.cpu().double(), rows, **kw)
        g = torch.autograd.grad(phi.sum(), rows, create_graph=True)[0]
        h1 = torch.autograd.grad(g[:, 0].sum(), rows, retain_graph=True)[0]
        h2 = torch.autograd.grad(g[:, 1].sum(), rows)[0]
    return torch.stack((h1[:, 0], h1[:, 1], h2[:, 1]), dim=1).detach()


def _lockstep(kind, dev, n_steps, scale=None):
    from mmpde_amd.rollout import MMPDERollout

    pde, model, model_b, itp, dmm, gc, B, u0, sd = _case(kind, dev, scale)
    plain = MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev)
    eng = MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev)
    eng.mesh_check = True
    assert eng.mesh_report() is None
    u = u0.to(dev)
    total = torch.zeros(B, dtype=torch.int64)
    for i, s in enumerate(range(1, 1 + n_steps)):
        want = plain.step(u, s).clone()
        got = eng.step(u, s).clone()
        assert _eq(got, want), (kind, s, "the monitor changed the prediction")
        assert _eq(eng.mesh, plain.mesh), (kind, s, "the monitor changed the mesh")
        mesh, hess, det, detmin, folds = dmm.mesh_hess(u, eng.xi)
        torch.cuda.synchronize()
        assert _eq(mesh, eng.mesh)
        assert _eq(hess, eng.mesh_hess) and _eq(det, eng.mesh_det)
        assert _eq(detmin, eng.mesh_detmin) and _eq(folds, eng.mesh_folds)
        total += folds.cpu().long()
        rep = eng.mesh_report()
        assert rep["folds"] == folds.tolist() and _eq(torch.tensor(rep["detmin"], dtype=torch.float32), detmin.cpu())
        assert rep["folds_total"] == total.tolist()
        if i == 0:
            ref = _hess_ref(kind, sd, u, eng.xi, B)
            err = (hess.double().cpu() - ref).abs().max().item()
            scale_h = ref.abs().max().item()
            dref = ((1 + ref[:, 0]) * (1 + ref[:, 2]) - ref[:, 1] ** 2).reshape(B, -1)
            print(f"{kind} scale {scale}: step {s} max|H_ref| {scale_h:.3e} max|err| {err:.3e} = "
                  f"{err / (H_BAR * scale_h):.3f} bar; folds {folds.tolist()} (float64 reference "
                  f"{(~(dref > 0)).sum(1).tolist()}) detmin {detmin.tolist()}")
            assert err <= H_BAR * scale_h
            first = folds.clone()
        u = got
    # a default engine holds no monitor state
    assert plain.mesh_check is False and plain.hess_cache is None and plain.mesh_det is None
    assert plain.mesh_folds_total is None and plain.mesh_report() is None
    return first, total


def test_cylinder_monitor_reports_without_changing_the_step(dev):
    first, total = _lockstep("cy", dev, 3)
    assert int(first.sum()) == 0, "the synthetic DMM folds its own mesh"


def test_cylinder_scaled_head_reports_folds(dev):
    first, total = _lockstep("cy", dev, 3, scale=(64.0, 8.0))
    assert bool((first > 0).all()) and bool((total >= first.cpu().long()).all())


def test_burgers_monitor_reports_without_changing_the_step(dev):
    _lockstep("burgers", dev, 1)


def test_graph_replay_with_the_monitor_on(dev):
    from mmpde_amd.rollout import MMPDERollout

    pde, model, model_b, itp, dmm, gc, B, u0, sd = _case("cy", dev, scale=(64.0, 8.0))
    eager = MMPDERollout("cy", model, model_b, itp, dmm, gc, B, dev)
    eng = MMPDERollout("cy", model, model_b, itp, dmm, gc, B, dev)
    eager.mesh_check = eng.mesh_check = True
    u = u0.to(dev)
    # weight images and caches; the kNN table policy's read-back of the first
    # step is consumed by the second (it cannot be queried inside a capture)
    eng.step(u, 1)
    torch.cuda.synchronize()
    eng.step(u, 1)
    eng.enable_graph(u)
    before = torch.tensor(eng.mesh_report()["folds_total"])
    for s in (1, 2):
        want = eager.step(u, s).clone()
        got = eng.graph_step(u, s).clone()
        torch.cuda.synchronize()
        assert _eq(got, want), (s, "replay differs from the eager step")
        assert _eq(eng.mesh, eager.mesh) and _eq(eng.mesh_det, eager.mesh_det)
        assert _eq(eng.mesh_hess, eager.mesh_hess)
        assert _eq(eng.mesh_detmin, eager.mesh_detmin) and _eq(eng.mesh_folds, eager.mesh_folds)
        rep = eng.mesh_report()
        assert sum(rep["folds"]) > 0
        # the cumulative counter advances on every replay
        assert rep["folds_total"] == (before + torch.tensor(rep["folds"])).tolist()
        before = torch.tensor(rep["folds_total"])
        u = got
