"""DMM.mesh_guarded (mesh_hess, then mmpde_dmm_mesh_relax) on the device, for
every case of mesh_guard_cases.py (what they hold: test_mesh_guard_cases.py).

Per case: hess and folds_before are bitwise DMM.mesh_hess's; lam_b is within
2.5 h_bar of float64 and the guarded set is float64's; alpha_b is within the
alpha bar on guarded trajectories and exactly alpha_max on the others; with the
GPU's alpha_b and the float64 H every node keeps 1 + alpha_b lam_n >= delta - 2.5
h_bar; folds_after == 0 on every trajectory; the mesh is bitwise alpha_b x1 + (1 -
alpha_b) xi in float32 with x1 = DMM.mesh, so unguarded trajectories' rows are
DMM.mesh's at alpha_max = 1.  On the unscaled base cases the whole mesh is
DMM.mesh's and every alpha is 1.  floor = None is DMM.mesh plus the plain
relaxation; train mode and a floor outside (0, 1) are refused.

Measured on MI355X (11 cases, under 1 s): lam within 0.016 - 0.037 h_bar of
float64 (bar 2.5), alpha within 0.007 - 0.016 of its bar, the guarded set
float64's on every trajectory, min_n 1 + alpha_b lam_ref,n - delta between
-4.7e-07 and 5.7e-08 (allowed -2.5 h_bar = -3.2e-05 or lower), folds_after 0
everywhere, no differing mesh bit.
"""
import pytest
import torch

import dmm_hess_cases as H
import mesh_guard_cases as G

pytestmark = pytest.mark.gpu


def _kw(c, dev):
    return {"nbr": c.nbr.to(dev)} if c.mode == "graph" else {}


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", [g[0] for g in G.GUARD_CASES])
def test_guard_case(dev, name):
    r = G.guard_ref(name)
    c, B, N = r.c, r.c.B, r.c.xi.shape[0]
    dmm = H.dmm_with(c, r.sd).to(dev)
    u, xi, kw = c.u.to(dev), c.xi.to(dev), _kw(c, dev)
    x1 = dmm.mesh(u, xi, **kw).cpu()
    _, hess0, det0, detmin0, folds0 = dmm.mesh_hess(u, xi, **kw)
    total = torch.zeros(B, dtype=torch.int32, device=dev)
    mesh, alpha, lam, hess, det, detmin, folds, folds_before = dmm.mesh_guarded(
        u, xi, floor=r.delta, alpha=r.alpha_max, guarded_total=total, **kw)
    torch.cuda.synchronize()
    assert _bits(hess, hess0) and _bits(folds_before, folds0), "the guard changed the monitor's outputs"
    mesh, alpha, lam, det, detmin, folds = (t.cpu() for t in (mesh, alpha, lam, det, detmin, folds))
    e = G.LAM_BARS * r.h_bar
    lam_err = (lam.double() - r.lam_b).abs().max().item()
    guarded = alpha < r.alpha_max
    worst = max(abs(alpha[b].item() - r.alpha[b].item()) / G.alpha_bar(r.alpha[b].item(), r.lam_b[b].item(), r.h_bar)
                for b in range(B) if r.guarded[b])
    after = (1 + alpha.double()[:, None] * r.lam_n).min(1).values
    print(f"{name}: lam {lam_err / r.h_bar:.3f} h_bar (bar 2.5); alpha {worst:.3f} of its bar; guarded "
          f"{int(guarded.sum())} / {B}; min 1 + alpha lam_ref - delta {(after - r.delta).min().item():.2e}; folds "
          f"before {folds_before.tolist()} after {folds.tolist()}; alpha {[round(x, 4) for x in alpha.tolist()]}")
    assert lam_err <= e
    assert torch.equal(guarded, r.guarded), "the guarded set is not float64's"
    assert worst <= 1.0 and bool((alpha[~r.guarded] == r.alpha_max).all())
    assert bool((after >= r.delta - e).all())
    assert int(folds.sum()) == 0 and bool((detmin > 0).all())
    d = det.reshape(B, N)
    assert _bits(detmin, d.min(1).values) and torch.equal(folds, (~(d > 0)).sum(1).to(torch.int32))
    det64, tol = G.det_alpha64(hess.cpu(), alpha)
    assert ((d.double() - det64).abs() <= tol).all()
    # the mesh: the reference's line in float32 on DMM.mesh's rows, bit for bit
    assert _bits(mesh, G.relax32(x1, c.xi, alpha))
    keep = (~r.guarded)[:, None].expand(B, N).reshape(-1)
    if r.alpha_max == 1.0:
        assert _bits(mesh[keep], x1[keep]), "an unguarded trajectory's rows are not DMM.mesh's"
    assert bool((mesh[~keep] != x1[~keep]).any()), "the guard moved nothing"
    assert torch.equal(total.cpu(), r.guarded.to(torch.int32))
    # with the rollout's caches and buffers: the same bits
    hc, kc = dmm.head_cache(xi), dmm.hess_cache(xi)
    out2 = dmm.mesh_guarded(u, xi, floor=r.delta, alpha=r.alpha_max, head_cache=hc, hess_cache=kc,
                            out=torch.empty(B * N, 2, device=dev), det_out=torch.empty(B * N, device=dev),
                            alpha_out=torch.empty(B, device=dev), guarded_total=total, **kw)
    torch.cuda.synchronize()
    assert _bits(out2[0].cpu(), mesh) and _bits(out2[1].cpu(), alpha) and _bits(out2[4].cpu(), det)
    assert torch.equal(total.cpu(), 2 * r.guarded.to(torch.int32))


@pytest.mark.parametrize("args", G.BASE_CASES, ids=lambda a: "-".join(str(x) for x in a))
def test_base_case_keeps_its_mesh(dev, args):
    c = H.base_case(*args)
    dmm, u, xi, kw = c.dmm.to(dev), c.u.to(dev), c.xi.to(dev), _kw(c, dev)
    x1 = dmm.mesh(u, xi, **kw)
    for floor in (0.1, 0.5):
        mesh, alpha, lam, hess, det, detmin, folds, folds_before = dmm.mesh_guarded(u, xi, floor=floor, **kw)
        torch.cuda.synchronize()
        assert _bits(mesh, x1) and bool((alpha == 1.0).all())
        assert int(folds.sum()) == 0 and int(folds_before.sum()) == 0
        ref, _ = H.hess_ref(c, key="base")
        lam_ref = G.lam_min(G.lam_of(ref).reshape(c.B, -1))
        assert (lam.double().cpu() - lam_ref).abs().max().item() <= G.LAM_BARS * H.h_bar(ref)


def test_floor_none_is_the_plain_relaxation_and_refusals(dev):
    c = H.base_case("graph", 130, 3)
    dmm, u, xi, kw = c.dmm.to(dev), c.u.to(dev), c.xi.to(dev), _kw(c, dev)
    x1 = dmm.mesh(u, xi, **kw).cpu()
    out = dmm.mesh_guarded(u, xi, floor=None, alpha=0.5, **kw)
    torch.cuda.synchronize()
    assert all(t is None for t in out[2:]) and bool((out[1] == 0.5).all())
    assert _bits(out[0].cpu(), G.relax32(x1, c.xi, torch.full((c.B,), 0.5)))
    assert _bits(dmm.mesh_guarded(u, xi, floor=None, **kw)[0].cpu(), x1)
    for bad in (dict(floor=0.0), dict(floor=1.0), dict(alpha=1.5), dict(floor=None, alpha=-0.5)):
        with pytest.raises(ValueError):
            dmm.mesh_guarded(u, xi, **bad, **kw)
    dmm.train()
    try:
        with pytest.raises(NotImplementedError):
            dmm.mesh_guarded(u, xi, **kw)
    finally:
        dmm.eval()
    torch.cuda.synchronize()
