"""DMM.mesh_hess (dmm.hip: hess_k_kernel, mesh_hess_wave_kernel<8>,
mesh_hess_kernel, det_reduce_kernel) against float64 autograd.  Inputs and
references: dmm_shape_cases.py, dmm_hess_cases.py; that the bars can see a
dropped unit and what the fold cases hold: test_dmm_hess_cases.py.

(a) hess vs float64, bar 2e-5 of max|H_ref|, on every GRAPH_MESH_CASES /
    ARRAY_MESH_CASES entry: heads off the shipped one (L' != 512: the generic
    kernel), n_per around the wave kernel's four-point workgroup, B = 32 (its
    LDS limit), 33 and 65 (the generic kernel), array mode.
(b) the mesh is torch.equal to DMM.mesh's, with and without caches.
(c) det_out within 2^-22 (1 + max|H|)^2 (fp32 rounding of the determinant's
    terms) of the float64 determinant of the GPU's own hess_out; detmin and
    folds are exactly the min and the !(det > 0) count of det_out; folds_total
    after two calls is twice folds.
(d) fold cases (head scaled until det changes sign): the sign of det_out is the
    reference's outside the margin m (at most 1 % of the nodes inside), the
    per-trajectory counts agree up to the nodes inside, |detmin - min det_ref|
    <= m.
(e) the same bits with both caches, either one, none; on a workspace of 0xFF
    bytes and a zeroed one; on a repeat call; for a trajectory in a batch of
    32 | 33 and 64 | 65.
(f) a NaN trajectory counts every node as folded and leaves the others' bits.
(g) undersized workspaces, caches and outputs raise ValueError; train mode is
    refused.

Measured on MI355X (23 cases, 5 s):
    hess      worst 0.047 bar (9.4e-7 of max|H|, graph B = 33), else <= 0.027 bar;
              fold cases (max|H| 0.66 - 1.06) <= 0.081 bar
    det       <= 6.6e-8 from the float64 det of hess_out (bar 2.4e-7 - 2.7e-7)
    folds     11 / 13 / 15, 4 - 6 per trajectory (161), 0 / 0 / 26: the reference's
              counts on every trajectory, no node inside the margin,
              |detmin - min det_ref| <= 8.8e-7 (m 6.2e-5 - 1.3e-4)
    (b), (e), (f)  no differing bit (before hess_acc's explicit fma order the two
              kernels differed in hess's last bit at 32 | 33)
"""
import pytest
import torch

import dmm_hess_cases as H
import dmm_shape_cases as C

pytestmark = pytest.mark.gpu

NAMES = ("mesh", "hess", "det", "detmin", "folds")


def _ids(cases):
    return ["-".join(str(x) for x in (c if not isinstance(c[-1], tuple) else c[:-1] + c[-1])) for c in cases]


def _ws(dmm, B, n, dev, byte):
    """A workspace of mmpde_dmm_hess_workspace_bytes filled with `byte`."""
    from mmpde_amd import _lib as L

    _, hd = dmm.device_params()
    nb = L.lib().mmpde_dmm_hess_workspace_bytes(B, n, hd.latent, hd.hidden)
    assert nb > 0 and nb % 4 == 0
    return torch.full((nb,), byte, dtype=torch.uint8, device=dev).view(torch.float32)


def _n_ws(c):
    return c.grid.shape[0] if c.mode == "graph" else max(c.xi.shape[0], c.s * c.s)


def _kw(c, dev):
    return {"nbr": c.nbr.to(dev)} if c.mode == "graph" else {}


def _same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        # NaN rows compare as bits
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{name} differs: {what}"


def _variants(c, dev, dmm=None, u=None):
    """mesh_hess with both caches on a 0xFF workspace; the same bits without
    caches (0xFF and zeroed workspaces), with either cache alone and on a repeat
    call.  Returns the first call's outputs."""
    dmm = c.dmm.to(dev) if dmm is None else dmm
    u = (c.u if u is None else u).to(dev)
    xi = c.xi.to(dev)
    kw = _kw(c, dev)
    B, n = u.shape[0], _n_ws(c)
    hc, kc = dmm.head_cache(xi), dmm.hess_cache(xi)
    assert kc.numel() == 3 * xi.shape[0] * c.head[2]
    base = dmm.mesh_hess(u, xi, workspace=_ws(dmm, B, n, dev, 0xFF), head_cache=hc, hess_cache=kc, **kw)
    for what, h, k, byte in (("no cache, 0xFF workspace", None, None, 0xFF), ("no cache, zeroed workspace", None, None, 0),
                             ("head cache alone", hc, None, 0xFF), ("hess cache alone", None, kc, 0xFF),
                             ("repeat call", hc, kc, 0)):
        _same(base, dmm.mesh_hess(u, xi, workspace=_ws(dmm, B, n, dev, byte), head_cache=h, hess_cache=k, **kw), what)
    _same(base, dmm.mesh_hess(u, xi, head_cache=hc, hess_cache=kc, **kw), "own workspace")
    torch.cuda.synchronize()
    return base


def _reductions_are_those_of_det(out, B):
    mesh, hess, det, detmin, folds = out
    d = det.reshape(B, -1)
    assert detmin.shape == (B,) and folds.shape == (B,) and folds.dtype == torch.int32
    assert torch.equal(detmin, d.min(1).values), "detmin is not the min of det_out"
    assert torch.equal(folds, (~(d > 0)).sum(1).to(torch.int32)), "folds is not the !(det > 0) count of det_out"


def _check_case(c, dev, tag):
    ref, _ = H.hess_ref(c, key="base")
    scale, bar = ref.abs().max().item(), H.h_bar(ref)
    dmm, u, xi, kw = c.dmm.to(dev), c.u.to(dev), c.xi.to(dev), _kw(c, dev)
    B, N = c.B, c.xi.shape[0]
    out = _variants(c, dev)
    mesh, hess, det, detmin, folds = out
    assert mesh.shape == (B * N, 2) and hess.shape == ref.shape == (B * N, 3) and det.shape == (B * N,)
    # (a)
    err = (hess.double().cpu() - ref).abs().max().item()
    print(f"{tag}: max|H_ref| {scale:.3e} max|err| {err:.3e} = {err / bar:.3f} bar ({err / scale:.2e} of max|H|)")
    assert torch.isfinite(hess).all() and err <= bar, (tag, err, bar)
    # (b)
    assert torch.equal(mesh, dmm.mesh(u, xi, **kw)), "mesh_hess moved the mesh"
    assert torch.equal(mesh, dmm.mesh(u, xi, head_cache=dmm.head_cache(xi), **kw)), "mesh_hess moved the cached mesh"
    # (c)
    det64 = H.det_of(hess.double().cpu())
    derr = (det.double().cpu() - det64).abs().max().item()
    dbar = 2.0 ** -22 * (1 + hess.abs().max().item()) ** 2
    print(f"{tag}: det vs float64 det of hess_out {derr:.3e} (bar {dbar:.3e}); det in "
          f"[{det.min().item():.4f}, {det.max().item():.4f}] folds {int(folds.sum())}")
    assert derr <= dbar, (tag, derr, dbar)
    _reductions_are_those_of_det(out, B)
    assert int(folds.sum()) == 0, "an unscaled case folded"
    total = torch.zeros(B, dtype=torch.int32, device=dev)
    total[0] = 5      # accumulated, never reset by the call
    for _ in range(2):
        dmm.mesh_hess(u, xi, folds_total=total, **kw)
    expect = 2 * folds
    expect[0] += 5
    assert torch.equal(total, expect)


@pytest.mark.parametrize("n_per,B,head", C.GRAPH_MESH_CASES, ids=_ids(C.GRAPH_MESH_CASES))
def test_graph_hess_vs_float64(dev, n_per, B, head):
    _check_case(C.graph_case(n_per, 5, 1, B, head, False), dev, f"graph hess n_per={n_per} B={B} head={head}")


@pytest.mark.parametrize("s,B", C.ARRAY_MESH_CASES, ids=_ids(C.ARRAY_MESH_CASES))
def test_array_hess_vs_float64(dev, s, B):
    _check_case(C.array_case(s, B), dev, f"array hess s={s} B={B}")


# --------------------------------------------------------------------------- (d) folds
@pytest.mark.parametrize("name", [f[0] for f in H.FOLD_CASES])
def test_fold_case(dev, name):
    c, sd = H.fold_case(name)
    ref, _ = H.hess_ref(c, sd=sd, key=name)
    det_ref = H.det_of(ref).reshape(c.B, -1)
    m, bar = H.sign_margin(ref), H.h_bar(ref)
    dmm = H.dmm_with(c, sd).to(dev)
    out = _variants(c, dev, dmm=dmm)
    mesh, hess, det, detmin, folds = out
    _reductions_are_those_of_det(out, c.B)
    assert torch.equal(mesh, dmm.mesh(c.u.to(dev), c.xi.to(dev), **_kw(c, dev)))
    err = (hess.double().cpu() - ref).abs().max().item()
    inside = det_ref.abs() <= m
    folds_ref = (~(det_ref > 0)).sum(1)
    d = det.double().cpu().reshape(c.B, -1)
    dmin_err = (detmin.double().cpu() - det_ref.min(1).values).abs().max().item()
    print(f"{name}: max|H_ref| {ref.abs().max().item():.3f} hess {err / bar:.3f} bar; folds {folds.tolist()} "
          f"reference {folds_ref.tolist()}; {int(inside.sum())} nodes inside the margin {m:.2e}; "
          f"max|detmin - min det_ref| {dmin_err:.2e}")
    assert err <= bar
    assert int(inside.sum()) <= 0.01 * inside.numel()
    assert torch.equal((d > 0)[~inside], (det_ref > 0)[~inside]), "a sign outside the margin differs"
    assert int(folds.sum()) > 0
    assert bool(((folds.cpu().long() - folds_ref).abs() <= inside.sum(1)).all())
    assert dmin_err <= m


# --------------------------------------------------------------------------- (e) independence of B
@pytest.mark.parametrize("b1,b2", [(32, 33), (64, 65)])
@pytest.mark.parametrize("mode", ["graph", "array"])
def test_trajectory_does_not_depend_on_its_batch(dev, mode, b1, b2):
    """32 | 33 is mesh_hess_wave_kernel<8> against mesh_hess_kernel, 64 | 65 the
    first row past the skinny linears' 64-row scratch."""
    c = H.base_case(mode, 130 if mode == "graph" else 33, b2)
    dmm, xi, kw = c.dmm.to(dev), c.xi.to(dev), _kw(c, dev)
    n = c.xi.shape[0]
    big = dmm.mesh_hess(c.u.to(dev), xi, **kw)
    small = dmm.mesh_hess(c.u[:b1].to(dev), xi, **kw)
    torch.cuda.synchronize()
    for name, x, y, rows in zip(NAMES, big, small, (b1 * n, b1 * n, b1 * n, b1, b1)):
        assert y.shape[0] == rows
        assert torch.equal(x[:rows], y), f"{name} of a trajectory depends on its batch ({b1} | {b2})"


# --------------------------------------------------------------------------- (f) NaN
@pytest.mark.parametrize("B", [3, 33])
def test_nan_trajectory_counts_as_folded(dev, B):
    c = H.base_case("graph", 130, B)
    n = c.xi.shape[0]
    clean = _variants(c, dev)
    u = c.u.clone()
    u[1] = float("nan")
    out = _variants(c, dev, u=u)
    mesh, hess, det, detmin, folds = out
    assert int(folds[1]) == n and bool(torch.isnan(detmin[1])) and bool(torch.isnan(det[n:2 * n]).all())
    keep = torch.arange(B, device=dev) != 1
    for name, x, y, per in zip(NAMES, out, clean, (n, n, n, 1, 1)):
        x, y = x.reshape(B, per, -1)[keep], y.reshape(B, per, -1)[keep]
        assert torch.equal(x, y), f"{name} of a clean trajectory changed beside a NaN one"
    assert int(folds[keep].sum()) == 0


# --------------------------------------------------------------------------- argument checks
def test_undersized_buffers_and_train_mode_are_refused(dev):
    c = H.base_case("graph", 130, 3)
    dmm, u, xi, kw = c.dmm.to(dev), c.u.to(dev), c.xi.to(dev), _kw(c, dev)
    hc, kc = dmm.head_cache(xi), dmm.hess_cache(xi)
    ws = _ws(dmm, c.B, 130, dev, 0)
    for bad in (dict(workspace=ws[:-1]), dict(head_cache=hc[:-1]), dict(hess_cache=kc[:-1]),
                dict(hess_out=torch.empty(c.B * 130, 2, device=dev)), dict(det_out=torch.empty(c.B * 130 - 1, device=dev)),
                dict(folds_total=torch.zeros(c.B, dtype=torch.int64, device=dev))):
        with pytest.raises(ValueError):
            dmm.mesh_hess(u, xi, **bad, **kw)
    with pytest.raises(ValueError):
        dmm.hess_cache(xi, workspace=torch.empty(16, device=dev))
    dmm.train()
    try:
        with pytest.raises(NotImplementedError):
            dmm.mesh_hess(u, xi, **kw)
        with pytest.raises(NotImplementedError):
            dmm.hess_cache(xi)
    finally:
        dmm.eval()
    torch.cuda.synchronize()
