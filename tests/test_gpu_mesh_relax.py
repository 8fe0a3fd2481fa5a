"""ops.mesh_relax (dmm.hip: relax_alpha_kernel, mesh_relax_kernel, then
det_reduce_kernel) alone, on hand-made tensors: the entry takes Hess phi as
data, so the kernels are driven at their edge shapes without a DMM.

N in {1, 63, 64, 65, 255, 256, 257, 2521} x B in {1, 3, 33}: one point, around
a wave and a 256-row block, and a trajectory of ten blocks whose boundaries fall
inside a 256-thread stride of the flat row index.  xi and x1 uniform in (0, 1),
H uniform in +-0.3 (lambda_n >= -0.73: nothing guarded at delta = 0.1), and in
chosen trajectories one planted node with lambda = -(1.6 + 0.05 b) (alpha_b from
0.56 down to 0.28, different per trajectory) at index 0, N - 1 or the last index before
a 256 boundary, in turn.  N = 64: no trajectory planted; (N, B) = (257, 33) and
(2521, 3): trajectory B - 1 alone; else every even trajectory.

Against the float32 / float64 host restatement of the contract
(mesh_guard_cases.py): lam_out within 4 ulp of the host's float32 evaluation, and
bit for bit the formula with every operation correctly rounded by itself
(lam_of_rounded32: the kernel fuses nothing; a host's own float32 kernels need
not be that exact); alpha_out within 4 ulp of
(1 - delta) / (-lam_out) and within the alpha bar of float64; the guarded set is
float64's; the mesh is bitwise alpha x1 + (1 - alpha) xi in float32 with the
returned alpha, rows of alpha == 1 bitwise x1; det_out within the rounding bound
of det_of of det(I + alpha H) in float64, detmin_out / folds_out exactly the
reductions of det_out; guarded_total accumulates; a second call from x1 gives
the same bits.  Guard off: alpha 0 gives xi, 1 gives x1, 0.5 the formula.  One
NaN in one trajectory's H: alpha 0, mesh xi, lam NaN, the others untouched.

Measured on MI355X (35 cases, 3 s): lam 0 ulp from the correctly rounded formula
and <= 2 ulp from the host's float32 torch evaluation (whose sqrt or sum was 1
ulp off on that host); alpha 0 ulp from (1 - delta) / (-lam), <= 1.2e-3 of the
float64 alpha bar; det <= 0.16 of its rounding bound; no differing mesh bit.
"""
import pytest
import torch

import mesh_guard_cases as G

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 255, 256, 257, 2521)
BS = (1, 3, 33)
DELTA = 0.1


def _planted(N, B):
    """{trajectory: node index} of the planted extremes."""
    if N == 64:
        return {}
    spots = [0, N - 1] + ([(N - 1) // 256 * 256 - 1] if N > 256 else [])
    if (N, B) in ((257, 33), (2521, 3)):
        return {B - 1: spots[-1]}
    return {b: spots[(b // 2) % len(spots)] for b in range(0, B, 2)}


def _inputs(N, B, seed=0):
    g = torch.Generator().manual_seed(1000 * N + B + seed)
    xi = torch.rand(N, 2, generator=g)
    x1 = torch.rand(B * N, 2, generator=g)
    h = 0.6 * torch.rand(B * N, 3, generator=g) - 0.3
    for b, i in _planted(N, B).items():
        # eigenvalues 0.2 + 0.05 b and -(1.6 + 0.05 b), rotated off the axes
        lo, hi, t = -(1.6 + 0.05 * b), 0.2 + 0.05 * b, 0.3 + 0.1 * b
        cs, sn = torch.cos(torch.tensor(t)).item(), torch.sin(torch.tensor(t)).item()
        h[b * N + i] = torch.tensor([lo * cs * cs + hi * sn * sn, (lo - hi) * cs * sn, lo * sn * sn + hi * cs * cs])
    return xi, x1, h


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _run(dev, xi, x1, h, B, alpha_max, floor, total):
    from mmpde_amd import ops

    mesh = x1.to(dev).clone()
    det = torch.empty(x1.shape[0], device=dev)
    out = ops.mesh_relax(mesh, xi.to(dev), h.to(dev), batches=B, alpha=alpha_max, floor=floor, det_out=det,
                         guarded_total=total)
    torch.cuda.synchronize()
    assert out[0] is mesh
    return [t.cpu() for t in out] + [det.cpu()]


def _check(dev, N, B, alpha_max, tag):
    xi, x1, h = _inputs(N, B)
    am, dl = G.f32(alpha_max), G.f32(DELTA)
    total = torch.zeros(B, dtype=torch.int32, device=dev)
    total[0] = 7          # accumulated, never reset by the call
    mesh, alpha, lam, detmin, folds, det = _run(dev, xi, x1, h, B, alpha_max, DELTA, total)
    # the float32 and float64 restatements
    lam32 = G.lam_min(G.lam_of(h).reshape(B, N))
    lam64 = G.lam_min(G.lam_of(h.double()).reshape(B, N))
    a64 = G.alpha_of(lam64, am, dl)
    guarded64 = (1 + am * lam64) < dl
    h_bar = 2e-5 * h.abs().max().item()
    assert bool((((1 + am * lam64) - dl).abs() > G.MARGIN_BARS * h_bar).all()), "inputs: a decision is undefined"
    assert guarded64.tolist() == [b in _planted(N, B) for b in range(B)]
    # lam
    lam_ulps = max(abs(x - y) / G.ulp32(y) for x, y in zip(lam.tolist(), lam32.tolist()))
    assert lam_ulps <= 4, (tag, lam_ulps)
    # and bit for bit the formula with every operation correctly rounded by itself
    assert _bits(lam, G.lam_min(G.lam_of_rounded32(h).reshape(B, N))), (tag, "lam: an operation is fused or not IEEE")
    # alpha: from the returned lam in float32, against float64, and the guarded set
    a_from_lam = G.alpha_of(lam, am, dl)
    a_ulps = max(abs(x - y) / G.ulp32(y) for x, y in zip(alpha.tolist(), a_from_lam.tolist()))
    assert a_ulps <= 4, (tag, a_ulps)
    assert ((alpha < am) == guarded64).all(), (tag, alpha, guarded64)
    assert bool((alpha[~guarded64] == am).all())
    worst = 0.0
    for b in range(B):
        if guarded64[b]:
            bar = G.alpha_bar(a64[b].item(), lam64[b].item(), h_bar)
            worst = max(worst, abs(alpha[b].item() - a64[b].item()) / bar)
    assert worst <= 1.0, (tag, worst)
    # the mesh, bit for bit
    assert _bits(mesh, G.relax32(x1, xi, alpha)), (tag, "mesh is not alpha x1 + (1 - alpha) xi in float32")
    if am == 1.0:
        keep = (~guarded64)[:, None].expand(B, N).reshape(-1)
        assert _bits(mesh[keep], x1[keep]), "rows of an alpha == 1 trajectory changed"
    # det after the guard and its reductions
    det64, tol = G.det_alpha64(h, alpha)
    derr = ((det.double().reshape(B, N) - det64).abs() / tol).max().item()
    assert derr <= 1.0, (tag, derr)
    d = det.reshape(B, N)
    assert _bits(detmin, d.min(1).values) and torch.equal(folds, (~(d > 0)).sum(1).to(torch.int32))
    lower, upper = (det64 < -tol).sum(1), (~(det64 > tol)).sum(1)
    assert bool((folds >= lower).all()) and bool((folds <= upper).all()), (tag, folds, lower, upper)
    assert int(folds.sum()) == 0, "1 + alpha lam_n >= delta at every node, so det > 0"
    # a second call from x1: the same bits, the counter advanced again
    again = _run(dev, xi, x1, h, B, alpha_max, DELTA, total)
    for name, x, y in zip(("mesh", "alpha", "lam", "detmin", "folds", "det"),
                          (mesh, alpha, lam, detmin, folds, det), again):
        assert _bits(x, y), (tag, name, "differs on a repeat call")
    expect = 2 * (alpha < am).to(torch.int32)
    expect[0] += 7
    assert torch.equal(total.cpu(), expect)
    print(f"{tag}: guarded {int(guarded64.sum())} / {B}; lam {lam_ulps:.1f} ulp of float32, alpha {a_ulps:.1f} ulp of "
          f"(1 - delta) / (-lam), {worst:.2e} of the alpha bar; det {derr:.3f} of its bound")


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("N", NS)
def test_guard_at_edge_shapes(dev, N, B):
    _check(dev, N, B, 1.0, f"relax N={N} B={B}")


@pytest.mark.parametrize("N,B", [(257, 3), (2521, 33)])
def test_guard_below_alpha_max(dev, N, B):
    """alpha_max = 0.8: unguarded trajectories are relaxed by 0.8 (1 - 0.8 x 0.73 >
    0.1), planted ones by less."""
    _check(dev, N, B, 0.8, f"relax N={N} B={B} alpha_max=0.8")


@pytest.mark.parametrize("N,B", [(1, 3), (257, 3), (2521, 33)])
def test_guard_off_is_the_plain_relaxation(dev, N, B):
    from mmpde_amd import ops

    xi, x1, h = _inputs(N, B)
    for a in (0.0, 0.5, 1.0):
        mesh = x1.to(dev).clone()
        total = torch.zeros(B, dtype=torch.int32, device=dev)
        out = ops.mesh_relax(mesh, xi.to(dev), batches=B, alpha=a, guarded_total=total)
        torch.cuda.synchronize()
        assert out[2] is None and out[3] is None and out[4] is None
        assert torch.equal(out[1].cpu(), torch.full((B,), a)) and int(total.sum()) == 0
        want = {0.0: xi.repeat(B, 1), 1.0: x1}.get(a, G.relax32(x1, xi, torch.full((B,), a)))
        assert _bits(mesh.cpu(), want), (N, B, a)
    # with the Hessian and no floor: lam and det of the plain relaxation, nothing guarded
    mesh = x1.to(dev).clone()
    _, alpha, lam, detmin, folds = ops.mesh_relax(mesh, xi.to(dev), h.to(dev), batches=B, alpha=0.5)
    torch.cuda.synchronize()
    assert bool((alpha == 0.5).all()) and _bits(mesh.cpu(), G.relax32(x1, xi, torch.full((B,), 0.5)))
    lam32 = G.lam_min(G.lam_of(h).reshape(B, N))
    assert max(abs(x - y) / G.ulp32(y) for x, y in zip(lam.tolist(), lam32.tolist())) <= 4


@pytest.mark.parametrize("N,B", [(65, 3), (2521, 33)])
def test_one_nan_in_one_trajectory(dev, N, B):
    xi, x1, h = _inputs(N, B)
    total = torch.zeros(B, dtype=torch.int32, device=dev)
    clean = _run(dev, xi, x1, h, B, 1.0, DELTA, total)
    hn = h.clone()
    hn[1 * N + N // 2, 1] = float("nan")
    mesh, alpha, lam, detmin, folds, det = _run(dev, xi, x1, hn, B, 1.0, DELTA, total)
    assert alpha[1] == 0.0 and bool(torch.isnan(lam[1])) and _bits(mesh[N:2 * N], xi)
    assert bool(torch.isnan(detmin[1])) and int(folds[1]) == 1      # det(I + 0 NaN) at that node alone
    keep = torch.arange(B) != 1
    for name, x, y, per in zip(("mesh", "alpha", "lam", "detmin", "folds", "det"),
                               (mesh, alpha, lam, detmin, folds, det), clean, (N, 1, 1, 1, 1, N)):
        assert _bits(x.reshape(B, per, -1)[keep], y.reshape(B, per, -1)[keep]), f"{name} changed beside a NaN trajectory"
    assert total.cpu()[1] == (2 if 1 in _planted(N, B) else 1)


def test_argument_checks(dev):
    from mmpde_amd import ops

    xi, x1, h = _inputs(65, 3)
    mesh, xi_d, h_d = x1.to(dev), xi.to(dev), h.to(dev)
    for bad in (dict(alpha=1.5), dict(alpha=-0.1), dict(floor=0.0, hess=h_d), dict(floor=1.0, hess=h_d),
                dict(floor=0.1), dict(lam_out=torch.empty(3, device=dev)), dict(hess=h_d[:-1]),
                dict(hess=h_d, alpha_out=torch.empty(2, device=dev)),
                dict(hess=h_d, folds_out=torch.empty(3, device=dev)),
                dict(guarded_total=torch.zeros(3, dtype=torch.int64, device=dev)), dict(batches=2)):
        kw = dict(dict(batches=3), **bad)
        with pytest.raises(ValueError):
            ops.mesh_relax(mesh, xi_d, kw.pop("hess", None), **kw)
    with pytest.raises(ValueError):
        ops.mesh_relax(mesh.double(), xi_d, batches=3)
    with pytest.raises(ValueError):
        ops.mesh_relax(mesh.t().contiguous().t(), xi_d, batches=3)
    torch.cuda.synchronize()
    assert _bits(mesh.cpu(), x1), "a refused call touched the mesh"
