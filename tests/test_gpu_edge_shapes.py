"""The message_net_2 edge stage (gnn_2d.py:59-63 + PyG aggr='mean'),

    mean_i = 1 / max(deg_i, 1) * sum_{e < deg_i} relu(W2 relu(a_i + b_nbr(i,e)) + b2),

kernel by kernel against a plain float64 evaluation, at the shapes where the
kernels take another path: one row, partial and whole 16-row tiles, a whole
tile of degree-0 rows, k around the 36-slot unroll of the split-scale gathers
(edge_wave.hip pass_scale, layer.hpp nbr_bmax), k around the 64-slot limit of
the ReLU mask and the fp16x3 backward (edge_bwd.hip FKMAX), k = 1 streams
whose summation units span many tiles, and side blocks capped by the tile
count.  All 128 channels of every row are compared.

Forward variants:
    mean         mmpde_gnn_edge_mean        (edge_mean_kernel, fixed degree only)
    f32          mmpde_gnn_edge_mean_ex     F32, no mask    (ring kernel)
    f32+mask     mmpde_gnn_edge_mean_ex     F32, ReLU mask  (ring kernel)
    f16x3+mask   mmpde_gnn_edge_mean_ex     F16X3, mask     (row_scale_kernel + ring kernel)
    f16x3-wave   mmpde_gnn_edge_mean_ex     F16X3, no mask  (wave kernel + edge_finish_kernel)

Bars: every variant max|out - ref| <= 2e-5 max|ref| (the edge-stage bar of
test_gpu_train.py); the f16x3 variants also max and rms error <= 4 x the larger
of the f32 variant's and a CPU fp32 torch evaluation's (+ 1e-12, the rule of
test_gpu_precision.py); every variant bitwise equal to a second run.

ReLU mask bits ([n k][4] words, bit c % 32 of word c / 32): equal to the sign
of the float64 z2 wherever |z2| > tol, tol = 4 * 129 * 2^-24 * (|W2| z1 + |b2|):
the gamma_129 bound of a 129-term fp32 dot product, doubled twice for the
split's operand and cross-term error.  The elements inside tol are counted
and capped (1e-3 of the live elements; 2 elements below 5000 live elements).
Padding-slot bits are unspecified.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS_TILES = [(1, 1), (5, 3), (16, 4), (17, 5), (37, 35), (203, 9)]
UNROLL_36 = [(100, 35), (100, 36), (100, 37), (100, 40)]
MASK_LIMIT = [(64, 63), (64, 64), (50, 65), (50, 70)]
LONG_UNITS = [(704, 1), (1123, 1)]
SIDE_BLOCKS = [(48, 64)]
SHAPES = ROWS_TILES + UNROLL_36 + MASK_LIMIT + LONG_UNITS + SIDE_BLOCKS
MASK_SHAPES = [s for s in SHAPES if s[1] <= 64]
BWD_SHAPES = [(1, 1), (5, 3), (17, 5), (37, 35), (100, 37), (64, 64), (50, 65)]
VARIANTS = ("mean", "f32", "f32+mask", "f16x3+mask", "f16x3-wave")


# --------------------------------------------------------------------------- inputs and references
def _edge_mean_ref(a, b, w2, b2, nbr, deg):
    """The edge stage in plain torch (test_gpu_train.py's): padding slots
    (e >= deg) masked, in the dtype of its inputs."""
    n, k = nbr.shape
    live = (torch.arange(k)[None, :] < deg[:, None]).to(a.dtype)
    z1 = a[:, None, :] + b[nbr.clamp(min=0).long()]
    m = torch.relu(torch.relu(z1) @ w2.t() + b2) * live[..., None]
    return m.sum(1) / deg.clamp(min=1).to(a.dtype)[:, None]


def _inputs(n, k, ragged, seed, hub=False):
    g = torch.Generator().manual_seed(seed)
    a = 0.5 * torch.randn(n, 128, generator=g)
    b = 0.5 * torch.randn(n, 128, generator=g)
    w2 = torch.randn(128, 128, generator=g) / math.sqrt(128)
    b2 = 0.1 * torch.randn(128, generator=g)
    nbr = torch.randint(0, n, (n, k), generator=g, dtype=torch.int32)
    if hub:
        nbr[:, 0] = 7                     # one source with n in-edges
    if ragged:
        deg = torch.randint(0, k + 1, (n,), generator=g, dtype=torch.int32)
        deg[:3] = 0                       # isolated targets: mean 0, no gradient
        if n >= 32:
            deg[16:32] = 0                # a whole 16-row tile of them
        if n > 3:
            deg[3] = k                    # and a full row
    else:
        deg = torch.full((n,), k, dtype=torch.int32)
    return dict(n=n, k=k, ragged=ragged, a=a, b=b, w2=w2, b2=b2, nbr=nbr, deg=deg, gen=g)


def _pad(c):
    """Padding entries are -1, as test_gpu_train.py writes them."""
    c["nbr"][torch.arange(c["k"])[None, :] >= c["deg"][:, None]] = -1
    return c


def _with_refs(c):
    c["ref"] = _edge_mean_ref(c["a"].double(), c["b"].double(), c["w2"].double(), c["b2"].double(),
                              c["nbr"], c["deg"])
    c["cpu32"] = _edge_mean_ref(c["a"], c["b"], c["w2"], c["b2"], c["nbr"], c["deg"]).double()
    return c


@functools.lru_cache(maxsize=None)
def _case(n, k, ragged):
    """Inputs, the float64 reference and the CPU fp32 evaluation of one shape
    (built once, shared by every test of the shape, never modified)."""
    return _with_refs(_pad(_inputs(n, k, ragged, 1000 * n + 10 * k + ragged)))


@functools.lru_cache(maxsize=None)
def _late_case(ragged):
    """n = 300, k = 40: six source rows H carry b 2^12 above the rest and are
    referenced by slot 38 of twelve target rows T only -- past the 36 slots the
    split-scale gathers load unrolled.  Ragged: half of T has deg 39 (slot 38
    live), half deg 37 (slot 38 is padding that still holds its index into H:
    the kernels must ignore it)."""
    n, k = 300, 40
    c = _inputs(n, k, ragged, 77 + ragged)
    g = c["gen"]
    rows = 32 + torch.randperm(n - 32, generator=g)[:18]      # clear of the forced-degree rows
    hot, tgt = rows[:6], rows[6:]
    cold = torch.ones(n, dtype=torch.bool)
    cold[hot] = False
    cold = torch.nonzero(cold).reshape(-1).to(torch.int32)
    c["nbr"] = cold[torch.randint(0, cold.numel(), (n, k), generator=g)]
    c["nbr"][tgt, 38] = hot[torch.randint(0, 6, (12,), generator=g)].to(torch.int32)
    c["b"][hot] *= float(2 ** 12)
    if ragged:
        c["deg"][tgt[:6]] = 39
        c["deg"][tgt[6:]] = 37
        keep = c["nbr"][tgt[6:], 38].clone()
        _pad(c)
        c["nbr"][tgt[6:], 38] = keep
    live = torch.arange(k)[None, :] < c["deg"][:, None]
    refs_hot = torch.isin(c["nbr"].long(), hot) & live
    assert int(refs_hot.sum()) == (6 if ragged else 12) and not refs_hot[:, :38].any()
    c["hot"], c["tgt"] = hot, tgt
    # the row's own magnitude m_i * ||W2||_inf, m_i = max over its live slots of |a_i + b_j|
    s = (c["a"].double()[:, None, :] + c["b"].double()[c["nbr"].clamp(min=0).long()]).abs().amax(2)
    c["mag"] = (s * live).amax(1) * c["w2"].double().abs().sum(1).max()
    return _with_refs(c)


def _forward(variant, c, dev):
    """(mean [n, 128], mask words [n k, 4] or None) of one variant on the device."""
    from mmpde_amd import _lib as L
    from mmpde_amd.gnn_2d import EdgeGraph, _edge_mean_fwd

    a, b, w2, b2 = (c[x].to(dev) for x in ("a", "b", "w2", "b2"))
    nbr = c["nbr"].to(dev)
    if variant == "mean":
        assert not c["ragged"]
        out = torch.empty((c["n"], 128), dtype=torch.float32, device=dev)
        L.check(L.lib().mmpde_gnn_edge_mean(L.ptr(a), L.ptr(b), L.ptr(nbr), c["n"], c["k"], L.ptr(w2), L.ptr(b2),
                                            L.ptr(out), L.stream(dev)), "mmpde_gnn_edge_mean")
        return out, None
    graph = EdgeGraph(nbr, c["deg"].to(dev) if c["ragged"] else None)
    mode, _, tail = variant.partition("+")
    mode, _, wave = mode.partition("-")
    keep = tail == "mask"
    assert keep or mode == "f32" or wave == "wave"
    out, mask = _edge_mean_fwd(a, b, w2, b2, graph, mode, keep_mask=keep)
    assert (mask is not None) == (keep and c["k"] <= 64)
    return out, mask


def _errs(out, ref, scale=None):
    """(max, rms) of |out - ref| (/ scale, per row)."""
    d = (out.double().cpu() - ref).abs()
    if scale is not None:
        d = d / scale[:, None]
    return (d.max().item(), d.pow(2).mean().sqrt().item()) if d.numel() else (0.0, 0.0)


_F32_OUT = {}


def _f32_out(key, c, dev):
    """The f32 variant's output of a case (the fp32 floor of the 4x rule), computed once."""
    if key not in _F32_OUT:
        _F32_OUT[key] = _forward("f32", c, dev)[0].double().cpu()
    return _F32_OUT[key]


def _runs(variant, k):
    if variant == "mean":
        return [False]
    return [False, True]


def _variant_cases():
    for v in VARIANTS:
        for (n, k) in SHAPES:
            if v.endswith("+mask") and k > 64:
                continue
            for ragged in _runs(v, k):
                yield pytest.param(v, n, k, ragged, id=f"{v}-{n}x{k}-{'ragged' if ragged else 'fixed'}")


# --------------------------------------------------------------------------- forward
@pytest.mark.parametrize("variant,n,k,ragged", list(_variant_cases()))
def test_edge_mean_forward_shapes(dev, variant, n, k, ragged):
    c = _case(n, k, ragged)
    ref = c["ref"]
    out, _ = _forward(variant, c, dev)
    again, _ = _forward(variant, c, dev)
    torch.cuda.synchronize()
    assert torch.equal(out, again)
    scale = ref.abs().max().item()
    e = _errs(out, ref)
    msg = f"{variant} n={n} k={k} {'ragged' if ragged else 'fixed'}: max|ref| {scale:.3e} max|err| {e[0]:.3e} " \
          f"rel {e[0] / max(scale, 1e-300):.2e} rms {e[1]:.3e}"
    if variant.startswith("f16x3"):
        f32 = _errs(_f32_out((n, k, ragged), c, dev), ref)
        cpu = _errs(c["cpu32"], ref)
        floor = [max(f32[i], cpu[i]) for i in (0, 1)]
        msg += f"; f32 {f32[0]:.3e} / {f32[1]:.3e} cpu-f32 {cpu[0]:.3e} / {cpu[1]:.3e}; f16x3 / fp32 " \
               f"max {e[0] / max(floor[0], 1e-300):.2f} rms {e[1] / max(floor[1], 1e-300):.2f}"
    print(msg)
    assert torch.isfinite(out).all(), msg
    assert e[0] <= 2e-5 * scale, msg
    if variant.startswith("f16x3"):
        for i in (0, 1):
            assert e[i] <= 4.0 * floor[i] + 1e-12, msg


# --------------------------------------------------------------------------- late-neighbour scale
@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
@pytest.mark.parametrize("variant", ["f16x3+mask", "f16x3-wave"])
def test_edge_mean_late_neighbour_scale(dev, variant, ragged):
    """A row whose only large neighbour sits in slot 38: a split scale taken
    from the first 36 slots alone would push relu(a + b) s past the fp16 range
    on the rows where that slot is live (inf / NaN), and a scale that counted
    the padding slot would cost the other half of T 12 bits."""
    c = _late_case(ragged)
    ref, mag, deg = c["ref"], c["mag"], c["deg"]
    outs = {"cpu-f32": c["cpu32"], "f32": _f32_out(("late", ragged), c, dev)}
    out, _ = _forward(variant, c, dev)
    again, _ = _forward(variant, c, dev)
    torch.cuda.synchronize()
    assert torch.equal(out, again)
    assert torch.isfinite(out).all()
    outs[variant] = out.double().cpu()
    empty = deg == 0
    assert not outs[variant][empty].abs().max().item() if empty.any() else True
    in_t = torch.zeros(c["n"], dtype=torch.bool)
    in_t[c["tgt"]] = True
    msg = [f"{variant} {'ragged' if ragged else 'fixed'}: row magnitude T "
           f"{mag[in_t].min().item():.3g}..{mag[in_t].max().item():.3g} others "
           f"{mag[~in_t & ~empty].min().item():.3g}..{mag[~in_t & ~empty].max().item():.3g}"]
    for name, rows in (("T", in_t), ("others", ~in_t & ~empty)):
        e = {m: _errs(o[rows], ref[rows], mag[rows]) for m, o in outs.items()}
        msg.append(f"{name} rows ({int(rows.sum())}) rel err max / rms: "
                   + ", ".join(f"{m} {e[m][0]:.3e} / {e[m][1]:.3e}" for m in e))
        for i in (0, 1):
            assert e[variant][i] <= 4.0 * max(e["f32"][i], e["cpu-f32"][i]) + 1e-12, "\n".join(msg)
    print("\n".join(msg))


# --------------------------------------------------------------------------- ReLU mask bits
@functools.lru_cache(maxsize=None)
def _z2_ref(n, k, ragged):
    """float64 z2 and the tolerance of its sign, [n, k, 128], and the live slots [n, k]."""
    c = _case(n, k, ragged)
    a, b, w2, b2 = (c[x].double() for x in ("a", "b", "w2", "b2"))
    z1 = torch.relu(a[:, None, :] + b[c["nbr"].clamp(min=0).long()])
    z2 = z1 @ w2.t() + b2
    mag = z1 @ w2.abs().t() + b2.abs()
    tol = 4 * 129 * 2.0 ** -24 * mag
    live = torch.arange(k)[None, :] < c["deg"][:, None]
    return z2, tol, live


def _mask_cases():
    for v in ("f32+mask", "f16x3+mask"):
        for (n, k) in MASK_SHAPES:
            for ragged in (False, True):
                yield pytest.param(v, n, k, ragged, id=f"{v}-{n}x{k}-{'ragged' if ragged else 'fixed'}")


@pytest.mark.parametrize("variant,n,k,ragged", list(_mask_cases()))
def test_relu_mask_bits_vs_float64(dev, variant, n, k, ragged):
    c = _case(n, k, ragged)
    z2, tol, live = _z2_ref(n, k, ragged)
    _, words = _forward(variant, c, dev)
    w = words.cpu().to(torch.int64) & 0xFFFFFFFF                   # [n k, 4]
    ch = torch.arange(128)
    bits = ((w[:, ch // 32] >> (ch % 32)) & 1).bool().reshape(n, k, 128)
    sure = (z2.abs() > tol) & live[..., None]
    wrong = sure & (bits != (z2 > 0))
    n_live = int(live.sum()) * 128
    excused = n_live - int(sure.sum())
    cap = 2 if n_live < 5000 else 1e-3 * n_live
    print(f"{variant} n={n} k={k} {'ragged' if ragged else 'fixed'}: live {n_live} wrong {int(wrong.sum())} "
          f"excused (|z2| <= tol) {excused} share {excused / max(n_live, 1):.2e}")
    if wrong.any():
        i, e, col = (int(x) for x in torch.nonzero(wrong)[0])
        raise AssertionError(f"{int(wrong.sum())} wrong bits; first at row {i} slot {e} channel {col}: "
                             f"z2 {z2[i, e, col].item():.3e} tol {tol[i, e, col].item():.3e}")
    assert excused <= cap, (excused, cap)


# --------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=None)
def _bwd_case(n, k, ragged, hub=False):
    """Inputs, gout and the float64 autograd gradients (shared by both edge_gemm modes)."""
    c = _pad(_inputs(n, k, ragged, 500000 + 1000 * n + 10 * k + 2 * ragged + hub, hub=hub))
    c["gout"] = torch.randn(n, 128, generator=c["gen"])
    ref_in = [c[x].double().requires_grad_() for x in ("a", "b", "w2", "b2")]
    ref = _edge_mean_ref(*ref_in, c["nbr"], c["deg"])
    (ref * c["gout"].double()).sum().backward()
    c["ref"] = ref.detach()
    c["grads"] = [t.grad for t in ref_in]
    return c


def _bwd_cases():
    for gemm in ("f32", "f16x3"):
        for (n, k) in BWD_SHAPES:
            for ragged in (False, True):
                yield pytest.param(gemm, n, k, ragged, False, id=f"{gemm}-{n}x{k}-{'ragged' if ragged else 'fixed'}")
        for ragged in (False, True):
            yield pytest.param(gemm, 203, 9, ragged, True, id=f"{gemm}-hub-203x9-{'ragged' if ragged else 'fixed'}")


@pytest.mark.parametrize("edge_gemm,n,k,ragged,hub", list(_bwd_cases()))
def test_edge_mean_backward_shapes(dev, edge_gemm, n, k, ragged, hub):
    from mmpde_amd.gnn_2d import EdgeGraph, EdgeMean, _edge_mean_fwd

    c = _bwd_case(n, k, ragged, hub)
    graph = EdgeGraph(c["nbr"].to(dev), c["deg"].to(dev) if ragged else None)
    got_in = [c[x].to(dev).requires_grad_() for x in ("a", "b", "w2", "b2")]
    gout = c["gout"].to(dev)
    if k > 64:
        # no ReLU mask past 64 slots: the f16x3 forward then runs the wave kernel
        # and the f16x3 backward the F32 kernel, which recomputes z2
        assert _edge_mean_fwd(*(t.detach() for t in got_in), graph, edge_gemm)[1] is None
    out = EdgeMean.apply(*got_in, graph, edge_gemm)
    (out * gout).sum().backward()
    torch.cuda.synchronize()
    tag = f"{edge_gemm} n={n} k={k} {'ragged' if ragged else 'fixed'}{' hub' if hub else ''}"
    checks = [("mean", out, c["ref"])] + [(f"d/d{name}", t.grad, r)
                                          for name, t, r in zip(("a", "b", "W2", "b2"), got_in, c["grads"])]
    msg = []
    for what, got, ref in checks:
        err = (got.detach().double().cpu() - ref).abs().max().item()
        scale = ref.abs().max().item()
        msg.append(f"{tag} {what}: max|err| {err:.3e} max|ref| {scale:.3e} rel {err / max(scale, 1e-300):.2e}")
    print("\n".join(msg))
    for (what, got, ref), line in zip(checks, msg):
        assert torch.isfinite(got).all(), line
        assert (got.detach().double().cpu() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item(), line
    # deterministic: a second backward gives the same bits
    grads = [t.grad.clone() for t in got_in]
    for t in got_in:
        t.grad = None
    EdgeMean.apply(*got_in, graph, edge_gemm).mul(gout).sum().backward()
    for t, g0 in zip(got_in, grads):
        assert torch.equal(t.grad, g0)
