"""The cases of itp_net_cases.py on the CPU: every case is usable (max|ref| and
the one-wrong-unit shift, in float64), torch fp32 against float64, and the host
side of the mmpde_itp_net entries (sizing and refusals, no GPU needed).

torch fp32 on the CPU against float64, as a fraction of max|ref|, over the 96
cases: 3.4e-9 .. 1.0e-6, at most 0.045 bar (the 256^4 net: 9.0e-8 .. 1.0e-6);
the smallest drop-one-unit shift is 63 bars.
The assertion is a tenth of the bar: 2e-6 max|ref| is about 34 fp32 roundings of
max|ref|, and the evaluation is at most five chained dot products of at most
256 terms whose roundings add in quadrature (16 roundings of a term's size
each, passed on through tanh' <= 1 and weight rows of norm below 1).
"""
import ctypes

import pytest
import torch

import itp_net_cases as C

INVALID = -1   # MMPDE_ERR_INVALID_ARG
CASES = C.all_cases()
IDS = [C.case_id(*k) for k in CASES]


def test_case_lists_are_the_issue_s():
    assert [list(h) for h in C.HIDDEN] == [[], [1], [16], [17], [64, 32], [96, 40], [128, 64], [255, 33],
                                           [256, 256], [32, 48, 16], [40, 24, 56, 8], [256, 256, 256, 256]]
    assert C.SHAPES == ((1, 30, 1), (1, 30, 17), (3, 45, 33), (2, 37, 100))
    assert set(C.INPUT_SEED) <= set(CASES)


@pytest.mark.parametrize("hidden,shape,mode", CASES, ids=IDS)
def test_case_is_usable_and_fp32_is_inside_the_bar(hidden, shape, mode):
    c = C.case(hidden, shape, mode)
    scale, bars = C.usable(c, c["wb"])
    assert scale == c["ref"].abs().max().item()
    floor = (c["cpu32"] - c["ref"]).abs().max().item()
    print(f"{C.case_id(hidden, shape, mode)}: max|ref| {scale:.3e}, drop-one-unit shift "
          f"{'-' if bars is None else format(bars, '.1f')} bars, torch fp32 {floor:.3e} "
          f"({floor / scale:.2e} of max|ref|, {floor / C.bar(scale):.4f} bar)")
    assert scale >= C.MIN_SCALE
    assert (bars is None) == (len(hidden) == 0)
    if bars is not None:
        assert bars >= C.MUTATION_BARS
    assert floor <= 0.1 * C.bar(scale)
    assert [tuple(w.shape) for w, _ in c["wb"]] == list(zip(list(hidden) + [30], [62] + list(hidden)))


def test_modes_are_two_nets():
    for hidden in ((), (17,), (256, 256, 256, 256)):
        w1, w2 = C.weights(hidden, "1"), C.weights(hidden, "2")
        assert not torch.equal(w1[0][0], w2[0][0])


# ---------------------------------------------------------------- host entries
def _net(widths, n_layers=None):
    from mmpde_amd import _lib as L

    net = L.ItpNetShape(n_layers=len(widths) - 1 if n_layers is None else n_layers)
    for i, w in enumerate(widths[:L.ITP_MAX_LAYERS + 1]):
        net.widths[i] = w
    return net


def _pad(w):
    return -(-w // 16) * 16


BAD = [([62, 30], 0), ([62, 30], 6), ([62, 30], -1), ([62, 8, 8, 8, 8, 8, 30], 6),
       ([61, 30], None), ([64, 16, 30], None), ([62, 31], None), ([62, 16, 32], None),
       ([62, 0, 30], None), ([62, -4, 30], None), ([62, 257, 30], None), ([62, 16, 300, 30], None),
       ([62, 8, 8, 8, 1000, 30], None)]


def test_abi_version():
    from mmpde_amd import _lib

    assert _lib.ABI_VERSION == 12302 and _lib.lib().mmpde_version() == 12302
    assert (_lib.ITP_MAX_LAYERS, _lib.ITP_MAX_WIDTH) == (5, 256)


def test_pack_bytes_without_gpu():
    from mmpde_amd import _lib as L

    lib = L.lib()
    assert lib.mmpde_itp_net_pack_bytes(None) == 0
    for widths, n in BAD:
        assert lib.mmpde_itp_net_pack_bytes(ctypes.byref(_net(widths, n))) == 0, (widths, n)
    for hidden in C.HIDDEN:
        widths = [62] + list(hidden) + [30]
        want = 4 * sum(_pad(o) * (_pad(i) + 1) for i, o in zip(widths[:-1], widths[1:]))
        assert lib.mmpde_itp_net_pack_bytes(ctypes.byref(_net(widths))) == want > 0, hidden
    # monotone in the padded widths: the same inside a 16-unit step, larger across it
    sizes = [lib.mmpde_itp_net_pack_bytes(ctypes.byref(_net([62, w, 40, 30]))) for w in range(1, 257)]
    for w in range(2, 257):
        a, b = sizes[w - 2], sizes[w - 1]
        assert (b == a) if _pad(w) == _pad(w - 1) else (b > a), w
    # the default widths: the specialised image's size (the same padding, 62 -> 64 and 30 -> 32)
    assert lib.mmpde_itp_net_pack_bytes(ctypes.byref(_net([62, 128, 64, 30]))) == lib.mmpde_itp_pack_bytes()


def test_refusals_without_gpu():
    """Every refusal of mmpde_hip.h, with dummy non-null pointers (never read: the
    entries return before any launch)."""
    from mmpde_amd import _lib as L

    lib = L.lib()
    raw = ctypes.create_string_buffer(4096 + 64)
    p = (ctypes.addressof(raw) + 63) & ~63           # 64-byte aligned host address
    good = _net([62, 17, 30])
    nbytes = lib.mmpde_itp_net_pack_bytes(ctypes.byref(good))
    assert nbytes > 0

    def interp(src=p, vals=p, qry=p, idx=p, B=1, ns=30, nq=1, shape=good, packed=p, pb=nbytes, out=p):
        sh = ctypes.byref(shape) if shape is not None else None
        return lib.mmpde_itp_interp_net(src, vals, qry, idx, B, ns, nq, sh, packed, pb, None, None, out, None)

    for name in ("src", "vals", "qry", "idx", "shape", "packed", "out"):
        assert interp(**{name: None}) == INVALID, name
    for widths, n in BAD:
        assert interp(shape=_net(widths, n), pb=1 << 30) == INVALID, (widths, n)
    assert interp(packed=p + 4) == INVALID and interp(packed=p + 8) == INVALID
    assert interp(pb=nbytes - 1) == INVALID and interp(pb=0) == INVALID
    # an image built for a smaller shape is never read with a larger one
    assert interp(shape=_net([62, 33, 30]), pb=nbytes) == INVALID
    assert interp(B=0) == INVALID and interp(B=-1) == INVALID
    assert interp(ns=29) == INVALID and interp(nq=0) == INVALID

    def pack(net=good, packed=p, pb=nbytes, ptrs=True):
        if net is not None and ptrs:
            for i in range(max(0, min(net.n_layers, L.ITP_MAX_LAYERS))):
                net.w[i] = net.b[i] = p
        return lib.mmpde_itp_net_pack(ctypes.byref(net) if net is not None else None, packed, pb, None)

    assert pack(net=None) == INVALID and pack(packed=None) == INVALID
    for widths, n in BAD:
        assert pack(net=_net(widths, n), pb=1 << 30) == INVALID, (widths, n)
    assert pack(packed=p + 4) == INVALID and pack(pb=nbytes - 1) == INVALID
    assert pack(net=_net([62, 17, 30]), ptrs=False) == INVALID      # null w / b of a used layer
