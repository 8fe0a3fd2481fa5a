"""The stages of the fused eval forward (mmpde_gnn_forward_ex: gnn_embed_kernel,
the edge stage, gnn_node_kernel<NEXT | HEAD> and the fused head, layer.hip)
against the float64 oracle at the shapes of gnn_stage_cases.py, in both
edge_gemm modes: rows around the 32-row tile, time windows 1, 2, 3, 16, depths
0 .. 3, a different t in every row, ragged tables with degree-0 rows, 1/Lx,
1/Ly, 1/tmax other than 1, and trajectory segments.

Compared per case: the last layer's node features (exec.h_last), every row
relative to its own float64 magnitude (max and rms over the rows), and `out`
[n, tw] relative to max|out64|.  Bars: 4 x the float32 CPU oracle's error over
the case table (gnn_stage_cases.FP32_FLOOR_H / _OUT, measured on the CPU; the
4 x rule of test_gpu_precision.py).  Both buffers are longer than the kernels
may write: rows [n, n + 32) of h_last and 64 floats after out hold a sentinel
that must come back bit for bit, the rows before it start as NaN and must come
back finite.

Further: the (x, y) + t and (x, y) + t_slot position forms against the
three-column form, bit for bit, on h_last and out; the forward with no layer
(embed0 + GEMM, then mmpde_gnn_head) against the oracle's hidden_layer = 0;
mmpde_gnn_embed through the C ABI against the oracle's embedding rows.
"""
import copy
import ctypes
import functools

import pytest
import torch

import gnn_stage_cases as C

pytestmark = pytest.mark.gpu

MODES = ("f32", "f16x3")
PAD_ROWS = 32
PAD_OUT = 64
SENTINEL = 12345.675


@functools.lru_cache(maxsize=None)
def _model(tw, depth, scales, dev):
    return copy.deepcopy(C.solver(tw, depth, *scales)).to(dev)


def _data(c, dev, const_t=False, form="txy"):
    from mmpde_amd.graph import Data

    d = C.graph(c, const_t)
    data = Data(x=d.u.to(dev))
    data.nbr = d.nbr.to(dev)
    if d.deg is not None:
        data.deg = d.deg.to(dev)
    if d.seg_n:
        data.seg_n = d.seg_n
    if form == "txy":
        data.pos = d.pos.to(dev)
        return data
    assert const_t
    data.pos = d.pos[:, 1:].contiguous().to(dev)
    if form == "xy+t":
        data.t = float(d.pos[0, 0])
    else:
        data.t_slot = d.pos[0, :1].clone().to(dev)
    return data


def _guarded(rows, width, pad, dev):
    """A [rows * width + pad] buffer, NaN then SENTINEL, and a copy of its bits."""
    buf = torch.full((rows * width + pad,), float("nan"), dtype=torch.float32, device=dev)
    buf[rows * width:] = SENTINEL
    return buf, buf.view(torch.int32).clone()


def _check_guard(buf, bits, live, what):
    """The first `live` floats finite, everything after them bit-unchanged."""
    assert torch.isfinite(buf[:live]).all(), f"{what}: rows the kernel did not store"
    assert torch.equal(buf.view(torch.int32)[live:], bits[live:]), f"{what}: stored past its last row"


def _forward(c, mode, dev, data=None):
    """(h_last [n, 128] or None without layers, out [n, tw]) of one guarded
    forward through mmpde_gnn_forward_ex."""
    from mmpde_amd import _lib as L

    model = _model(c.tw, c.depth, c.scales, dev)
    data = _data(c, dev) if data is None else data
    n = c.n
    hbuf, hbits = _guarded(n, 128, PAD_ROWS * 128, dev)
    obuf, obits = _guarded(n, c.tw, PAD_OUT, dev)
    out = obuf[:n * c.tw].view(n, c.tw)
    trace = L.GnnExec(None, None, 0, None)
    trace.h_last = L.ptr(hbuf)
    if c.depth:
        model.edge_gemm = mode
        got = model(data, out=out, trace=trace)
        model.edge_gemm = "f32"
        assert got.data_ptr() == obuf.data_ptr()
    else:
        # no layer: nothing to pack for f16x3, so the module's own forward cannot ask
        # for that mode; the C entry point takes it (and runs the same fp32 kernels)
        call, _, keep = model._call(data, out, None, trace)
        trace.edge_gemm = L.EDGE_GEMM[mode]
        L.check(L.lib().mmpde_gnn_forward_ex(call.u, call.pos, call.n, call.k, call.nbr, call.sc, call.emb,
                                             call.layers, call.n_layers, call.head, call.workspace, call.out,
                                             call.exec, L.stream(dev)), "mmpde_gnn_forward_ex")
        del keep
    torch.cuda.synchronize()
    _check_guard(obuf, obits, n * c.tw, "out")
    if not c.depth:
        # no node kernel ran: h_last is not written at all
        assert torch.equal(hbuf.view(torch.int32), hbits)
        return None, out
    _check_guard(hbuf, hbits, n * 128, "h_last")
    return hbuf[:n * 128].view(n, 128), out


def _params():
    return [pytest.param(c, mode, id=f"{C.case_id(c)}-{mode}") for c in C.CASES for mode in MODES]


@pytest.mark.parametrize("c,mode", _params())
def test_forward_stages_vs_float64(dev, c, mode):
    out64, hs64 = C.reference(c)
    h, out = _forward(c, mode, dev)
    assert out.shape == (c.n, c.tw)
    e_out = C.out_rel_err(out, out64)
    e_h = C.row_rel_err(h, hs64[c.depth]) if h is not None else (0.0, 0.0)
    print(f"{C.case_id(c)} {mode}: h_last row-relative max {e_h[0]:.3e} rms {e_h[1]:.3e} "
          f"({e_h[0] / C.FP32_FLOOR_H:.2f} / {e_h[1] / C.FP32_FLOOR_H:.2f} floors), out {e_out:.3e} of max|out64| "
          f"({e_out / C.FP32_FLOOR_OUT:.2f} floors)")
    assert e_h[0] <= C.FACTOR * C.FP32_FLOOR_H
    assert e_h[1] <= C.FACTOR * C.FP32_FLOOR_H
    assert e_out <= C.FACTOR * C.FP32_FLOOR_OUT


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", C.CONST_T, ids=[C.case_id(c) for c in C.CONST_T])
def test_position_forms_bit_for_bit(dev, c, mode):
    h3, out3 = _forward(c, mode, dev, _data(c, dev, True))
    for form in ("xy+t", "xy+t_slot"):
        h, out = _forward(c, mode, dev, _data(c, dev, True, form))
        assert torch.equal(h, h3), form
        assert torch.equal(out, out3), form
    # and the per-row t of the case proper gives other values: t is read at all
    h, _ = _forward(c, mode, dev)
    assert not torch.equal(h, h3)


EMBED_CASES = C.DEPTH0 + [c for c in C.NONUNIT if c.tw == 1]


@pytest.mark.parametrize("c", EMBED_CASES, ids=[C.case_id(c) for c in EMBED_CASES])
def test_gnn_embed_entry_point_vs_float64(dev, c):
    """mmpde_gnn_embed (embed0_kernel + the 128 x 128 GEMM; tw = 1) through the
    C ABI against the oracle's embedding rows."""
    from mmpde_amd import _lib as L

    model = _model(c.tw, c.depth, c.scales, dev)
    sc, emb, _, _ = model.device_params()
    d = C.graph(c)
    u, pos = d.u.reshape(-1).to(dev), d.pos.to(dev)
    n = c.n
    lib = L.lib()
    ws = torch.empty((lib.mmpde_gnn_workspace_bytes(n) // 4,), dtype=torch.float32, device=dev)
    hbuf, hbits = _guarded(n, 128, PAD_ROWS * 128, dev)
    L.check(lib.mmpde_gnn_embed(L.ptr(u), L.ptr(pos), n, sc, ctypes.addressof(emb), L.ptr(ws), L.ptr(hbuf),
                                L.stream(dev)), "mmpde_gnn_embed")
    torch.cuda.synchronize()
    _check_guard(hbuf, hbits, n * 128, "h0")
    e = C.row_rel_err(hbuf[:n * 128].view(n, 128), C.reference(c)[1][0])
    print(f"{C.case_id(c)} mmpde_gnn_embed: h0 row-relative max {e[0]:.3e} rms {e[1]:.3e} "
          f"({e[0] / C.FP32_FLOOR_H:.2f} / {e[1] / C.FP32_FLOOR_H:.2f} floors)")
    assert e[0] <= C.FACTOR * C.FP32_FLOOR_H
    assert e[1] <= C.FACTOR * C.FP32_FLOOR_H
