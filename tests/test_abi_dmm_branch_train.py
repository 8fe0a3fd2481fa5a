"""The train-mode graph branch's entry points (mmpde_dmm_gnn_train_* and
mmpde_dmm_decode_train_*) are declared, exported and bound, size their
workspaces by host arithmetic -- rows per node and per workgroup, and the one
4-floats-per-edge buffer -- and refuse bad arguments before any launch; the
model's switch is off by default and not part of the state dict (no GPU needed)."""
import ctypes
import os
import re

from conftest import ROOT

NEW = ("mmpde_dmm_gnn_train_workspace_bytes", "mmpde_dmm_gnn_train_forward", "mmpde_dmm_gnn_train_backward",
       "mmpde_dmm_decode_train_workspace_bytes", "mmpde_dmm_decode_train_forward",
       "mmpde_dmm_decode_train_backward")
INVALID, UNSUPPORTED = -1, -2


def test_symbols_declared_exported_and_bound():
    from mmpde_amd import _lib

    src = open(os.path.join(ROOT, "include", "mmpde_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert hasattr(h, name), name
        assert name in _lib.EXPORTS, name
    assert "mmpde_dmm_gnn_weights" in code
    assert re.search(r"#define\s+MMPDE_DMM_GNN_TRAIN_GRADS\s+124\b", code) and _lib.DMM_GNN_TRAIN_GRADS == 124
    assert re.search(r"#define\s+MMPDE_DMM_DECODE_TRAIN_GRADS\s+769\b", code) and _lib.DMM_DECODE_TRAIN_GRADS == 769
    assert ctypes.sizeof(_lib.DmmGnnWeights) == 8 * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.ABI_VERSION == 12302 and _lib.lib().mmpde_version() == 12302      # added without a version step
    mk = open(os.path.join(ROOT, "mm-pde_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bdmm_branch_train\.hip\b", mk, flags=re.M)


def test_workspaces_grow_with_nodes_and_workgroups_only():
    from mmpde_amd import _lib

    lib = _lib.lib()
    ws = lib.mmpde_dmm_gnn_train_workspace_bytes
    # the reference's Adam shape: 160 trajectories of the 2521-node cylinder grid, kNN-35
    B, n, k = 160, 2521, 35
    nb = ws(B, n, k)
    edge = 16 * B * n * k                      # 4 floats per edge, once
    rows = nb - edge
    print(f"layer workspace {nb} bytes: {edge} per edge, {rows} in rows")
    assert nb % 16 == 0 and 0 < rows <= 16 * B * n + 4 * 124 * B * ((n + 127) // 128) + 16
    # doubling k changes nothing but the per-edge buffer
    assert ws(B, n, 2 * k) - nb == edge
    # rows per node and per workgroup: linear in B, and in n up to the workgroup rounding
    assert ws(2 * B, n, k) == 2 * nb or abs(ws(2 * B, n, k) - 2 * nb) <= 16
    assert ws(B, 2 * n, k) - 2 * nb <= 4 * 124 * B + 16
    for bad in ((0, n, k), (B, 0, k), (B, n, 0), (-1, n, k)):
        assert ws(*bad) == 0, bad
    dec = lib.mmpde_dmm_decode_train_workspace_bytes
    nd = dec(B * n)
    print(f"decoder workspace {nd} bytes; one [n, 128] fp32 table {B * n * 128 * 4}")
    assert nd % 16 == 0 and 0 < nd <= B * n * 4 + 4096        # under one float per node
    assert dec(0) == 0 and dec(-5) == 0 and dec(1) == dec(1024) < dec(1025)


def test_layer_refusals_before_launch():
    from mmpde_amd import _lib

    lib = _lib.lib()
    p = ctypes.c_void_p(16)     # non-null, 16-B aligned, never dereferenced before the refusal
    w = _lib.DmmGnnWeights(*([16] * 8))
    fwd, bwd = lib.mmpde_dmm_gnn_train_forward, lib.mmpde_dmm_gnn_train_backward

    def f(h=p, u=p, grid=p, B=2, n=10, nbr=p, k=3, hidden=4, wp=w, upd=p):
        return fwd(h, u, grid, B, n, nbr, k, hidden, ctypes.byref(wp) if wp is not None else None, upd, None)

    def b(h=p, u=p, grid=p, B=2, n=10, nbr=p, k=3, hidden=4, ro=p, re_=p, wp=w, du=p, dh=p, gr=p, ws=p):
        return bwd(h, u, grid, B, n, nbr, k, hidden, ro, re_, ctypes.byref(wp) if wp is not None else None, du, dh,
                   gr, ws, None)

    for name in ("h", "u", "grid", "nbr", "wp", "upd"):
        assert f(**{name: None}) == INVALID, name
    for name in ("h", "u", "grid", "nbr", "ro", "re_", "wp", "du", "dh", "gr", "ws"):
        assert b(**{name: None}) == INVALID, name
    names = [n for n, _ in _lib.DmmGnnWeights._fields_]
    for hole in names:          # every tensor of the layer is required
        part = _lib.DmmGnnWeights(**{n: (None if n == hole else 16) for n in names})
        assert f(wp=part) == INVALID and b(wp=part) == INVALID, hole
    for call in (f, b):
        assert call(B=0) == INVALID and call(n=0) == INVALID
        assert call(h=ctypes.c_void_p(24)) == INVALID           # misaligned rows (16 B)
        assert call(hidden=8) == UNSUPPORTED and call(hidden=3) == UNSUPPORTED
        assert call(k=0) == UNSUPPORTED and call(k=-1) == UNSUPPORTED
        assert call(B=65536) == UNSUPPORTED
    assert b(ws=ctypes.c_void_p(24)) == INVALID


def test_decoder_refusals_before_launch():
    from mmpde_amd import _lib

    lib = _lib.lib()
    p = ctypes.c_void_p(16)
    fwd, bwd = lib.mmpde_dmm_decode_train_forward, lib.mmpde_dmm_decode_train_backward
    for hole in range(6):       # h, w0, b0, w1, b1, out
        a = [p] * 6
        a[hole] = None
        assert fwd(a[0], 10, 4, a[1], a[2], a[3], a[4], a[5], None) == INVALID, hole
    for hole in range(8):       # h, w0, b0, w1, d_out, d_h, grads, workspace
        a = [p] * 8
        a[hole] = None
        assert bwd(a[0], 10, 4, a[1], a[2], a[3], a[4], a[5], a[6], a[7], None) == INVALID, hole
    assert fwd(p, 0, 4, p, p, p, p, p, None) == INVALID
    assert bwd(p, 0, 4, p, p, p, p, p, p, p, None) == INVALID
    assert fwd(ctypes.c_void_p(24), 10, 4, p, p, p, p, p, None) == INVALID
    assert fwd(p, 10, 8, p, p, p, p, p, None) == UNSUPPORTED
    assert bwd(p, 10, 8, p, p, p, p, p, p, p, None) == UNSUPPORTED


def test_switch_is_off_by_default_and_not_in_the_state_dict():
    import inspect

    import torch

    from mmpde_amd import DMM, dmm_train, ops

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        dmm = DMM(mode="graph", grid=torch.rand(9, 2), branch_layer=[4, 1], trunk_layer=[2, 3, 8],
                  out_layer=[16, 128, 1])
    assert dmm.hip_branch_train is False
    assert not any("hip_branch" in k for k in dmm.state_dict())
    assert "hip_branch_train" not in dict(dmm.named_parameters()) and "hip_branch_train" not in dict(dmm.named_buffers())
    assert inspect.signature(dmm_train.train_MA_res).parameters["hip_branch"].default is False
    assert inspect.signature(dmm._branch_train).parameters["nbr"].default is None
    assert issubclass(ops.DmmGnnLayerTrain, torch.autograd.Function)
    assert issubclass(ops.DmmDecodeTrain, torch.autograd.Function)
