"""The train-mode array branch's entry points (mmpde_dmm_convnet_train_*) are
declared, exported and bound, size their workspace by the number of fields
alone, refuse bad arguments before any launch, and carry one resolution limit
in the header, _lib and ops; the model's switch is off by default and not part
of the state dict (no GPU needed)."""
import ctypes
import os
import re

from conftest import ROOT

NEW = ("mmpde_dmm_convnet_train_workspace_bytes", "mmpde_dmm_convnet_train_forward",
       "mmpde_dmm_convnet_train_backward")
INVALID, UNSUPPORTED = -1, -2


def _header():
    src = open(os.path.join(ROOT, "include", "mmpde_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_symbols_declared_exported_and_bound():
    from mmpde_amd import _lib

    src, code = _header()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert hasattr(h, name), name
        assert name in _lib.EXPORTS, name
    assert "mmpde_dmm_convnet_weights" in code
    assert "mesh/dmm_model.py:48-81" in src[src.index("The array branch of DMM in train() mode"):][:600]
    assert re.search(r"#define\s+MMPDE_DMM_CONVNET_TRAIN_GRADS\s+6833\b", code) and _lib.DMM_CONVNET_TRAIN_GRADS == 6833
    assert 6833 == 8 * 25 + 8 + 16 * 8 * 25 + 16 + 8 * 16 * 25 + 8 + 8 * 25 + 1
    assert ctypes.sizeof(_lib.DmmConvnetWeights) == 8 * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.ABI_VERSION == 12302 and _lib.lib().mmpde_version() == 12302      # added without a version step
    mk = open(os.path.join(ROOT, "mm-pde_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bdmm_convnet_train\.hip\b", mk, flags=re.M)


def test_one_limit_in_header_lib_and_ops():
    from mmpde_amd import _lib, ops

    _, code = _header()
    m = re.search(r"#define\s+MMPDE_DMM_CONVNET_TRAIN_MAX_S\s+(\d+)\b", code)
    assert m
    limit = int(m.group(1))
    assert limit == _lib.DMM_CONVNET_TRAIN_MAX_S == ops.CONVNET_TRAIN_MAX_S and limit >= 48
    import dmm_convnet_train_cases as C

    assert C.MAX_S == limit and (limit, 2) in C.CASES
    assert ops.convnet_out_sizes(48) == (24, 12) and ops.convnet_out_sizes(1) == (1, 1)
    assert [ops.convnet_out_sizes(s) for s in (5, 6, 7, 8, 9)] == [(3, 2), (3, 2), (4, 2), (4, 2), (5, 3)]


def test_workspace_grows_with_the_fields_and_not_otherwise():
    from mmpde_amd import _lib

    ws = _lib.lib().mmpde_dmm_convnet_train_workspace_bytes
    one = ws(1)
    print(f"workspace per field {one} bytes (6833 gradient sums)")
    assert one % 16 == 0 and 4 * 6833 <= one <= 4 * 6833 + 16
    for B in (2, 3, 65, 160, 4096):
        assert ws(B) == B * one, B
    for bad in (0, -1, (1 << 24) + 1):
        assert ws(bad) == 0, bad
    assert ws(1 << 24) == (1 << 24) * one


def test_refusals_before_launch():
    from mmpde_amd import _lib

    lib = _lib.lib()
    p = ctypes.c_void_p(16)     # non-null, 16-B aligned, never dereferenced before the refusal
    w = _lib.DmmConvnetWeights(*([16] * 8))
    fwd, bwd = lib.mmpde_dmm_convnet_train_forward, lib.mmpde_dmm_convnet_train_backward
    limit = _lib.DMM_CONVNET_TRAIN_MAX_S
    need = lib.mmpde_dmm_convnet_train_workspace_bytes(2)

    def f(u=p, B=2, s=48, wp=w, out=p):
        return fwd(u, B, s, ctypes.byref(wp) if wp is not None else None, out, None)

    def b(u=p, B=2, s=48, wp=w, df=p, gr=p, ws=p, nb=need):
        return bwd(u, B, s, ctypes.byref(wp) if wp is not None else None, df, gr, ws, nb, None)

    for name in ("u", "wp", "out"):
        assert f(**{name: None}) == INVALID, name
    for name in ("u", "wp", "df", "gr", "ws"):
        assert b(**{name: None}) == INVALID, name
    names = [n for n, _ in _lib.DmmConvnetWeights._fields_]
    for hole in names:          # every tensor of the stack is required
        part = _lib.DmmConvnetWeights(**{n: (None if n == hole else 16) for n in names})
        assert f(wp=part) == INVALID and b(wp=part) == INVALID, hole
    for call in (f, b):
        assert call(B=0) == INVALID and call(B=-3) == INVALID
        assert call(s=0) == INVALID and call(s=-1) == INVALID
        assert call(u=ctypes.c_void_p(18)) == INVALID             # misaligned floats
        assert call(s=limit + 1) == UNSUPPORTED and call(s=4096) == UNSUPPORTED
        assert call(B=(1 << 24) + 1) == UNSUPPORTED
    assert b(nb=need - 1) == INVALID and b(nb=0) == INVALID       # a short workspace
    assert b(nb=lib.mmpde_dmm_convnet_train_workspace_bytes(1)) == INVALID
    assert b(ws=ctypes.c_void_p(24)) == INVALID                   # workspace rows are 16-B aligned


def test_switch_is_off_by_default_and_not_in_the_state_dict():
    import inspect

    import torch

    from mmpde_amd import DMM, dmm_train, ops

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        dmm = DMM(s=9, mode="array", branch_layer=7, trunk_layer=[2, 3, 8], out_layer=[16, 128, 1])
    assert dmm.hip_branch_train is False
    assert not any("hip_branch" in k for k in dmm.state_dict())
    assert "hip_branch_train" not in dict(dmm.named_parameters()) and "hip_branch_train" not in dict(dmm.named_buffers())
    assert inspect.signature(dmm_train.train_MA_res).parameters["hip_branch"].default is False
    assert issubclass(ops.ConvNetTrain, torch.autograd.Function)
    assert callable(dmm.branch.forward_train_hip)
