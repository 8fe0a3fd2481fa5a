"""The training jet's entry points (mmpde_dmm_jet, mmpde_dmm_jet_grad and
mmpde_dmm_jet_workspace_bytes) are declared, exported and bound, size their
workspace by host arithmetic -- below one [n, L'] table at the reference's Adam
shape -- and refuse bad arguments before any launch (no GPU needed)."""
import ctypes
import os
import re

from conftest import ROOT

NEW = ("mmpde_dmm_jet_workspace_bytes", "mmpde_dmm_jet", "mmpde_dmm_jet_grad")
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
    for struct in ("mmpde_dmm_jet_out", "mmpde_dmm_jet_cot", "mmpde_dmm_jet_grads"):
        assert struct in code, struct
    # added without a version step
    assert _lib.ABI_VERSION == 12302 and _lib.lib().mmpde_version() == 12302
    assert [n for n, _ in _lib.DmmJetOut._fields_] == ["phi", "phi_x", "phi_y", "phi_xx", "phi_xy", "phi_yy"]
    assert ctypes.sizeof(_lib.DmmJetOut) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.DmmJetGrads) == 9 * ctypes.sizeof(ctypes.c_void_p)
    mk = open(os.path.join(ROOT, "mm-pde_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bdmm_jet\.hip\b", mk, flags=re.M)


def test_workspace_is_below_one_table_at_the_adam_shape():
    from mmpde_amd import _lib

    lib = _lib.lib()
    # --batch_size_x_adam 120 x --batch_size_u_adam 160, head (32, 512, 512)
    B, n, th, L, Lp = 160, 19200, 32, 512, 512
    nb = lib.mmpde_dmm_jet_workspace_bytes(B, n, L, Lp, th)
    print(f"workspace {nb} bytes; one [n, L'] fp32 table {n * Lp * 4}")
    assert 0 < nb < n * Lp * 4 and nb % 16 == 0
    # it holds at least P [L', th] and c_b [B, L'], which both calls use
    for b, ng, lat, lp, t in ((1, 1, 8, 128, 1), (3, 195, 64, 1024, 7), (3, 2100, 512, 512, 16), (B, n, L, Lp, th)):
        got = lib.mmpde_dmm_jet_workspace_bytes(b, ng, lat, lp, t)
        assert got >= (lp * t + b * lp) * 4 and got % 16 == 0, (b, ng, lat, lp, t)
    # the boundary sides of the same draw (30 rows per field) stay below the interior's
    assert lib.mmpde_dmm_jet_workspace_bytes(B, B * 30, L, Lp, th) <= nb
    for bad in ((0, 10, 8, 128, 1), (2, 0, 8, 128, 1), (2, 10, 0, 128, 1), (2, 10, 8, 0, 1), (2, 10, 8, 128, 0),
                (2, 10, 8, 128, 65), (3, 10, 8, 128, 1)):
        assert lib.mmpde_dmm_jet_workspace_bytes(*bad) == 0, bad


def test_jet_refusals_before_launch():
    from mmpde_amd import _lib

    lib = _lib.lib()
    ok = _lib.DmmHead(None, None, None, None, 16, 512, None, None, None, 512)
    out = _lib.DmmJetOut()
    p = ctypes.c_void_p(16)     # non-null, 16-B aligned, never dereferenced before the refusal
    call = lib.mmpde_dmm_jet
    assert call(None, 2, None, 10, None, None, None, None, None) == INVALID
    for hole in range(5):       # each mandatory pointer in turn (o1_b is nullable)
        a = [p, p, ctypes.byref(ok), p, ctypes.byref(out)]
        a[hole] = None
        assert call(a[0], 2, a[1], 10, a[2], None, a[3], a[4], None) == INVALID, hole
    good = (ctypes.byref(ok), None, p, ctypes.byref(out), None)
    assert call(p, 3, p, 10, *good) == INVALID      # n_grid % B
    assert call(p, 0, p, 10, *good) == INVALID
    assert call(p, 2, p, 0, *good) == INVALID
    # misaligned: workspace (16 B), grid (8 B), branch, the bias and an output (4 B)
    assert call(p, 2, p, 10, ctypes.byref(ok), None, ctypes.c_void_p(24), ctypes.byref(out), None) == INVALID
    assert call(p, 2, ctypes.c_void_p(20), 10, *good) == INVALID
    assert call(ctypes.c_void_p(18), 2, p, 10, *good) == INVALID
    assert call(p, 2, p, 10, ctypes.byref(ok), ctypes.c_void_p(18), p, ctypes.byref(out), None) == INVALID
    bad = _lib.DmmJetOut(None, None, 18, None, None, None)
    assert call(p, 2, p, 10, ctypes.byref(ok), None, p, ctypes.byref(bad), None) == INVALID
    # the heads mmpde_dmm_phi does not take
    for hd in (_lib.DmmHead(None, None, None, None, 16, 512, None, None, None, 100),
               _lib.DmmHead(None, None, None, None, 65, 512, None, None, None, 512),
               _lib.DmmHead(None, None, None, None, 16, 12, None, None, None, 512)):
        assert call(p, 2, p, 10, ctypes.byref(hd), None, p, ctypes.byref(out), None) == UNSUPPORTED
        assert lib.mmpde_dmm_phi(p, 2, p, 10, ctypes.byref(hd), None, p, p, None, None) == UNSUPPORTED


def test_jet_grad_refusals_before_launch():
    from mmpde_amd import _lib

    lib = _lib.lib()
    ok = _lib.DmmHead(None, None, None, None, 16, 512, None, None, None, 512)
    cot = _lib.DmmJetOut()      # every cotangent null: zero
    names = [n for n, _ in _lib.DmmJetGrads._fields_]
    full = _lib.DmmJetGrads(*([16] * 9))
    p = ctypes.c_void_p(16)
    call = lib.mmpde_dmm_jet_grad
    assert call(None, 2, None, 10, None, None, None, None, None, None) == INVALID
    for hole in range(6):       # branch, grid, hd, workspace, cot, grads
        a = [p, p, ctypes.byref(ok), p, ctypes.byref(cot), ctypes.byref(full)]
        a[hole] = None
        assert call(a[0], 2, a[1], 10, a[2], None, a[3], a[4], a[5], None) == INVALID, hole
    for name in names:          # every gradient is required, 4-B aligned
        for v in (None, 18):
            g = _lib.DmmJetGrads(**{n: (v if n == name else 16) for n in names})
            assert call(p, 2, p, 10, ctypes.byref(ok), None, p, ctypes.byref(cot), ctypes.byref(g), None) == INVALID, name
    good = (ctypes.byref(cot), ctypes.byref(full), None)
    assert call(p, 3, p, 10, ctypes.byref(ok), None, p, *good) == INVALID
    assert call(p, 0, p, 10, ctypes.byref(ok), None, p, *good) == INVALID
    assert call(p, 2, p, 0, ctypes.byref(ok), None, p, *good) == INVALID
    assert call(p, 2, p, 10, ctypes.byref(ok), None, ctypes.c_void_p(24), *good) == INVALID
    assert call(p, 2, ctypes.c_void_p(20), 10, ctypes.byref(ok), None, p, *good) == INVALID
    assert call(ctypes.c_void_p(18), 2, p, 10, ctypes.byref(ok), None, p, *good) == INVALID
    badc = _lib.DmmJetOut(None, 18, None, None, None, None)
    assert call(p, 2, p, 10, ctypes.byref(ok), None, p, ctypes.byref(badc), ctypes.byref(full), None) == INVALID
    for hd in (_lib.DmmHead(None, None, None, None, 16, 512, None, None, None, 100),
               _lib.DmmHead(None, None, None, None, 65, 512, None, None, None, 512)):
        assert call(p, 2, p, 10, ctypes.byref(hd), None, p, *good) == UNSUPPORTED


def test_python_side_refuses_before_it_asks_for_a_device():
    import pytest
    import torch

    from mmpde_amd import DMM

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        dmm = DMM(s=7, mode="array", branch_layer=7, trunk_layer=[2, 3, 512], out_layer=[1024, 128, 1])
    # no CPU fallback: the jet needs device tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dmm.jet(torch.zeros(2, 7, 7), torch.zeros(4, 2))
