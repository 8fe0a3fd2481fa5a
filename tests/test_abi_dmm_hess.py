"""The mesh-Jacobian entry points (mmpde_dmm_hess_*, mmpde_dmm_mesh_*_hess) are
declared, exported and bound, size their buffers by host arithmetic and refuse
null arguments and an unsupported head before any launch (no GPU needed)."""
import ctypes
import os
import re

from conftest import ROOT

NEW = ("mmpde_dmm_hess_cache_bytes", "mmpde_dmm_hess_prepare", "mmpde_dmm_hess_workspace_bytes",
       "mmpde_dmm_mesh_graph_hess", "mmpde_dmm_mesh_array_hess")


def test_symbols_declared_exported_and_bound():
    from mmpde_amd import _lib

    src = open(os.path.join(ROOT, "include", "mmpde_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert hasattr(h, name), name
        assert name in _lib.EXPORTS, name
    assert "mmpde_dmm_hess_io" in code
    # the header cites what the entries replace
    assert "data_creator_2d.py:115-137" in src and "mesh/dmm_utils.py:507-552" in src
    assert _lib.ABI_VERSION == 12302 and _lib.lib().mmpde_version() == 12302
    assert [n for n, _ in _lib.DmmHessIO._fields_] == ["head_cache", "hess_cache", "hess_out", "det_out",
                                                       "detmin_out", "folds_out", "folds_total"]
    assert ctypes.sizeof(_lib.DmmHessIO) == 7 * ctypes.sizeof(ctypes.c_void_p)


def test_sizing_helpers():
    from mmpde_amd import _lib

    lib = _lib.lib()
    for n, lp in ((6, 128), (2521, 512), (65536, 512)):
        assert lib.mmpde_dmm_hess_cache_bytes(n, lp) == 3 * n * lp * 4
    assert lib.mmpde_dmm_hess_cache_bytes(0, 512) == 0
    for b, n, lat, lp in ((1, 6, 8, 128), (16, 2521, 512, 512), (65, 130, 512, 512), (2, 65536, 512, 512)):
        mesh = lib.mmpde_dmm_workspace_bytes(b, n, lat, lp)
        hess = lib.mmpde_dmm_hess_workspace_bytes(b, n, lat, lp)
        # the mesh workspace, K when no cache is given, a det scratch when no det_out is
        assert hess >= mesh + 3 * n * lp * 4 + b * n * 4 and hess % 4 == 0
    # the mesh call's own sizes did not move
    assert lib.mmpde_dmm_head_cache_bytes(2521, 512) == 3 * 2521 * 512 * 4


def test_null_arguments_and_unsupported_head_are_refused_before_launch():
    from mmpde_amd import _lib

    lib = _lib.lib()
    assert lib.mmpde_dmm_hess_prepare(None, 100, None, None, None, None) == -1
    assert lib.mmpde_dmm_mesh_graph_hess(None, None, 2, 100, None, 35, None, None, None, None, None, None) == -1
    assert lib.mmpde_dmm_mesh_array_hess(None, None, 2, 100, None, None, None, None, None, None) == -1
    io = _lib.DmmHessIO()
    ok = _lib.DmmHead(None, None, None, None, 16, 512, None, None, None, 512)
    # a null io alone, and null data pointers with everything else in place
    gb, ab = _lib.DmmGraphBranch(), _lib.DmmArrayBranch()
    ab.s = 5
    p = ctypes.c_void_p(16)    # non-null, 16-B aligned, never dereferenced before the refusal
    assert lib.mmpde_dmm_mesh_graph_hess(p, p, 2, 100, p, 35, ctypes.byref(gb), ctypes.byref(ok), None, p, p,
                                         None) == -1
    assert lib.mmpde_dmm_mesh_array_hess(p, p, 2, 100, ctypes.byref(ab), ctypes.byref(ok), None, p, p, None) == -1
    assert lib.mmpde_dmm_mesh_graph_hess(None, None, 2, 100, None, 35, None, ctypes.byref(ok), ctypes.byref(io),
                                         None, None, None) == -1
    assert lib.mmpde_dmm_mesh_array_hess(None, None, 2, 100, None, ctypes.byref(ok), ctypes.byref(io), None,
                                         None, None) == -1
    # a head the kernels do not cover (hidden no multiple of 128; th > 64) is
    # refused once the pointers are there, before any launch
    unsupported = -2   # MMPDE_ERR_UNSUPPORTED
    assert lib.mmpde_status_string(unsupported) not in (b"ok", b"invalid argument")
    for hd in (_lib.DmmHead(None, None, None, None, 16, 512, None, None, None, 100),
               _lib.DmmHead(None, None, None, None, 65, 512, None, None, None, 512)):
        assert lib.mmpde_dmm_mesh_graph_hess(p, p, 2, 100, p, 35, ctypes.byref(gb), ctypes.byref(hd),
                                             ctypes.byref(io), p, p, None) == unsupported
        assert lib.mmpde_dmm_mesh_array_hess(p, p, 2, 100, ctypes.byref(ab), ctypes.byref(hd), ctypes.byref(io),
                                             p, p, None) == unsupported
        assert lib.mmpde_dmm_hess_prepare(p, 100, ctypes.byref(hd), p, p, None) == unsupported
