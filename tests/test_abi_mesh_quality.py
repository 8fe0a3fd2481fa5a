"""The mesh-quality entry points (mmpde_mesh_monitor_*, mmpde_mesh_quality and
its sizing helper) are declared, exported and bound without a version step,
size their workspace by host arithmetic and refuse null or absurd arguments
before any launch (no GPU needed)."""
import ctypes
import os
import re

from conftest import ROOT

NEW = ("mmpde_mesh_monitor_array", "mmpde_mesh_monitor_grad", "mmpde_mesh_quality_workspace_bytes",
       "mmpde_mesh_quality")
INVALID = -1   # MMPDE_ERR_INVALID_ARG


def test_symbols_declared_exported_and_bound():
    from mmpde_amd import _lib

    src = open(os.path.join(ROOT, "include", "mmpde_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert hasattr(h, name), name
        assert name in _lib.EXPORTS, name
    assert "mmpde_mesh_quality_io" in code
    # the header cites what the entries replace
    assert "mesh/dmm_utils.py:1162-1284" in src and "dmm_utils.py:233-249" in src
    assert "dmm_utils.py:1264-1267" in src and "dmm_utils.py:209-210" in src
    # only exports were added
    assert _lib.ABI_VERSION == 12302 and _lib.lib().mmpde_version() == 12302
    assert [n for n, _ in _lib.MeshQualityIO._fields_] == ["mean", "std", "range", "inverted", "area_ratio_min",
                                                          "inverted_total", "mg"]
    assert ctypes.sizeof(_lib.MeshQualityIO) == 7 * ctypes.sizeof(ctypes.c_void_p)
    m = re.search(r"#define\s+MMPDE_MESH_QUALITY_MAX_N\s+(\d+)", src)
    from mmpde_amd import ops
    assert m and int(m.group(1)) == ops.MESH_QUALITY_MAX_N == 256
    mk = open(os.path.join(ROOT, "mm-pde_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bmesh_quality\.hip\b", mk, flags=re.M)


def test_sizing_helper():
    from mmpde_amd import _lib

    lib = _lib.lib()
    for b, c in ((1, 1), (3, 25), (2, 64), (16, 5022), (32, 2209), (65535, 65025)):
        assert lib.mmpde_mesh_quality_workspace_bytes(b, c) == ((b * c + 3) // 4) * 16
    for b, c in ((0, 5), (5, 0), (-1, 5), (5, -1)):
        assert lib.mmpde_mesh_quality_workspace_bytes(b, c) == 0


def test_refusals_before_launch():
    from mmpde_amd import _lib

    lib = _lib.lib()
    p = ctypes.c_void_p(16)    # non-null, 16-B aligned, never dereferenced before the refusal
    io = _lib.MeshQualityIO()  # every output null: allowed
    rio = ctypes.byref(io)

    def quality(mesh=p, xi=p, b=2, n_per=9, cells=p, c=4, arity=4, m=p, n=3, io_=rio, ws=p):
        return lib.mmpde_mesh_quality(mesh, xi, b, n_per, cells, c, arity, m, n, io_, ws, None)

    # null required pointers, one at a time and all together
    assert lib.mmpde_mesh_quality(None, None, 2, 9, None, 4, 4, None, 3, None, None, None) == INVALID
    for kw in ("mesh", "xi", "cells", "m", "io_"):
        assert quality(**{kw: None}) == INVALID, kw
    assert quality(ws=None) == INVALID           # no mg and no workspace: nowhere for the per-cell values
    # arity
    for a in (0, 2, 5, -3):
        assert quality(arity=a) == INVALID, a
    # C < 1; n < 2, n > 256; N < arity; B < 1
    for c in (0, -1):
        assert quality(c=c) == INVALID
    for n in (1, 0, -4, 257, 1 << 20):
        assert quality(n=n) == INVALID, n
    assert quality(n_per=3) == INVALID and quality(arity=3, n_per=2) == INVALID
    for b in (0, -2, 65536):
        assert quality(b=b) == INVALID
    # misaligned tables
    assert quality(cells=ctypes.c_void_p(20)) == INVALID and quality(mesh=ctypes.c_void_p(20)) == INVALID

    for fn in (lib.mmpde_mesh_monitor_array, lib.mmpde_mesh_monitor_grad):
        assert fn(None, 2, 5, None, None, None, None) == INVALID
        for i in range(4):
            args = [p, p, p, p]
            args[i] = None
            assert fn(args[0], 2, 5, args[1], args[2], args[3], None) == INVALID, i
        for n in (1, 0, -1, 257):
            assert fn(p, 2, n, p, p, p, None) == INVALID, n
        for b in (0, -1):
            assert fn(p, b, 5, p, p, p, None) == INVALID


def test_python_side_refusals_need_no_device():
    """What ops checks on the host before it looks for a device."""
    import pytest
    import torch

    from mmpde_amd import ops

    with pytest.raises(ValueError):
        ops.mesh_cells_lattice(1)
    with pytest.raises(ValueError):
        ops.MeshCells(torch.tensor([[0, 1, 9]]), 9, "cpu")       # index out of range
    with pytest.raises(ValueError):
        ops.MeshCells(torch.tensor([[0, 1, -1, 2]]), 9, "cpu")
    with pytest.raises(ValueError):
        ops.MeshCells(torch.zeros((0, 3), dtype=torch.int32), 9, "cpu")
    with pytest.raises(ValueError):
        ops.MeshCells(torch.zeros((4, 5), dtype=torch.int32), 9, "cpu")
    c = ops.MeshCells(torch.tensor([[0, 1, 2], [2, 1, 3]]), 4, "cpu")
    assert c.arity == 3 and c.n_cells == 2 and c.table.dtype == torch.int32
    assert c.table.tolist() == [[0, 1, 2, 2], [2, 1, 3, 3]]
