"""CPU-only: what the fold-guard cases of mesh_guard_cases.py were chosen for,
on the float64 reference alone, and the C entry mmpde_dmm_mesh_relax without a
GPU (declared, exported, bound; refusals before any launch).

Per case (float64, dmm_hess_cases.hess_ref): lam_b per trajectory, the
classification margin | 1 + alpha_max lam_b - delta | > 100 h_bar on every
trajectory, alpha_ref; with alpha_ref every node has 1 + alpha lam_n >= delta -
1e-12 and det(I + alpha H) > 0 (folds_after == 0); guarded trajectories fold
before the guard; the 'mixed' cases hold guarded and unguarded trajectories
side by side.  The unscaled base cases guard nothing at any delta <= 0.5.

Measured (float64, CPU):
    array-33-B3 (64 / 64)    lam_b -0.7040 -0.7799 -1.2071; delta 0.1: alpha 1, 1, 0.7456;
                             delta 0.25: 1, 0.9617, 0.6213; alpha_max 0.9: 0.9, 0.9, 0.7456
    graph-130-B3 (16 / 16)   lam_b -1.0510 -1.0513 -1.0618; alpha 0.8563 0.8561 0.8476
    graph-130-B33 (64 / 8)   lam_b -1.0745 .. -1.0312; alpha 0.8376 .. 0.8728
    graph-130-B3 (24 / 64)   lam_b -0.9064 -0.8320 -0.8805; delta 0.1438: alpha 0.9446, 1, 0.9724
    graph-130-B33 (56 / 8)   lam_b -0.9402 .. -0.9023; delta 0.0901: 30 guarded, 3 not
                             (margin 0.0022 against 100 h_bar = 0.0018)
    base cases               lam_b -0.0789 (graph B = 3), -0.0153 (graph B = 33), -0.0094 (array)
"""
import ctypes
import os
import re

import pytest
import torch

import dmm_hess_cases as H
import mesh_guard_cases as G
from conftest import ROOT


@pytest.mark.parametrize("name", [g[0] for g in G.GUARD_CASES])
def test_guard_case_is_what_it_was_chosen_for(name):
    r = G.guard_ref(name)
    c = r.c
    assert r.H.dtype == torch.float64 and r.lam_n.shape == (c.B, c.xi.shape[0])
    margin = ((1 + r.alpha_max * r.lam_b) - r.delta).abs()
    print(f"{name}: delta {r.delta:.4f} alpha_max {r.alpha_max:.2f} h_bar {r.h_bar:.3e} lam_b "
          f"{[round(x, 4) for x in r.lam_b.tolist()]} alpha_ref {[round(x, 4) for x in r.alpha.tolist()]} "
          f"guarded {int(r.guarded.sum())} / {c.B} min margin {margin.min().item():.3e} "
          f"({margin.min().item() / r.h_bar:.0f} h_bar)")
    assert bool((margin > G.MARGIN_BARS * r.h_bar).all()), "a trajectory's decision is not defined in float32"
    assert int(r.guarded.sum()) > 0, "nothing to guard"
    # the largest step that keeps every eigenvalue at delta
    assert bool((r.alpha[r.guarded] < r.alpha_max).all()) and bool((r.alpha[~r.guarded] == r.alpha_max).all())
    assert bool((r.alpha[r.guarded] > 0.5).all()), "a case that barely moves"
    after = 1 + r.alpha[:, None] * r.lam_n
    assert bool((after.min(1).values >= r.delta - 1e-12).all())
    assert bool(((after.min(1).values - r.delta).abs()[r.guarded] <= 1e-12).all()), "not the largest step"
    det_after, _ = G.det_alpha64(r.H, r.alpha)
    assert int((~(det_after > 0)).sum()) == 0, "folds after the guard"
    # the full move folds where the guard acts at alpha_max = 1 (an eigenvalue of dx/dxi below 0)
    if r.alpha_max == 1.0:
        folded = (1 + r.lam_b) < 0
        assert bool((r.guarded | ~folded).all())
    if "mixed" in name or "a09" in name:
        assert 0 < int(r.guarded.sum()) < c.B, "no guarded and unguarded trajectories side by side"
    if name.endswith("-all"):
        assert bool(r.guarded.all())


def test_mixed_cases_pin_the_trajectory_index():
    """Guarded and unguarded trajectories alternate in the B = 3 mixed cases, and
    no two guarded trajectories of a case share alpha_ref within the alpha bar."""
    assert G.guard_ref("array-33-B3-mixed").guarded.tolist() == [False, False, True]
    assert G.guard_ref("array-33-B3-d025").guarded.tolist() == [False, True, True]
    assert G.guard_ref("graph-130-B3-mixed").guarded.tolist() == [True, False, True]
    r = G.guard_ref("graph-130-B33-mixed")
    assert int((~r.guarded).sum()) == 3
    for name in ("array-33-B3-d025", "graph-130-B3-mixed"):
        r = G.guard_ref(name)
        a = r.alpha[r.guarded]
        assert (a[0] - a[1]).abs().item() > 100 * G.alpha_bar(a[0].item(), r.lam_b[r.guarded][0].item(), r.h_bar)


@pytest.mark.parametrize("args", G.BASE_CASES, ids=lambda a: "-".join(str(x) for x in a))
def test_base_cases_guard_nothing(args):
    c = H.base_case(*args)
    ref, _ = H.hess_ref(c, key="base")
    lam_b = G.lam_min(G.lam_of(ref).reshape(c.B, -1))
    print(f"{args}: min lam {lam_b.min().item():.4f} .. {lam_b.max().item():.4f}")
    assert bool((lam_b > -0.1).all()) and bool((lam_b < 0).all())
    assert bool((G.alpha_of(lam_b, 1.0, 0.5) == 1.0).all())
    assert bool((1 + lam_b - 0.5 > G.MARGIN_BARS * H.h_bar(ref)).all())


def test_host_restatement():
    """alpha_of and relax32 on hand values (float32)."""
    lam = torch.tensor([-0.5, -1.5, float("nan"), -0.95, 0.25], dtype=torch.float32)
    a = G.alpha_of(lam, 1.0, G.f32(0.1))
    assert a[0] == 1.0 and a[2] == 0.0 and a[4] == 1.0
    assert a[1] == (torch.tensor(1.0) - torch.tensor(0.1)) / torch.tensor(1.5)
    assert a[3] == (torch.tensor(1.0) - torch.tensor(0.1)) / torch.tensor(0.95)
    # the correctly rounded formula against the host's own float32 kernels and float64
    h = 0.6 * torch.rand(4096, 3, generator=torch.Generator().manual_seed(3)) - 0.3
    exact = G.lam_of_rounded32(h)
    assert exact.dtype == torch.float32
    big = torch.maximum(h.abs().max(1).values, exact.abs())     # ulp of the operands: lam may cancel
    assert bool(((exact - G.lam_of(h)).abs() <= 4 * 2.0 ** -23 * big).all())
    assert bool(((exact.double() - G.lam_of(h.double())).abs() <= 4 * 2.0 ** -23 * big.double()).all())
    x1 = torch.rand(6, 2)
    xi = torch.rand(2, 2)
    out = G.relax32(x1, xi, torch.tensor([1.0, 0.25, 0.0]))
    assert torch.equal(out[:2], x1[:2]) and torch.equal(out[4:], xi)
    assert torch.equal(out[2:4], 0.25 * x1[2:4] + 0.75 * xi)
    assert G.ulp32(1.0) == 2.0 ** -23 and G.ulp32(0.75) == 2.0 ** -24


# --------------------------------------------------------------------------- the C entry, no GPU
def test_symbol_declared_exported_and_bound():
    from mmpde_amd import _lib

    src = open(os.path.join(ROOT, "include", "mmpde_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    h = ctypes.CDLL(_lib.LIB_PATH)
    name = "mmpde_dmm_mesh_relax"
    assert re.search(r"\b" + name + r"\s*\(", code) and "mmpde_dmm_relax_io" in code
    assert hasattr(h, name) and name in _lib.EXPORTS
    assert "data_creator_2d.py:109-111,133-135" in src
    assert [n for n, _ in _lib.DmmRelaxIO._fields_] == ["alpha_out", "lam_out", "det_out", "detmin_out",
                                                        "folds_out", "guarded_total"]
    assert ctypes.sizeof(_lib.DmmRelaxIO) == 6 * ctypes.sizeof(ctypes.c_void_p)
    # additive: the version and the Hessian io did not move
    assert _lib.ABI_VERSION == 12302 and _lib.lib().mmpde_version() == 12302
    assert ctypes.sizeof(_lib.DmmHessIO) == 7 * ctypes.sizeof(ctypes.c_void_p)
    from mmpde_amd import ops
    assert callable(ops.mesh_relax)


def test_bad_arguments_are_refused_before_launch():
    """Every call below would fault on its made-up pointers if a kernel ran."""
    from mmpde_amd import _lib

    relax = _lib.lib().mmpde_dmm_mesh_relax
    inval = -1
    assert _lib.lib().mmpde_status_string(inval) == b"invalid argument"
    p = ctypes.c_void_p(64)            # non-null, aligned, never dereferenced before the refusal
    nan = float("nan")

    def io(**kw):
        s = _lib.DmmRelaxIO()
        for k, v in kw.items():
            setattr(s, k, v)
        return ctypes.byref(s)

    full = dict(alpha_out=64, lam_out=64, det_out=64, detmin_out=64, folds_out=64, guarded_total=64)
    # null mesh / xi
    assert relax(None, p, p, 2, 100, 1.0, 0.1, io(**full), None) == inval
    assert relax(p, None, p, 2, 100, 1.0, 0.1, io(**full), None) == inval
    # misaligned: mesh and xi are float2 rows, the rest floats
    assert relax(ctypes.c_void_p(68), p, p, 2, 100, 1.0, 0.1, io(**full), None) == inval
    assert relax(p, ctypes.c_void_p(68), p, 2, 100, 1.0, 0.1, io(**full), None) == inval
    assert relax(p, p, ctypes.c_void_p(66), 2, 100, 1.0, 0.1, io(**full), None) == inval
    for k in full:
        assert relax(p, p, p, 2, 100, 1.0, 0.1, io(**dict(full, **{k: 66})), None) == inval, k
    # ranges
    for b, n in ((0, 100), (2, 0), (-1, 100), (2, -5)):
        assert relax(p, p, p, b, n, 1.0, 0.1, io(**full), None) == inval
    for am in (-0.01, 1.01, nan, float("inf")):
        assert relax(p, p, p, 2, 100, am, 0.1, io(**full), None) == inval, am
    for fl in (1.0, 1.5, nan, float("inf")):
        assert relax(p, p, p, 2, 100, 1.0, fl, io(**full), None) == inval, fl
    # the guard needs the Hessian and a place for alpha; lam / det need the Hessian;
    # the reductions need det_out
    assert relax(p, p, None, 2, 100, 1.0, 0.1, io(**full), None) == inval
    assert relax(p, p, p, 2, 100, 1.0, 0.1, None, None) == inval
    assert relax(p, p, p, 2, 100, 1.0, 0.1, io(**dict(full, alpha_out=None)), None) == inval
    assert relax(p, p, None, 2, 100, 0.5, 0.0, io(lam_out=64), None) == inval
    assert relax(p, p, None, 2, 100, 0.5, 0.0, io(det_out=64), None) == inval
    assert relax(p, p, p, 2, 100, 0.5, 0.0, io(detmin_out=64), None) == inval
    assert relax(p, p, p, 2, 100, 0.5, 0.0, io(folds_out=64), None) == inval


def test_a_library_without_the_symbol_raises(tmp_path, monkeypatch):
    """_lib.lib() names a missing export instead of failing inside ctypes later."""
    from mmpde_amd import _lib

    monkeypatch.setattr(_lib, "_LIB", None)
    monkeypatch.setitem(_lib._SIGS, "mmpde_dmm_no_such_entry", (ctypes.c_int, []))
    with pytest.raises(_lib.HipExtensionMissing, match="mmpde_dmm_no_such_entry"):
        _lib.lib()
    monkeypatch.delitem(_lib._SIGS, "mmpde_dmm_no_such_entry")
    assert _lib.lib().mmpde_version() == 12302
