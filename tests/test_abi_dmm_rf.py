"""The random-feature phase's entry points (mmpde_dmm_rf_features,
mmpde_rf_objective, mmpde_sym_matvec, mmpde_bfgs_update and their sizing
helpers) are declared, exported and bound, size their buffers by host
arithmetic, and refuse bad arguments before any launch (no GPU needed)."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

NEW = ("mmpde_dmm_rf_features_workspace_bytes", "mmpde_dmm_rf_features", "mmpde_rf_objective_workspace_bytes",
       "mmpde_rf_objective", "mmpde_sym_matvec", "mmpde_bfgs_update_workspace_bytes", "mmpde_bfgs_update")
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
    assert "mmpde_dmm_rf_out" in code and "mmpde_rf_problem" in code
    assert re.search(r"#define\s+MMPDE_BFGS_MAX_N\s+1024\b", code) and _lib.BFGS_MAX_N == 1024
    # the header cites what the entries replace and states the two differences
    for cite in ("mesh/dmm_utils.py:785-1076", "dmm_utils.py:883-905", "random_feature_torch2"):
        assert cite in src, cite
    assert "s_xy and s_yx separately" in src and "contributes 0" in src
    # added without a version step
    assert _lib.ABI_VERSION == 12302 and _lib.lib().mmpde_version() == 12302
    assert [n for n, _ in _lib.DmmRfOut._fields_] == ["s", "s_x", "s_y", "s_xx", "s_xy", "s_yy"]
    assert ctypes.sizeof(_lib.DmmRfOut) == 6 * ctypes.sizeof(ctypes.c_void_p)
    # 15 pointers, two int64, three int, four float (+ tail padding to 8)
    assert ctypes.sizeof(_lib.RfProblem) == 15 * 8 + 2 * 8 + 3 * 4 + 4 * 4 + 4
    # the source is part of the build
    mk = open(os.path.join(ROOT, "mm-pde_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bdmm_rf\.hip\b", mk, flags=re.M)


def test_sizing_helpers():
    from mmpde_amd import _lib

    lib = _lib.lib()
    for b, n, lat, lp, th in ((1, 1, 8, 128, 1), (20, 320, 512, 512, 16), (3, 195, 64, 1024, 7)):
        phi = lib.mmpde_dmm_phi_workspace_bytes(b, n, lat, lp, th)
        rf = lib.mmpde_dmm_rf_features_workspace_bytes(b, n, lat, lp, th)
        # mmpde_dmm_phi's workspace, K [n, L', 3] and an s scratch [n, L']
        assert rf >= phi + 4 * n * lp * 4 and rf % 16 == 0
    assert lib.mmpde_dmm_rf_features_workspace_bytes(0, 10, 8, 128, 1) == 0
    assert lib.mmpde_dmm_rf_features_workspace_bytes(2, 10, 8, 128, 0) == 0
    for m, mb in ((1, 1), (80, 8), (320, 80)):
        nb = lib.mmpde_rf_objective_workspace_bytes(m, mb)
        # p [5 m + 4 mb], query [2 m], ux, uy [m] each, df/dp [5 m], two VJPs [2 m] each
        assert nb >= (18 * m + 4 * mb) * 4 and nb % 16 == 0
    assert lib.mmpde_rf_objective_workspace_bytes(320, 0) == 0
    assert lib.mmpde_rf_objective_workspace_bytes(0, 80) == 0
    for n in (1, 33, 512, 1024):
        nb = lib.mmpde_bfgs_update_workspace_bytes(n)
        assert nb >= (n + 3) * 4 and nb % 16 == 0
    assert lib.mmpde_bfgs_update_workspace_bytes(1025) == 0 and lib.mmpde_bfgs_update_workspace_bytes(0) == 0


def test_features_refusals_before_launch():
    from mmpde_amd import _lib

    lib = _lib.lib()
    ok = _lib.DmmHead(None, None, None, None, 16, 512, None, None, None, 512)
    out = _lib.DmmRfOut()
    p = ctypes.c_void_p(16)     # non-null, 16-B aligned, never dereferenced before the refusal
    call = lib.mmpde_dmm_rf_features
    assert call(None, 2, None, 10, None, None, None, None) == INVALID
    for hole in range(5):       # each mandatory pointer in turn
        a = [p, p, ctypes.byref(ok), p, ctypes.byref(out)]
        a[hole] = None
        assert call(a[0], 2, a[1], 10, a[2], a[3], a[4], None) == INVALID, hole
    assert call(p, 3, p, 10, ctypes.byref(ok), p, ctypes.byref(out), None) == INVALID     # n_grid % B
    assert call(p, 0, p, 10, ctypes.byref(ok), p, ctypes.byref(out), None) == INVALID
    assert call(p, 2, p, 0, ctypes.byref(ok), p, ctypes.byref(out), None) == INVALID
    # misaligned: workspace (16 B), grid (8 B), branch and a table (4 B)
    assert call(p, 2, p, 10, ctypes.byref(ok), ctypes.c_void_p(24), ctypes.byref(out), None) == INVALID
    assert call(p, 2, ctypes.c_void_p(20), 10, ctypes.byref(ok), p, ctypes.byref(out), None) == INVALID
    assert call(ctypes.c_void_p(18), 2, p, 10, ctypes.byref(ok), p, ctypes.byref(out), None) == INVALID
    bad = _lib.DmmRfOut(None, None, 18, None, None, None)
    assert call(p, 2, p, 10, ctypes.byref(ok), p, ctypes.byref(bad), None) == INVALID
    # the heads mmpde_dmm_phi does not take
    for hd in (_lib.DmmHead(None, None, None, None, 16, 512, None, None, None, 100),
               _lib.DmmHead(None, None, None, None, 65, 512, None, None, None, 512)):
        assert call(p, 2, p, 10, ctypes.byref(hd), p, ctypes.byref(out), None) == UNSUPPORTED
        assert lib.mmpde_dmm_phi(p, 2, p, 10, ctypes.byref(hd), None, p, p, None, None) == UNSUPPORTED


def _problem(_lib, **kw):
    p = 16
    f = dict(so_x=p, so_y=p, so_xx=p, so_xy=p, so_yy=p, b_x0=p, b_x1=p, b_y0=p, b_y1=p, x=p, ux=p, uy=p, alpha=p,
             rhs=p, lattice=p, m=80, mb=8, hidden=512, bu=10, n=48, w0=1.0, w1=1000.0, w2=1.0, convex_rel=0.0)
    f.update(kw)
    return _lib.RfProblem(**f)


def test_objective_refusals_before_launch():
    from mmpde_amd import _lib

    lib = _lib.lib()
    p = ctypes.c_void_p(16)
    call = lib.mmpde_rf_objective
    good = _problem(_lib)
    assert call(None, None, None, None, None, None, None, None) == INVALID
    for hole in range(6):       # w, pb, workspace, f, g, parts (lhs is nullable)
        a = [p, ctypes.byref(good), p, p, p, p]
        a[hole] = None
        assert call(*a, None, None) == INVALID, hole
    for name in ("so_x", "so_y", "so_xx", "so_xy", "so_yy", "b_x0", "b_x1", "b_y0", "b_y1", "x", "ux", "uy",
                 "alpha", "rhs", "lattice"):
        pb = _problem(_lib, **{name: None})
        assert call(p, ctypes.byref(pb), p, p, p, p, None, None) == INVALID, name
    for kw in (dict(mb=0), dict(m=0), dict(hidden=0), dict(bu=0), dict(n=1), dict(m=81), dict(x=20),
               dict(lattice=12)):
        pb = _problem(_lib, **kw)
        assert call(p, ctypes.byref(pb), p, p, p, p, None, None) == INVALID, kw
    assert call(p, ctypes.byref(good), ctypes.c_void_p(24), p, p, p, None, None) == INVALID
    assert call(ctypes.c_void_p(18), ctypes.byref(good), p, p, p, p, None, None) == INVALID
    assert call(p, ctypes.byref(good), p, p, p, p, ctypes.c_void_p(18), None) == INVALID


def test_dense_refusals_before_launch():
    from mmpde_amd import _lib, ops

    lib = _lib.lib()
    p = ctypes.c_void_p(16)
    assert lib.mmpde_sym_matvec(p, p, 1025, p, 1.0, None) == INVALID
    assert lib.mmpde_sym_matvec(p, p, 0, p, 1.0, None) == INVALID
    assert lib.mmpde_bfgs_update(p, p, p, 1025, p, None) == INVALID
    assert lib.mmpde_bfgs_update(p, p, p, 0, p, None) == INVALID
    for hole in range(3):
        a = [p, p, p]
        a[hole] = None
        assert lib.mmpde_sym_matvec(a[0], a[1], 33, a[2], 1.0, None) == INVALID
        assert lib.mmpde_bfgs_update(a[0], a[1], a[2], 33, p, None) == INVALID
    assert lib.mmpde_bfgs_update(p, p, p, 33, None, None) == INVALID
    assert lib.mmpde_bfgs_update(p, p, p, 33, ctypes.c_void_p(24), None) == INVALID
    assert lib.mmpde_sym_matvec(ctypes.c_void_p(18), p, 33, p, 1.0, None) == INVALID
    # the Python side says so before it asks for a device
    big = torch.zeros(1025)
    with pytest.raises(ValueError, match="1024"):
        ops.sym_matvec(torch.zeros(1025, 1025), big)
    with pytest.raises(ValueError, match="1024"):
        ops.bfgs_update(torch.zeros(1025, 1025), big, big)
    from mmpde_amd.minimize import HipDense, minimize_bfgs
    with pytest.raises(ValueError, match="1024"):
        minimize_bfgs(lambda x: (0.0, x), big + 1.0, 3, HipDense())


def _rf_args(**kw):
    a = dict(experiment="burgers", bound_constraint="soft", batch_size_x_adam=8, batch_size_u_adam=4,
             batch_size_x_lbfgs=8, batch_size_u_lbfgs=4, train_sample_grid=0, lr_adam=2e-4, lr_lbfgs=1e-3,
             weight_decay=1e-5, gamma_adam=0.2, gamma_lbfgs=0.2, loss_weight0=1.0, loss_weight1=1000.0,
             loss_weight2=1.0, loss_convex=True, rf=True, rf_opt_alg="BFGS", epochs_rf=1, max_iter=5,
             batch_size_x_rf=8, batch_size_u_rf=4, convex_rel=0.0)
    a.update(kw)
    return SimpleNamespace(**a)


def test_empty_sides_and_newton_are_refused():
    from mmpde_amd import DMM, dmm_train as T, ops

    # Mb == 0: the objective itself, and the phase through batch_size_x_rf < 4
    tab = torch.zeros(8, 16)
    feats = ops.RfFeatures(tab, tab, tab, tab, tab, tab)
    empty = [torch.zeros(0, 16)] * 4
    with pytest.raises(ValueError, match="Mb == 0"):
        ops.RfObjective(feats, empty, torch.zeros(8, 2), torch.zeros(2, 6, 6), torch.zeros(2, 6, 6),
                        torch.ones(2), torch.ones(2), 1.0, 1000.0, 1.0, 0.0)
    with pytest.raises(ValueError, match="Mb == 0"):
        T.random_feature_epoch(None, _rf_args(batch_size_x_rf=3), None, "cpu")
    # Newton-CG is not built, and the message says what is
    with pytest.raises(NotImplementedError, match="Newton.*BFGS"):
        T.random_feature_epoch(None, _rf_args(rf_opt_alg="Newton"), None, "cpu")
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        dmm = DMM(s=7, mode="array", branch_layer=7, trunk_layer=[2, 3, 512], out_layer=[1024, 16, 1])
    before = {k: v.clone() for k, v in dmm.state_dict().items()}
    u = torch.zeros(4, 7, 7)
    with pytest.raises(NotImplementedError, match="Newton"):
        T.train_MA_res(u, u, u, _rf_args(rf_opt_alg="Newton"), dmm, False, 0, 0, "cpu", save_dir=False,
                       evaluate_every=0)
    assert all(torch.equal(v, before[k]) for k, v in dmm.state_dict().items())
    with pytest.raises(ValueError):
        T.random_feature_epoch(None, _rf_args(rf_opt_alg="Adam"), None, "cpu")
