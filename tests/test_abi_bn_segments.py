"""mmpde_batch_norm_rows_train_segments without a GPU: the exports, every refusal
its header comment lists (dummy pointers: a refused call launches nothing and
reads none of them), the workspace size against its restatement, and the
batch= argument of dmm_train.evaluate / evaluate_tri / train_MA_res refusing a
count below 1 before the device is touched."""
import ctypes

import pytest
import torch

INVALID = -1                     # MMPDE_ERR_INVALID_ARG
A = 0x10000                      # a 16-byte aligned dummy address


def _lib():
    from mmpde_amd import _lib as L
    return L


def _bn_ws(n, C):
    """mmpde_batch_norm_rows_workspace_bytes for n <= 64 * 64 rows: ceil(n / 64)
    workgroups (fewer than four per CU of any device) of 2 C + 4 floats."""
    assert 0 < n <= 64 * 64
    return -(-n // 64) * (2 * C + 4) * 4


def test_exports():
    L = _lib()
    h = ctypes.CDLL(L.LIB_PATH)
    for name in ("mmpde_batch_norm_rows_train_segments", "mmpde_batch_norm_rows_train_segments_workspace_bytes"):
        assert hasattr(h, name), name
        assert name in L.EXPORTS, name


@pytest.mark.parametrize("S,n,C", [(1, 2, 4), (3, 2, 4), (4, 3, 12), (2, 257, 4), (5, 2521, 4), (150, 37, 4),
                                   (3, 65, 128), (2, 64, 1024), (65535, 4096, 8)])
def test_workspace_bytes(S, n, C):
    lib = _lib().lib()
    got = lib.mmpde_batch_norm_rows_train_segments_workspace_bytes(S, n, C)
    # per segment: the partials of one mmpde_batch_norm_rows_train call on n rows, and C unbiased variances
    assert got == S * (lib.mmpde_batch_norm_rows_workspace_bytes(n, C) + 4 * C)
    assert got == S * (_bn_ws(n, C) + 4 * C)
    assert got % 16 == 0


def test_workspace_bytes_of_no_work():
    lib = _lib().lib()
    for S, n, C in ((0, 5, 4), (-1, 5, 4), (2, 0, 4), (2, 5, 0)):
        assert lib.mmpde_batch_norm_rows_train_segments_workspace_bytes(S, n, C) == 0


def _call(**kw):
    """The entry with one argument set changed; the rest would be a valid call
    of S = 3 segments of 65 rows by 128 channels."""
    lib = _lib().lib()
    S, n, C = kw.get("S", 3), kw.get("n", 65), kw.get("C", 128)
    need = S * (_bn_ws(n, C) + 4 * C) if 0 < n <= 4096 and S > 0 and C > 0 else 1 << 20
    a = dict(x=A, res=A, S=S, n=n, C=C, weight=A, bias=A, eps=1e-5, factor=0.1, rm=A, rv=A, y=A, stats=A,
             workspace=A, workspace_bytes=need)
    a.update(kw)
    return lib.mmpde_batch_norm_rows_train_segments(
        a["x"], a["res"], a["S"], a["n"], a["C"], a["weight"], a["bias"], a["eps"], a["factor"], a["rm"], a["rv"],
        a["y"], a["stats"], a["workspace"], a["workspace_bytes"], None)


@pytest.mark.parametrize("kw", [
    dict(x=None), dict(y=None), dict(stats=None), dict(workspace=None),                     # nulls
    dict(S=0), dict(S=-2), dict(S=65536),                                                    # segments
    dict(n=0), dict(n=-1),                                                                   # rows of a segment
    dict(C=0), dict(C=6), dict(C=1028), dict(C=-4),                                          # channels
    dict(x=A + 4), dict(res=A + 8), dict(y=A + 4), dict(stats=A + 12), dict(workspace=A + 4),   # alignment
    dict(workspace_bytes=3 * (_bn_ws(65, 128) + 4 * 128) - 1), dict(workspace_bytes=0),     # workspace too small
    dict(workspace_bytes=_bn_ws(3 * 65, 128) + 12 * 128),                                   # sized for one batch of S n
], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_refusals(kw):
    assert _call(**kw) == INVALID


def test_refused_everything_null():
    lib = _lib().lib()
    assert lib.mmpde_batch_norm_rows_train_segments(None, None, 3, 10, 128, None, None, 1e-5, 0.1, None, None, None,
                                                    None, None, 0, None) == INVALID


@pytest.mark.parametrize("batch", [0, -3, 2.0, True])
def test_evaluate_batch_below_one_raises_before_the_device(batch):
    """ValueError before any tensor goes to the device: the device named here
    need not exist, and the model is never called."""
    from mmpde_amd import dmm_train as T

    u = torch.zeros(2, 4, 4)
    with pytest.raises(ValueError, match="batch"):
        T.evaluate(None, u, "cuda:0", batch=batch)
    with pytest.raises(ValueError, match="batch"):
        T.evaluate_tri(None, u.reshape(2, 16), torch.zeros(16, 2), "cuda:0", batch=batch)
    with pytest.raises(ValueError, match="batch"):
        T.train_MA_res(None, u, u, None, None, False, 1, 0, "cuda:0", eval_batch=batch)
