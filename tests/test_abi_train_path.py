"""The GNN training entry points (csrc/edge_bwd.hip, csrc/head_train.hip, the
skinny weight gradient and the reverse adjacency of csrc/train_rows.hip)
refuse bad arguments with the invalid-argument status before any launch.
Every call breaks exactly one MMPDE_REQUIRE of its entry point (each is read
from the source first) and leaves the others satisfied; the pointers are
non-null dummies that a refusal never dereferences.  Without a GPU only: a
refusal that regressed shows as a failed assertion here, not as a fault on a
shared card."""
import ctypes

import pytest
import torch

import train_path_cases as T

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers: for machines without a GPU")

INVALID = -1
P = ctypes.c_void_p(4096)              # aligned to 256 bytes
ODD = ctypes.c_void_p(4096 + 4)        # 4-byte aligned only
P16 = ctypes.c_void_p(4096 + 16)       # 16-byte but not 256-byte aligned
BIG = 1 << 50
F32, F16X3 = 0, 1


def _lib():
    from mmpde_amd import _lib

    return _lib.lib()


def _requires(name, entry, *conditions):
    lines = " ; ".join(" ".join(x.split()) for x in T.require_lines(T.source(name), entry))
    for cond in conditions:
        assert cond in lines, (entry, cond, lines)


def test_rows_grad_weight_refusals():
    lib = _lib()
    _requires("train_rows.hip", "mmpde_rows_grad_weight", "k <= KMAX", "n_out <= 128", "ldy >= n_out", "ldx >= k",
              "k > 0 || db", "outs <= 1280", "workspace_bytes >= mmpde_rows_grad_weight_workspace_bytes")
    assert "constexpr int KMAX = 64;" in T.source("train_rows.hip")

    def call(x=P, ldx=None, rows=100, k=8, dy=P, ldy=None, n_out=4, dw=P, db=P, ws=P, ws_bytes=None):
        ldx = k if ldx is None else ldx
        ldy = n_out if ldy is None else ldy
        need = lib.mmpde_rows_grad_weight_workspace_bytes(rows, k, n_out)
        return lib.mmpde_rows_grad_weight(x, ldx, rows, k, dy, ldy, n_out, dw, db, ws,
                                          need if ws_bytes is None else need + ws_bytes, None)

    assert call(k=65, n_out=1) == INVALID                        # k > 64 (65 + 1 outputs: inside the cap)
    assert call(k=4, n_out=129) == INVALID                       # n_out > 128 (645 outputs)
    assert call(k=10, n_out=128) == INVALID                      # 1280 + 128 outputs
    assert call(k=20, n_out=64) == INVALID                       # 1280 + 64
    assert call(ldx=7) == INVALID and call(ldy=3) == INVALID
    assert call(k=0, db=None, x=None, dw=None) == INVALID        # nothing to compute
    assert call(ws_bytes=-1) == INVALID and call(ws=None) == INVALID
    assert lib.mmpde_rows_grad_weight_workspace_bytes(100, 8, 4) > 0


def test_head_train_refusals():
    lib = _lib()
    _requires("head_train.hip", "mmpde_head_train_forward", "ldh >= HX && ldh % 4 == 0 && al16(h)")
    _requires("head_train.hip", "mmpde_head_train_backward",
              "ldh >= HX && ldh % 4 == 0 && al16(h) && lddh >= HX && lddh % 4 == 0 && al16(dh)",
              "workspace && workspace_bytes >= mmpde_head_train_workspace_bytes(n)")
    assert "constexpr int HX = 128;" in T.source("head_train.hip")
    n = 100
    need = lib.mmpde_head_train_workspace_bytes(n)
    assert need == 2 * T.HEAD_GRADS * 4 and lib.mmpde_head_train_workspace_bytes(0) == 0

    def fwd(h=P, ldh=128):
        return lib.mmpde_head_train_forward(h, ldh, n, P, P, P, P, P, P, P, None)

    def bwd(h=P, ldh=128, dh=P, lddh=128, ws=P, ws_bytes=need):
        return lib.mmpde_head_train_backward(h, ldh, n, P, P, P, P, P, P, P, dh, lddh, P, ws, ws_bytes, None)

    assert fwd(ldh=124) == INVALID and fwd(ldh=130) == INVALID and fwd(h=ODD) == INVALID
    assert bwd(ldh=124) == INVALID and bwd(ldh=130) == INVALID and bwd(h=ODD) == INVALID
    assert bwd(lddh=124) == INVALID and bwd(lddh=130) == INVALID and bwd(dh=ODD) == INVALID
    assert bwd(ws_bytes=need - 1) == INVALID and bwd(ws=None) == INVALID


def test_reverse_adjacency_refusals():
    lib = _lib()
    _requires("train_rows.hip", "mmpde_reverse_adjacency", "slots < (int64_t)INT32_MAX",
              "scratch_bytes >= mmpde_reverse_adjacency_scratch_bytes(n_tgt, k, n_src)",
              "(((uintptr_t)scratch) & 255) == 0")

    def call(n_tgt=100, k=3, n_src=50, scratch=P, scratch_bytes=BIG):
        return lib.mmpde_reverse_adjacency(P, n_tgt, k, P, n_src, P, P, P, scratch, scratch_bytes, P, None)

    need = lib.mmpde_reverse_adjacency_scratch_bytes(100, 3, 50)
    assert need >= 2 * 1280 + 2560                               # the keys and values, before the sort's own
    assert call(scratch_bytes=need - 1) == INVALID
    assert call(scratch=P16) == INVALID                          # 16-byte aligned is not enough
    assert call(n_tgt=2 ** 28, k=8) == INVALID                   # n_tgt k = 2^31
    assert call(n_tgt=2 ** 31 - 1, k=1) == INVALID               # slots < INT32_MAX


def test_edge_backward_refusals():
    lib = _lib()
    src = T.source("edge_bwd.hip")
    _requires("edge_bwd.hip", "mmpde_gnn_edge_backward_sorted", "slot_pos", "!relu_mask || k <= FKMAX")
    assert "MMPDE_REQUIRE(edge_gemm == MMPDE_EDGE_GEMM_F32 || edge_gemm == MMPDE_EDGE_GEMM_F16X3);" in src
    assert src.count("MMPDE_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)msg2_w | (uintptr_t)grad_mean") == 2

    def ex(a=P, k=3, gemm=F32):
        return lib.mmpde_gnn_edge_backward_ex(a, P, P, None, 10, k, P, P, P, P, P, P, P, P, gemm, None)

    def srt(a=P, k=3, pos=P, mask=None, gemm=F16X3):
        return lib.mmpde_gnn_edge_backward_sorted(a, P, P, None, 10, k, P, P, P, pos, mask, P, P, P, P, P, gemm, None)

    assert ex(gemm=2) == INVALID and ex(gemm=-1) == INVALID and srt(gemm=2) == INVALID
    assert srt(pos=None) == INVALID and srt(pos=None, gemm=F32) == INVALID
    assert srt(mask=P, k=65) == INVALID and srt(mask=P, k=65, gemm=F32) == INVALID
    assert ex(a=ODD) == INVALID and ex(a=ODD, gemm=F16X3) == INVALID and srt(a=ODD, mask=P) == INVALID
    assert lib.mmpde_gnn_edge_backward(ODD, P, P, None, 10, 3, P, P, P, P, P, P, P, P, None) == INVALID
