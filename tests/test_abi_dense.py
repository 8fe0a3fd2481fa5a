"""The dense, smoother and row-reduction entry points (csrc/dense.hip,
csrc/smooth.hip, mmpde_segment_sum) refuse bad arguments with the
invalid-argument status before any launch (no GPU needed): the pointers are
non-null and never dereferenced before the refusal."""
import ctypes

INVALID = -1
P = ctypes.c_void_p(16)
ZEROS, CIRCULAR = 0, 1


def _lib():
    from mmpde_amd import _lib

    return _lib.lib()


def _conv(lib, **kw):
    a = dict(x=P, batches=2, cin=3, h=8, w=8, weight=P, bias=P, cout=4, ks=3, stride=1, pad=1, pad_mode=ZEROS,
             residual=None, res_after_act=0, act=0, y=P)
    a.update(kw)
    return lib.mmpde_conv2d_ex(a["x"], a["batches"], a["cin"], a["h"], a["w"], a["weight"], a["bias"], a["cout"],
                               a["ks"], a["stride"], a["pad"], a["pad_mode"], a["residual"], a["res_after_act"],
                               a["act"], a["y"], None)


def test_conv2d_ex_refusals():
    lib = _lib()
    assert _conv(lib, stride=3) == INVALID and _conv(lib, stride=0) == INVALID
    assert _conv(lib, pad_mode=2) == INVALID and _conv(lib, pad_mode=-1) == INVALID
    assert _conv(lib, res_after_act=1) == INVALID                     # ... without a residual
    assert _conv(lib, h=2, w=8, ks=7, pad=3, pad_mode=CIRCULAR) == INVALID    # wraps more than once: pad > h
    assert _conv(lib, h=8, w=2, ks=7, pad=3, pad_mode=CIRCULAR) == INVALID
    assert _conv(lib, act=4) == INVALID and _conv(lib, pad=-1) == INVALID
    assert _conv(lib, h=2, w=2, ks=5, pad=0) == INVALID               # no output
    for hole in ("x", "weight", "y"):
        assert _conv(lib, **{hole: None}) == INVALID, hole
    for zero in ("batches", "cin", "cout", "ks"):
        assert _conv(lib, **{zero: 0}) == INVALID, zero


def _gw(lib, **kw):
    a = dict(x=P, batches=2, cin=3, h=8, w=8, dy=P, cout=2, ks=3, pad=1, pad_mode=ZEROS, dw=P, db=None)
    a.update(kw)
    return lib.mmpde_conv2d_grad_weight(a["x"], a["batches"], a["cin"], a["h"], a["w"], a["dy"], a["cout"], a["ks"],
                                        a["pad"], a["pad_mode"], a["dw"], a["db"], None)


def test_conv2d_grad_weight_refusals():
    lib = _lib()
    assert _gw(lib, h=40, w=40, ks=17, pad=8) == INVALID              # 289 taps: more than a workgroup
    assert _gw(lib, ks=4, pad=2) == INVALID and _gw(lib, ks=2, pad=1) == INVALID and _gw(lib, ks=2, pad=0) == INVALID
    assert _gw(lib, ks=3, pad=0) == INVALID and _gw(lib, ks=3, pad=2) == INVALID and _gw(lib, ks=5, pad=1) == INVALID
    assert _gw(lib, pad_mode=2) == INVALID
    assert _gw(lib, h=2, w=8, ks=7, pad=3, pad_mode=CIRCULAR) == INVALID
    for hole in ("x", "dy", "dw"):
        assert _gw(lib, **{hole: None}) == INVALID, hole
    for zero in ("batches", "cin", "cout", "h", "w", "ks"):
        assert _gw(lib, **{zero: 0}) == INVALID, zero


def test_softmax_interp_refusals():
    lib = _lib()
    for grad in (False, True):
        def call(n_pts=10, pts_sets=1, val_sets=1, n_q=12, pts=P, vals=P, qry=P, out=P, g=P):
            if grad:
                return lib.mmpde_softmax_interp_grad(pts, n_pts, pts_sets, vals, val_sets, qry, n_q, 1.0, g, out, None)
            return lib.mmpde_softmax_interp(pts, n_pts, pts_sets, vals, val_sets, qry, n_q, 1.0, out, None)

        assert call(pts_sets=5) == INVALID and call(val_sets=5) == INVALID    # 12 queries over 5 sets
        assert call(pts_sets=5, val_sets=5) == INVALID and call(pts_sets=24) == INVALID
        assert call(n_pts=0) == INVALID and call(n_q=0) == INVALID
        assert call(pts_sets=0) == INVALID and call(val_sets=0) == INVALID
        for hole in ("pts", "vals", "qry", "out") + (("g",) if grad else ()):
            assert call(**{hole: None}) == INVALID, hole


def test_outer_rows_and_transpose_refusals():
    lib = _lib()

    def outer(g=P, ldg=8, x=P, ldx=20, m=4, n=8, k=20, dw=P, lddw=20):
        return lib.mmpde_outer_rows(g, ldg, x, ldx, m, n, k, dw, lddw, None, None)

    assert outer(ldg=7) == INVALID and outer(ldx=19) == INVALID and outer(lddw=19) == INVALID
    assert outer(m=0) == INVALID and outer(n=0, ldg=8) == INVALID and outer(k=0) == INVALID
    assert outer(g=None) == INVALID and outer(x=None) == INVALID and outer(dw=None) == INVALID

    def transpose(x=P, rows=5, cols=9, ldx=9, y=P, ldy=5):
        return lib.mmpde_transpose(x, rows, cols, ldx, y, ldy, None)

    assert transpose(ldx=8) == INVALID and transpose(ldy=4) == INVALID
    assert transpose(rows=0) == INVALID and transpose(cols=0) == INVALID
    assert transpose(x=None) == INVALID and transpose(y=None) == INVALID
    assert lib.mmpde_tanh_bwd(P, P, 0, P, None) == INVALID and lib.mmpde_tanh_bwd(None, P, 4, P, None) == INVALID
    assert lib.mmpde_tanh_bwd(P, None, 4, P, None) == INVALID and lib.mmpde_tanh_bwd(P, P, 4, None, None) == INVALID


def test_traj_mse_and_resample_refusals():
    lib = _lib()
    assert lib.mmpde_traj_mse(P, P, 3, 0, P, None) == INVALID         # n_per = 0
    assert lib.mmpde_traj_mse(P, P, 0, 5, P, None) == INVALID
    assert lib.mmpde_traj_mse(P, P, 2 ** 31, 5, P, None) == INVALID   # one workgroup per trajectory
    for hole in range(3):
        a = [P, P, P]
        a[hole] = None
        assert lib.mmpde_traj_mse(a[0], a[1], 3, 5, a[2], None) == INVALID, hole
    assert lib.mmpde_resample_bilinear(P, 1, 4, 4, 0, 3, P, None) == INVALID
    assert lib.mmpde_resample_bilinear(P, 0, 4, 4, 3, 3, P, None) == INVALID
    assert lib.mmpde_resample_bilinear(None, 1, 4, 4, 3, 3, P, None) == INVALID


def test_linear_skinny_refusals():
    lib = _lib()

    def call(x=P, ldx=20, m=3, k=20, w=P, ldw=20, n=8, act=0, y=P, ldy=8):
        return lib.mmpde_linear_skinny_ws(x, ldx, m, k, w, ldw, None, n, act, y, ldy, None, 0, None)

    assert call(ldx=19) == INVALID and call(ldw=19) == INVALID and call(ldy=7) == INVALID
    assert call(act=3) == INVALID and call(m=4097) == INVALID and call(m=0) == INVALID
    assert call(x=None) == INVALID and call(w=None) == INVALID and call(y=None) == INVALID
    assert lib.mmpde_linear_skinny(P, 19, 3, 20, P, 20, None, 8, 0, P, 8, None) == INVALID
    assert lib.mmpde_linear_skinny_workspace_bytes(0, 8, 20) == 0
    assert lib.mmpde_linear_skinny_workspace_bytes(3, 20, 512) == 0   # one chunk: never split


def test_segment_sum_refusals():
    """The header documents out[j, :] for n output rows of any width; the guard
    takes n > 0, width > 0 and four non-null pointers."""
    lib = _lib()

    def call(rows=P, width=3, off=P, edge=P, n=5, out=P):
        return lib.mmpde_segment_sum(rows, width, off, edge, n, out, None)

    for hole in ("rows", "off", "edge", "out"):
        assert call(**{hole: None}) == INVALID, hole
    assert call(n=0) == INVALID and call(n=-1) == INVALID and call(width=0) == INVALID
