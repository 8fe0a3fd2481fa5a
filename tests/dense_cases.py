"""Inputs and float64 references of the dense, smoother and row-reduction shape
tests (test_gpu_dense_shapes.py and test_gpu_row_reduce_shapes.py on the
device, test_dense_cases.py on the CPU alone): the kernels of csrc/dense.hip
(mmpde_conv2d_ex, mmpde_conv2d_grad_weight, mmpde_resample_bilinear,
mmpde_linear_skinny[_ws], mmpde_outer_rows, mmpde_transpose, mmpde_tanh_bwd,
mmpde_traj_mse), csrc/smooth.hip (mmpde_softmax_interp[_grad]),
mmpde_segment_sum (csrc/edge_bwd.hip) and the BatchNorm rows kernels of
csrc/train_rows.hip, at their block, slice, chunk and row-group edges.

A case is a dict: `bufs` (name -> flat fp32 CPU tensor, never modified), `at`
(name -> offset in floats of the tensor inside its buffer), `ibufs` (int64
index lists) and the call's shape.  Every input tensor sits in a buffer that
is NaN in front of it, behind it and in every stride pad; every output buffer
is SENT (an accumulating output: its old values) and what the call does not
own must come back bitwise unchanged.  The references are the formulas of
include/mmpde_hip.h in torch float64 (float32 for the CPU floor check).

Bars (rel of max|ref| + abs), each the bar the project already uses:
conv2d 2e-5; conv2d_grad_weight 1e-5 + 1e-6; resample_bilinear 5e-6 + 1e-6;
linear_skinny 1e-6 (1 + max|ref|) max(1, sqrt(k / 512)); BatchNorm y and
running statistics 1e-5, gradients 2e-5; softmax interp 1e-5 + 1e-7, its VJP
2e-5 + 1e-6; outer_rows 1e-5; traj_mse 1e-5 of each trajectory's value;
tanh_bwd 1e-6; segment_sum 2e-5 (and bitwise the sequential float32 sum);
transpose bitwise.  test_dense_cases.py holds the float32 evaluation of every
reference to a quarter of its bar.

What was changed to fit that quarter (the bars were not): the grad-weight
reference adds tap by tap as a matrix product (gw_reference), and the
BatchNorm inputs at n = 2 (BN_NOTES).  The smoother cases fit as listed
(SMOOTH_NOTES).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

SENT = 777.125
NAN = float("nan")
FLOOR_SHARE = 0.25                   # the fp32 CPU evaluation must stay within this share of the bar
SIGNAL_FLOOR = 1e-3                  # max|ref| of every judged group is at least this (or exactly 0)
SENSITIVITY = 10.0                   # one wrong element moves the float64 result by this many bars

ACT = {0: lambda v: v, 1: torch.tanh, 2: torch.relu, 3: F.elu}


# --------------------------------------------------------------------------- buffers
def view(flat, off, nrows, ncols, ld):
    return flat.as_strided((nrows, ncols), (ld, 1), off)


class Bufs:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.t, self.at = {}, {}

    def randn(self, *shape, scale=1.0):
        return torch.randn(*shape, generator=self.g) * scale

    def _alloc(self, name, nrows, ld, front, fill):
        self.t[name] = torch.full((front + (nrows + 1) * ld + 8,), fill, dtype=torch.float32)
        self.at[name] = front

    def inp(self, name, values, ld=None, front=4):
        """values [rows, cols] (or any shape, taken as one contiguous row) inside NaN."""
        v = values.reshape(1, -1) if (ld is None or values.dim() != 2) else values
        ld = ld or v.shape[1]
        self._alloc(name, v.shape[0], ld, front, NAN)
        view(self.t[name], front, v.shape[0], v.shape[1], ld).copy_(v)

    def out(self, name, nrows, ncols, ld=None, front=4, old=None):
        ld = ld or ncols
        self._alloc(name, nrows, ld, front, SENT)
        if old is not None:
            view(self.t[name], front, nrows, ncols, ld).copy_(old)


def case(kind, name, b, **kw):
    return dict(kind=kind, name=name, bufs=b.t, at=b.at, ibufs={}, **kw)


def _t(c, name, nrows, ncols, ld, dtype):
    return view(c["bufs"][name], c["at"][name], nrows, ncols, ld).to(dtype)


def _flat(c, name, shape, dtype):
    n = math.prod(shape)
    return c["bufs"][name][c["at"][name]:c["at"][name] + n].to(dtype).reshape(shape)


flat = _flat


def region(c, name, values, rel, abs_=0.0, grp=None, ld=None, exact=False, extra=0):
    """An output the call owns: values [rows, cols] float64 at c.at[name] + extra."""
    v = values.reshape(1, -1) if (ld is None or values.dim() != 2) else values
    return dict(buf=name, off=c["at"][name] + extra, rows=v.shape[0], cols=v.shape[1], ld=ld or v.shape[1],
                values=v, rel=rel, abs=abs_, grp=grp or name, exact=exact)


# --------------------------------------------------------------------------- conv2d_ex
# (batches, cin, cout, h, w, ks, stride, pad, circular, bias, act, residual)
CONV = [
    (3, 3, 5, 13, 11, 5, 1, 2, True, True, 3, "after"),       # the suite's one earlier case
    (1, 6, 6, 13, 11, 3, 2, 1, False, False, 2, "before"),
    (3, 3, 5, 13, 11, 3, 2, 1, True, True, 1, None),
    (3, 1, 1, 13, 11, 5, 1, 0, False, False, 0, None),
    (1, 3, 5, 13, 11, 1, 1, 0, True, True, 3, "before"),
    (1, 1, 1, 12, 10, 5, 2, 2, False, True, 0, None),
    (3, 3, 5, 12, 10, 3, 1, 2, False, True, 3, "after"),      # pad = ks/2 + 1
    (1, 6, 6, 12, 10, 1, 1, 0, False, True, 1, None),
    (3, 3, 5, 12, 10, 1, 2, 0, False, False, 2, None),
    (1, 3, 5, 12, 10, 1, 1, 1, False, True, 0, "before"),     # ks 1, pad = ks/2 + 1
    (1, 6, 6, 12, 10, 5, 1, 2, True, True, 2, "after"),
    (3, 6, 6, 12, 10, 3, 2, 1, True, False, 1, "before"),
    (1, 6, 6, 12, 10, 1, 1, 0, True, True, 0, None),
    (1, 1, 1, 7, 7, 3, 1, 0, False, True, 0, None),
    (3, 6, 6, 7, 7, 5, 1, 3, False, True, 1, "before"),       # pad = ks/2 + 1
    (1, 3, 5, 7, 7, 5, 2, 2, True, False, 2, "after"),
    (3, 6, 6, 7, 7, 3, 1, 1, True, True, 0, "before"),
    (1, 3, 5, 7, 7, 1, 2, 0, True, True, 3, None),
    (3, 3, 5, 2, 2, 5, 1, 2, True, True, 3, None),            # circular, pad == h == w
    (1, 1, 1, 2, 2, 5, 2, 2, True, True, 0, None),            # ... and stride 2: one output
    (3, 6, 6, 2, 2, 3, 1, 1, False, True, 2, "before"),
    (1, 3, 5, 2, 2, 1, 2, 0, False, False, 1, None),
    (1, 3, 5, 2, 2, 3, 1, 2, False, True, 0, "after"),        # pad = ks/2 + 1
    (3, 3, 5, 1, 5, 3, 1, 1, True, True, 1, "after"),         # circular, pad == h
    (1, 1, 1, 1, 5, 1, 1, 0, True, False, 0, None),
    (1, 6, 6, 1, 5, 3, 2, 1, False, True, 2, None),
    (1, 3, 5, 1, 5, 5, 1, 2, False, True, 3, "before"),       # rows of taps that see padding only
    (3, 1, 1, 1, 5, 5, 1, 3, False, True, 0, None),           # pad = ks/2 + 1
]


def conv_out(h, w, ks, stride, pad):
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


def conv_name(p):
    bt, cin, cout, h, w, ks, st, pad, circ, bias, act, res = p
    return f"conv-{h}x{w}-b{bt}-c{cin}to{cout}-k{ks}-s{st}-p{pad}-{'circ' if circ else 'zero'}-" \
           f"{'bias' if bias else 'nobias'}-act{act}-res{res}"


def conv_case(idx):
    p = CONV[idx]
    bt, cin, cout, h, w, ks, st, pad, circ, bias, act, res = p
    b = Bufs(100 + idx)
    oh, ow = conv_out(h, w, ks, st, pad)
    b.inp("x", b.randn(bt, cin, h, w))
    b.inp("w", b.randn(cout, cin, ks, ks, scale=(cin * ks * ks) ** -0.5), front=5)
    if bias:
        b.inp("bias", b.randn(cout), front=3)
    if res:
        b.inp("res", b.randn(bt, cout, oh, ow))
    b.out("y", 1, bt * cout * oh * ow, front=7)
    return case("conv", conv_name(p), b, p=p, oh=oh, ow=ow)


def conv_reference(c, dtype=torch.float64):
    bt, cin, cout, h, w, ks, st, pad, circ, bias, act, res = c["p"]
    x = _flat(c, "x", (bt, cin, h, w), dtype)
    if pad:
        x = F.pad(x, (pad,) * 4, mode="circular" if circ else "constant")
    y = F.conv2d(x, _flat(c, "w", (cout, cin, ks, ks), dtype), _flat(c, "bias", (cout,), dtype) if bias else None,
                 stride=st)
    assert y.shape == (bt, cout, c["oh"], c["ow"])
    if res == "before":
        y = y + _flat(c, "res", y.shape, dtype)
    y = ACT[act](y)
    if res == "after":
        y = _flat(c, "res", y.shape, dtype) + y
    return [region(c, "y", y, 2e-5)]


def conv_mutant(c):
    """The centre tap of the last output channel (first input channel) zeroed."""
    bt, cin, cout, h, w, ks, st, pad, circ, bias, act, res = c["p"]
    m = _clone(c)
    o = c["at"]["w"] + ((cout - 1) * cin * ks + ks // 2) * ks + ks // 2
    m["bufs"]["w"][o] = 0.0
    return m, ["y"]


# --------------------------------------------------------------------------- conv2d_grad_weight
GW_THREADS = 256
# (batches, cin, cout, h, w, ks, circular, db)
GW = [
    (1, 1, 1, 2, 2, 1, False, True),          # 256 slices, four pixels
    (3, 3, 2, 2, 2, 1, True, True),
    (3, 3, 2, 1, 1, 3, True, True),           # every tap wraps onto the one pixel
    (1, 1, 1, 1, 1, 3, False, False),
    (3, 3, 2, 12, 10, 1, False, False),
    (1, 1, 1, 12, 10, 3, True, True),
    (3, 3, 2, 12, 10, 5, False, True),
    (1, 3, 2, 12, 10, 7, True, True),
    (3, 1, 1, 12, 10, 9, False, False),
    (1, 3, 2, 12, 10, 15, True, True),
    (3, 1, 1, 12, 10, 15, False, True),
    (3, 3, 2, 64, 128, 3, True, True),        # 8192 pixels: the LDS path at its 64 KB limit
    (1, 1, 1, 64, 128, 15, False, True),
    (1, 3, 2, 64, 128, 7, False, False),
    (3, 3, 2, 91, 91, 5, False, True),        # 8281 pixels: the global path
    (1, 1, 1, 91, 91, 9, True, False),
    (3, 1, 1, 91, 91, 1, True, True),
    (1, 3, 2, 91, 91, 15, True, True),
]


def gw_form(h, w, ks):
    """(LDS instantiation?, slices per tap) as mmpde_conv2d_grad_weight picks them."""
    return 2 * h * w * 4 <= 64 * 1024, GW_THREADS // (ks * ks)


def gw_name(p):
    bt, cin, cout, h, w, ks, circ, db = p
    return f"gw-{h}x{w}-b{bt}-c{cin}to{cout}-k{ks}-{'circ' if circ else 'zero'}-{'db' if db else 'nodb'}"


def gw_case(idx):
    p = GW[idx]
    bt, cin, cout, h, w, ks, circ, db = p
    b = Bufs(200 + idx)
    b.inp("x", b.randn(bt, cin, h, w))
    b.inp("dy", b.randn(bt, cout, h, w), front=5)
    b.out("dw", 1, cout * cin * ks * ks, front=3)
    if db:
        b.out("db", 1, cout, front=6)
    return case("gw", gw_name(p), b, p=p)


def gw_reference(c, dtype=torch.float64):
    """dw[co, ci, ky, kx] = sum dy[b, co, y, x] xpad[b, ci, y + ky, x + kx]; db = sum dy."""
    bt, cin, cout, h, w, ks, circ, db = c["p"]
    pad = ks // 2
    x, dy = _flat(c, "x", (bt, cin, h, w), dtype), _flat(c, "dy", (bt, cout, h, w), dtype)
    if pad:
        x = F.pad(x, (pad,) * 4, mode="circular" if circ else "constant")
    # tap by tap as one matrix product over (batch, pixel): F.conv2d with the
    # plane as its kernel adds 24576 float32 products one after the other and
    # alone comes to 3e-6 of max|ref| (the kernel adds per slice, then the slices)
    dyf = dy.transpose(0, 1).reshape(cout, bt * h * w)
    dw = torch.empty(cout, cin, ks, ks, dtype=dtype)
    for ky in range(ks):
        for kx in range(ks):
            xs = x[:, :, ky:ky + h, kx:kx + w].transpose(0, 1).reshape(cin, bt * h * w)
            dw[:, :, ky, kx] = dyf @ xs.t()
    out = [region(c, "dw", dw, 1e-5, 1e-6)]
    if db:
        out.append(region(c, "db", dy.sum((0, 2, 3)), 1e-5, 1e-6))
    return out


def gw_mutant(c):
    """One x pixel (last batch, first channel, where |dy| of channel 0 is largest) moved by 4."""
    bt, cin, cout, h, w, ks, circ, db = c["p"]
    m = _clone(c)
    dy = _flat(c, "dy", (bt, cout, h * w), torch.float64)
    pix = int(dy[bt - 1, 0].abs().argmax())
    m["bufs"]["x"][c["at"]["x"] + (bt - 1) * cin * h * w + pix] += 4.0
    return m, ["dw"]


# --------------------------------------------------------------------------- resample_bilinear
# (planes, h, w, oh, ow)
RESAMPLE = [(3, 48, 48, 48, 48), (5, 7, 5, 3, 9), (1, 5, 1, 4, 4), (5, 1, 6, 3, 3), (1, 7, 5, 1, 1),
            (5, 48, 48, 1, 1), (3, 48, 48, 1, 7), (5, 13, 11, 17, 19), (1, 1, 1, 3, 2)]


def resample_case(idx):
    p = RESAMPLE[idx]
    b = Bufs(300 + idx)
    b.inp("x", b.randn(p[0], p[1], p[2]))
    b.out("y", 1, p[0] * p[3] * p[4], front=5)
    return case("resample", "resample-p{}-{}x{}-to-{}x{}".format(*p), b, p=p)


def _coords(n_in, n_out):
    """PyTorch's align_corners=True source coordinates, formed in fp32."""
    f32 = np.float32
    sc = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    cc = np.array([f32(sc * f32(i)) for i in range(n_out)], dtype=np.float32)
    i0 = cc.astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = (cc - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, lam, (f32(1) - lam).astype(np.float32)


def resample_reference(c, dtype=torch.float64):
    """The step-by-step restatement of upsample_bilinear2d: fp32 coordinates and
    lambdas, the blend hy (hx a + lx b) + ly (hx c + lx d) in `dtype`."""
    planes, h, w, oh, ow = c["p"]
    x = _flat(c, "x", (planes, h, w), dtype)
    y0, y1, ly, hy = _coords(h, oh)
    x0, x1, lx, hx = _coords(w, ow)
    ly, hy = (torch.from_numpy(v).to(dtype)[:, None] for v in (ly, hy))
    lx, hx = (torch.from_numpy(v).to(dtype) for v in (lx, hx))
    a, bb = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    cc, d = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    y = hy * (hx * a + lx * bb) + ly * (hx * cc + lx * d)
    return [region(c, "y", y, 5e-6, 1e-6, exact=(h, w) == (oh, ow))]


def resample_torch(c):
    planes, h, w, oh, ow = c["p"]
    x = _flat(c, "x", (planes, 1, h, w), torch.float32)
    return F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=True).reshape(-1)


def resample_mutant(c):
    m = _clone(c)
    m["bufs"]["x"][c["at"]["x"]] += 1.0                   # the corner pixel: output (0, 0) of plane 0 is it
    return m, ["y"]


# --------------------------------------------------------------------------- linear_skinny
SK_CHUNK, SK_MAXZ = 512, 16
SKINNY_SHAPES = [(3, 512, 20), (17, 513, 17), (2, 2048, 40)]
# (strided, bias, act, workspace, through ops)
SKINNY_FORMS = [(True, True, 1, True, False), (True, False, 0, True, False), (True, True, 2, False, False),
                (False, True, 1, True, True)]


def skinny_splits(n, k, cus):
    """The K splits of mmpde_linear_skinny_ws with a workspace (1 without)."""
    ctiles, chunks = (n + 15) // 16, (k + SK_CHUNK - 1) // SK_CHUNK
    z = max(1, min((4 * cus + ctiles - 1) // ctiles, chunks, SK_MAXZ))
    if z > 1:
        nchz = (chunks + z - 1) // z
        z = (chunks + nchz - 1) // nchz
    return z


def skinny_case(si, fi):
    (m, k, n), (strided, bias, act, ws, ops) = SKINNY_SHAPES[si], SKINNY_FORMS[fi]
    b = Bufs(400 + 10 * si + fi)
    ldx, ldw, ldy = (k + 3, k + 5, n + 7) if strided else (k, k, n)
    b.inp("x", b.randn(m, k), ld=ldx)
    b.inp("w", b.randn(n, k, scale=0.02), ld=ldw, front=5)
    if bias:
        b.inp("bias", b.randn(n), front=3)
    b.out("y", m, n, ld=ldy, front=4 if ops else 6)
    name = f"skinny-m{m}-k{k}-n{n}-{'strided' if strided else 'tight'}-{'bias' if bias else 'nobias'}-act{act}-" \
           f"{'ws' if ws else 'nows'}"
    return case("skinny", name, b, m=m, k=k, n=n, ldx=ldx, ldw=ldw, ldy=ldy, bias=bias, act=act, ws=ws, ops=ops)


def skinny_reference(c, dtype=torch.float64):
    m, k, n = c["m"], c["k"], c["n"]
    y = _t(c, "x", m, k, c["ldx"], dtype) @ _t(c, "w", n, k, c["ldw"], dtype).t()
    if c["bias"]:
        y = y + _flat(c, "bias", (n,), dtype)
    y = ACT[c["act"]](y)
    f = 1e-6 * max(1.0, math.sqrt(k / 512))               # _bound of test_gpu_dense.py
    return [region(c, "y", y, f, f, ld=c["ldy"])]


def skinny_mutant(c):
    """One weight (column n - 1, the last k) moved by 0.02: one weight's scale."""
    m = _clone(c)
    m["bufs"]["w"][c["at"]["w"] + (c["n"] - 1) * c["ldw"] + c["k"] - 1] += 0.02
    return m, ["y"]


# --------------------------------------------------------------------------- outer_rows
# (m, n, k, db): the diagonal of the three lists, then off-diagonal triples
OUTER = [(1, 1, 1, True), (31, 15, 3, True), (32, 16, 63, False), (33, 17, 64, True), (70, 40, 65, True),
         (70, 1, 130, True), (1, 40, 130, False), (33, 16, 1, True), (32, 17, 130, True), (31, 40, 64, False),
         (70, 15, 63, True), (33, 1, 65, True)]


def _odd(v):
    return v | 1


def outer_case(idx):
    m, n, k, db = OUTER[idx]
    b = Bufs(500 + idx)
    ldg, ldx, lddw = _odd(n + 2), _odd(k + 4), _odd(k + 2)
    b.inp("g", b.randn(m, n), ld=ldg)
    b.inp("x", b.randn(m, k), ld=ldx, front=5)
    b.out("dw", n, k, ld=lddw, front=3)
    if db:
        b.out("db", 1, n, front=6)
    return case("outer", f"outer-m{m}-n{n}-k{k}-{'db' if db else 'nodb'}", b, m=m, n=n, k=k, db=db, ldg=ldg,
                ldx=ldx, lddw=lddw)


def outer_reference(c, dtype=torch.float64):
    g, x = _t(c, "g", c["m"], c["n"], c["ldg"], dtype), _t(c, "x", c["m"], c["k"], c["ldx"], dtype)
    out = [region(c, "dw", g.t() @ x, 1e-5, ld=c["lddw"])]
    if c["db"]:
        out.append(region(c, "db", g.sum(0), 1e-5))
    return out


def outer_mutant(c):
    """The last row's last x moved by 1 (a row of the second 32-row pass where there is one)."""
    m = _clone(c)
    m["bufs"]["x"][c["at"]["x"] + (c["m"] - 1) * c["ldx"] + c["k"] - 1] += 1.0
    return m, ["dw"]


# --------------------------------------------------------------------------- transpose
TRANSPOSE = [(1, 1), (31, 33), (32, 32), (33, 31), (70, 1), (1, 70), (70, 70), (32, 33), (31, 70), (33, 32)]


def transpose_case(idx):
    rows, cols = TRANSPOSE[idx]
    b = Bufs(600 + idx)
    b.inp("x", b.randn(rows, cols), ld=cols + 3, front=5)
    b.out("y", cols, rows, ld=rows + 5, front=3)
    return case("transpose", f"transpose-{rows}x{cols}", b, rows=rows, cols=cols, ldx=cols + 3, ldy=rows + 5)


def transpose_reference(c, dtype=torch.float64):
    x = _t(c, "x", c["rows"], c["cols"], c["ldx"], dtype)
    return [region(c, "y", x.t().contiguous(), 0.0, ld=c["ldy"], exact=True)]


# --------------------------------------------------------------------------- tanh_bwd
TANH_N = [1, 255, 256, 257]


def tanh_case(idx):
    n = TANH_N[idx]
    b = Bufs(700 + idx)
    b.inp("dy", b.randn(n))
    b.inp("t", torch.tanh(b.randn(n, scale=1.5)), front=5)
    b.out("dz", 1, n, front=3)
    return case("tanh", f"tanh_bwd-n{n}", b, n=n)


def tanh_reference(c, dtype=torch.float64):
    t = _flat(c, "t", (c["n"],), dtype)
    return [region(c, "dz", _flat(c, "dy", (c["n"],), dtype) * (1 - t * t), 1e-6)]


def tanh_mutant(c):
    m = _clone(c)
    m["bufs"]["dy"][c["at"]["dy"] + c["n"] - 1] += 1.0
    return m, ["dz"]


# --------------------------------------------------------------------------- traj_mse
MSE = [(bt, n_per) for n_per in (1, 255, 256, 257, 2521) for bt in (1, 3)]


def mse_case(idx):
    bt, n_per = MSE[idx]
    b = Bufs(800 + idx)
    lab = b.randn(bt, n_per)
    b.inp("lab", lab, front=5)
    b.inp("pred", lab + b.randn(bt, n_per, scale=0.1))
    b.out("out", 1, bt, front=3)
    return case("mse", f"traj_mse-b{bt}-n{n_per}", b, bt=bt, n_per=n_per)


def mse_reference(c, dtype=torch.float64):
    """Each trajectory's loss is judged against its own value (a relative bar)."""
    d = _flat(c, "pred", (c["bt"], c["n_per"]), dtype) - _flat(c, "lab", (c["bt"], c["n_per"]), dtype)
    v = (d * d).mean(1)
    return [region(c, "out", v[i:i + 1], 1e-5, grp=f"out{i}", extra=i) for i in range(c["bt"])]


def mse_mutant(c):
    m = _clone(c)
    m["bufs"]["pred"][c["at"]["pred"] + c["bt"] * c["n_per"] - 1] += 1.0
    return m, [f"out{c['bt'] - 1}"]


# --------------------------------------------------------------------------- softmax_interp
SMOOTH_NPTS = [1, 63, 64, 65, 200]
SMOOTH_NQ = [1, 3, 4, 5, 12]
SMOOTH_SETS = [("1", "S"), ("S", "S"), ("S", "1")]        # (pts_sets, val_sets) where 3 divides n_q
SMOOTH_NOTES = """Queries lie up to 0.1 outside the unit square and the scales are 1, sqrt(n_pts) and
48 as listed; the points are drawn uniformly in the square.  Values are randn."""


def smooth_table():
    t = []
    for i, n_pts in enumerate(SMOOTH_NPTS):
        for j, n_q in enumerate(SMOOTH_NQ):
            sets = SMOOTH_SETS[(i + j // 2) % 3] if n_q % 3 == 0 else ("1", "1")
            scale = ("one", "sqrt", "48")[(i + 2 * j) % 3]
            t.append((n_pts, n_q, sets, scale))
    return t


SMOOTH = smooth_table()


def smooth_case(idx):
    n_pts, n_q, sets, sc = SMOOTH[idx]
    ps, vs = (3 if s == "S" else 1 for s in sets)
    scale = {"one": 1.0, "sqrt": float(np.float32(math.sqrt(n_pts))), "48": 48.0}[sc]
    b = Bufs(900 + idx)
    pts = torch.rand(ps, n_pts, 2, generator=b.g)
    qry = torch.rand(n_q, 2, generator=b.g) * 1.2 - 0.1
    planted = []
    if n_pts >= 2:
        # two points on one horizontal line in every set; the last query exactly
        # on the first, the one before it (if any) on their bisector
        pts[:, 0] = torch.tensor([0.25, 0.5])
        pts[:, 1] = torch.tensor([0.75, 0.5])
        qry[n_q - 1] = pts[ps - 1, 0]
        planted.append("on-point")
        if n_q >= 2:
            qry[n_q - 2] = torch.tensor([0.5, 0.375])
            planted.append("equidistant")
    b.inp("pts", pts)
    b.inp("vals", b.randn(vs, n_pts), front=5)
    b.inp("qry", qry, front=6)
    b.inp("g", b.randn(n_q), front=3)
    b.out("out", 1, n_q, front=5)
    b.out("gq", 1, 2 * n_q, front=6)
    name = f"smooth-p{n_pts}-q{n_q}-sets{ps}x{vs}-scale{sc}"
    return case("smooth", name, b, n_pts=n_pts, n_q=n_q, ps=ps, vs=vs, scale=scale, planted=planted)


def smooth_reference(c, dtype=torch.float64):
    """The dense softmax, differentiated by autograd (torch.norm: 0 at a coinciding point)."""
    n_pts, n_q, ps, vs = c["n_pts"], c["n_q"], c["ps"], c["vs"]
    pts = _flat(c, "pts", (ps, n_pts, 2), dtype).repeat_interleave(n_q // ps, 0)     # [n_q, n_pts, 2]
    vals = _flat(c, "vals", (vs, n_pts), dtype).repeat_interleave(n_q // vs, 0)
    q = _flat(c, "qry", (n_q, 2), dtype).clone().requires_grad_(True)
    d = torch.norm(q[:, None, :] - pts, dim=-1)
    out = (torch.softmax(-c["scale"] * d, dim=1) * vals).sum(1)
    (out * _flat(c, "g", (n_q,), dtype)).sum().backward()
    one = n_pts == 1                                       # the value itself; a zero gradient
    return [region(c, "out", out.detach(), 1e-5, 1e-7, exact=one),
            region(c, "gq", torch.zeros_like(q.grad) if one else q.grad, 2e-5, 1e-6, exact=one)]


def smooth_mutant(c):
    """The value of the point nearest to query 0 (in its value set: set 0) moved by 1."""
    m = _clone(c)
    pts = _flat(c, "pts", (c["ps"], c["n_pts"], 2), torch.float64)[0]
    q0 = _flat(c, "qry", (c["n_q"], 2), torch.float64)[0]
    j = int(torch.norm(pts - q0, dim=-1).argmin())
    m["bufs"]["vals"][c["at"]["vals"] + j] += 1.0
    return m, ["out"] if c["n_pts"] == 1 else ["out", "gq"]


# --------------------------------------------------------------------------- segment_sum
# (sources, width, pattern)
SEGSUM = [(1, 1, "single"), (1, 3, "empty"), (1, 257, "hub"), (5, 1, "mixed"), (5, 3, "mixed"), (5, 30, "hub"),
          (5, 128, "empty"), (5, 257, "mixed"), (300, 1, "rand"), (300, 3, "hub"), (300, 30, "rand"),
          (300, 128, "rand"), (300, 257, "rand")]
HUB = 1000
SEG_ROWS = 64                                              # rows of the summed table; 7 of them never referenced


def segsum_case(idx):
    n, width, pattern = SEGSUM[idx]
    b = Bufs(1000 + idx)
    g = b.g
    live = SEG_ROWS - 7

    def draw(cnt):
        return torch.randint(0, live, (cnt,), generator=g)

    if pattern == "empty":
        lens = [0] * n
    elif pattern == "single":
        lens = [1] * n
    elif pattern == "hub":
        lens = [int(v) for v in torch.randint(0, 4, (n,), generator=g)]
        lens[n // 2] = HUB
    elif pattern == "mixed":                               # empty, single, a hub, short lists
        lens = ([0, 1, HUB, 3, 0] * ((n + 4) // 5))[:n]
    else:
        lens = [int(v) for v in torch.randint(0, 6, (n,), generator=g)]
        lens[0], lens[-1] = 0, 0
    off = torch.zeros(n + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int64), 0)
    edge = draw(int(off[-1])) if int(off[-1]) else torch.zeros(0, dtype=torch.int64)
    if edge.numel() >= 2:
        edge[1] = edge[0]                                  # an index that repeats inside one list
    b.inp("rows", b.randn(SEG_ROWS, width))
    b.out("out", n, width, front=5)
    c = case("segsum", f"segsum-n{n}-w{width}-{pattern}", b, n=n, width=width, pattern=pattern, lens=lens)
    # the index lists: 8 entries of -(2^40) behind what the call may read
    c["ibufs"] = dict(off=off, edge=torch.cat((edge, torch.full((8,), -(2 ** 40), dtype=torch.int64))))
    return c


def segsum_reference(c, dtype=torch.float64):
    rows = _t(c, "rows", SEG_ROWS, c["width"], c["width"], dtype)
    off, edge = c["ibufs"]["off"], c["ibufs"]["edge"]
    out = torch.zeros(c["n"], c["width"], dtype=dtype)
    if dtype == torch.float32:
        out = torch.from_numpy(segsum_sequential(c))
    else:
        seg = torch.repeat_interleave(torch.arange(c["n"]), off[1:] - off[:-1])
        out.index_add_(0, seg, rows[edge[:int(off[-1])]])
    return [region(c, "out", out, 2e-5)]


def segsum_sequential(c):
    """numpy.float32 accumulation in list order: what the kernel computes, bit for bit."""
    rows = _t(c, "rows", SEG_ROWS, c["width"], c["width"], torch.float32).numpy()
    off, edge = c["ibufs"]["off"].numpy(), c["ibufs"]["edge"].numpy()
    out = np.zeros((c["n"], c["width"]), dtype=np.float32)
    for j in range(c["n"]):
        acc = np.zeros(c["width"], dtype=np.float32)
        for q in range(off[j], off[j + 1]):
            acc = (acc + rows[edge[q]]).astype(np.float32)
        out[j] = acc
    return out


def segsum_mutant(c):
    """The first entry of the longest list left out (its row set to 0 there: the list points at a zero row)."""
    m = _clone(c)
    j = int(np.argmax(c["lens"]))
    q = int(c["ibufs"]["off"][j])
    m["ibufs"] = dict(c["ibufs"], edge=c["ibufs"]["edge"].clone())
    m["bufs"]["rows"][m["at"]["rows"] + (SEG_ROWS - 1) * c["width"]:][:c["width"]] = 0.0
    m["ibufs"]["edge"][q] = SEG_ROWS - 1                   # a row no list references
    return m, ["out"]


# --------------------------------------------------------------------------- BatchNorm rows
# (n, C, residual, affine): every n and every C at least twice
BN = [(2, 4, True, True), (3, 12, False, True), (63, 128, True, False), (64, 1024, False, True),
      (65, 4, False, False), (129, 12, True, True), (1000, 128, False, True), (2, 1024, True, True),
      (3, 128, False, False), (63, 4, True, True), (64, 12, False, True), (65, 1024, True, False),
      (129, 128, True, True), (1000, 4, True, True), (1000, 12, False, False), (129, 1024, False, True),
      (64, 4, True, False)]
BN_EPS, BN_FACTOR, BN_OFFSET = 1e-5, 0.1, 2.0
BN_NOTES = """x = 2.0 + randn (the mean offset of test_gpu_train_rows.py), the residual 0.5 randn.
Changed for n = 2, to fit the quarter and the signal floor with the offset kept:
two rows 2 d apart give y = +-d / sqrt(d^2 + eps) and an input gradient that
cancels down to eps / (d^2 + eps) of its terms.  y = v a + c with c = bias -
mean a (the kernel's form and torch's own on the CPU) carries 2^-24 |mean| a,
which at the smallest d of 1024 randn channels is 3e-5 of max|y| (bar 1e-5);
and max|dx| of four randn channels is 1e-4 of cancelling terms of size 1.  So
at n = 2 x and the residual are multiples of 1/16 (x + res and the mean are
exact in float32), the rows are at least 0.5 apart in every channel but 0, and
in channel 0 x = 2, res = -2 in both rows: the one channel with no variance
and no mean, where dx = (dy0 - dy1) / (2 sqrt(eps)) does not cancel and gives
the input gradient its scale.  Both n = 2 cases carry a residual."""


def bn_row_groups(C):
    """Row groups of a workgroup of bn_stats_partial_kernel / bn_bwd_partial_kernel."""
    return 256 // (C // 4)


def bn_case(idx):
    n, C, res, affine = BN[idx]
    b = Bufs(1100 + idx)
    x, r = BN_OFFSET + b.randn(n, C), b.randn(n, C, scale=0.5)
    if n == 2:                                             # BN_NOTES
        x, r = BN_OFFSET + torch.round(16 * (x - BN_OFFSET)) / 16, torch.round(16 * r) / 16
        gap = 0.5 + torch.round(16 * b.randn(C).abs()) / 16
        x[1] = x[0] + r[0] - r[1] + torch.where(b.randn(C) > 0, gap, -gap)
        x[:, 0], r[:, 0] = BN_OFFSET, -BN_OFFSET
    b.inp("x", x)
    if res:
        b.inp("res", r)
    if affine:
        b.inp("weight", 1.0 + b.randn(C, scale=0.1))
        b.inp("bias", b.randn(C, scale=0.1))
    b.inp("dy", b.randn(n, C))
    b.out("rm", 1, C, old=b.randn(C, scale=0.1))
    b.out("rv", 1, C, old=1.0 + 0.1 * torch.rand(C, generator=b.g))
    b.out("y", 1, n * C)
    b.out("dx", 1, n * C)
    if affine:
        b.out("dw", 1, C)
        b.out("db", 1, C)
    return case("bn", f"bn-n{n}-C{C}-{'res' if res else 'nores'}-{'affine' if affine else 'plain'}", b, n=n, C=C,
                res=res, affine=affine)


def bn_reference(c, dtype=torch.float64, skip_last_row=False):
    """F.batch_norm in training mode with autograd; dx is dres as well.
    skip_last_row: the statistics of rows [0, n - 1) applied to every row (the mutant)."""
    n, C = c["n"], c["C"]
    x = _flat(c, "x", (n, C), dtype).requires_grad_(True)
    v = x + _flat(c, "res", (n, C), dtype) if c["res"] else x
    w = _flat(c, "weight", (C,), dtype).requires_grad_(True) if c["affine"] else None
    bb = _flat(c, "bias", (C,), dtype).requires_grad_(True) if c["affine"] else None
    rm, rv = _flat(c, "rm", (C,), dtype).clone(), _flat(c, "rv", (C,), dtype).clone()
    if skip_last_row:
        mean, var = v[:-1].mean(0), v[:-1].var(0, unbiased=False)
        y = (v - mean) / torch.sqrt(var + BN_EPS)
        return [region(c, "y", (y * w + bb if c["affine"] else y).detach(), 1e-5)]
    y = F.batch_norm(v, rm, rv, w, bb, training=True, momentum=BN_FACTOR, eps=BN_EPS)
    (y * _flat(c, "dy", (n, C), dtype)).sum().backward()
    out = [region(c, "y", y.detach(), 1e-5), region(c, "rm", rm, 1e-5), region(c, "rv", rv, 1e-5),
           region(c, "dx", x.grad, 2e-5)]
    if c["affine"]:
        out += [region(c, "dw", w.grad, 2e-5), region(c, "db", bb.grad, 2e-5)]
    return out


# --------------------------------------------------------------------------- tables and judging
def _clone(c):
    m = dict(c, bufs={k: v.clone() for k, v in c["bufs"].items()})
    m.pop("_ref64", None)
    return m


KINDS = {
    "conv": (CONV, conv_case, conv_reference, conv_mutant),
    "gw": (GW, gw_case, gw_reference, gw_mutant),
    "resample": (RESAMPLE, resample_case, resample_reference, resample_mutant),
    "outer": (OUTER, outer_case, outer_reference, outer_mutant),
    "transpose": (TRANSPOSE, transpose_case, transpose_reference, None),
    "tanh": (TANH_N, tanh_case, tanh_reference, tanh_mutant),
    "mse": (MSE, mse_case, mse_reference, mse_mutant),
    "smooth": (SMOOTH, smooth_case, smooth_reference, smooth_mutant),
    "segsum": (SEGSUM, segsum_case, segsum_reference, segsum_mutant),
    "bn": (BN, bn_case, bn_reference, None),
}


@functools.lru_cache(maxsize=4)
def build(kind, idx):
    if kind == "skinny":
        c = skinny_case(*idx)
    else:
        c = KINDS[kind][1](idx)
    for flat in c["bufs"].values():
        assert flat.data_ptr() % 16 == 0
    return c


def table(kind):
    """The indices of a kind's cases."""
    if kind == "skinny":
        return [(si, fi) for si in range(len(SKINNY_SHAPES)) for fi in range(len(SKINNY_FORMS))]
    return list(range(len(KINDS[kind][0])))


def ids(kind):
    return [build(kind, i)["name"] for i in table(kind)]


ALL_KINDS = list(KINDS) + ["skinny"]


def reference(c, dtype=torch.float64):
    """The regions the call owns with their values; the float64 ones are computed once per case."""
    fn = skinny_reference if c["kind"] == "skinny" else KINDS[c["kind"]][2]
    if dtype != torch.float64:
        return fn(c, dtype)
    if "_ref64" not in c:
        c["_ref64"] = fn(c, dtype)
    return c["_ref64"]


def mutant(c):
    fn = skinny_mutant if c["kind"] == "skinny" else KINDS[c["kind"]][3]
    return fn(c) if fn else None


def owned(c, regions):
    """name -> bool mask of the floats of each output buffer the call owns."""
    m = {}
    for r in regions:
        own = m.setdefault(r["buf"], torch.zeros_like(c["bufs"][r["buf"]], dtype=torch.bool))
        view(own, r["off"], r["rows"], r["cols"], r["ld"]).fill_(True)
    return m


def scales(regions):
    s = {}
    for r in regions:
        s[r["grp"]] = max(s.get(r["grp"], 0.0), r["values"].abs().max().item() if r["values"].numel() else 0.0)
    return s


def bars(regions):
    """grp -> the absolute bar: rel max|ref| + abs."""
    s = scales(regions)
    return {r["grp"]: r["rel"] * s[r["grp"]] + r["abs"] for r in regions}


def judge(c, got, share=1.0, record=None):
    """got: name -> flat fp32 CPU tensor of every output buffer after the call.
    Asserts the bars (times share), the bitwise outputs, no NaN, and every float
    the call does not own bitwise as it was.  Returns the largest error as a
    share of max|ref|."""
    regions = reference(c)
    for name, own in owned(c, regions).items():
        before, after = c["bufs"][name], got[name]
        assert torch.equal(after[~own].view(torch.int32), before[~own].view(torch.int32)), \
            (c["name"], name, "a float outside the output was written")
    s, bar = scales(regions), bars(regions)
    worst = 0.0
    for r in regions:
        y = view(got[r["buf"]], r["off"], r["rows"], r["cols"], r["ld"])
        assert not torch.isnan(y).any(), (c["name"], r["grp"], "NaN let through")
        if r["exact"]:
            assert torch.equal(y.view(torch.int32), r["values"].float().view(torch.int32)), \
                (c["name"], r["grp"], "not bitwise the reference")
            continue
        err = (y.double() - r["values"]).abs().max().item() if y.numel() else 0.0
        scale = s[r["grp"]]
        if bar[r["grp"]] == 0.0:
            assert err == 0.0 and not (y != 0).any(), (c["name"], r["grp"], "not an exact zero", err)
            continue
        print(f"{c['name']} {r['grp']}: max|err| {err:.3e} max|ref| {scale:.3e} bar {bar[r['grp']]:.3e}")
        assert err <= share * bar[r["grp"]], (c["name"], r["grp"], err, scale, bar[r["grp"]])
        if scale > 0:
            worst = max(worst, err / scale)
    if record is not None:
        record[c["kind"]] = max(record.get(c["kind"], (0.0, "")), (worst, c["name"]))
    return worst


# --------------------------------------------------------------------------- the device side's plumbing (torch only)
def to_device(c, dev):
    d = {name: t.to(dev) for name, t in c["bufs"].items()}
    d.update({name: t.to(dev) for name, t in c["ibufs"].items()})
    return d


def ptr(c, d, name, extra=0):
    """The device address of a case tensor (None where the case has none)."""
    return d[name].data_ptr() + 4 * (c["at"][name] + extra) if name in c["at"] else None


def tensor(c, d, name, shape):
    """A contiguous case tensor as a view of its fenced device buffer."""
    return d[name][c["at"][name]:c["at"][name] + math.prod(shape)].view(shape) if name in c["at"] else None


def outputs(c, d):
    torch.cuda.synchronize()
    return {name: d[name].cpu() for name in owned(c, reference(c))}


def fresh_outputs(c, d, dev):
    return dict(d, **{name: c["bufs"][name].to(dev) for name in owned(c, reference(c))})


def same_bits(c, a, b, what):
    for name in a:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), (c["name"], name, what)


def evaluate_fp32(c):
    """The outputs as torch float32 arithmetic on the CPU gives them."""
    got = {name: c["bufs"][name].clone() for name in owned(c, reference(c))}
    for r in reference(c, torch.float32):
        view(got[r["buf"]], r["off"], r["rows"], r["cols"], r["ld"]).copy_(r["values"].float())
    return got
