"""mmpde_batch_norm_rows_train_segments (train-mode BatchNorm over S row segments,
each a batch of its own) at the smallest shapes where the segment arithmetic can
go wrong, through ctypes on fenced buffers (as dense_cases.py fences them: inputs
inside NaN, outputs and the workspace inside a sentinel that must come back
bitwise, the workspace fenced at the byte count the library reports).

Asserted per case: y, stats and the running statistics are bitwise those of S
consecutive mmpde_batch_norm_rows_train calls on the segments; a second call on
a workspace of 0xFF bytes repeats the bits of the first on a zeroed one; y and
the running statistics are within dense_cases.py's BatchNorm bar (1e-5 of
max|ref|) of a float64 evaluation per segment; where S = 3, segment 1 computed
alone has its bits of the batch.

Inputs: x = 2 + randn and the residual 0.5 randn, as dense_cases.py.  With
n <= 3 rows the sum x + res is instead built from multiples of 1/16 whose rows
are at least 0.5 apart in every channel: dense_cases.BN_NOTES explains why a
channel of two nearly equal rows cannot be held to that bar in float32."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import dense_cases as C

pytestmark = pytest.mark.gpu

EPS, FACTOR = C.BN_EPS, C.BN_FACTOR
FRONT, BACK = 4, 8                       # floats of fence in front of and behind every tensor (16-byte multiples)
TAIL = 64                                # fence bytes behind the workspace

# (S, n, C)
SHAPES = [(1, 2, 4), (3, 2, 4), (4, 3, 12),            # small segments
          (2, 255, 4), (2, 256, 4), (2, 257, 4),       # around a 256-row workgroup
          (5, 2521, 4),                                # the cylinder mesh's segment length
          (150, 37, 4),                                # many short segments, n no multiple of anything
          (3, 65, 128),                                # 8 row groups, the segment not a multiple of them
          (2, 64, 1024)]                               # one row group
FORMS = list(itertools.product((True, False), repeat=3))   # (residual, affine, running statistics)


def _id(shape, form):
    return "S{}-n{}-C{}-{}-{}-{}".format(*shape, "res" if form[0] else "nores", "affine" if form[1] else "plain",
                                         "running" if form[2] else "norunning")


CASES = [(s, f) for s in SHAPES for f in FORMS]


def _inputs(S, n, ch, res, affine, running):
    g = torch.Generator().manual_seed(7000 + 131 * S + 17 * n + ch)
    rows = S * n
    r = 0.5 * torch.randn(rows, ch, generator=g)
    if n <= 3:
        r = torch.round(16 * r) / 16
        v = torch.round(16 * torch.randn(S, 1, ch, generator=g)) / 16 + C.BN_OFFSET
        gap = 0.5 + torch.round(16 * torch.randn(S, n, ch, generator=g).abs()) / 16
        sign = torch.where(torch.randn(S, 1, ch, generator=g) > 0, 1.0, -1.0)
        v = (v + sign * torch.cumsum(gap, dim=1)).reshape(rows, ch)
        x = v - r if res else v
    else:
        x = C.BN_OFFSET + torch.randn(rows, ch, generator=g)
    d = dict(x=x.float(), res=r.float() if res else None)
    d["weight"] = 1.0 + 0.1 * torch.randn(ch, generator=g) if affine else None
    d["bias"] = 0.1 * torch.randn(ch, generator=g) if affine else None
    d["rm"] = 0.1 * torch.randn(ch, generator=g) if running else None
    d["rv"] = 1.0 + 0.1 * torch.rand(ch, generator=g) if running else None
    return d


class Fenced:
    """A float32 tensor on the device inside FRONT / BACK floats of `fill`."""

    def __init__(self, values, numel, fill, dev):
        flat = torch.full((FRONT + numel + BACK,), fill, dtype=torch.float32)
        if values is not None:
            flat[FRONT:FRONT + numel] = values.reshape(-1)
        self.fence = torch.full((1,), fill, dtype=torch.float32).view(torch.int32).item()
        self.numel = numel
        self.flat = flat.to(dev)

    def ptr(self, offset=0):
        return self.flat.data_ptr() + 4 * (FRONT + offset)

    def body(self):
        return self.flat[FRONT:FRONT + self.numel].cpu()

    def check(self, what):
        bits = self.flat.view(torch.int32).cpu()
        assert bool((bits[:FRONT] == self.fence).all()) and bool((bits[FRONT + self.numel:] == self.fence).all()), \
            f"{what}: written outside the tensor"


def _device_inputs(d, dev):
    """x, res, weight, bias inside NaN (None stays None)."""
    return {k: (Fenced(d[k], d[k].numel(), C.NAN, dev) if d[k] is not None else None)
            for k in ("x", "res", "weight", "bias")}


def _outputs(d, rows, ch, S, dev):
    """y, stats inside the sentinel; the running statistics hold their old values inside it."""
    o = dict(y=Fenced(None, rows * ch, C.SENT, dev), stats=Fenced(None, S * 4 * ch, C.SENT, dev))
    for k in ("rm", "rv"):
        o[k] = Fenced(d[k], ch, C.SENT, dev) if d[k] is not None else None
    return o


def _p(f, offset=0):
    return f.ptr(offset) if f is not None else None


def _read(o):
    return {k: (v.body() if v is not None else None) for k, v in o.items()}


def run_segments(d, S, n, ch, dev, ws_byte):
    """One call of the segmented entry; the workspace pre-filled with ws_byte."""
    from mmpde_amd import _lib as L
    lib = L.lib()
    rows = S * n
    i, o = _device_inputs(d, dev), _outputs(d, rows, ch, S, dev)
    nb = lib.mmpde_batch_norm_rows_train_segments_workspace_bytes(S, n, ch)
    assert nb > 0 and nb % 16 == 0
    ws = torch.full((nb + TAIL,), ws_byte, dtype=torch.uint8, device=dev)
    ws[nb:] = 0xA5
    assert ws.data_ptr() % 16 == 0
    L.check(lib.mmpde_batch_norm_rows_train_segments(
        _p(i["x"]), _p(i["res"]), S, n, ch, _p(i["weight"]), _p(i["bias"]), EPS, FACTOR, _p(o["rm"]), _p(o["rv"]),
        _p(o["y"]), _p(o["stats"]), ws.data_ptr(), nb, L.stream(dev)), "mmpde_batch_norm_rows_train_segments")
    torch.cuda.synchronize()
    assert bool((ws[nb:] == 0xA5).all()), "written beyond the workspace size the library reports"
    for k, f in list(i.items()) + list(o.items()):
        if f is not None:
            f.check(k)
    return _read(o)


def run_sequential(d, S, n, ch, dev):
    """S calls of mmpde_batch_norm_rows_train, segment after segment, on the same buffers."""
    from mmpde_amd import _lib as L
    lib = L.lib()
    i, o = _device_inputs(d, dev), _outputs(d, S * n, ch, S, dev)
    nb = lib.mmpde_batch_norm_rows_workspace_bytes(n, ch)
    ws = torch.zeros((nb // 4,), dtype=torch.float32, device=dev)
    for s in range(S):
        off = s * n * ch
        L.check(lib.mmpde_batch_norm_rows_train(
            _p(i["x"], off), _p(i["res"], off), n, ch, _p(i["weight"]), _p(i["bias"]), EPS, FACTOR, _p(o["rm"]),
            _p(o["rv"]), _p(o["y"], off), _p(o["stats"], s * 4 * ch), ws.data_ptr(), nb, L.stream(dev)),
            "mmpde_batch_norm_rows_train")
    torch.cuda.synchronize()
    return _read(o)


def reference(d, S, n, ch):
    """float64, segment after segment: F.batch_norm in training mode."""
    f64 = {k: (v.double() if v is not None else None) for k, v in d.items()}
    v = f64["x"] + f64["res"] if f64["res"] is not None else f64["x"]
    rm, rv = (f64["rm"].clone(), f64["rv"].clone()) if f64["rm"] is not None else (None, None)
    y = torch.cat([F.batch_norm(v[s * n:(s + 1) * n], rm, rv, f64["weight"], f64["bias"], training=True,
                                momentum=FACTOR, eps=EPS) for s in range(S)])
    return dict(y=y.reshape(-1), rm=rm, rv=rv)


def _same(a, b, what):
    for k in a:
        if a[k] is None:
            assert b[k] is None
            continue
        x, y = a[k].view(torch.int32), b[k].view(torch.int32)
        bad = (x != y).nonzero().reshape(-1)
        assert bad.numel() == 0, f"{what}: {k} differs in {bad.numel()} of {x.numel()} words, first at {int(bad[0])}"


@pytest.mark.parametrize("shape,form", CASES, ids=[_id(s, f) for s, f in CASES])
def test_segments(dev, shape, form):
    S, n, ch = shape
    res, affine, running = form
    d = _inputs(S, n, ch, res, affine, running)
    got = run_segments(d, S, n, ch, dev, 0x00)
    _same(got, run_sequential(d, S, n, ch, dev), "against S calls of mmpde_batch_norm_rows_train")
    _same(run_segments(d, S, n, ch, dev, 0xFF), got, "second call, the workspace 0xFF bytes")
    ref = reference(d, S, n, ch)
    for k in ("y", "rm", "rv"):
        if ref[k] is None:
            continue
        err = (got[k].double() - ref[k]).abs().max().item()
        scale = ref[k].abs().max().item()
        print(f"{_id(shape, form)} {k}: max|err| {err:.3e} bar {1e-5 * scale:.3e} max|ref| {scale:.3e}")
        assert err <= 1e-5 * scale, (k, err, scale)
    if S == 3:   # segment 1 alone: its y and its row of stats as in the batch
        one = {k: (t[n:2 * n] if k in ("x", "res") and t is not None else t) for k, t in d.items()}
        alone = run_segments(one, 1, n, ch, dev, 0x00)
        assert torch.equal(alone["y"].view(torch.int32), got["y"][n * ch:2 * n * ch].view(torch.int32)), \
            "segment 1 alone: y differs from its rows of the batch"
        assert torch.equal(alone["stats"].view(torch.int32), got["stats"][4 * ch:8 * ch].view(torch.int32)), \
            "segment 1 alone: stats differ from row 1 of the batch"


def test_wrapper_segments(dev):
    """ops.batch_norm_rows(segments=S) against S calls of ops.batch_norm_rows on
    the segments: the same bits in y and in the running statistics,
    num_batches_tracked advanced by S; an input that requires grad, rows that do
    not divide into the segments and segments < 1 raise."""
    from mmpde_amd import ops
    S, n, ch = 3, 65, 128
    d = _inputs(S, n, ch, True, True, True)

    def module():
        bn = torch.nn.BatchNorm1d(ch, eps=EPS, momentum=FACTOR)
        with torch.no_grad():
            bn.weight.copy_(d["weight"])
            bn.bias.copy_(d["bias"])
            bn.running_mean.copy_(d["rm"])
            bn.running_var.copy_(d["rv"])
        return bn.to(dev).train()

    x, r = d["x"].to(dev), d["res"].to(dev)
    a, b = module(), module()
    with torch.no_grad():
        ya = ops.batch_norm_rows(a, x, r, segments=S)
        yb = torch.cat([ops.batch_norm_rows(b, x[s * n:(s + 1) * n], r[s * n:(s + 1) * n]) for s in range(S)])
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32))
    assert torch.equal(a.running_mean.view(torch.int32), b.running_mean.view(torch.int32))
    assert torch.equal(a.running_var.view(torch.int32), b.running_var.view(torch.int32))
    assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == S
    with pytest.raises(ValueError):
        ops.batch_norm_rows(a, x.clone().requires_grad_(), r, segments=S)
    with pytest.raises(ValueError):
        ops.batch_norm_rows(a, x, r, segments=S)          # grad enabled: the module's parameters require grad
    with torch.no_grad():
        with pytest.raises(ValueError):
            ops.batch_norm_rows(a, x[:-1], r[:-1], segments=S)
        with pytest.raises(ValueError):
            ops.batch_norm_rows(a, x, r, segments=0)
        # momentum=None: a factor per segment, the per-segment calls
        c, e = module(), module()
        c.momentum = e.momentum = None
        yc = ops.batch_norm_rows(c, x, r, segments=S)
        ye = torch.cat([ops.batch_norm_rows(e, x[s * n:(s + 1) * n], r[s * n:(s + 1) * n]) for s in range(S)])
    assert torch.equal(yc.view(torch.int32), ye.view(torch.int32))
    assert torch.equal(c.running_var.view(torch.int32), e.running_var.view(torch.int32))
    assert int(c.num_batches_tracked) == S
    assert int(a.num_batches_tracked) == S                # the refused calls advanced nothing
