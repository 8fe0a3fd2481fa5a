"""The kernels of csrc/dense.hip and csrc/smooth.hip at their block, slice,
chunk and lane edges, against float64 (cases and references: dense_cases.py;
their CPU-side checks: test_dense_cases.py): mmpde_conv2d_ex,
mmpde_conv2d_grad_weight (both instantiations, every slice count, the 64 KB
LDS limit), mmpde_resample_bilinear, mmpde_linear_skinny[_ws] on strided
operands, mmpde_outer_rows, mmpde_transpose, mmpde_tanh_bwd, mmpde_traj_mse
and mmpde_softmax_interp[_grad].

Every case: the entry point through ctypes on NaN-fenced inputs and
sentinel-fenced outputs, within the bar of dense_cases.py, no NaN from the
fences, every float outside the outputs bitwise untouched; the Python wrapper
on the same inputs gives the same bits."""
import pytest
import torch

import dense_cases as C

pytestmark = pytest.mark.gpu

CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
WORST = {}


def _L():
    from mmpde_amd import _lib as L
    return L


def _put(c, d, name, t):
    """A wrapper's result into the case's output buffer (its owned region is contiguous)."""
    C.tensor(c, d, name, tuple(t.shape)).copy_(t)


def _cases(kind):
    return pytest.mark.parametrize("idx", C.table(kind), ids=C.ids(kind))


# --------------------------------------------------------------------------- conv2d_ex
def run_conv(c, d, dev):
    L = _L()
    bt, cin, cout, h, w, ks, st, pad, circ, bias, act, res = c["p"]
    L.check(L.lib().mmpde_conv2d_ex(C.ptr(c, d, "x"), bt, cin, h, w, C.ptr(c, d, "w"), C.ptr(c, d, "bias"), cout, ks,
                                    st, pad, L.PAD_CIRCULAR if circ else L.PAD_ZEROS, C.ptr(c, d, "res"),
                                    int(res == "after"), act, C.ptr(c, d, "y"), L.stream(dev)), "mmpde_conv2d_ex")


@_cases("conv")
def test_conv2d_ex(dev, idx):
    from mmpde_amd import ops
    c = C.build("conv", idx)
    bt, cin, cout, h, w, ks, st, pad, circ, bias, act, res = c["p"]
    d = C.to_device(c, dev)
    run_conv(c, d, dev)
    got = C.outputs(c, d)
    C.judge(c, got, record=WORST)
    d2 = C.fresh_outputs(c, d, dev)
    y = ops.conv2d(C.tensor(c, d, "x", (bt, cin, h, w)), C.tensor(c, d, "w", (cout, cin, ks, ks)),
                   C.tensor(c, d, "bias", (cout,)), st, pad, act,
                   residual=C.tensor(c, d, "res", (bt, cout, c["oh"], c["ow"])), circular=circ,
                   res_after_act=res == "after")
    assert y.shape == (bt, cout, c["oh"], c["ow"])
    _put(c, d2, "y", y)
    C.same_bits(c, C.outputs(c, d2), got, "ops.conv2d differs from the entry point")


# --------------------------------------------------------------------------- conv2d_grad_weight
def run_gw(c, d, dev):
    L = _L()
    bt, cin, cout, h, w, ks, circ, db = c["p"]
    L.check(L.lib().mmpde_conv2d_grad_weight(C.ptr(c, d, "x"), bt, cin, h, w, C.ptr(c, d, "dy"), cout, ks, ks // 2,
                                             L.PAD_CIRCULAR if circ else L.PAD_ZEROS, C.ptr(c, d, "dw"),
                                             C.ptr(c, d, "db"), L.stream(dev)), "mmpde_conv2d_grad_weight")


@_cases("gw")
def test_conv2d_grad_weight(dev, idx):
    from mmpde_amd import ops
    c = C.build("gw", idx)
    bt, cin, cout, h, w, ks, circ, db = c["p"]
    d = C.to_device(c, dev)
    run_gw(c, d, dev)
    got = C.outputs(c, d)
    C.judge(c, got, record=WORST)
    d2 = C.fresh_outputs(c, d, dev)
    run_gw(c, d2, dev)
    C.same_bits(c, C.outputs(c, d2), got, "second call differs")
    d3 = C.fresh_outputs(c, d, dev)
    dw, gb = ops.conv2d_grad_weight(C.tensor(c, d, "x", (bt, cin, h, w)), C.tensor(c, d, "dy", (bt, cout, h, w)),
                                    ks, ks // 2, circ, bias=db)
    _put(c, d3, "dw", dw.reshape(-1))
    assert (gb is not None) == db
    if db:
        _put(c, d3, "db", gb)
    C.same_bits(c, C.outputs(c, d3), got, "ops.conv2d_grad_weight differs from the entry point")


@pytest.mark.parametrize("circular", [False, True])
def test_conv2d_same_autograd_on_the_global_path(dev, circular):
    """ops.Conv2dSame differentiated at 91 x 91 (planes beyond the LDS) against float64 autograd."""
    import torch.nn.functional as F

    from mmpde_amd.ops import Conv2dSame
    g = torch.Generator().manual_seed(91 + circular)
    x, w, b = torch.randn(2, 3, 91, 91, generator=g), torch.randn(2, 3, 5, 5, generator=g) / 75 ** 0.5, \
        torch.randn(2, generator=g)
    dy = torch.randn(2, 2, 91, 91, generator=g)
    assert not C.gw_form(91, 91, 5)[0]
    r = [t.double().requires_grad_() for t in (x, w, b)]
    xp = F.pad(r[0], (2,) * 4, mode="circular" if circular else "constant")
    yr = F.conv2d(xp, r[1], r[2])
    (yr * dy.double()).sum().backward()
    t = [v.to(dev).requires_grad_() for v in (x, w, b)]
    y = Conv2dSame.apply(t[0], t[1], t[2], circular)
    (y * dy.to(dev)).sum().backward()
    for name, got, ref, rel, abs_ in (("y", y, yr, 2e-5, 0.0), ("dx", t[0].grad, r[0].grad, 2e-5, 0.0),
                                     ("dw", t[1].grad, r[1].grad, 1e-5, 1e-6), ("db", t[2].grad, r[2].grad, 1e-5, 1e-6)):
        err = (got.detach().double().cpu() - ref.detach()).abs().max().item()
        scale = ref.detach().abs().max().item()
        print(f"Conv2dSame 91x91 circular={circular} {name}: max|err| {err:.3e} max|ref| {scale:.3e}")
        assert got.shape == ref.shape and err <= rel * scale + abs_, (name, err, scale)


# --------------------------------------------------------------------------- resample_bilinear
@_cases("resample")
def test_resample_bilinear(dev, idx):
    from mmpde_amd import ops
    L = _L()
    c = C.build("resample", idx)
    planes, h, w, oh, ow = c["p"]
    d = C.to_device(c, dev)
    L.check(L.lib().mmpde_resample_bilinear(C.ptr(c, d, "x"), planes, h, w, oh, ow, C.ptr(c, d, "y"), L.stream(dev)),
            "mmpde_resample_bilinear")
    got = C.outputs(c, d)
    C.judge(c, got, record=WORST)
    # torch's own CPU F.interpolate, to the same bar
    r = C.reference(c)[0]
    y = got["y"][r["off"]:r["off"] + r["cols"]]
    ref = C.resample_torch(c)
    err, scale = (y.double() - ref.double()).abs().max().item(), ref.abs().max().item()
    print(f"{c['name']} against F.interpolate: max|err| {err:.3e} max|ref| {scale:.3e}")
    assert err <= 5e-6 * scale + 1e-6, (c["name"], err, scale)
    d2 = C.fresh_outputs(c, d, dev)
    _put(c, d2, "y", ops.resample_bilinear(C.tensor(c, d, "x", (planes, h, w)), oh, ow).reshape(-1))
    C.same_bits(c, C.outputs(c, d2), got, "ops.resample_bilinear differs from the entry point")


# --------------------------------------------------------------------------- linear_skinny
@pytest.mark.parametrize("idx", C.table("skinny"), ids=C.ids("skinny"))
def test_linear_skinny_strided(dev, idx):
    from mmpde_amd import ops
    L = _L()
    lib = L.lib()
    c = C.build("skinny", idx)
    m, k, n = c["m"], c["k"], c["n"]
    d = C.to_device(c, dev)
    z = C.skinny_splits(n, k, CUS)
    wsb = lib.mmpde_linear_skinny_workspace_bytes(m, n, k)
    assert (wsb > 0) == (z > 1) and (z > 1) == ((m, k, n) != (3, 512, 20))

    def call(dd):
        if c["ops"]:
            x, w = C.view(dd["x"], c["at"]["x"], m, k, c["ldx"]), C.view(dd["w"], c["at"]["w"], n, k, c["ldw"])
            y = ops.linear_skinny(x, w, C.tensor(c, dd, "bias", (n,)), c["act"])
            C.view(dd["y"], c["at"]["y"], m, n, c["ldy"]).copy_(y)
            return None
        args = (C.ptr(c, dd, "x"), c["ldx"], m, k, C.ptr(c, dd, "w"), c["ldw"], C.ptr(c, dd, "bias"), n, c["act"],
                C.ptr(c, dd, "y"), c["ldy"])
        if not c["ws"]:
            L.check(lib.mmpde_linear_skinny(*args, L.stream(dev)), "mmpde_linear_skinny")
            return None
        ws = torch.zeros(wsb // 4 + 16, dtype=torch.float32, device=dev)
        ws[wsb // 4:] = C.SENT
        L.check(lib.mmpde_linear_skinny_ws(*args, ws.data_ptr(), wsb, L.stream(dev)), "mmpde_linear_skinny_ws")
        return ws

    ws = call(d)
    got = C.outputs(c, d)
    C.judge(c, got, record=WORST)
    if ws is not None:
        assert bool((ws[wsb // 4:] == C.SENT).all()), "written beyond the workspace"
        if wsb:
            assert int(ws[:4096].view(torch.int32).abs().sum()) == 0, "ticket words left non-zero"
    d2 = C.fresh_outputs(c, d, dev)
    call(d2)
    C.same_bits(c, C.outputs(c, d2), got, "second call differs")


# --------------------------------------------------------------------------- outer_rows / transpose / tanh_bwd
@_cases("outer")
def test_outer_rows(dev, idx):
    L = _L()
    c = C.build("outer", idx)
    d = C.to_device(c, dev)

    def call(dd):
        L.check(L.lib().mmpde_outer_rows(C.ptr(c, dd, "g"), c["ldg"], C.ptr(c, dd, "x"), c["ldx"], c["m"], c["n"],
                                         c["k"], C.ptr(c, dd, "dw"), c["lddw"], C.ptr(c, dd, "db"), L.stream(dev)),
                "mmpde_outer_rows")

    call(d)
    got = C.outputs(c, d)
    C.judge(c, got, record=WORST)
    d2 = C.fresh_outputs(c, d, dev)
    call(d2)
    C.same_bits(c, C.outputs(c, d2), got, "second call differs")


@_cases("transpose")
def test_transpose(dev, idx):
    L = _L()
    c = C.build("transpose", idx)
    d = C.to_device(c, dev)
    L.check(L.lib().mmpde_transpose(C.ptr(c, d, "x"), c["rows"], c["cols"], c["ldx"], C.ptr(c, d, "y"), c["ldy"],
                                    L.stream(dev)), "mmpde_transpose")
    C.judge(c, C.outputs(c, d), record=WORST)


@_cases("tanh")
def test_tanh_bwd_and_its_in_place_form(dev, idx):
    L = _L()
    c = C.build("tanh", idx)
    n = c["n"]
    d = C.to_device(c, dev)
    L.check(L.lib().mmpde_tanh_bwd(C.ptr(c, d, "dy"), C.ptr(c, d, "t"), n, C.ptr(c, d, "dz"), L.stream(dev)),
            "mmpde_tanh_bwd")
    got = C.outputs(c, d)
    C.judge(c, got, record=WORST)
    # dz is dy: the same bits, and the fence around dy untouched
    L.check(L.lib().mmpde_tanh_bwd(C.ptr(c, d, "dy"), C.ptr(c, d, "t"), n, C.ptr(c, d, "dy"), L.stream(dev)),
            "mmpde_tanh_bwd")
    torch.cuda.synchronize()
    after, before = d["dy"].cpu(), c["bufs"]["dy"]
    a, o = c["at"]["dy"], c["at"]["dz"]
    assert torch.equal(after[a:a + n].view(torch.int32), got["dz"][o:o + n].view(torch.int32))
    keep = torch.ones_like(before, dtype=torch.bool)
    keep[a:a + n] = False
    assert torch.equal(after[keep].view(torch.int32), before[keep].view(torch.int32))


def test_few_rows_mlp_backward_uses_them(dev):
    """ops.FewRowsMlp (mmpde_outer_rows, mmpde_transpose, mmpde_tanh_bwd in place behind the
    skinny forward) against float64 autograd at widths off the 16 / 32 / 64 tiles."""
    from mmpde_amd.ops import FewRowsMlp
    g = torch.Generator().manual_seed(77)
    widths = [130, 65, 33, 17]
    m = 33
    x = torch.randn(m, widths[0], generator=g)
    params = []
    for a, b in zip(widths, widths[1:]):
        params += [torch.randn(b, a, generator=g) / a ** 0.5, torch.randn(b, generator=g)]
    dy = torch.randn(m, widths[-1], generator=g)
    r = [t.double().requires_grad_() for t in [x] + params]
    h = r[0]
    for i in range(3):
        h = h @ r[1 + 2 * i].t() + r[2 + 2 * i]
        h = torch.tanh(h) if i < 2 else h
    (h * dy.double()).sum().backward()
    t = [v.to(dev).requires_grad_() for v in [x] + params]
    y = FewRowsMlp.apply(*t)
    (y * dy.to(dev)).sum().backward()
    for i, (got, ref) in enumerate(zip([y] + [v.grad for v in t], [h] + [v.grad for v in r])):
        err = (got.detach().double().cpu() - ref.detach()).abs().max().item()
        scale = ref.detach().abs().max().item()
        print(f"FewRowsMlp output {i}: max|err| {err:.3e} max|ref| {scale:.3e}")
        assert got.shape == ref.shape and err <= 1e-5 * scale, (i, err, scale)


# --------------------------------------------------------------------------- traj_mse
@_cases("mse")
def test_traj_mse_alone_and_in_a_batch(dev, idx):
    from mmpde_amd import dist
    L = _L()
    c = C.build("mse", idx)
    bt, n_per = c["bt"], c["n_per"]
    d = C.to_device(c, dev)
    L.check(L.lib().mmpde_traj_mse(C.ptr(c, d, "pred"), C.ptr(c, d, "lab"), bt, n_per, C.ptr(c, d, "out"),
                                   L.stream(dev)), "mmpde_traj_mse")
    got = C.outputs(c, d)
    C.judge(c, got, record=WORST)
    # each trajectory launched alone: the bits it has inside the batch
    d2 = C.fresh_outputs(c, d, dev)
    for i in range(bt):
        L.check(L.lib().mmpde_traj_mse(C.ptr(c, d2, "pred", i * n_per), C.ptr(c, d2, "lab", i * n_per), 1, n_per,
                                       C.ptr(c, d2, "out", i), L.stream(dev)), "mmpde_traj_mse")
    C.same_bits(c, C.outputs(c, d2), got, "a trajectory alone differs from the batch")
    d3 = C.fresh_outputs(c, d, dev)
    _put(c, d3, "out", dist.per_trajectory_mse(C.tensor(c, d, "pred", (bt, n_per)), C.tensor(c, d, "lab", (bt, n_per)),
                                               bt))
    C.same_bits(c, C.outputs(c, d3), got, "dist.per_trajectory_mse differs from the entry point")


# --------------------------------------------------------------------------- softmax_interp
@_cases("smooth")
def test_softmax_interp_and_grad(dev, idx):
    from mmpde_amd.dmm_train import SoftmaxInterp
    L = _L()
    lib = L.lib()
    c = C.build("smooth", idx)
    n_pts, n_q, ps, vs = c["n_pts"], c["n_q"], c["ps"], c["vs"]
    d = C.to_device(c, dev)
    head = (C.ptr(c, d, "pts"), n_pts, ps, C.ptr(c, d, "vals"), vs, C.ptr(c, d, "qry"), n_q, c["scale"])
    L.check(lib.mmpde_softmax_interp(*head, C.ptr(c, d, "out"), L.stream(dev)), "mmpde_softmax_interp")
    L.check(lib.mmpde_softmax_interp_grad(*head, C.ptr(c, d, "g"), C.ptr(c, d, "gq"), L.stream(dev)),
            "mmpde_softmax_interp_grad")
    got = C.outputs(c, d)
    C.judge(c, got, record=WORST)
    d2 = C.fresh_outputs(c, d, dev)
    q = C.tensor(c, d, "qry", (n_q, 2)).clone().requires_grad_()
    out = SoftmaxInterp.apply(C.tensor(c, d, "pts", (ps, n_pts, 2)), C.tensor(c, d, "vals", (vs, n_pts)), q, c["scale"])
    (out * C.tensor(c, d, "g", (n_q,))).sum().backward()
    _put(c, d2, "out", out.detach())
    _put(c, d2, "gq", q.grad.reshape(-1))
    C.same_bits(c, C.outputs(c, d2), got, "SoftmaxInterp differs from the entry points")


def test_report_largest_errors(dev):
    """A record, not a bar."""
    for kind in sorted(WORST):
        print(f"{kind}: largest error {WORST[kind][0]:.2e} of max|ref| ({WORST[kind][1]})")
