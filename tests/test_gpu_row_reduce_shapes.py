"""The row reductions at their block and row-group edges, against float64
(cases and references: dense_cases.py; their CPU-side checks:
test_dense_cases.py): mmpde_segment_sum (the backward of ops.GatherRows; also
bitwise the sequential float32 sum in list order) and the BatchNorm rows
kernels mmpde_batch_norm_rows_train / _backward (256, 85, 8 and 1 row groups,
row counts around the 64-row blocks, fewer rows than row groups), through
ctypes on fenced buffers and through ops.GatherRows / ops.batch_norm_rows."""
import numpy as np
import pytest
import torch

import dense_cases as C

pytestmark = pytest.mark.gpu

WORST = {}


def _L():
    from mmpde_amd import _lib as L
    return L


# --------------------------------------------------------------------------- segment_sum
@pytest.mark.parametrize("idx", C.table("segsum"), ids=C.ids("segsum"))
def test_segment_sum(dev, idx):
    L = _L()
    c = C.build("segsum", idx)
    d = C.to_device(c, dev)

    def call(dd):
        L.check(L.lib().mmpde_segment_sum(C.ptr(c, dd, "rows"), c["width"], dd["off"].data_ptr(),
                                          dd["edge"].data_ptr(), c["n"], C.ptr(c, dd, "out"), L.stream(dev)),
                "mmpde_segment_sum")

    call(d)
    got = C.outputs(c, d)
    C.judge(c, got, record=WORST)
    o = c["at"]["out"]
    seq = torch.from_numpy(C.segsum_sequential(c)).reshape(-1)
    assert torch.equal(got["out"][o:o + seq.numel()].view(torch.int32), seq.view(torch.int32)), \
        (c["name"], "not the sequential float32 sum in list order")
    d2 = C.fresh_outputs(c, d, dev)
    call(d2)
    C.same_bits(c, C.outputs(c, d2), got, "second call differs")


@pytest.mark.parametrize("idx", [i for i in C.table("segsum") if C.SEGSUM[i][2] != "empty"],
                         ids=[n for n, i in zip(C.ids("segsum"), C.table("segsum")) if C.SEGSUM[i][2] != "empty"])
def test_gather_rows_backward(dev, idx):
    """GatherRows.apply(rows, idx).backward: every source row's gradient is the
    sum of its gathered rows' in index order (float32, bit for bit), within
    2e-5 of max|ref| of float64 index_add_; rows never gathered get 0."""
    from mmpde_amd.ops import GatherRows
    c = C.build("segsum", idx)
    n, width = c["n"], c["width"]
    g = torch.Generator().manual_seed(2000 + idx)
    src = torch.repeat_interleave(torch.arange(n), torch.tensor(c["lens"]))
    src = src[torch.randperm(src.numel(), generator=g)]
    rows = torch.randn(n, width, generator=g)
    dy = torch.randn(src.numel(), width, generator=g)
    ref = torch.zeros(n, width, dtype=torch.float64).index_add_(0, src, dy.double())
    seq = np.zeros((n, width), dtype=np.float32)
    dyn = dy.numpy()
    for q, j in enumerate(src.tolist()):
        seq[j] = (seq[j] + dyn[q]).astype(np.float32)
    grads = []
    for _ in range(2):
        r = rows.to(dev).requires_grad_()
        out = GatherRows.apply(r, src.to(dev), True)
        assert torch.equal(out.detach().cpu(), rows[src])
        (out * dy.to(dev)).sum().backward()
        grads.append(r.grad.cpu())
    err, scale = (grads[0].double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"GatherRows backward n={n} w={width} {c['pattern']}: max|err| {err:.3e} max|ref| {scale:.3e}")
    assert err <= 2e-5 * scale, (err, scale)
    assert torch.equal(grads[0].view(torch.int32), torch.from_numpy(seq).view(torch.int32))
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32)), "second call differs"


# --------------------------------------------------------------------------- BatchNorm rows
def run_bn(c, d, dev):
    L = _L()
    lib = L.lib()
    n, ch = c["n"], c["C"]
    nb = lib.mmpde_batch_norm_rows_workspace_bytes(n, ch) + 12 * ch
    stats = torch.empty(4 * ch, dtype=torch.float32, device=dev)
    ws = torch.full((nb // 4 + 16,), C.SENT, dtype=torch.float32, device=dev)
    st = L.stream(dev)
    L.check(lib.mmpde_batch_norm_rows_train(C.ptr(c, d, "x"), C.ptr(c, d, "res"), n, ch, C.ptr(c, d, "weight"),
                                            C.ptr(c, d, "bias"), C.BN_EPS, C.BN_FACTOR, C.ptr(c, d, "rm"),
                                            C.ptr(c, d, "rv"), C.ptr(c, d, "y"), stats.data_ptr(), ws.data_ptr(), nb,
                                            st), "mmpde_batch_norm_rows_train")
    L.check(lib.mmpde_batch_norm_rows_backward(C.ptr(c, d, "x"), C.ptr(c, d, "res"), C.ptr(c, d, "dy"), n, ch,
                                               C.ptr(c, d, "weight"), stats.data_ptr(), C.ptr(c, d, "dx"),
                                               C.ptr(c, d, "dw"), C.ptr(c, d, "db"), ws.data_ptr(), nb, st),
            "mmpde_batch_norm_rows_backward")
    torch.cuda.synchronize()
    assert bool((ws[nb // 4:] == C.SENT).all()), "written beyond the workspace"


def _module(c, dev, **kw):
    bn = torch.nn.BatchNorm1d(c["C"], eps=C.BN_EPS, affine=c["affine"], **kw)
    with torch.no_grad():
        if c["affine"]:
            bn.weight.copy_(C.flat(c, "weight", (c["C"],), torch.float32))
            bn.bias.copy_(C.flat(c, "bias", (c["C"],), torch.float32))
        if bn.track_running_stats:
            bn.running_mean.copy_(C.flat(c, "rm", (c["C"],), torch.float32))
            bn.running_var.copy_(C.flat(c, "rv", (c["C"],), torch.float32))
    return bn


@pytest.mark.parametrize("idx", C.table("bn"), ids=C.ids("bn"))
def test_batch_norm_rows(dev, idx):
    from mmpde_amd import ops
    c = C.build("bn", idx)
    n, ch = c["n"], c["C"]
    d = C.to_device(c, dev)
    run_bn(c, d, dev)
    got = C.outputs(c, d)
    C.judge(c, got, record=WORST)
    d2 = C.fresh_outputs(c, d, dev)
    run_bn(c, d2, dev)
    C.same_bits(c, C.outputs(c, d2), got, "second call differs")
    # nn.BatchNorm1d through ops.batch_norm_rows: the same bits, dres = dx
    bn = _module(c, dev, momentum=C.BN_FACTOR).to(dev).train()
    x = C.tensor(c, d, "x", (n, ch)).clone().requires_grad_()
    r = C.tensor(c, d, "res", (n, ch)).clone().requires_grad_() if c["res"] else None
    y = ops.batch_norm_rows(bn, x, r)
    (y * C.tensor(c, d, "dy", (n, ch))).sum().backward()
    d3 = C.fresh_outputs(c, d, dev)
    for name, t in (("y", y.detach()), ("rm", bn.running_mean), ("rv", bn.running_var), ("dx", x.grad)):
        C.tensor(c, d3, name, (t.numel(),)).copy_(t.reshape(-1))
    if c["affine"]:
        C.tensor(c, d3, "dw", (ch,)).copy_(bn.weight.grad)
        C.tensor(c, d3, "db", (ch,)).copy_(bn.bias.grad)
    C.same_bits(c, C.outputs(c, d3), got, "ops.batch_norm_rows differs from the entry points")
    assert int(bn.num_batches_tracked) == 1
    if c["res"]:
        assert torch.equal(r.grad, x.grad)


WRAPPER_CASES = [0, 4, 7, 9, 12, 14]          # every C, n = 2 ... 1000, with and without residual / affine


@pytest.mark.parametrize("idx", WRAPPER_CASES, ids=[C.ids("bn")[i] for i in WRAPPER_CASES])
def test_batch_norm_rows_without_running_stats(dev, idx):
    """track_running_stats=False: the batch statistics alone; y as with them, bit for bit."""
    from mmpde_amd import ops
    c = C.build("bn", idx)
    n, ch = c["n"], c["C"]
    d = C.to_device(c, dev)
    bn = _module(c, dev, track_running_stats=False).to(dev).train()
    assert bn.running_mean is None and bn.num_batches_tracked is None
    y = ops.batch_norm_rows(bn, C.tensor(c, d, "x", (n, ch)), C.tensor(c, d, "res", (n, ch)))
    ref = next(r for r in C.reference(c) if r["grp"] == "y")
    err, scale = (y.double().cpu().reshape(-1) - ref["values"].reshape(-1)).abs().max().item(), \
        ref["values"].abs().max().item()
    assert err <= 1e-5 * scale, (c["name"], err, scale)
    run_bn(c, d, dev)
    assert torch.equal(y.reshape(-1), C.tensor(c, d, "y", (n * ch,)))


@pytest.mark.parametrize("idx", WRAPPER_CASES, ids=[C.ids("bn")[i] for i in WRAPPER_CASES])
def test_batch_norm_rows_cumulative_momentum(dev, idx):
    """momentum=None: the factor is 1 / num_batches_tracked, 1 then 1/2 over two calls."""
    from mmpde_amd import ops
    c = C.build("bn", idx)
    n, ch = c["n"], c["C"]
    d = C.to_device(c, dev)
    bn = _module(c, dev, momentum=None).to(dev).train()
    ref = _module(c, dev, momentum=None).double().train()
    x, r = C.tensor(c, d, "x", (n, ch)), C.tensor(c, d, "res", (n, ch))
    for call in (1, 2):
        # the second batch: the first scaled and shifted (other statistics; 1.5 x - 1 keeps x = 2 where it is 2,
        # the channel without variance of the n = 2 cases)
        sx = x if call == 1 else x * 1.5 - 1.0
        y = ops.batch_norm_rows(bn, sx, r)
        yr = ref(sx.double().cpu() + (r.double().cpu() if c["res"] else 0.0))
        assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == call
        for name, got, want in (("y", y, yr), ("running_mean", bn.running_mean, ref.running_mean),
                                ("running_var", bn.running_var, ref.running_var)):
            err = (got.detach().double().cpu() - want.detach()).abs().max().item()
            scale = want.detach().abs().max().item()
            print(f"{c['name']} momentum=None call {call} {name}: max|err| {err:.3e} max|ref| {scale:.3e}")
            assert err <= 1e-5 * scale, (c["name"], call, name, err, scale)


def test_report_largest_errors(dev):
    """A record, not a bar."""
    for kind in sorted(WORST):
        print(f"{kind}: largest error {WORST[kind][0]:.2e} of max|ref| ({WORST[kind][1]})")
