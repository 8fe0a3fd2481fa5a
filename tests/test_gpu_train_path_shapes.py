"""The Conv1d head (csrc/head_train.hip), the skinny weight gradient and the
reverse adjacency (csrc/train_rows.hip) at their block, row-group and key-bit
edges, against float64 / the host construction, through ctypes on fenced
buffers (cases and references: train_path_cases.py; their CPU-side checks:
test_train_path_cases.py).

Bars (the project's): head y and dL/dh 2e-5 of max|ref|, its six weight / bias
gradients 5e-5 each; mmpde_rows_grad_weight 2e-5; the reverse adjacency bit for
bit.  Every call twice: the same bits.  Workspaces are fenced at the byte
counts the library reports."""
import functools

import pytest
import torch

import train_path_cases as T

pytestmark = pytest.mark.gpu

D = T.D
H = T.H
WORST = {}


def _L():
    from mmpde_amd import _lib as L
    return L


def _record(kind, worst, name):
    WORST[kind] = max(WORST.get(kind, (0.0, "")), (worst, name))


def _bits(t):
    return t.view(torch.int32)


# --------------------------------------------------------------------------- head
def _head_run(c, dev):
    """name -> flat fp32 CPU tensors of y, dh (its whole fenced buffer) and the 525 gradients."""
    L = _L()
    lib = L.lib()
    n = c["n"]
    d = {x: t.to(dev) for x, t in c["bufs"].items()}
    win = [T.fenced_in(t) for t in c["w"]]
    w = [t.to(dev) for t in win]
    dy_in = T.fenced_in(c["dy"])
    dy = dy_in.to(dev)
    y, grads = T.fenced_out(n).to(dev), T.fenced_out(T.HEAD_GRADS).to(dev)
    nb = lib.mmpde_head_train_workspace_bytes(n)
    assert nb == (n + 63) // 64 * T.HEAD_GRADS * 4
    ws = torch.full((nb // 4 + 16,), T.SENT, dtype=torch.float32, device=dev)
    wp = [t.data_ptr() + 4 * T.FRONT for t in w]
    hp, dhp = D.ptr(c, d, "h"), D.ptr(c, d, "dh")
    st = L.stream(dev)
    L.check(lib.mmpde_head_train_forward(hp, c["ldh"], n, *wp, y.data_ptr() + 4 * T.FRONT, st),
            "mmpde_head_train_forward")
    L.check(lib.mmpde_head_train_backward(hp, c["ldh"], n, *wp, dy.data_ptr() + 4 * T.FRONT, dhp, c["lddh"],
                                          grads.data_ptr() + 4 * T.FRONT, ws.data_ptr(), nb, st),
            "mmpde_head_train_backward")
    torch.cuda.synchronize()
    assert bool((ws[nb // 4:] == T.SENT).all()), "written beyond the workspace"
    assert not torch.isnan(ws[:nb // 4]).any() and bool((ws[:nb // 4] != T.SENT).any())
    assert torch.equal(_bits(d["h"].cpu()), _bits(c["bufs"]["h"])) and torch.equal(_bits(dy.cpu()), _bits(dy_in))
    for a, b in zip(w, win):
        assert torch.equal(_bits(a.cpu()), _bits(b)), "a weight was written"
    return dict(y=y.cpu(), dh=d["dh"].cpu(), grads=grads.cpu())


def _head_judge(c, out):
    n, ref = c["n"], c["ref"]
    assert T.fence_intact(out["y"], n) and T.fence_intact(out["grads"], T.HEAD_GRADS), (c["name"], "fence written")
    own = torch.zeros_like(out["dh"], dtype=torch.bool)
    D.view(own, c["at"]["dh"], n, H, c["lddh"]).fill_(True)
    assert torch.equal(_bits(out["dh"][~own]), _bits(c["bufs"]["dh"][~own])), (c["name"], "dh: a pad was written")
    got = [("y", T.inside(out["y"], n), ref["y"], T.HEAD_Y_BAR),
           ("dh", D.view(out["dh"], c["at"]["dh"], n, H, c["lddh"]), ref["dh"], T.HEAD_Y_BAR)]
    parts, rparts = T.head_parts(T.inside(out["grads"], T.HEAD_GRADS)), T.head_parts(ref["grads"])
    got += [("d" + name, parts[name], rparts[name], T.HEAD_GRAD_BAR) for name in T.HEAD_LAYOUT]
    worst = 0.0
    for what, y, r, bar in got:
        assert not torch.isnan(y).any(), (c["name"], what, "NaN")
        e, s = T.errs(y, r)[0], r.abs().max().item()
        print(f"head {c['name']} {what}: max|err| {e:.3e} max|ref| {s:.3e} bar {bar * s:.3e}")
        assert e <= bar * s, (c["name"], what, e, s)
        worst = max(worst, e / s if s > 0 else 0.0)
    _record("head", worst, c["name"])


@pytest.mark.parametrize("p", T.head_table(), ids=[T.head_name(p) for p in T.head_table()])
def test_head_train(dev, p):
    c = T.head_case(*p)
    out = _head_run(c, dev)
    _head_judge(c, out)
    again = _head_run(c, dev)
    for x in out:
        assert torch.equal(_bits(out[x]), _bits(again[x])), (c["name"], x, "second call differs")


def test_head_train_wrapper_equals_entry_points(dev):
    """ops.HeadTrain at n = 65: the raw calls' bits."""
    from mmpde_amd import ops
    c = T.head_case(65, 128, 128, False)
    out = _head_run(c, dev)
    h = c["h"].to(dev).requires_grad_()
    w = [t.to(dev).requires_grad_() for t in c["w"]]
    y = ops.HeadTrain.apply(h, *w)
    y.backward(c["dy"].to(dev)[:, None])
    torch.cuda.synchronize()
    assert torch.equal(y.detach().cpu().reshape(-1), T.inside(out["y"], 65))
    assert torch.equal(h.grad.cpu(), D.view(out["dh"], c["at"]["dh"], 65, H, 128))
    parts = T.head_parts(T.inside(out["grads"], T.HEAD_GRADS))
    for name, t in zip(T.HEAD_LAYOUT, w):
        assert torch.equal(t.grad.cpu().reshape(-1), parts[name]), name


# --------------------------------------------------------------------------- skinny weight gradient
@functools.lru_cache(maxsize=None)
def _cus(dev_index):
    return torch.cuda.get_device_properties(dev_index).multi_processor_count


def _rgw_names():
    return [p["name"].replace(str(16 * 4 * 256 + 17), "cap") for p in T.rgw_table(256)]


def _rgw_run(c, dev):
    L = _L()
    lib = L.lib()
    d = {x: t.to(dev) for x, t in c["bufs"].items()}
    nb = lib.mmpde_rows_grad_weight_workspace_bytes(c["rows"], c["k"], c["n_out"])
    ws = torch.full((nb // 4 + 16,), T.SENT, dtype=torch.float32, device=dev)
    L.check(lib.mmpde_rows_grad_weight(D.ptr(c, d, "x"), c["ldx"], c["rows"], c["k"], D.ptr(c, d, "dy"), c["ldy"],
                                       c["n_out"], D.ptr(c, d, "dw"), D.ptr(c, d, "db"), ws.data_ptr(), nb,
                                       L.stream(dev)), "mmpde_rows_grad_weight")
    torch.cuda.synchronize()
    assert bool((ws[nb // 4:] == T.SENT).all()), "written beyond the workspace"
    for x in ("x", "dy"):
        if x in d:
            assert torch.equal(_bits(d[x].cpu()), _bits(c["bufs"][x])), (x, "an input was written")
    return {x: d[x].cpu() for x in ("dw", "db") if x in d}


def _rgw_judge(c, out):
    worst = 0.0
    res = {}
    for x, shape in (("dw", (c["n_out"], c["k"])), ("db", (1, c["n_out"]))):
        if x not in out:
            continue
        numel = shape[0] * shape[1]
        at = c["at"][x]
        own = torch.zeros_like(out[x], dtype=torch.bool)
        own[at:at + numel] = True
        assert torch.equal(_bits(out[x][~own]), _bits(c["bufs"][x][~own])), (c["name"], x, "fence written")
        y, r = out[x][at:at + numel].reshape(shape), c["ref"][x].reshape(shape)
        assert not torch.isnan(y).any(), (c["name"], x, "NaN")
        e, s = T.errs(y, r)[0], r.abs().max().item()
        print(f"rows_grad_weight {c['name']} [{c['route']}] {x}: max|err| {e:.3e} max|ref| {s:.3e}")
        assert e <= T.RGW_BAR * s, (c["name"], c["route"], x, e, s)
        worst = max(worst, e / s if s > 0 else 0.0)
        res[x] = y
    _record(c["route"], worst, c["name"])
    return res


@pytest.mark.parametrize("i", range(len(T.rgw_table(256))), ids=_rgw_names())
def test_rows_grad_weight(dev, i):
    cus = _cus(dev.index or 0)
    p = T.rgw_table(cus)[i]
    c = T.rgw_case(T.rgw_key(p))
    out = _rgw_run(c, dev)
    res = _rgw_judge(c, out)
    again = _rgw_run(c, dev)
    for x in out:
        assert torch.equal(_bits(out[x]), _bits(again[x])), (c["name"], x, "second call differs")
    if p["x_front"] % 4:
        # the aligned twin (the column kernel) agrees within the bar
        twin = next(q for q in T.rgw_table(cus) if q["name"] + "-xoff1" == p["name"])
        ct = T.rgw_case(T.rgw_key(twin))
        assert ct["route"].startswith("cols") and c["route"].startswith("partial")
        rt = _rgw_judge(ct, _rgw_run(ct, dev))
        for x in res:
            s = c["ref"][x].abs().max().item()
            assert (res[x].double() - rt[x].double()).abs().max().item() <= T.RGW_BAR * s, (c["name"], x)


# --------------------------------------------------------------------------- reverse adjacency
def _ifence(numel, dtype, front=8, back=8):
    """An integer output inside a sentinel."""
    return torch.full((front + numel + back,), T.INT_SENT, dtype=dtype)


def _rev_run(c, dev):
    L = _L()
    lib = L.lib()
    n_tgt, k, n_src, slots = c["n_tgt"], c["k"], c["n_src"], c["slots"]
    F = 8
    off = _ifence(n_src + 1, torch.int64).to(dev)
    edge = _ifence(slots, torch.int64).to(dev)
    pos = _ifence(slots, torch.int32).to(dev)
    bad = _ifence(1, torch.int32).to(dev)
    nbr = c["nbr"].to(dev)
    deg = c["deg"].to(dev) if c["deg"] is not None else None
    nb = lib.mmpde_reverse_adjacency_scratch_bytes(n_tgt, k, n_src)
    assert 0 < nb < 1 << 30
    scratch = torch.full((nb + 256,), 0x5A, dtype=torch.uint8, device=dev)
    assert scratch.data_ptr() % 256 == 0
    L.check(lib.mmpde_reverse_adjacency(nbr.data_ptr(), n_tgt, k, deg.data_ptr() if deg is not None else None, n_src,
                                        off.data_ptr() + 8 * F, edge.data_ptr() + 8 * F, pos.data_ptr() + 4 * F,
                                        scratch.data_ptr(), nb, bad.data_ptr() + 4 * F, L.stream(dev)),
            "mmpde_reverse_adjacency")
    torch.cuda.synchronize()
    assert bool((scratch[nb:] == 0x5A).all()), "written beyond the scratch"
    assert torch.equal(nbr.cpu(), c["nbr"])
    out = {}
    for name, t, m in (("off", off, n_src + 1), ("edge", edge, slots), ("pos", pos, slots), ("bad", bad, 1)):
        t = t.cpu()
        assert bool((t[:F] == T.INT_SENT).all()) and bool((t[F + m:] == T.INT_SENT).all()), (c["name"], name, "fence")
        out[name] = t[F:F + m]
    return out


@pytest.mark.parametrize("i", range(len(T.REV)), ids=[r[0] for r in T.REV])
def test_reverse_adjacency(dev, i):
    c = T.rev_case(i)
    out = _rev_run(c, dev)
    live = c["n_live"]
    assert int(out["bad"][0]) == c["bad"], (c["name"], "live out-of-range entries", int(out["bad"][0]), c["bad"])
    assert torch.equal(out["off"], c["rev_off"]), (c["name"], "rev_off")
    assert torch.equal(out["edge"][:live], c["rev_edge"][:live]), (c["name"], "the live part of rev_edge")
    pos = out["pos"].long()
    assert torch.equal(torch.sort(pos).values, torch.arange(c["slots"])), (c["name"], "slot_pos is no permutation")
    assert int(out["edge"].min()) >= 0 and int(out["edge"].max()) < c["slots"]
    assert torch.equal(pos[out["edge"]], torch.arange(c["slots"])), (c["name"], "slot_pos[rev_edge[p]] != p")
    assert torch.equal(out["pos"], c["slot_pos"]), (c["name"], "dead slots: ascending past the live ones")
    again = _rev_run(c, dev)
    for x in out:
        assert torch.equal(out[x], again[x]), (c["name"], x, "second call differs")
    _record("reverse_adjacency", 0.0, c["name"])


def test_report_largest_errors(dev):
    """A record, not a bar."""
    for kind in sorted(WORST):
        print(f"{kind}: largest error {WORST[kind][0]:.2e} of max|ref| ({WORST[kind][1]})")
