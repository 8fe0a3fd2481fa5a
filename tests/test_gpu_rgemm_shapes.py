"""The training row GEMMs at their tile, grid and segment edges, against
float64 (cases and references: rgemm_cases.py; their CPU-side checks:
test_rgemm_cases.py):

A  rgemm_ws_kernel: the seven mmpde_rgemm launches of GnnLayerTrain as units at
   n = 1 .. 65 and at a row count where the persistent workgroups take two and
   three tiles (there also bitwise against the same call on one-tile-per-
   workgroup row slices), kh = 32 with partial and empty waves, parts with and
   without a small segment in one launch, all 24 instantiations;
B  rgemm_kernel (the 128 x 128 tile form), all 16 instantiations;
C  mmpde_rgemm_tn over gcols, kx, segments, ns, signs, chunk sizes; run twice,
   bitwise equal;
D  mmpde_rows_small, all four forms, and rows striding over the workgroups;
E  ops.LinearRows through every route of the dispatcher.

Every case: outputs within the bar of rgemm_cases.py, no NaN from the NaN
pads, and every float outside the outputs bitwise untouched."""
import pytest
import torch

import rgemm_cases as C

pytestmark = pytest.mark.gpu

CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
TABLES = {"A": C.cases_a(CUS), "B": C.cases_b(), "C": C.cases_c(), "D": C.cases_d(CUS)}
WORST = {}


def _p(d, ref, extra=0):
    from mmpde_amd import rows
    return None if ref is None else rows._p(d[ref[0]], ref[1] + extra)


def _device(c, dev):
    d = {name: t.to(dev) for name, t in c["bufs"].items()}
    form = {"rgemm": C.rgemm_form, "tn": C.tn_form, "small": C.small_form}[c["kind"]]
    assert form(c, lambda name: d[name].data_ptr()) == form(c), "the device pointers change the kernel form"
    return d


def _outputs(c, d):
    torch.cuda.synchronize()
    return {name: d[name].cpu() for name in C.owned(c, C.reference(c))}


def _fresh_outputs(c, d, dev):
    return dict(d, **{name: c["bufs"][name].to(dev) for name in C.owned(c, C.reference(c))})


def _record(c, worst):
    WORST[c["group"]] = max(WORST.get(c["group"], (0.0, "")), (worst, c["name"]))


def run_rgemm(c, d, dev, r0=0, r1=None):
    from mmpde_amd import _lib as L
    from mmpde_amd import rows
    r1 = c["m"] if r1 is None else r1
    parts = [dict(out=_p(d, p["out"], r0 * p["ldo"]), ldo=p["ldo"], wc=p["wc"], wk=p["wk"], ncols=p["ncols"],
                  bias=_p(d, p["bias"]), omask=_p(d, p["omask"], r0 * p["ldom"]), ldom=p["ldom"], acc=p["acc"],
                  ns=p["ns"], xw=_p(d, p["xw"]), xscale=p["xscale"]) for p in c["parts"]]
    lda = c["lda"]
    rows.rgemm(r1 - r0, c["kh"], c["layout"], tuple(_p(d, w) for w in c["w"]), c["ldw"],
               tuple(_p(d, a, r0 * lda[h]) for h, a in enumerate(c["a"])), lda, parts,
               amask=tuple(_p(d, a, r0 * lda[h]) for h, a in enumerate(c["amask"])), relu=c["relu"],
               xs=_p(d, c["xs"], r0 * c["ldxs"]), ldxs=c["ldxs"], ldxw=c["ldxw"], stream=L.stream(dev))


def run_tn(c, d, dev):
    from mmpde_amd import _lib as L
    from mmpde_amd import rows
    rows.rgemm_tn(c["m"], _p(d, c["g"]), c["ldg"], c["gcols"],
                  [(_p(d, x), ldx, kx, dwcol) for x, ldx, kx, dwcol in c["segs"]], d["dw"][c["dw"][1]:], C.LDDW,
                  db=d["db"][c["db"][1]:] if c["db"] is not None else None, gmask=_p(d, c["gmask"]),
                  xs=_p(d, c["xs"]), ldxs=c["ldxs"], ns=c["ns"], dwcol_s=c["dwcol_s"], sign_s=c["sign"],
                  accumulate_s=c["acc"], stream=L.stream(dev))


def run_small(c, d, dev, r0=0, r1=None):
    from mmpde_amd import _lib as L
    from mmpde_amd import rows
    r1 = c["n"] if r1 is None else r1
    if c["ldy"] == c["kout"] and c["y"][1] % 4 == 0 and (r0, r1) == (0, c["n"]):
        # a tight, aligned output: through rows.rows_small, which allocates it
        x = C.view(d["x"], c["x"][1], c["n"], c["kin"], c["ldx"])
        w = C.view(d["w"], c["w"][1], c["no"], c["ki"], c["ldw"])
        b = d["bias"][c["bias"][1]:c["bias"][1] + c["kout"]] if c["bias"] is not None else None
        y = rows.rows_small(x, w, b, c["layout"])
        C.view(d["y"], c["y"][1], c["n"], c["kout"], c["ldy"]).copy_(y)
        return
    L.check(L.lib().mmpde_rows_small(_p(d, c["x"], r0 * c["ldx"]), c["ldx"], r1 - r0, c["ki"], _p(d, c["w"]),
                                     c["ldw"], c["layout"], _p(d, c["bias"]), c["no"],
                                     _p(d, c["y"], r0 * c["ldy"]), c["ldy"], L.stream(dev)), "mmpde_rows_small")


def _sliced_equal(c, run, dev, full, step):
    """The same call on row slices of `step` rows: bitwise the full call's rows."""
    n = c["m"] if c["kind"] == "rgemm" else c["n"]
    d = _fresh_outputs(c, _device(c, dev), dev)
    for r0 in range(0, n, step):
        run(c, d, dev, r0, min(n, r0 + step))
    for name, t in _outputs(c, d).items():
        assert torch.equal(t.view(torch.int32), full[name].view(torch.int32)), (c["name"], name, "sliced run differs")


@pytest.mark.parametrize("name", list(TABLES["A"]))
def test_ws_form(dev, name):
    c = C.build("A", name, CUS)
    assert C.rgemm_form(c)[0] == "ws"
    d = _device(c, dev)
    run_rgemm(c, d, dev)
    got = _outputs(c, d)
    _record(c, C.judge(c, got))
    if name.endswith("-multi"):
        slots = C.ws_slots(c["kh"], len(c["parts"]), CUS)
        assert (c["m"] + 31) // 32 > 2 * slots
        _sliced_equal(c, run_rgemm, dev, got, 32 * slots)


@pytest.mark.parametrize("name", list(TABLES["B"]))
def test_tile_form(dev, name):
    c = C.build("B", name, CUS)
    assert C.rgemm_form(c)[0] == "tile"
    d = _device(c, dev)
    run_rgemm(c, d, dev)
    _record(c, C.judge(c, _outputs(c, d)))


@pytest.mark.parametrize("name", list(TABLES["C"]))
def test_rgemm_tn(dev, name, monkeypatch):
    from mmpde_amd import rows
    c = C.build("C", name, CUS)
    monkeypatch.setattr(rows, "CHUNK_ROWS", c["chunk"])
    d = _device(c, dev)
    run_tn(c, d, dev)
    got = _outputs(c, d)
    _record(c, C.judge(c, got))
    d = _fresh_outputs(c, d, dev)
    run_tn(c, d, dev)
    for bname, t in _outputs(c, d).items():
        assert torch.equal(t.view(torch.int32), got[bname].view(torch.int32)), (name, bname, "second run differs")


@pytest.mark.parametrize("name", list(TABLES["D"]))
def test_rows_small(dev, name):
    c = C.build("D", name, CUS)
    d = _device(c, dev)
    run_small(c, d, dev)
    got = _outputs(c, d)
    _record(c, C.judge(c, got))
    if name.endswith("-strided"):
        one_pass = C.small_blocks(c["kin"], c["kout"], CUS) * C.small_rpb(c["kout"])
        assert c["n"] > one_pass
        _sliced_equal(c, run_small, dev, got, one_pass)


@pytest.mark.parametrize("k,nout", C.MAPS_E)
@pytest.mark.parametrize("n", C.ROWS_E)
def test_linear_rows_routes(dev, n, k, nout):
    from mmpde_amd.ops import LinearRows
    c = C.linear_case(n, k, nout)
    x, w, b = (c[q].to(dev).requires_grad_() for q in "xwb")
    y = LinearRows.apply(x, w, b)
    (y * c["dy"].to(dev)).sum().backward()
    ref = c[torch.float64]
    for q, t in (("y", y), ("dx", x.grad), ("dw", w.grad), ("db", b.grad)):
        r = ref[q]
        err, scale = (t.detach().double().cpu() - r).abs().max().item(), r.abs().max().item()
        print(f"LinearRows n={n} k={k} N={nout} {q}: max|err| {err:.3e} max|ref| {scale:.3e}")
        assert t.shape == r.shape and err <= c["bars"][q] * scale, (q, err, scale)
        WORST["E"] = max(WORST.get("E", (0.0, "")), (err / scale, f"n{n}-k{k}-N{nout}-{q}"))


def test_report_largest_errors(dev):
    """A record, not a bar."""
    for grp in sorted(WORST):
        print(f"group {grp}: largest error {WORST[grp][0]:.2e} of its scale ({WORST[grp][1]})")
