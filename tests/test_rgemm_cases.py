"""CPU-only check of the inputs of test_gpu_rgemm_shapes.py: every case
builds with the NaN / sentinel layout the device tests rely on, the float32
evaluation of every reference stays within a quarter of the case's bar (so
the bars have room over correct fp32 arithmetic whatever the summation order),
every kernel instantiation of csrc/rgemm.hip and csrc/rows_small.hip and every
route of the LinearRows dispatcher is named by at least one case, and the case
tables hold the shapes they are meant to hold."""
import itertools

import pytest
import torch

import rgemm_cases as C

CUS = 256
TABLES = {"A": C.cases_a(CUS), "B": C.cases_b(), "C": C.cases_c(), "D": C.cases_d(CUS)}
ALL = [(g, n) for g, t in TABLES.items() for n in t]
FORM = {"rgemm": C.rgemm_form, "tn": C.tn_form, "small": C.small_form}


@pytest.mark.parametrize("group,name", ALL, ids=[n for _, n in ALL])
def test_case_layout_and_fp32_floor(group, name):
    c = C.build(group, name, CUS)
    regions = C.reference(c)
    outs = C.owned(c, regions)
    for bname, flat in c["bufs"].items():
        if bname in outs:
            own = outs[bname]
            assert bool((flat[~own] == C.SENT).all()) and not torch.isnan(flat[own]).any()
            assert int(own.sum()) == sum(r["rows"] * r["cols"] for r in regions if r["ref"][0] == bname)
        else:
            # inputs: NaN in front, behind and in every pad
            assert torch.isnan(flat[0]) and torch.isnan(flat[-8:]).all()
    for r in regions:
        assert r["values"].dtype == torch.float64 and bool(torch.isfinite(r["values"]).all()), (name, r["grp"])
    worst = C.judge(c, C.evaluate_fp32(c), share=C.FLOOR_SHARE)
    print(f"{name}: fp32 CPU evaluation {worst:.2e} of scale, bar {c['bar']:.0e}")


def test_mask_values_are_planted():
    v = C.mask_values(torch.Generator().manual_seed(0), 64, 64)
    bits = v.view(torch.int32)
    assert int((bits == 0).sum()) > 200 and int((bits == -2 ** 31).sum()) > 200 and int((v == C.TINY).sum()) > 200
    nz = v[v != 0].abs()
    assert float(nz.min()) >= C.TINY                      # no denormals


def _forms(group):
    return {name: FORM[(c := C.build(group, name, CUS))["kind"]](c) for name in TABLES[group]}


def test_every_rgemm_instantiation_is_named():
    fa, fb = _forms("A"), _forms("B")
    assert all(f[0] == "ws" for f in fa.values()) and all(f[0] == "tile" for f in fb.values())
    ws = {f[1:] for f in fa.values()}
    assert ws == set(itertools.product(("NT", "NN"), (32, 64, 128), (False, True), (False, True)))    # 24
    tile = set(itertools.product(("NT", "NN"), (False, True), (False, True), (False, True)))          # 16
    assert set(C.TILE_COVERAGE) == tile
    for key, name in C.TILE_COVERAGE.items():
        assert fb[name] == ("tile",) + key, (name, fb[name])


def test_every_tn_and_small_instantiation_is_named():
    three = set(itertools.product((False, True), repeat=3))
    assert set(_forms("C").values()) == three                                                          # 8
    assert set(_forms("D").values()) == set(itertools.product((False, True), repeat=2))                # 4


def test_production_cases_are_the_layer_launches():
    """kh, layout, parts, small segments and masks of GnnLayerTrain's seven launches (gnn_2d.py)."""
    want = {1: ("ws", "NT", 64, False, True), 2: ("ws", "NT", 128, False, True), 3: ("ws", "NT", 64, False, False),
            4: ("ws", "NN", 64, True, False), 5: ("ws", "NN", 64, False, False),
            6: ("ws", "NN", 128, False, False), "6s": ("ws", "NN", 128, False, False),
            7: ("ws", "NN", 64, False, False)}
    for idx, form in want.items():
        for n in C.ROWS_A:
            c = C.build("A", f"prod{idx}-n{n}", CUS)
            assert C.rgemm_form(c) == form and c["m"] == n and len(c["parts"]) == C.PROD[idx][1]
            assert c["lda"] == (128, 128) and c["ldw"] == (128 if idx in (3, 4) else 260)
        kh, nparts = C.PROD[idx]
        m = C.build("A", f"prod{idx}-multi", CUS)["m"]
        slots = (1 if kh == 128 else 2) * CUS // nparts
        tiles = (m + 31) // 32
        assert 2 * slots < tiles <= 3 * slots and tiles % slots != 0 and m % 32 != 0
    c = C.build("A", "prod1-n33", CUS)
    assert [(p["ns"], p["wk"], p["xscale"]) for p in c["parts"]] == [(4, 0, 1.0), (3, 128, -1.0)]
    c = C.build("A", "prod2-n33", CUS)
    assert c["relu"] and c["xs"][1] % 4 == 3 and torch.isnan(c["bufs"]["ext"][c["xs"][1] - 1])
    c = C.build("A", "prod7-n33", CUS)
    assert (c["parts"][0]["ncols"], c["parts"][0]["ldo"], c["parts"][0]["acc"]) == (1, 4, True)
    assert bool((C.view(c["bufs"]["dext"], c["parts"][0]["out"][1] - 3, 33, 3, 4) == C.SENT).all())
    c = C.build("A", "prod6s-n33", CUS)
    assert (c["parts"][0]["ncols"], c["parts"][0]["ldo"]) == (4, 4) and c["w"][0][1] % 260 == (4 + 256) % 260
    for ns in ("40", "03"):
        for lay in ("NT", "NN"):
            c = C.build("A", f"ws64-{lay}-ns{ns}", CUS)
            assert [str(p["ns"]) for p in c["parts"]] == list(ns) and c["m"] == 33
            assert torch.isnan(c["bufs"]["xs"][c["xs"][1] - 1])


def test_tables_hold_their_shapes():
    b = [C.build("B", n, CUS) for n in TABLES["B"]]
    assert {c["m"] for c in b} >= set(C.ROWS_B) and {p["ncols"] for c in b for p in c["parts"]} >= set(C.COLS_B)
    assert {c["kh"] for c in b} >= {0, 1, 2, 3, 4, 5, 8, 36, 37, 132, 148}
    assert any(c["kh"] == 64 and c["parts"][0]["wk"] == 2 for c in b)
    assert any(c["lda"][0] % 2 == 1 for c in b) and any(c["kh"] and c["a"][0][1] % 4 == 1 for c in b)
    feats = [(len(c["parts"]) == 2, c["relu"], any(p["acc"] for p in c["parts"]),
              any(p["omask"] is not None for p in c["parts"]), any(p["bias"] is not None for p in c["parts"]))
             for c in b]
    assert all(any(f[i] for f in feats) for i in range(5))
    # a non-unit xscale on a live small segment in all four (layout, VEC) corners
    assert {(c["layout"], C.rgemm_form(c)[2]) for c in b if c["kh"]
            for p in c["parts"] if p["ns"] and p["xscale"] != 1.0} == set(itertools.product((C.NT, C.NN), (False, True)))
    t = [C.build("C", n, CUS) for n in TABLES["C"]]
    at256 = [c for c in t if c["chunk"] == 256]
    assert {c["m"] for c in at256} >= set(C.ROWS_C) and {c["gcols"] for c in t} == set(C.GCOLS_C) | {61, 62, 33}
    assert {kx for c in t for _, _, kx, _ in c["segs"]} >= {1, 2, 3, 63, 64, 65, 128, 131}
    assert {len(c["segs"]) for c in t} == {1, 2, 3} and {c["ns"] for c in t} == {0, 1, 2, 3, 4}
    assert {(c["chunk"], c["m"]) for c in t if c["chunk"] != 256} == \
        {(2, 1), (2, 5), (2, 130), (6, 17), (258, 261), (1024, 1027)}
    for key in ("sign", "acc", "gmask", "db"):
        assert len({(c[key] is not None) if key in ("gmask", "db") else c[key] for c in t if c["ns"]}) == 2, key
    # the VEC case with clamped pairs at odd columns; odd strides; an offset pointer
    assert any(C.tn_form(c)[1] and c["gcols"] % 2 and c["segs"][0][2] % 2 for c in t)
    assert any(c["ldg"] % 2 for c in t) and any(c["segs"][0][1] % 2 for c in t) and any(c["g"][1] % 2 for c in t)
    d = [C.build("D", n, CUS) for n in TABLES["D"] if not n.endswith("strided")]
    assert {c["kin"] for c in d} == {1, 4, 5, 16, 17, 62, 128} and {c["kout"] for c in d} == {1, 3, 4, 5, 8, 30, 100, 128}
    assert {(c["kin"], c["kout"]) for c in d} >= {(128, 128), (1, 1), (128, 1)}
    assert {c["bias"] is not None for c in d if c["layout"] == C.NT} == {False, True}
    for c in d:
        rpb = C.small_rpb(c["kout"])
        assert c["n"] in (1, 7, rpb - 1, rpb + 1) and 4 * (256 // rpb) >= c["kout"]
    s = C.build("D", "small-NT-128to128-strided", CUS)
    assert s["n"] == 8197 and s["n"] > C.small_blocks(128, 128, CUS) * C.small_rpb(128)


ROUTES = {(128, 128): (("rgemm", 64, 0), ("rgemm", 64, 0)),
          (257, 128): (("rgemm", 128, 1), ("rgemm", 64, 0)),
          (260, 300): (("rgemm", 128, 4), ("rgemm", 148, 4)),
          (264, 20): (("rgemm", 132, 0), ("rgemm", 8, 4)),
          (72, 40): (("small",), ("small",)),
          (4, 128): (("small",), ("small",)),
          (64, 30): (("rgemm", 32, 0), ("small",))}


def test_dispatcher_routes():
    """One shape per route through rows.linear_fwd / linear_bwd_input: the
    weight-stationary form with and without the small segment, the tile form
    (VEC) with and without it, rows_small in both directions, and one shape
    whose forward and input gradient take different kernels."""
    assert set(ROUTES) == set(C.MAPS_E)
    for (k, nout), (fwd, dx) in ROUTES.items():
        r = C.linear_routes(k, nout)
        assert (r["fwd"], r["dx"], r["dw"]) == (fwd, dx, ("tn",)), ((k, nout), r)
    for n, (k, nout) in itertools.product(C.ROWS_E, C.MAPS_E):
        c = C.linear_case(n, k, nout)
        for q, bar in c["bars"].items():
            r64, r32 = c[torch.float64][q], c[torch.float32][q]
            err = (r32.double() - r64).abs().max().item()
            assert err <= C.FLOOR_SHARE * bar * r64.abs().max().item(), (n, k, nout, q, err)
