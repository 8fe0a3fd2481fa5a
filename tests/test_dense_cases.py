"""CPU-only check of the inputs of test_gpu_dense_shapes.py and
test_gpu_row_reduce_shapes.py (dense_cases.py): every case builds with the NaN
/ sentinel layout the device tests rely on; the float32 evaluation of every
reference stays within a quarter of the case's bar; max|ref| of every judged
group is at least SIGNAL_FLOOR (1e-3), or exactly 0 where the output is an
exact zero; one wrong element moves the float64 result by at least ten bars;
and the dispatch arithmetic of the kernels, restated on the host, shows every
instantiation, slice count, split and row-group count named by a case."""
import pytest
import torch

import dense_cases as C

ALL = [(k, i) for k in C.ALL_KINDS for i in C.table(k)]
IDS = [C.build(k, i)["name"] for k, i in ALL]
assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("kind,idx", ALL, ids=IDS)
def test_case_layout_floor_signal_and_sensitivity(kind, idx):
    c = C.build(kind, idx)
    regions = C.reference(c)
    outs = C.owned(c, regions)
    for bname, flat in c["bufs"].items():
        if bname in outs:
            own = outs[bname]
            assert bool((flat[~own] == C.SENT).all()) and not torch.isnan(flat[own]).any()
            assert int(own.sum()) == sum(r["rows"] * r["cols"] for r in regions if r["buf"] == bname)
        else:
            # inputs: NaN in front, behind and in every pad
            at = c["at"][bname]
            assert at >= 3 and torch.isnan(flat[:at]).all() and torch.isnan(flat[-8:]).all()
            assert not torch.isnan(flat[at]), bname
    for r in regions:
        assert r["values"].dtype == torch.float64 and bool(torch.isfinite(r["values"]).all()), (c["name"], r["grp"])
    # signal
    for grp, s in C.scales(regions).items():
        assert s == 0.0 or s >= C.SIGNAL_FLOOR, (c["name"], grp, s)
        if s == 0.0:
            assert kind in ("segsum", "smooth"), (c["name"], grp)
    # fp32 floor
    worst = C.judge(c, C.evaluate_fp32(c), share=C.FLOOR_SHARE)
    print(f"{c['name']}: fp32 CPU evaluation {worst:.2e} of scale")
    # sensitivity
    mut = C.mutant(c)
    if mut is not None and not (kind == "segsum" and c["pattern"] == "empty"):
        m, grps = mut
        bar = C.bars(regions)
        moved = {r["grp"]: (r["values"] - q["values"]).abs().max().item()
                 for r, q in zip(regions, C.reference(m)) if r["grp"] in grps}
        assert set(moved) == set(grps)
        for grp, d in moved.items():
            print(f"{c['name']} {grp}: the mutant moves {d / bar[grp]:.1f} bars")
            assert d >= C.SENSITIVITY * bar[grp], (c["name"], grp, d, bar[grp])


@pytest.mark.parametrize("idx", C.table("bn"), ids=C.ids("bn"))
def test_bn_row_left_out_of_the_statistics_is_seen(idx):
    c = C.build("bn", idx)
    regions = C.reference(c)
    y = next(r for r in regions if r["grp"] == "y")
    d = (y["values"] - C.bn_reference(c, skip_last_row=True)[0]["values"]).abs().max().item()
    assert d >= C.SENSITIVITY * C.bars(regions)["y"], (c["name"], d)


def test_resample_torch_agrees_with_the_restatement():
    for idx in C.table("resample"):
        c = C.build("resample", idx)
        r = C.reference(c)[0]
        err = (C.resample_torch(c).double() - r["values"].reshape(-1)).abs().max().item()
        assert err <= C.FLOOR_SHARE * C.bars([r])["y"], (c["name"], err)
    c = C.build("resample", 0)
    assert C.reference(c)[0]["exact"] and c["p"][1:3] == c["p"][3:5] == (48, 48)
    assert torch.equal(C.reference(c)[0]["values"].reshape(-1).float(),
                       c["bufs"]["x"][c["at"]["x"]:][:3 * 48 * 48])
    shapes = {C.build("resample", i)["p"] for i in C.table("resample")}
    assert {(5, 7, 5, 3, 9), (1, 5, 1, 4, 4), (5, 1, 6, 3, 3), (3, 48, 48, 1, 7)} <= shapes
    assert any(p[3:] == (1, 1) for p in shapes) and {p[0] for p in shapes} >= {1, 5}
    assert any(p[0] * p[3] * p[4] > 256 and (p[0] * p[3] * p[4]) % 256 for p in shapes)


def test_conv_table_holds_its_shapes():
    t = C.CONV
    assert len(set(t)) == len(t)
    assert {(p[3], p[4]) for p in t} == {(13, 11), (12, 10), (7, 7), (2, 2), (1, 5)}
    assert {p[5] for p in t} == {1, 3, 5} and {p[6] for p in t} == {1, 2} and {p[0] for p in t} == {1, 3}
    assert {(p[1], p[2]) for p in t} == {(1, 1), (3, 5), (6, 6)}
    assert {p[9] for p in t} == {False, True} and {p[10] for p in t} == {0, 1, 2, 3}
    assert {p[11] for p in t} == {None, "before", "after"}
    for ks in (1, 3, 5):
        pads = {(p[7], p[8]) for p in t if p[5] == ks}
        want = {(ks // 2, False), (ks // 2, True), (ks // 2 + 1, False)} | ({(0, False)} if ks > 1 else set())
        assert pads >= want, (ks, pads)
    assert any(p[8] and p[7] == 0 for p in t)                               # circular without padding
    assert all(not p[8] or (p[7] <= p[3] and p[7] <= p[4]) for p in t)      # what the entry point accepts
    assert any(p[8] and p[7] == p[3] == 2 and p[5] == 5 for p in t)         # circular, pad == h, ks 5 on 2 x 2
    assert any(p[8] and p[7] == p[3] == 1 for p in t)
    assert any(p[8] and p[6] == 2 and p[7] > 0 for p in t)                  # circular with stride 2
    # every activation with and without a residual before it; after it with a non-trivial one
    assert {(p[10], p[11]) for p in t} >= {(1, "before"), (2, "before"), (3, "before"), (1, "after"), (2, "after"),
                                           (3, "after")}
    totals = []
    for p in t:
        oh, ow = C.conv_out(p[3], p[4], p[5], p[6], p[7])
        assert oh > 0 and ow > 0
        totals.append(p[0] * p[2] * oh * ow)
    assert min(totals) == 1 and any(v < 256 for v in totals) and any(v > 256 and v % 256 for v in totals)
    assert any(256 < v < 512 for v in totals) or any(v > 512 for v in totals)


def test_grad_weight_forms_slices_and_planes():
    forms = {p: C.gw_form(p[3], p[4], p[5]) for p in C.GW}
    assert {lds for lds, _ in forms.values()} == {False, True}              # both instantiations
    assert {s for _, s in forms.values()} == {256, 28, 10, 5, 3, 1}         # ks 1, 3, 5, 7, 9, 15
    assert {p[5] for p in C.GW} == {1, 3, 5, 7, 9, 15}
    at_limit = [p for p in C.GW if p[3] * p[4] == 8192]
    assert at_limit and all(forms[p][0] for p in at_limit) and 2 * 8192 * 4 == 64 * 1024
    assert {p[0] for p in at_limit} == {1, 3}
    assert any(not forms[p][0] and p[3] * p[4] == 8281 and p[0] == 3 for p in C.GW)
    assert any(p[3:6] == (2, 2, 1) and forms[p][1] > p[3] * p[4] for p in C.GW)       # more slices than pixels
    assert any(p[3:7] == (1, 1, 3, True) for p in C.GW)
    assert {(p[1], p[2]) for p in C.GW} == {(1, 1), (3, 2)} and {p[0] for p in C.GW} == {1, 3}
    assert {p[6] for p in C.GW} == {False, True} and {p[7] for p in C.GW} == {False, True}
    for lds in (False, True):                                               # batches restaged; both pad modes
        assert {p[0] for p in C.GW if forms[p][0] == lds} == {1, 3}
        assert {p[6] for p in C.GW if forms[p][0] == lds} == {False, True}
    assert all(p[5] * p[5] <= C.GW_THREADS and (not p[6] or p[5] // 2 <= min(p[3], p[4])) for p in C.GW)


def test_skinny_splits_and_strides():
    z = {s: C.skinny_splits(s[2], s[1], 256) for s in C.SKINNY_SHAPES}
    assert z == {(3, 512, 20): 1, (17, 513, 17): 2, (2, 2048, 40): 4}
    for cus in (1, 64, 256, 304, 1024):                                     # "split on any chip" / never split
        assert C.skinny_splits(40, 2048, cus) > 1 and C.skinny_splits(20, 512, cus) == 1
    cs = [C.build("skinny", i) for i in C.table("skinny")]
    for s in C.SKINNY_SHAPES:
        mine = [c for c in cs if (c["m"], c["k"], c["n"]) == s]
        assert any((c["ldx"], c["ldw"], c["ldy"]) == (s[1] + 3, s[1] + 5, s[2] + 7) for c in mine)
        assert {c["bias"] for c in mine} == {False, True} and {c["ws"] for c in mine} == {False, True}
        assert any(c["ops"] for c in mine) and {c["act"] for c in mine} == {0, 1, 2}
    # 17 x 513 x 17: one k in the second chunk, one row and one column in the second tiles
    assert 513 - C.SK_CHUNK == 1 and 17 - 16 == 1
    c = next(c for c in cs if c["ldx"] != c["k"])
    x = C.view(c["bufs"]["x"], c["at"]["x"], c["m"], c["ldx"], c["ldx"])
    assert torch.isnan(x[:, c["k"]:]).all() and not torch.isnan(x[:, :c["k"]]).any()


def test_small_dense_tables_hold_their_shapes():
    o = C.OUTER
    assert {p[0] for p in o} == {1, 31, 32, 33, 70} and {p[1] for p in o} == {1, 15, 16, 17, 40}
    assert {p[2] for p in o} == {1, 3, 63, 64, 65, 130} and {p[3] for p in o} == {False, True}
    for i in C.table("outer"):
        c = C.build("outer", i)
        assert c["ldg"] % 2 == c["ldx"] % 2 == c["lddw"] % 2 == 1
        assert c["ldg"] > c["n"] and c["ldx"] > c["k"] and c["lddw"] > c["k"]
    assert {r for r, _ in C.TRANSPOSE} == {c for _, c in C.TRANSPOSE} == {1, 31, 32, 33, 70}
    assert C.TANH_N == [1, 255, 256, 257]
    assert set(C.MSE) == {(b, n) for b in (1, 3) for n in (1, 255, 256, 257, 2521)}


def test_smooth_table_holds_its_shapes():
    cs = [C.build("smooth", i) for i in C.table("smooth")]
    assert {(c["n_pts"], c["n_q"]) for c in cs} == {(p, q) for p in C.SMOOTH_NPTS for q in C.SMOOTH_NQ}
    assert {(c["ps"], c["vs"]) for c in cs} == {(1, 1), (1, 3), (3, 3), (3, 1)}
    assert all(c["n_q"] % c["ps"] == 0 and c["n_q"] % c["vs"] == 0 for c in cs)
    for p in C.SMOOTH_NPTS:
        sc = {round(c["scale"], 3) for c in cs if c["n_pts"] == p}
        assert len(sc) == (3 if p > 1 else 2), (p, sc)                      # sqrt(1) = 1
        assert any(c["ps"] == 3 for c in cs if c["n_pts"] == p) and any(c["vs"] == 3 for c in cs if c["n_pts"] == p)
    assert {c["scale"] for c in cs} >= {1.0, 48.0, 8.0}
    outside = 0.0
    for c in cs:
        q = c["bufs"]["qry"][c["at"]["qry"]:][:2 * c["n_q"]].reshape(-1, 2)
        outside = max(outside, float(-q.min()), float(q.max() - 1))
        assert float(q.min()) >= -0.1 and float(q.max()) <= 1.1
        if "on-point" in c["planted"]:
            p = c["bufs"]["pts"][c["at"]["pts"]:][:2 * c["ps"] * c["n_pts"]].reshape(c["ps"], -1, 2)
            assert torch.equal(q[-1], p[-1, 0])
            # that point's term of the gradient is 0 (torch.norm's backward), the result finite
            assert bool(torch.isfinite(C.reference(c)[1]["values"]).all())
        if "equidistant" in c["planted"]:
            p = c["bufs"]["pts"][c["at"]["pts"]:][:4]
            assert torch.norm(q[-2] - p[:2]) == torch.norm(q[-2] - p[2:4])
        if c["n_pts"] == 1:
            out, gq = C.reference(c)
            assert out["exact"] and gq["exact"] and not gq["values"].any()
            assert torch.equal(out["values"].reshape(-1).float(),
                               c["bufs"]["vals"][c["at"]["vals"]:][:c["vs"]].repeat_interleave(c["n_q"] // c["vs"]))
    assert outside > 0.08
    assert sum("equidistant" in c["planted"] for c in cs) >= 10


def test_segsum_table_holds_its_shapes():
    cs = [C.build("segsum", i) for i in C.table("segsum")]
    assert {c["n"] for c in cs} == {1, 5, 300} and {c["width"] for c in cs} == {1, 3, 30, 128, 257}
    assert any((c["n"] * c["width"]) % 256 and c["n"] * c["width"] > 256 for c in cs)
    lens = [l for c in cs for l in c["lens"]]
    assert 0 in lens and 1 in lens and C.HUB in lens
    for c in cs:
        off, edge = c["ibufs"]["off"], c["ibufs"]["edge"]
        assert off[0] == 0 and off.numel() == c["n"] + 1 and int(off[-1]) == edge.numel() - 8 == sum(c["lens"])
        live = edge[:int(off[-1])]
        assert live.numel() == 0 or (0 <= int(live.min()) and int(live.max()) < C.SEG_ROWS - 7)   # rows never referenced
        if live.numel() >= 2:
            assert live[0] == live[1]                                       # an index that repeats
        # the float32 reference is the sequential sum, the float64 one index_add_
        r32 = C.reference(c, torch.float32)[0]["values"]
        assert r32.dtype == torch.float32
        assert torch.equal(r32.reshape(-1), torch.from_numpy(C.segsum_sequential(c)).reshape(-1))


def test_bn_table_holds_its_shapes():
    ns, cs = [p[0] for p in C.BN], [p[1] for p in C.BN]
    for n in (2, 3, 63, 64, 65, 129, 1000):
        assert ns.count(n) >= 2, n
    for ch in (4, 12, 128, 1024):
        assert cs.count(ch) >= 2, ch
    assert {C.bn_row_groups(ch) for ch in set(cs)} == {256, 85, 8, 1}
    assert any(n < C.bn_row_groups(ch) for n, ch, _, _ in C.BN)             # empty row groups: nb == 0 in the merge
    assert any(n < C.bn_row_groups(ch) and ch == 4 for n, ch, _, _ in C.BN)
    assert {(p[2], p[3]) for p in C.BN} == {(False, False), (False, True), (True, False), (True, True)}
    assert C.BN_OFFSET >= 2.0
    for i in C.table("bn"):
        c = C.build("bn", i)
        x = c["bufs"]["x"][c["at"]["x"]:][:c["n"] * c["C"]]
        assert c["n"] < 8 or abs(float(x.mean()) - 2.0) < 0.2
