"""The cases of train_path_cases.py, checked on the CPU alone: the lattice
inputs make every ReLU pre-activation exact in float32 (a condition of the
device tests, not a tolerance), the references agree with the project's
plain-torch edge stage, and every instantiation, tile / grid regime and list
length the device tests are there for is named by at least one case."""
import os
import re

import pytest
import torch

import train_path_cases as T
from test_gpu_edge_shapes import _edge_mean_ref

GRID = T.FALLBACK_GRID
EDGE_CASES = [(n, k, r, lists) for (n, k, lists) in T.edge_shapes(GRID) for r in (0, 1, 2)]
EDGE_IDS = [f"{n}x{k}-{T.RAGGED_NAME[r]}" + ("-lists" if lists else "") for n, k, r, lists in EDGE_CASES]


def _same(x32, x64):
    return torch.equal(x32.double(), x64)


# --------------------------------------------------------------------------- A
@pytest.mark.parametrize("n,k,ragged,lists", EDGE_CASES, ids=EDGE_IDS)
def test_edge_case_is_exact_and_consistent(n, k, ragged, lists):
    c = T.edge_case(n, k, ragged, lists)
    ref, f32 = c["ref"], c["cpu32"]
    # float32 pre-activations are the float64 ones, bit for bit
    assert _same(f32["z1"], ref["z1"]) and _same(f32["z2"], ref["z2"])
    # ... in a second summation order (channels reversed, in two halves)
    r1 = torch.relu(f32["z1"]).flip(-1)
    w = c["w2"].flip(1)
    z2b = (r1[..., :64] @ w[:, :64].t() + c["b2"]) + r1[..., 64:] @ w[:, 64:].t()
    assert _same(z2b, ref["z2"])
    # ... and through the fp16 hi + lo split of the fp16x3 kernel
    z2s, lo_nonzero, total = T.edge_z2_split(c)
    assert _same(z2s, ref["z2"])
    live = c["live"]
    ties2 = int(((ref["z2"] == 0) & live[..., None]).sum())
    ties1 = int(((ref["z1"] == 0) & live[..., None]).sum())
    print(f"{c['name']}: lo parts non-zero {lo_nonzero / total:.3f}; exact ties z1 {ties1} z2 {ties2}")
    if n >= 1000:
        assert lo_nonzero > 0.05 * total            # a dropped lo term would flip signs
        assert ties1 >= 1 and ties2 >= 1
    # the graph is the project's plain edge stage: the same mean and gradients
    leaves = [c[x].double().requires_grad_() for x in ("a", "b", "w2", "b2")]
    mean = _edge_mean_ref(*leaves, c["nbr"], c["deg"])
    assert torch.equal(mean.detach(), ref["mean"])
    (mean * c["g"].double()).sum().backward()
    for name, t in zip(("ga", "gb", "gw2", "gb2"), leaves):
        assert torch.allclose(t.grad, ref[name], rtol=0, atol=1e-12 * max(ref[name].abs().max().item(), 1.0)), name
    gz1 = ref["gz1"].reshape(n, k, T.H)
    assert not gz1[~live].any()                      # padding slots carry no gradient
    assert torch.allclose(gz1.sum(1), ref["ga"], rtol=0, atol=1e-12 * max(ref["ga"].abs().max().item(), 1.0))
    gb = torch.zeros(n, T.H, dtype=torch.float64).index_add_(0, c["nbr_alt"].reshape(-1).long(), ref["gz1"])
    assert torch.allclose(gb, ref["gb"], rtol=0, atol=1e-12 * max(ref["gb"].abs().max().item(), 1.0))
    # the float32 CPU evaluation (the floor of the 4 x rule) is far inside the bar
    for name in ("ga", "gb", "gw2", "gb2", "gz1"):
        e, s = T.errs(f32[name], ref[name])[0], ref[name].abs().max().item()
        assert e <= 0.25 * T.EDGE_BAR * s, (name, e, s)
    # the two nbr copies differ in the padding entries alone, all in range
    assert torch.equal(c["nbr"][live], c["nbr_alt"][live]) and bool((c["nbr"][~live] == -1).all())
    assert int(c["nbr_alt"].min()) >= 0 and int(c["nbr_alt"].max()) < n
    # mask words: the float64 sign of z2; padding words all ones
    w = c["mask"].to(torch.int64) & 0xFFFFFFFF
    ch = torch.arange(T.H)
    bits = ((w[:, ch // 32] >> (ch % 32)) & 1).bool().reshape(n, k, T.H)
    assert torch.equal(bits[live], (ref["z2"] > 0)[live]) and bool(bits[~live].all())
    # reverse lists: a permutation, the live slots first, source-major, ascending within a source
    pos, off, edge = c["slot_pos"].long(), c["rev_off"], c["rev_edge"]
    assert torch.equal(torch.sort(pos).values, torch.arange(n * k))
    assert torch.equal(pos[edge], torch.arange(n * k)) and int(off[-1]) == int(live.sum())
    src = c["nbr_alt"].reshape(-1).long()[edge[:int(off[-1])]]
    assert torch.equal(src, torch.repeat_interleave(torch.arange(n), off[1:] - off[:-1]))
    for j in range(n):
        seg = edge[int(off[j]):int(off[j + 1])]
        assert bool((seg[1:] > seg[:-1]).all())
    assert bool((~live.reshape(-1)[edge[int(off[-1]):]]).all())


def test_edge_ragged_degrees():
    for n, k, lists in T.edge_shapes(GRID):
        for r in (T.RAGGED_LAST0, T.RAGGED_LASTK):
            deg = T.edge_case(n, k, r, lists)["deg"]
            assert int(deg[n - 1]) == (0 if r == T.RAGGED_LAST0 else k)
            if n >= 17:
                tiles = deg[:n // 16 * 16].reshape(-1, 16)
                assert bool((tiles == 0).all(1).any()), "a whole 16-row tile of zeros"
            if n >= 64:
                tiles = deg[:n // 32 * 32].reshape(-1, 32)
                assert bool((tiles == 0).all(1).any()), "a whole 32-row tile of zeros"
            if n >= 31 or r == T.RAGGED_LASTK:
                assert bool((deg == k).any()), "a full row"
        assert bool((T.edge_case(n, k, T.FIXED, lists)["deg"] == k).all())


def test_edge_shapes_name_every_regime():
    reg = {(n, k): T.edge_regime(n, k, GRID) for n, k, _ in T.edge_shapes(GRID)}
    # the tile edges of both kernels
    assert {n for n, k in reg if k == 3} >= {1, 15, 16, 17, 31, 32, 33}
    # partial_sum_kernel over fewer than 8 partials, and just above
    assert {r["g_f32"] for r in reg.values()} >= {1, 2, 3, 9}
    assert {r["g_f16"] for r in reg.values()} >= {1, 2, 5}
    assert any(r["g_f32"] == GRID and r["g_f16"] == GRID for r in reg.values())
    # slot staging passes and both slot parities at one n
    at40 = {k: reg[(40, k)] for k in (1, 2, 16, 17)}
    assert [at40[k]["stage_passes"] for k in (1, 2, 16, 17)] == [1, 1, 1, 2]
    # the 64-slot limit: the fp16x3 kernel up to 64, the fp32 one above
    assert reg[(64, 63)]["f16_kernel"] and reg[(64, 64)]["f16_kernel"] and not reg[(50, 65)]["f16_kernel"]
    # more than one tile per workgroup, odd and even k
    for n, k in T.edge_multi(GRID):
        r = reg[(n, k)]
        assert GRID < r["tiles_f16"] < 2 * GRID, "some workgroups two fp16x3 tiles, others one"
        assert r["tiles_f32"] > 2 * GRID and n % 32 and n % 16, "the last tile is partial"
        assert r["maxabs_capped"], "maxabs3_kernel walks past its 1024 workgroups"
    assert {k % 2 for _, k in T.edge_multi(GRID)} == {0, 1}
    src = T.source("edge_bwd.hip")
    for text in ("constexpr int BT = 16;", "constexpr int FT = 32;", "constexpr int FKMAX = 64;",
                 "i < FT * k; i += 512", "ceil_div(n4, 256), 1024)", "cus = 256;"):
        assert text in src, text


def test_edge_list_lengths():
    n, k, _ = T.EDGE_LISTS + (True,)
    for r in (0, 1, 2):
        c = T.edge_case(n, k, r, True)
        lens = set((c["rev_off"][1:] - c["rev_off"][:-1]).tolist())
        assert lens >= set(T.LIST_LENGTHS), (r, sorted(lens))
        hub = int(c["rev_off"][8] - c["rev_off"][7])
        assert hub == int((c["deg"] > 0).sum()) and hub > 65 and (r != T.FIXED or hub == n)
    assert all(x in (0, 1, 2, 31, 32, 33, 64, 65) for x in T.LIST_LENGTHS)      # the 32-row batches' edges


def test_edge_variants_cover_every_kernel():
    entries = {e for v in T.EDGE_VARIANTS.values() for e in v}
    assert {("backward", "f32", False), ("ex", "f32", False), ("sorted", "f32", True), ("ex", "f16x3", False),
            ("sorted", "f16x3", False), ("sorted", "f16x3", True)} <= entries
    assert not T.edge_variant_runs("f16x3+mask", 65) and T.edge_variant_runs("f16x3", 65)


# --------------------------------------------------------------------------- B
@pytest.mark.parametrize("p", T.head_table(), ids=[T.head_name(p) for p in T.head_table()])
def test_head_case_is_exact(p):
    c = T.head_case(*p)
    ref = c["ref"]
    z1, z2, y = T.head_forward(c["h"], c["w"], torch.float32)
    assert _same(z1, ref["z1"]) and _same(z2, ref["z2"])
    t1, t2 = int((ref["z1"] == 0).sum()), int((ref["z2"][:, :, :8] == 0).sum())
    print(f"{c['name']}: exact ties z1 {t1} z2 {t2}; y exact {_same(y, ref['y'])}")
    if c["n"] >= 4097:
        assert t1 >= 1 and t2 >= 1
    if c["tied"]:
        assert not ref["z1"][c["n"] // 2, 2].any() and not c["h"][c["n"] // 2].any()
    assert T.errs(y, ref["y"])[0] <= 0.25 * T.HEAD_Y_BAR * ref["y"].abs().max().item()
    assert ref["grads"].numel() == T.HEAD_GRADS


def test_head_table_and_layout():
    t = T.head_table()
    assert {p[0] for p in t} == {1, 63, 64, 65, 128, 4097}
    assert {(p[1], p[2]) for p in t} == set(T.HEAD_LD) and any(p[3] for p in t)
    assert (4097 + 63) // 64 == 65                  # 65 wave partials: lane 0 of the sum takes a second one
    with open(os.path.join(T.ROOT, "include", "mmpde_hip.h")) as f:
        header = f.read()
    assert "[dW1 | db1 | dW2 | db2 | dW3 | db3]" in header
    assert re.search(r"#define MMPDE_HEAD_TRAIN_GRADS (\d+)", header).group(1) == str(T.HEAD_GRADS)
    assert sum(T.HEAD_SIZES) == T.HEAD_GRADS
    c = T.head_case(65, 128, 128, False)
    parts = T.head_parts(c["ref"]["grads"])
    assert [parts[n].numel() for n in T.HEAD_LAYOUT] == [t.numel() for t in c["w"]]


# --------------------------------------------------------------------------- C
def test_rows_grad_routes_name_every_instantiation():
    src = T.source("train_rows.hip")
    # the dispatch predicates rgw_route mirrors
    for text in ("const bool vec = k % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0;",
                 "return k >= 16 && k <= KMAX && k % 4 == 0 && (n_out == 1 || n_out == 2 || n_out == 4 || n_out == 8);",
                 "const bool cols = vec && rows_grad_cols_shape(k, n_out);", "else if (k <= 4)", "else if (k <= 16)",
                 "constexpr int KMAX = 64;", "MMPDE_REQUIRE(outs <= 1280);",
                 "const int64_t per_block = (int64_t)(256 / n_out) * 8;",
                 "const int64_t per_block = 32 * (int64_t)(64 / (k / 4));"):
        assert text in src, text
    launched = set(re.findall(r"launch\((rows_grad_\w+<[\w, ]+>)\)", src))
    assert len(launched) == 11, launched
    cus = 256
    t = T.rgw_table(cus)
    assert len({p["name"] for p in t}) == len(t)
    assert {p["route"] for p in t} == set(T.RGW_ROUTES) and len(T.RGW_ROUTES) == 11
    for p in t:
        outs = p["k"] * p["n_out"] + (p["n_out"] if p["db"] else 0)
        assert outs <= T.RGW_CAP and p["k"] <= 64 and p["n_out"] <= 128 and (p["k"] or p["db"])
    cols = [p for p in t if p["route"].startswith("cols")]
    for k in T.COLS_K:
        mine = [p for p in cols if p["k"] == k]
        assert {p["rows"] for p in mine} >= set(T.cols_rows(k)), k
        assert {p["n_out"] for p in mine} == set(T.COLS_NOUT)
        assert any(T.rgw_blocks(p, cus)[1] > 1 for p in mine)
        # the offset twin takes the scalar partial kernel
        twin = [p for p in t if p["k"] == k and p["x_front"] % 4]
        assert len(twin) == 1 and twin[0]["route"] == "partial<%d,scalar>" % (16 if k == 16 else 64)
        assert any(p["name"] + "-xoff1" == twin[0]["name"] for p in mine)
    assert T.cols_R(20) * 5 < 64 and T.cols_R(48) * 12 < 64            # idle lanes
    assert {p["ldx"] - p["k"] for p in cols} == {0, 4} and {p["ldy"] - p["n_out"] for p in cols} == {0, 3}
    assert {p["db"] for p in cols} == {True, False}
    part = [p for p in t if p["route"].startswith("partial")]
    assert {p["k"] for p in part} >= set(T.PART_K) and {p["n_out"] for p in part} >= set(T.PART_NOUT)
    assert any(p["k"] == 20 and p["ldx"] % 2 for p in part)
    for k, n_out in ((9, 128), (19, 64)):
        assert any(p["k"] == k and p["n_out"] == n_out and p["db"] for p in part) and k * n_out + n_out == 1280
    assert any(p["k"] * p["n_out"] == 1280 and not p["db"] for p in part)
    assert any(p["k"] == 0 for p in part) and any(not p["db"] for p in part)
    assert {p["ldy"] - p["n_out"] for p in part} == {0, 3}
    for n_out in T.PART_NOUT:
        rg = 256 // n_out
        rows = {p["rows"] for p in part if p["n_out"] == n_out}
        assert rows >= set(T.part_rows(n_out)), (n_out, rows)
        assert (n_out & (n_out - 1) == 0 and n_out <= 64) or rg * n_out <= 256
    classes = {T.part_rows(p["n_out"]).index(p["rows"]) for p in part if p["rows"] in T.part_rows(p["n_out"])}
    assert classes == set(range(6))
    cap = [p for p in t if p["name"].endswith("-blockcap")]
    g0, g = T.rgw_blocks(cap[0], cus)
    assert g0 == 4 * cus and g > 64 and cap[0]["rows"] == 16 * 4 * cus + 17
    assert any(T.rgw_blocks(p, cus)[1] == 1 for p in part) and any(1 < T.rgw_blocks(p, cus)[1] <= 64 for p in part)


@pytest.mark.parametrize("i", range(0, len(T.rgw_table(256)), 7))
def test_rows_grad_float32_floor(i):
    c = T.rgw_case(T.rgw_key(T.rgw_table(256)[i]))
    for name in ("dw", "db"):
        s = c["ref"][name].abs().max().item() if c["ref"][name].numel() else 0.0
        assert T.errs(c["cpu32"][name], c["ref"][name])[0] <= 0.25 * T.RGW_BAR * s, (c["name"], name)
    if c["k"]:
        x = T.D.view(c["bufs"]["x"], c["at"]["x"], c["rows"], c["k"], c["ldx"])
        assert torch.equal(x, c["x"]) and c["bufs"]["x"].isnan().sum() == c["bufs"]["x"].numel() - x.numel()


def test_reverse_adjacency_cases():
    cases = [T.rev_case(i) for i in range(len(T.REV))]
    assert {c["n_src"] for c in cases} >= {1, 2, 255, 256, 257, 65535, 65536, 65537}
    assert {T.key_bits(n) for n in (255, 256, 65535, 65536)} == {8, 9, 16, 17}
    src = T.source("train_rows.hip")
    assert "while (b < 31 && ((int64_t)1 << b) <= n_src) ++b;" in src
    for c in cases:
        if c["n_src"] in (65535, 65536, 65537):
            assert 69000 <= c["slots"] <= 71000
    assert any(c["n_tgt"] > c["n_src"] and c["k"] == 1 for c in cases)
    assert any(c["n_tgt"] == 3 and c["n_src"] == 70000 for c in cases)
    assert {c["slots"] for c in cases} >= {255, 256, 257}
    assert any(c["n_live"] == 0 and c["bad"] == 0 for c in cases)
    assert any(c["deg"] is None and len(set(c["nbr"].reshape(-1).tolist())) == 1 for c in cases)
    assert any(c["n_src"] == 1 and c["n_live"] == c["slots"] for c in cases)
    assert any(c["pattern"] == "inner" and int(c["rev_off"][1]) == 0 and
               int(c["rev_off"][-1] - c["rev_off"][-2]) == 0 and c["n_live"] > 0 for c in cases)
    assert any(c["bad"] > 0 for c in cases)
    # a case at n_src = 256 whose dead slots must sort past key 255 (a key one bit short would not)
    assert any(c["n_src"] == 256 and c["n_live"] < c["slots"] for c in cases)
    for c in cases:
        pos = c["slot_pos"].long()
        assert torch.equal(torch.sort(pos).values, torch.arange(c["slots"]))
        assert torch.equal(pos[c["rev_edge"]], torch.arange(c["slots"]))
        assert int(c["rev_off"][-1]) == c["n_live"] and c["rev_off"].numel() == c["n_src"] + 1
