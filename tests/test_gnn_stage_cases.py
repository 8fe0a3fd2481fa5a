"""CPU-only check of the inputs of test_gpu_node_shapes.py: every case builds,
its float64 rows are large enough for a row-relative error, the ragged and
per-row-t properties the device tests rely on are really there, and the
float32 CPU oracle's own errors against float64 stay below the two floors
recorded in gnn_stage_cases.py (the device bars are 4 x those floors)."""
import pytest
import torch

import gnn_stage_cases as C

IDS = [C.case_id(c) for c in C.CASES]


def test_case_table():
    assert len(set(C.CASES)) == len(C.CASES) and len(set(IDS)) == len(IDS)
    main = {(c.n, c.tw, c.depth) for c in C.MAIN}
    assert main == {(n, tw, d) for n in (1, 15, 16, 17, 31, 32, 33, 65) for tw in (1, 2, 16) for d in (1, 2, 3)}
    assert all(c.k == 5 and not c.ragged and c.scales == C.UNIT for c in C.MAIN)
    assert {(c.n, c.tw) for c in C.RAGGED if c.k == 5} == {(n, tw) for n in (17, 33, 65) for tw in (1, 3)}
    assert sum(c.k == 35 for c in C.RAGGED) == 1 and all(c.ragged and c.depth == 2 for c in C.RAGGED)
    assert {(c.tw, c.scales) for c in C.NONUNIT} == {(tw, s) for tw in (1, 3) for s in C.SCALES}
    assert all(c.n == 33 and c.depth == 2 for c in C.NONUNIT)
    assert [(c.n, c.seg_n, c.depth) for c in C.SEGMENTS] == [(96, 32, 2), (111, 37, 2)]
    assert [(c.n, c.tw, c.depth) for c in C.DEPTH0] == [(1, 1, 0), (33, 1, 0)]
    assert all(c in C.CASES for c in C.CONST_T) and {c.n for c in C.CONST_T} == {17, 33}


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_case_builds(c):
    d = C.graph(c)
    n, k = c.n, c.k
    assert d.u.shape == (n, c.tw) and d.pos.shape == (n, 3) and d.nbr.shape == (n, k)
    assert d.u.dtype == d.pos.dtype == torch.float32 and d.nbr.dtype == torch.int32
    t = d.pos[:, 0]
    assert t.unique().numel() == n and float(t.min()) > 0.0 and float(t.max()) < c.scales[2]
    assert float(d.pos[:, 1].max()) < c.scales[0] and float(d.pos[:, 2].max()) < c.scales[1]
    seg = c.seg_n or n
    if c.ragged:
        assert d.deg.dtype == torch.int32 and int(d.deg.min()) == 0 and int(d.deg.max()) == k
        live = torch.arange(k)[None, :] < d.deg[:, None]
        assert bool((d.nbr[~live] == -1).all()) and int(d.nbr[live].min()) >= 0
        assert d.edge_index.shape == (2, int(d.deg.sum()))
    else:
        assert d.deg is None and d.edge_index.shape == (2, n * k)
    src, tgt = d.edge_index
    assert int(src.min()) >= 0 and int(src.max()) < n and bool((src // seg == tgt // seg).all())
    assert bool((tgt[1:] >= tgt[:-1]).all())
    model = C.solver(c.tw, c.depth, *c.scales)
    assert len(model.gnn_layers) == c.depth and not model.training
    assert (model.pde.Lx, model.pde.Ly, model.pde.tmax) == c.scales
    out64, hs64 = C.reference(c)
    assert out64.shape == (n, c.tw) and out64.dtype == torch.float64
    assert len(hs64) == c.depth + 1 and all(h.shape == (n, 128) for h in hs64)
    mags = [hs64[i].abs().amax(1).min().item() for i in {0, c.depth}]
    assert min(mags) >= C.MIN_ROW_MAG, mags
    if c.tw > 1:
        # the cumsum(dt) epilogue: the output columns differ
        assert float((out64[:, 1:] - out64[:, :1]).abs().max()) > 0.0


def test_const_t_variant_shares_everything_but_t():
    for c in C.CONST_T:
        a, b = C.graph(c), C.graph(c, True)
        assert torch.equal(a.u, b.u) and torch.equal(a.nbr, b.nbr) and torch.equal(a.pos[:, 1:], b.pos[:, 1:])
        assert b.pos[:, 0].unique().numel() == 1


def test_fp32_oracle_stays_below_the_recorded_floors():
    worst_h = worst_out = (0.0, None)
    for c in C.CASES:
        out64, hs64 = C.reference(c)
        out32, hs32 = C.reference(c, torch.float32)
        assert out32.dtype == torch.float32
        for i in {0, c.depth}:
            worst_h = max(worst_h, (C.row_rel_err(hs32[i], hs64[i])[0], C.case_id(c)))
        worst_out = max(worst_out, (C.out_rel_err(out32, out64), C.case_id(c)))
    print(f"fp32 CPU oracle vs float64 over {len(C.CASES)} cases: row-relative h {worst_h[0]:.3e} ({worst_h[1]}), "
          f"out {worst_out[0]:.3e} of max|out64| ({worst_out[1]}); floors {C.FP32_FLOOR_H:.2e} {C.FP32_FLOOR_OUT:.2e}")
    assert worst_h[0] <= C.FP32_FLOOR_H
    assert worst_out[0] <= C.FP32_FLOOR_OUT
    # a recorded floor far above the oracle's error would loosen the device bars
    assert worst_h[0] >= 0.5 * C.FP32_FLOOR_H and worst_out[0] >= 0.5 * C.FP32_FLOOR_OUT


def test_row_rel_err():
    h64 = torch.tensor([[1.0, -2.0], [0.5, 0.25]], dtype=torch.float64)
    h = h64.clone()
    h[0, 0] += 0.2
    h[1, 1] -= 0.05
    mx, rms = C.row_rel_err(h, h64)
    assert abs(mx - 0.1) < 1e-12 and abs(rms - (0.5 * (0.1 ** 2 + 0.1 ** 2)) ** 0.5) < 1e-12
