"""The cell-binned exact kNN (the binning kernels, csrc/knn_bins.hip;
knn_binned_kernel, csrc/knn.hip):
ops.knn_graph_nbr / ops.knn_query with method="binned", and the rollout's
knn_binned routing.

Bars: every index table torch.equal to the C oracle (oracle/knn_oracle.c) and
to method="full" on the same input; the degenerate and ties counts equal; no
tolerance anywhere.  The shapes are the smallest at which the design can go
wrong: one cell, per-trajectory grids, points exactly on cell boundaries with
the cut inside a tie shell that spans cells, list overflow, zero-size and
zero-width boxes, one heavy cell beside sparse ones, a box blown up by one far
point, queries outside the box, the sizes where "full" changes kernel.  The
work cap keeps a search that scans everything from passing.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import refcpu

pytestmark = pytest.mark.gpu

GOLDEN = f"{ROOT}/tests/golden"


def _stats(dev):
    return torch.zeros((2,), dtype=torch.int64, device=dev)


def _graph_case(pos, B, dev, k=35, stats=None):
    """Binned graph == oracle == full, degenerate counts too; returns the count."""
    from mmpde_amd import ops

    p = pos.to(dev)
    nbr, deg = ops.knn_graph_nbr(p, B, k, count_degenerate=True, method="binned", stats=stats)
    full, fdeg = ops.knn_graph_nbr(p, B, k, count_degenerate=True)
    _, ref, rdeg = refcpu.knn_graph(pos, k, B)
    assert torch.equal(nbr, full)
    assert torch.equal(nbr.cpu().long(), ref)
    assert int(deg.item()) == rdeg == int(fdeg.item())
    return rdeg


def _query_case(src, qry, B, dev, k=30, stats=None):
    """Binned query == oracle == full, ties counts too; returns the count."""
    from mmpde_amd import ops

    s, q = src.to(dev), qry.to(dev)
    ties = torch.zeros((1,), dtype=torch.int32, device=dev)
    fties = torch.zeros_like(ties)
    idx = ops.knn_query(s, q, B, k, ties=ties, method="binned", stats=stats)
    full = ops.knn_query(s, q, B, k, ties=fties)
    ref = refcpu.knn_query(src, qry, B, k)
    assert torch.equal(idx, full)
    assert torch.equal(idx.cpu().long().reshape(ref.shape), ref)
    assert int(ties.item()) == int(fties.item())
    return int(ties.item())


def _moved_lattice(side, seed):
    from mmpde_amd.synth import burgers_grid_points

    g = torch.Generator().manual_seed(seed)
    xi = burgers_grid_points(side)
    return xi, xi + (0.1 / (side - 1)) * torch.randn(xi.shape, generator=g)


# ============================================================================ graph, k = 35
@pytest.mark.parametrize("n", [36, 37])
def test_graph_one_cell(dev, n):
    """n = kk (every point a neighbour of every other) and one more."""
    torch.manual_seed(n)
    _graph_case(torch.rand(n, 2), 1, dev)


def test_graph_per_trajectory_boxes(dev):
    """Three trajectories with their own boxes and scales: per-trajectory grids,
    global indices with the batch offset, a box far from the origin."""
    torch.manual_seed(3)
    pos = torch.rand(3, 700, 2)
    pos[1] = pos[1] * 100.0 + 500.0
    pos[2] = pos[2] * torch.tensor([0.01, 3.0]) - 7.0
    _graph_case(pos.reshape(-1, 2), 3, dev)


def test_graph_lattice_on_cell_boundaries(dev):
    """49 x 49 lattice, 48 intervals per side = 2 x the 24-cell grid: every other
    grid line lies exactly on a cell boundary, and the 35th neighbour sits in
    the 8-point d^2 = 10 shell, whose members fall into different cells."""
    from mmpde_amd import ops
    from mmpde_amd.synth import burgers_grid_points

    side = 49
    g = ops.knn_bins_grid(side * side)
    assert g > 1 and (side - 1) % g == 0
    _graph_case(burgers_grid_points(side), 1, dev)
    # the same on exact coordinates (integers): exact ties, exact boundaries
    j = torch.arange(side, dtype=torch.float32)
    gx, gy = torch.meshgrid(j, j, indexing="ij")
    _graph_case(torch.stack((gx, gy), 2).reshape(-1, 2), 1, dev)


def test_graph_integer_lattice_golden(dev):
    from mmpde_amd import ops

    g = np.load(f"{GOLDEN}/knn35_lattice.npz")
    pos = torch.from_numpy(g["pos"])
    nbr = ops.knn_graph_nbr(pos.to(dev), 1, 35, method="binned")
    assert np.array_equal(nbr.cpu().numpy(), g["nbr"])
    _graph_case(pos, 1, dev)


def test_graph_coincident_run_overflows(dev):
    """300 of 1000 points coincide at consecutive indices: their candidate
    lists overflow into the full select (stats[1]), the threshold ties go in
    index order, and most of the run does not find itself (degenerate)."""
    torch.manual_seed(11)
    pos = torch.rand(1000, 2)
    pos[400:700] = pos[5]
    st = _stats(dev)
    assert _graph_case(pos, 1, dev, stats=st) >= 300 - 36
    assert int(st[1].item()) > 0


def test_graph_zero_size_box(dev):
    """100 coincident points: a box of zero extent, one cell."""
    _graph_case(torch.full((100, 2), 0.375), 1, dev)


def test_graph_collinear(dev):
    """500 points on a vertical line (one axis of zero extent) and on a diagonal."""
    torch.manual_seed(5)
    t = torch.rand(500)
    _graph_case(torch.stack((torch.full_like(t, 0.25), t), 1), 1, dev)
    _graph_case(torch.stack((t, 2.0 * t + 1.0), 1), 1, dev)


def test_graph_cluster_and_sparse(dev):
    """3700 points in a 0.01-wide box and 300 spread over the unit square: many
    rings for the sparse queries, one heavy cell for the others."""
    torch.manual_seed(7)
    pos = torch.cat((0.6 + 0.01 * torch.rand(3700, 2), torch.rand(300, 2)))
    _graph_case(pos[torch.randperm(4000)], 1, dev)


def test_graph_far_outlier(dev):
    """One point at (1000, 1000): the box puts nearly every other point in one cell."""
    torch.manual_seed(9)
    pos = torch.cat((torch.rand(2000, 2), torch.tensor([[1000.0, 1000.0]])))
    _graph_case(pos, 1, dev)


@pytest.mark.parametrize("k", [1, 63])
def test_graph_k_limits(dev, k):
    torch.manual_seed(k)
    _graph_case(torch.rand(2 * 900, 2), 2, dev, k=k)


@pytest.mark.parametrize("n", [4097, 16385])
def test_graph_where_full_changes_kernel(dev, n):
    torch.manual_seed(n)
    _graph_case(torch.rand(2 * n, 2), 2, dev)


# ============================================================================ query, k = 30
def test_query_small_shapes(dev):
    """n_src = k; one and three queries onto 500 points."""
    torch.manual_seed(2)
    _query_case(torch.rand(30, 2), torch.rand(17, 2), 1, dev)
    src = torch.rand(500, 2)
    _query_case(src, torch.rand(1, 2), 1, dev)
    _query_case(src, torch.rand(3, 2), 1, dev)


def test_query_on_source_points_and_outside_the_box(dev):
    """Queries equal to source points; queries 0.5 and 10 box extents outside,
    on every side."""
    torch.manual_seed(4)
    src = torch.rand(2 * 800, 2)
    _query_case(src, src.clone(), 2, dev)
    q = torch.rand(2 * 64, 2)
    off = torch.tensor([[1.5, 0.0], [-1.5, 0.0], [0.0, 1.5], [0.0, -1.5], [1.5, -1.5], [11.0, 0.0], [-11.0, 11.0],
                        [0.0, -11.0]])
    _query_case(src, q + off.repeat(16, 1), 2, dev)


def test_query_tie_counter(dev):
    """49 x 49 lattice: half the queries on lattice points (ties), half at
    jittered cell centres (none): the ties count against a numpy fp64 brute
    force over every source point."""
    from mmpde_amd.synth import burgers_grid_points

    src = burgers_grid_points(49)
    g = torch.Generator().manual_seed(5)
    qry = src[torch.randperm(src.shape[0], generator=g)[:300]].clone()
    qry[150:] += 0.5 / 48.0 + 1e-3 * torch.rand(150, 2, generator=g)
    s, q = src.double().numpy(), qry.double().numpy()
    dx, dy = q[:, None, 0] - s[None, :, 0], q[:, None, 1] - s[None, :, 1]
    d = np.sort(dx * dx + dy * dy, axis=1)[:, :31]
    want = int(np.any(d[:, 1:] == d[:, :-1], axis=1).sum())
    assert 100 < want < 300
    assert _query_case(src, qry, 1, dev) == want


@pytest.mark.parametrize("ns,nq", [(16385, 300), (36864, 200)])
def test_query_where_full_changes_kernel(dev, ns, nq):
    B = 2
    torch.manual_seed(ns + nq)
    src, qry = torch.rand(B * ns, 2), torch.rand(B * nq, 2)
    qry[:3] = src[:3]
    _query_case(src, qry, B, dev)


def test_one_binning_serves_graph_and_query(dev):
    """Bins built once, into a caller's workspace, searched by both kinds."""
    from mmpde_amd import _lib, ops

    torch.manual_seed(6)
    B, n = 2, 1500
    pos, qry = torch.rand(B * n, 2), torch.rand(B * 40, 2)
    ws = torch.empty((_lib.lib().mmpde_knn_bins_bytes(B, n) + 64,), dtype=torch.uint8, device=dev)
    bins = ops.knn_bins(pos.to(dev), B, out=ws)
    assert bins.data_ptr() == ws.data_ptr()
    nbr = ops.knn_graph_nbr(pos.to(dev), B, 35, method="binned", bins=bins)
    idx = ops.knn_query(pos.to(dev), qry.to(dev), B, 30, method="binned", bins=bins)
    assert torch.equal(nbr.cpu().long(), refcpu.knn_graph(pos, 35, B)[1])
    ref = refcpu.knn_query(pos, qry, B, 30)
    assert torch.equal(idx.cpu().long().reshape(ref.shape), ref)


# ============================================================================ work cap
@pytest.mark.parametrize("kind", ["uniform", "lattice"])
def test_work_cap(dev, kind):
    """The search examines a neighbourhood, not the trajectory: at most
    n_per / 8 points per query on average, and no list overflows.  (A numpy
    model of the stopping rule examined 93-158.)"""
    if kind == "uniform":
        torch.manual_seed(8)
        pos, qry = torch.rand(4097, 2), torch.rand(4097, 2)
    else:
        qry, pos = _moved_lattice(65, 8)        # the fixed lattice queried onto the moved one
    n = pos.shape[0]
    st = _stats(dev)
    _graph_case(pos, 1, dev, stats=st)
    per = int(st[0].item()) / n
    print(f"{kind}: graph examined {per:.1f} points per query (n_per = {n})")
    assert per <= n / 8 and int(st[1].item()) == 0
    assert per >= 36
    st = _stats(dev)
    _query_case(pos, qry, 1, dev, stats=st)
    per = int(st[0].item()) / qry.shape[0]
    print(f"{kind}: query examined {per:.1f} points per query (n_per = {n})")
    assert per <= n / 8 and int(st[1].item()) == 0
    assert per >= 30


# ============================================================================ limits
def test_limits(dev):
    from mmpde_amd import _lib, ops

    big = torch.zeros((65537, 2), device=dev)
    with pytest.raises(ValueError, match="65536"):
        ops.knn_graph_nbr(big, 1, 35)                        # the message "full" raises
    for call in (lambda: ops.knn_graph_nbr(big, 1, 35, method="binned"),
                 lambda: ops.knn_query(big, big[:10], 1, 30, method="binned"),
                 lambda: ops.knn_bins(big, 1)):
        with pytest.raises(ValueError, match="65536"):
            call()
    with pytest.raises(ValueError):
        ops.knn_graph_nbr(big[:100], 1, 35, method="cells")
    with pytest.raises(ValueError):
        ops.knn_bins(big[:100], 1, out=torch.empty((16,), dtype=torch.uint8, device=dev))
    lib = _lib.lib()
    p = big.data_ptr()
    out = torch.empty((64,), dtype=torch.int32, device=dev).data_ptr()
    inv = lib.mmpde_knn_graph(p, 1, 65537, 35, out, None, None)
    assert inv == -1
    assert lib.mmpde_knn_bin(p, 1, 65537, p, 1 << 30, None) == inv
    assert lib.mmpde_knn_graph_binned(p, p, 1, 65537, 35, out, None, None, None) == inv
    assert lib.mmpde_knn_query_binned(p, p, p, 1, 65537, 1, 30, out, None, None, None) == inv
    need = lib.mmpde_knn_bins_bytes(1, 1000)
    assert lib.mmpde_knn_bin(p, 1, 1000, p, need - 1, None) == inv       # workspace too small
    torch.cuda.synchronize()


# ============================================================================ rollout
def _engine(kind, dev, grid=None, B=2):
    from mmpde_amd.rollout import MMPDERollout
    from mmpde_amd.synth import build_models, burgers_grid_points, fields

    pde, model, model_b, itp, dmm, gc = build_models(kind, grid=grid) if grid is not None else build_models(kind)
    if kind == "cy":
        u0 = fields(pde.ori_grid, B, 30)[:, 3]
    else:
        u0 = fields(burgers_grid_points(), B, 31).reshape(B, 31, 48, 48)[:, 3]
    for m in (model, model_b, itp, dmm):
        m.to(dev)
    return MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev), u0.to(dev).contiguous()


def _run(eng, u0, binned, steps=3):
    eng.knn_binned = binned
    u, keep = u0, []
    for s in range(4, 4 + steps):
        u = eng.step(u, s)
        torch.cuda.synchronize()
        keep.append((u.clone(), eng.nbr_m.clone(), eng.idx2.clone(),
                     eng.idx1.clone() if eng.kind == "burgers" else None))
    return keep


def _same(a, b):
    for s, (x, y) in enumerate(zip(a, b)):
        for name, t, w in zip(("pred", "nbr_m", "idx2", "idx1"), x, y):
            assert (t is None and w is None) or torch.equal(t, w), (s, name)


def test_rollout_routes_large_meshes_through_bins(dev):
    """A 4500-point cylinder mesh has no candidate table: binned by default,
    and three steps equal the same engine with it off; then one graph-captured
    step with it on equals the eager one."""
    from mmpde_amd import ops
    from mmpde_amd.synth import generate_cy_mesh

    eng, u0 = _engine("cy", dev, grid=generate_cy_mesh(n=4500))
    assert eng.knn_cand is None and eng.N >= ops.KNN_BINNED_MIN_POINTS
    assert eng.knn_binned is True
    on = _run(eng, u0, True)
    assert set(eng.knn_modes().values()) == {"binned"}
    off = _run(eng, u0, False)
    assert "binned" not in eng.knn_modes().values()
    _same(on, off)
    eng.knn_binned = True
    eng.enable_graph(u0)
    g = eng.graph_step(u0, 4)
    torch.cuda.synchronize()
    assert torch.equal(g, on[0][0])
    assert torch.equal(eng.nbr_m, on[0][1]) and torch.equal(eng.idx2, on[0][2])


@pytest.mark.parametrize("kind", ["burgers", "cy"])
def test_rollout_small_meshes_default_off_forced_on(dev, kind):
    """Burgers 48 x 48 and the 2521-point cylinder keep their candidate tables
    by default; forced through the bins they compute the same step, idx1 (the
    static fixed-grid bins) included."""
    eng, u0 = _engine(kind, dev)
    assert eng.knn_binned is False
    off = _run(eng, u0, False)
    assert "binned" not in eng.knn_modes().values()
    on = _run(eng, u0, True)
    assert set(eng.knn_modes().values()) == {"binned"}
    _same(on, off)
