"""The cell-binned radius graph (radius_binned_kernel, csrc/knn_bins.hip):
ops.radius_graph_nbr with method="binned".

Bars: nbr and deg torch.equal to method="scan" on the same input and to the C
oracle (refcpu.radius_graph); no tolerance anywhere.  The shapes are the
smallest at which the design can go wrong: selection across more than one
batch of 64 hits, every query on the index-order fallback, per-trajectory
grids, points at distance exactly r and exactly on cell boundaries, coincident
runs that saturate a row by index order, zero-size and zero-width boxes, one
heavy cell beside sparse ones, a box blown up by one far point, trajectories
around the row width, the neighbour limits.  The work cap keeps a search that
scans everything from passing.
"""
import math

import pytest
import torch

from oracle import refcpu

pytestmark = pytest.mark.gpu


def _stats(dev):
    return torch.zeros((2,), dtype=torch.int64, device=dev)


def _case(pos, B, r, dev, mnn=32, stats=None, bins=None):
    """Binned == scan == oracle, nbr and deg; returns the oracle's (nbr, deg)."""
    from mmpde_amd import ops

    p = pos.to(dev)
    nbr, deg = ops.radius_graph_nbr(p, B, r, mnn, method="binned", stats=stats, bins=bins)
    snbr, sdeg = ops.radius_graph_nbr(p, B, r, mnn)
    _, rn, rd = refcpu.radius_graph(pos, r, B, mnn)
    assert nbr.shape == (pos.shape[0], mnn + 1) and nbr.dtype == torch.int32
    assert torch.equal(deg, sdeg)
    assert torch.equal(nbr, snbr)
    assert torch.equal(deg.cpu().long(), rd)
    assert torch.equal(nbr.cpu().long(), rn)
    return rn, rd


@pytest.fixture(scope="module")
def uniform():
    g = torch.Generator().manual_seed(8)
    return torch.rand(4097, 2, generator=g)


def _hits(pos, r):
    """Points within r of every point (itself included), fp64 on the host."""
    p = pos.double()
    return torch.cat([(torch.cdist(c, p) < r).sum(1) for c in p.split(1024)])


# ============================================================================ paths
def test_few_hits_and_work_cap(dev, uniform):
    """r below the cell side (1/32): no row saturates, a block of at most 3 x 3
    cells of about 4 points; nothing takes the index-order scan."""
    st = _stats(dev)
    _, rd = _case(uniform, 1, 0.0305, dev, stats=st)
    assert int(rd.max()) < 32 and 8 < rd.float().mean().item() < 16
    n = uniform.shape[0]
    per = int(st[0].item()) / n
    print(f"r = 0.0305: examined {per:.1f} points per query (n_per = {n}), mean degree {rd.float().mean():.1f}")
    assert per <= n / 8 and int(st[1].item()) == 0


def test_many_hits_cross_batches_of_64(dev, uniform):
    """r = 0.08: most queries have more than 64 hits (the running selection
    merges more than one batch) and saturate at the first 33 in index order;
    r = 0.12: more than 128 (three and more batches, the later ones thinned by
    the running 33rd smallest), the block still under the fallback share."""
    for r, most, top in ((0.08, 64, 100), (0.12, 128, 200)):
        h = _hits(uniform, r)
        assert (h > most).float().mean().item() > 0.5 and int(h.max()) > top
        st = _stats(dev)
        _, rd = _case(uniform, 1, r, dev, stats=st)
        assert (rd >= 32).float().mean().item() > 0.9
        assert int(st[1].item()) == 0


def test_fallback_and_work_cap(dev, uniform):
    """r = 1.5 covers the unit square: every query's block is the whole grid,
    every query takes the index-order scan, which saturates in its first step."""
    st = _stats(dev)
    _, rd = _case(uniform, 1, 1.5, dev, stats=st)
    n = uniform.shape[0]
    assert int(rd.min()) == 32
    per = int(st[0].item()) / n
    print(f"r = 1.5: examined {per:.1f} points per query, {int(st[1].item())} of {n} on the scan")
    assert int(st[1].item()) == n and per <= 128


def test_per_trajectory_boxes(dev):
    """Three trajectories with their own boxes and scales: per-trajectory grids,
    global indices with the batch offset, a box far from the origin."""
    torch.manual_seed(3)
    pos = torch.rand(3, 700, 2)
    pos[1] = pos[1] * 100.0 + 500.0
    pos[2] = pos[2] * torch.tensor([0.01, 3.0]) - 7.0
    _case(pos.reshape(-1, 2), 3, 0.06, dev)
    _, rd = _case(pos.reshape(-1, 2), 3, 4.0, dev)
    assert int(rd.reshape(3, -1).sum(1).min()) > 0      # every trajectory has edges at this r


def test_integer_lattice_exact_distances_and_boundaries(dev):
    """49 x 49 lattice on integer coordinates, 48 intervals = 2 x the 24-cell
    grid: every other grid line lies exactly on a cell boundary, and r = 1, 2,
    sqrt(10) put lattice points at distance exactly r (strict '<': outside)."""
    from mmpde_amd import ops

    side = 49
    g = ops.knn_bins_grid(side * side)
    assert g > 1 and (side - 1) % g == 0
    j = torch.arange(side, dtype=torch.float32)
    gx, gy = torch.meshgrid(j, j, indexing="ij")
    pos = torch.stack((gx, gy), 2).reshape(-1, 2)
    inner = (24 * side + 24)
    for r, want in ((1.0, 0), (2.0, 8), (math.sqrt(10.0), None)):
        _, rd = _case(pos, 1, r, dev)
        if want is not None:
            assert int(rd[inner]) == want
    # float(sqrt(10))^2 in double rounds to a float above or below 10: whichever, all three agree


def test_coincident_run_saturates_by_index_order(dev):
    """81 coincident points at consecutive indices: their rows hold the run's
    first 33 indices (itself dropped), whatever the order inside the cell."""
    torch.manual_seed(11)
    pos = torch.rand(400, 2)
    pos[100:181] = pos[3]
    rn, rd = _case(pos, 1, 0.05, dev)
    assert int(rd[150]) == 33 and 3 in rn[150].tolist() and 150 not in rn[150].tolist()
    # and with the run larger than two batches of 64
    pos = torch.rand(1000, 2)
    pos[400:600] = pos[5]
    _case(pos, 1, 0.02, dev)


def test_degenerate_boxes(dev):
    """100 coincident points (a zero-size box, one cell); a vertical line (one
    axis of zero extent) and a diagonal."""
    _, rd = _case(torch.full((100, 2), 0.375), 1, 0.1, dev)
    assert int(rd.min()) == 32
    torch.manual_seed(5)
    t = torch.rand(500)
    _case(torch.stack((torch.full_like(t, 0.25), t), 1), 1, 0.02, dev)
    _case(torch.stack((t, 2.0 * t + 1.0), 1), 1, 0.05, dev)


def test_cluster_and_sparse(dev):
    """3700 points in a 0.01-wide box and 300 spread over the unit square: the
    heavy cells' queries exceed the fallback share and scan, the sparse ones
    stay on the bins, in one launch."""
    torch.manual_seed(7)
    pos = torch.cat((0.6 + 0.01 * torch.rand(3700, 2), torch.rand(300, 2)))
    pos = pos[torch.randperm(4000)]
    for r in (0.004, 0.05):
        st = _stats(dev)
        _case(pos, 1, r, dev, stats=st)
        assert 0 < int(st[1].item()) < 4000


def test_far_outlier(dev):
    """One point at (1000, 1000): the box puts nearly every other point in one cell."""
    torch.manual_seed(9)
    pos = torch.cat((torch.rand(2000, 2), torch.tensor([[1000.0, 1000.0]])))
    _, rd = _case(pos, 1, 0.03, dev)
    assert int(rd[-1]) == 0


@pytest.mark.parametrize("n", [7, 33, 34, 40])
def test_small_trajectories(dev, n):
    """n_per below, at and above the row width w = 33 (grids of one and 2 x 2
    cells: every query scans), and 40 (3 x 3 cells: the smallest trajectories
    with queries on the bins), r covering all and few."""
    torch.manual_seed(n)
    pos = torch.rand(2 * n, 2)
    for r in (2.0, 0.2, 0.05):
        _case(pos, 2, r, dev)


@pytest.mark.parametrize("mnn", [1, 63])
def test_neighbour_limits(dev, mnn):
    torch.manual_seed(mnn)
    pos = torch.rand(2 * 900, 2)
    for r in (0.05, 0.2):
        _case(pos, 2, r, dev, mnn=mnn)


def test_one_binning_serves_knn_and_radius(dev):
    """Bins built once, searched by the kNN-35 graph, the kNN-30 query and the
    radius graph."""
    from mmpde_amd import ops

    torch.manual_seed(6)
    B, n = 2, 1500
    pos, qry = torch.rand(B * n, 2), torch.rand(B * 40, 2)
    bins = ops.knn_bins(pos.to(dev), B)
    keep = bins.clone()
    nbr = ops.knn_graph_nbr(pos.to(dev), B, 35, method="binned", bins=bins)
    idx = ops.knn_query(pos.to(dev), qry.to(dev), B, 30, method="binned", bins=bins)
    _case(pos, B, 0.05, dev, bins=bins)
    assert torch.equal(bins, keep)          # the searches only read them
    assert torch.equal(nbr.cpu().long(), refcpu.knn_graph(pos, 35, B)[1])
    ref = refcpu.knn_query(pos, qry, B, 30)
    assert torch.equal(idx.cpu().long().reshape(ref.shape), ref)


def test_moved_lattice(dev):
    """The rollout's input shape: a 65 x 65 lattice moved by a tenth of its
    spacing, at the reference's radius for neighbors = 2."""
    from mmpde_amd.synth import burgers_grid_points

    side = 65
    g = torch.Generator().manual_seed(8)
    xi = burgers_grid_points(side)
    pos = torch.cat([xi + (0.1 / (side - 1)) * torch.randn(xi.shape, generator=g) for _ in range(2)])
    x = torch.linspace(0, 1, side)
    dx = x[1] - x[0]
    r = float(2 * torch.sqrt(dx ** 2 + dx ** 2) + 0.0001)
    st = _stats(dev)
    _, rd = _case(pos, 2, r, dev, stats=st)
    assert int(st[1].item()) == 0 and 15 < rd.float().mean().item() < 32


# ============================================================================ limits
def test_limits(dev):
    from mmpde_amd import _lib, ops

    big = torch.zeros((65537, 2), device=dev)
    pts = big[:100]
    with pytest.raises(ValueError, match="65536"):
        ops.radius_graph_nbr(big, 1, 0.1, method="binned")
    with pytest.raises(ValueError):
        ops.radius_graph_nbr(pts, 1, 0.1, method="cells")
    with pytest.raises(ValueError):
        ops.radius_graph_nbr(pts, 1, 0.1, 64, method="binned")
    with pytest.raises(ValueError):
        ops.radius_graph_nbr(pts, 1, 0.0, method="binned")
    with pytest.raises(ValueError):
        ops.radius_graph_nbr(pts, 1, 0.1, bins=ops.knn_bins(pts, 1))          # bins with "scan"
    with pytest.raises(ValueError):
        ops.radius_graph_nbr(pts, 1, 0.1, method="binned",
                             bins=torch.empty((16,), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        ops.radius_graph_nbr(pts, 1, 0.1, method="binned", stats=torch.zeros(2, device=dev))
    lib = _lib.lib()
    p = big.data_ptr()
    out = torch.empty((100 * 64,), dtype=torch.int32, device=dev).data_ptr()
    f = lib.mmpde_radius_graph_binned
    assert f(None, p, 1, 100, 0.1, 32, out, out, None, None) == -1
    assert f(p, None, 1, 100, 0.1, 32, out, out, None, None) == -1
    assert f(p, p, 1, 100, 0.1, 32, None, out, None, None) == -1
    assert f(p, p, 1, 100, 0.1, 32, out, None, None, None) == -1
    assert f(p, p + 4, 1, 100, 0.1, 32, out, out, None, None) == -1       # bins not 8-byte aligned
    assert f(p, p, 1, 65537, 0.1, 32, out, out, None, None) == -1
    assert f(p, p, 1, 0, 0.1, 32, out, out, None, None) == -1
    assert f(p, p, 1, 100, 0.1, 64, out, out, None, None) == -1
    assert f(p, p, 1, 100, 0.1, 0, out, out, None, None) == -1
    assert f(p, p, 1, 100, 0.0, 32, out, out, None, None) == -1
    assert f(p, p, 1, 100, -1.0, 32, out, out, None, None) == -1
    assert f(p, p, 0, 100, 0.1, 32, out, out, None, None) == -1
    assert f(p, p, 65536, 100, 0.1, 32, out, out, None, None) == -1
    torch.cuda.synchronize()


# ============================================================================ graph creator
def test_graph_creator_radius_method_and_fixed_graph(dev):
    """create_graph with radius_method "binned" builds the scan's graph, and the
    cached fixed-grid graph honours connect_edge."""
    from mmpde_amd.synth import build_models, fields

    pde, _, _, _, _, gc = build_models("cy", moving_mesh=False)
    gc.e, gc.n = "radius", 2
    B, step = 2, 3
    u = fields(pde.ori_grid, B, 30)
    data, labels = gc.create_data(u, [step] * B)
    scan = gc.create_graph(None, data, labels, [step] * B, dev, None)
    gc.radius_method = "binned"
    binned = gc.create_graph(None, data, labels, [step] * B, dev, None)
    assert torch.equal(binned.nbr, scan.nbr) and torch.equal(binned.deg, scan.deg)
    grid = gc.uniform_grid(dev)
    nbr, deg = gc.fixed_graph(grid, B)
    assert torch.equal(nbr, scan.nbr) and torch.equal(deg, scan.deg)
    assert gc.fixed_graph(grid, B)[0] is nbr                      # cached
    gc.e, gc.n = "knn", 35
    nbr, deg = gc.fixed_graph(grid, B)
    assert deg is None and nbr is gc.fixed_graph_nbr(grid, B)
    gc.e = "delaunay"
    with pytest.raises(ValueError):
        gc.fixed_graph(grid, B)
