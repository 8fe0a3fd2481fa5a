"""The tiled kNN path (knn_tiled_kernel, csrc/knn.hip): trajectories of more
than 16384 points, up to ops.KNN_MAX_POINTS = 65536, searched from LDS tiles
of T = ops.KNN_TILE_POINTS points in two passes.

Bars: every index table bit-exact against the C oracle (oracle/knn_oracle.c),
the degenerate and ties counts exact.  The shapes are the smallest at which
the path can go wrong: one point past the old limit (which, T dividing 16384,
is also a last tile of one point), batch offsets, lattice ties at the cut
spanning tiles, coincident runs across a tile boundary (list overflow: the
radix select reading global memory), the moved-mesh entries' fall-through, the
Burgers data's native 192 x 192 grid through the public API, and the limit.
"""
import numpy as np
import pytest
import torch

from oracle import refcpu

pytestmark = pytest.mark.gpu

OLD_MAX = 16384           # knn_large_kernel's limit: above it the tiled path


def _graph_case(pos, B, dev, k=35):
    from mmpde_amd import ops

    nbr, deg = ops.knn_graph_nbr(pos.to(dev), B, k, count_degenerate=True)
    _, ref, rdeg = refcpu.knn_graph(pos, k, B)
    assert int(deg.item()) == rdeg
    assert torch.equal(nbr.cpu().long(), ref)
    return rdeg


def test_graph_random(dev):
    """One point past the old path; a last tile holding one point (the same
    shape when T divides 16384); two trajectories (global indices carry the
    batch offset)."""
    from mmpde_amd import ops

    done = []
    for n, B in ((OLD_MAX + 1, 1), (None, 1), (20000, 2)):
        if n is None:
            n = max(OLD_MAX, 2 * ops.KNN_TILE_POINTS) + 1
        if (n, B) in done:
            continue
        done.append((n, B))
        torch.manual_seed(n)
        _graph_case(torch.rand(n * B, 2), B, dev)


def test_graph_lattice_ties_at_the_cut(dev):
    """129 x 129 lattice: the 35th neighbour lies inside the 8-point d^2 = 10
    shell, whose members sit in different tiles; (key, index) order decides."""
    from mmpde_amd.synth import burgers_grid_points

    pos = burgers_grid_points(129)
    assert pos.shape[0] == 16641
    _graph_case(pos, 1, dev)


def test_graph_overflow_across_tile_boundary(dev):
    """801 coincident points at consecutive indices straddling a tile boundary
    and 1300 elsewhere: the candidate list overflows, the radix select takes
    the threshold ties in index order across tiles, and most of the run's
    queries do not find themselves among their k + 1 nearest (degenerate)."""
    from mmpde_amd import ops

    T = ops.KNN_TILE_POINTS
    n = 20000
    lo = (16400 // T) * T - 384                                 # the boundary 384 points into the run
    assert lo > 4300 and lo + 801 <= n and lo < (lo + 400) // T * T < lo + 801
    torch.manual_seed(17)
    pos = torch.rand(n, 2)
    pos[lo:lo + 801] = pos[5]
    pos[3000:4300] = 0.25
    assert _graph_case(pos, 1, dev) >= 766


@pytest.mark.parametrize("ns,nq,B", [(16385, 300, 1), (36864, 200, 2)])
def test_query_random(dev, ns, nq, B):
    from mmpde_amd import ops

    torch.manual_seed(ns + nq)
    src, qry = torch.rand(B * ns, 2), torch.rand(B * nq, 2)
    qry[:3] = src[:3]                                           # zero-distance hits
    idx = ops.knn_query(src.to(dev), qry.to(dev), B, 30)
    ref = refcpu.knn_query(src, qry, B, 30)
    assert torch.equal(idx.cpu().long().reshape(ref.shape), ref)


def test_query_tie_counter(dev):
    """Half the queries on lattice points (ties), half at jittered cell centres
    (none): the ties count against a numpy fp64 brute force over every source
    point, the table against the oracle."""
    from mmpde_amd import ops
    from mmpde_amd.synth import burgers_grid_points

    src = burgers_grid_points(129)
    g = torch.Generator().manual_seed(5)
    qry = src[torch.randperm(src.shape[0], generator=g)[:300]].clone()
    qry[150:] += 0.5 / 128.0 + 1e-3 * torch.rand(150, 2, generator=g)
    s, q = src.double().numpy(), qry.double().numpy()
    dx, dy = q[:, None, 0] - s[None, :, 0], q[:, None, 1] - s[None, :, 1]
    d = np.sort(dx * dx + dy * dy, axis=1)[:, :31]
    want = int(np.any(d[:, 1:] == d[:, :-1], axis=1).sum())
    assert 100 < want < 300
    ties = torch.zeros((1,), dtype=torch.int32, device=dev)
    idx = ops.knn_query(src.to(dev), qry.to(dev), 1, 30, ties=ties)
    ref = refcpu.knn_query(src, qry, 1, 30)
    assert torch.equal(idx.cpu().long().reshape(ref.shape), ref)
    assert int(ties.item()) == want


def test_moved_mesh_entries_fall_through(dev):
    """No candidate table above 4096 points: the moved-mesh entries are the
    plain searches, here the tiled ones."""
    from mmpde_amd import ops
    from mmpde_amd.synth import burgers_grid_points

    B = 2
    xi = burgers_grid_points(129)
    pos = (xi + 0.004 * torch.sin(9 * xi.flip(1))).repeat(B, 1)
    pos[xi.shape[0]:] += 0.001 * torch.cos(5 * xi)
    assert ops.knn_candidates(xi.to(dev)) is None
    moved = ops.knn_graph_moved(pos.to(dev), xi.to(dev), None, B, 35)
    assert torch.equal(moved, ops.knn_graph_nbr(pos.to(dev), B, 35))
    _, ref, _ = refcpu.knn_graph(pos, 35, B)
    assert torch.equal(moved.cpu().long(), ref)
    qry = xi.repeat(B, 1).to(dev)
    assert torch.equal(ops.knn_query_moved(pos.to(dev), qry, xi.to(dev), None, B, 30),
                       ops.knn_query(pos.to(dev), qry, B, 30))


def test_burgers_gnn_native_resolution_api(dev):
    """The Burgers data's native grid through the drop-in API: (31, 192, 192),
    36864 nodes per trajectory, moving_mesh=False (create_graph(..., None) ->
    model(graph)).  The kNN-35 graph is checked against the oracle on the same
    points.  The GNN's values at this size are NOT oracle-checked: the CPU
    restatement runs 2.0-2.5 k node-updates/s, about 16 s here; the edge and
    node stages at large segments are covered at 96 x 96
    (test_burgers_gnn_default_resolution_api_matches_oracle)."""
    from mmpde_amd.synth import build_models, burgers_grid_points, fields

    pde, model, _, _, _, gc = build_models("burgers", moving_mesh=False, seed=4)
    res = [31, 192, 192]
    pde.grid_size = pde.movingmesh_grid_size = pde.ori_grid_size = res
    B, step = 1, 7
    pts = burgers_grid_points(192)
    u = fields(pts, B, 31, seed=5).reshape(B, 31, 192, 192)
    data, labels = gc.create_data(u, [step] * B)
    model.to(dev)
    graph = gc.create_graph(None, data, labels, [step] * B, dev, None)
    edge_index, _, _ = refcpu.knn_graph(pts, 35, B)
    assert torch.equal(graph.edge_index.cpu(), edge_index), "kNN-35 graph, 36864 nodes"
    out = model(graph)
    assert out.shape == (36864, 1)
    assert bool(torch.isfinite(out).all())


def test_limit(dev):
    from mmpde_amd import _lib as L
    from mmpde_amd import ops

    torch.manual_seed(3)
    with pytest.raises(ValueError, match="65536"):
        ops.knn_graph_nbr(torch.rand(65537, 2, device=dev), 1, 35)
    pos = torch.rand(65537, 2, device=dev)
    nbr = torch.empty((65537, 35), dtype=torch.int32, device=dev)
    lib = L.lib()
    assert lib.mmpde_knn_graph(L.ptr(pos), 1, 65537, 35, L.ptr(nbr), L.ptr(None), L.stream(pos.device)) == -1
    deg = torch.zeros((1,), dtype=torch.int32, device=dev)
    assert lib.mmpde_knn_graph(L.ptr(pos), 1, 65536, 35, L.ptr(nbr), L.ptr(deg), L.stream(pos.device)) == 0
    torch.cuda.synchronize()
    assert int(deg.item()) == 0
    # 64 sampled rows against an fp64 brute force on the device: ascending, the
    # farthest no farther than the 36th smallest distance (self included)
    P = pos[:65536].double()
    qi = torch.arange(0, 65536, 1024, device=dev) + 7
    d = ((P[None] - P[qi][:, None]) ** 2).sum(-1)
    rows = nbr[qi].long()
    assert int(rows.min()) >= 0 and int(rows.max()) < 65536 and not bool((rows == qi[:, None]).any())
    got = d.gather(1, rows)
    assert bool((got[:, 1:] >= got[:, :-1] * (1 - 1e-5)).all())
    assert bool((got[:, -1] <= d.kthvalue(36, dim=1).values * (1 + 1e-5)).all())
