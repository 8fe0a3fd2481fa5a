"""The candidate path (mmpde_knn_graph_cand / mmpde_knn_query_cand,
csrc/knn_cand.hip) against the full search at the table's size limits, N = 128
(the smallest launch rung, cpl <= 4) and N = 4096 (the largest, cpl = 64).
Its fallback goes through launch_knn's ladder (csrc/knn.hip) in knn_kernel's
miss mode; at N = 4096 the three trajectories take that mode's three branches,
and the tables' answered shares are asserted so that each one is really taken.
No tolerance: the tables and counters are equal or the test fails."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3


def _meshes(rows, cols, dev):
    """xi: a rows x cols lattice of spacing h = 1 / cols, jittered by 0.3 h;
    pos: three trajectories moved from it: not at all, three nodes by 5 h (the
    queries within some 10 h of their cells miss), every node by 3 h randn (the
    table's margin R128 - R36 is about 3 h)."""
    gen = torch.Generator().manual_seed(11)
    h = 1.0 / cols
    ij = torch.stack(torch.meshgrid(torch.arange(rows), torch.arange(cols), indexing="ij"), -1).reshape(-1, 2)
    xi = (ij + 0.5 + 0.3 * (2 * torch.rand(ij.shape, generator=gen) - 1)) * h
    N = xi.shape[0]
    few = xi.clone()
    few[torch.randperm(N, generator=gen)[:3]] += 5 * h * torch.tensor([0.8, -0.6])
    far = xi + 3 * h * torch.randn(xi.shape, generator=gen)
    return xi.float().to(dev).contiguous(), torch.cat([xi, few, far]).float().to(dev).contiguous()


@pytest.mark.parametrize("rows, cols", [(8, 16), (64, 64)])   # N = 128: every point is a candidate
def test_candidate_path_equals_full_search_at_the_table_limits(dev, rows, cols):
    from mmpde_amd import ops

    xi, pos = _meshes(rows, cols, dev)
    N = xi.shape[0]
    assert N in (128, 4096)
    qry = xi.repeat(B, 1).contiguous()
    cand = ops.knn_candidates(xi)
    assert cand is not None and cand.shape == (N, ops.KNN_CAND)
    cells = ops.knn_moved_cells(pos, xi, B)
    nbr, deg = ops.knn_graph_moved(pos, xi, cand, B, 35, count_degenerate=True, cells=cells)
    t_c = torch.zeros((1,), dtype=torch.int32, device=dev)
    idx = ops.knn_query_moved(pos, qry, xi, cand, B, 30, cells=cells, ties=t_c)
    share = ops.knn_table_share(cells, B, N).cpu()
    print(f"N = {N}: table share per trajectory, graph {share[:, 0].tolist()} query {share[:, 1].tolist()}")
    nbr_f, deg_f = ops.knn_graph_nbr(pos, B, 35, count_degenerate=True)
    t_f = torch.zeros((1,), dtype=torch.int32, device=dev)
    idx_f = ops.knn_query(pos, qry, B, 30, ties=t_f)
    assert torch.equal(nbr, nbr_f) and int(deg.item()) == int(deg_f.item())
    assert torch.equal(idx, idx_f) and int(t_c.item()) == int(t_f.item())
    if N == 4096:
        for role in (0, 1):
            assert share[0, role] == 1.0           # none missed: the fallback returns at once
            assert 0.5 < share[1, role] < 1.0      # a minority missed: spread by rank
            assert share[2, role] < 0.5            # a majority missed: the plain branch
