"""The candidate kernels' select-before-sort (knn_cand_kernel: the candidates
with fp32 key at most thr = the largest moved key among the first kk, packed
into one register and sorted 64 wide; more than 64 of them: the 128-wide sort)
against the full search, bit for bit, on small point sets (B = 2, N = 256 /
300 > the 128-candidate table) built so that each branch is taken by queries
the TABLE answers (their miss flag in the scratch buffer is 0):
  a. small random displacement: every query selects m <= 64;
  b. one of a query's first kk candidates moved far: m > 64;
  c. a square lattice, unmoved: exact ties at the threshold and at rank kk;
  d. a tight cluster of exactly kk points: m == kk (rank kk is outside the set);
  e. two coincident points.
m is bounded on the CPU from the table itself: lo <= m <= hi count the keys
below thr (1 -+ 2e-5), a slack above the fp32 key's 2^-22 rounding and the
query variant's 64-ulp margin."""
import numpy as np
import pytest
import torch

from oracle import refcpu

pytestmark = pytest.mark.gpu

B, KG, KQ = 2, 35, 30     # graph: kk = KG + 1 (the self point), query: kk = KQ


def _m_bounds(pos_b, q_b, cand, kk):
    """(lo, hi) per query: lo <= m <= hi, m = the kernel's selected count."""
    d = pos_b.double().numpy()[cand] - q_b.double().numpy()[:, None, :]
    key = (d ** 2).sum(-1)
    u = key[:, :kk].max(1)[:, None]
    return (key <= u * (1 - 2e-5)).sum(1), (key <= u * (1 + 2e-5) + 1e-37).sum(1)


def _background(n, gen, holes, radius):
    """n uniform points of the unit square at least `radius` from every hole centre."""
    pts = torch.rand(40 * n, 2, generator=gen)
    keep = torch.ones(len(pts), dtype=torch.bool)
    for c in holes:
        keep &= (pts - torch.tensor(c)).norm(dim=1) >= radius
    pts = pts[keep][:n]
    assert len(pts) == n
    return pts


def _disc(n, centre, radius, gen):
    r = radius * torch.rand(n, generator=gen).sqrt()
    a = 6.2831853 * torch.rand(n, generator=gen)
    return torch.tensor(centre) + torch.stack((r * a.cos(), r * a.sin()), 1)


def _case(name):
    """(xi [N, 2], pos [B N, 2], about): `about` = the local indices of the
    queries the case is about (None: every query)."""
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    about = None
    if name == "small":
        xi = torch.rand(300, 2, generator=gen)
        pos = xi.repeat(B, 1) + 0.002 * torch.randn(B * 300, 2, generator=gen)
    elif name == "one_far":
        # 100 points within 0.01 of c, the rest at least 0.4 away: a cluster
        # point's first kk candidates are cluster points; one of them moved by
        # 0.05 puts thr above the whole cluster (m = 100) while the bound
        # (about 0.4 - 0.05) still holds
        c = (0.3, 0.3)
        xi = torch.cat((_disc(100, c, 0.01, gen), _background(200, gen, [c], 0.4)))
        pos = xi.repeat(B, 1) + 1e-4 * torch.randn(B * 300, 2, generator=gen)
        d0 = (xi[:100] - torch.tensor(c)).norm(dim=1)
        j = int(d0.argmin())                      # the most central: in many first-kk lists
        pos[j] += torch.tensor([0.05, 0.0])
        pos[300 + j] += torch.tensor([0.0, -0.05])
        about = torch.arange(100)
    elif name == "lattice":
        s = torch.arange(16, dtype=torch.float32) * 0.0625     # exact differences, exact ties
        xi = torch.stack(torch.meshgrid(s, s, indexing="xy"), -1).reshape(-1, 2)
        pos = xi.repeat(B, 1)
    elif name == "cluster_kk":
        # exactly KG + 1 points around ca and exactly KQ around cb, nothing else near
        ca, cb = (0.3, 0.3), (0.7, 0.7)
        na, nb = KG + 1, KQ
        xi = torch.cat((_disc(na, ca, 0.005, gen), _disc(nb, cb, 0.005, gen),
                        _background(300 - na - nb, gen, [ca, cb], 0.15)))
        pos = xi.repeat(B, 1) + 1e-4 * torch.randn(B * 300, 2, generator=gen)
        about = (torch.arange(na), na + torch.arange(nb))      # graph, query
    elif name == "coincident":
        xi = torch.rand(300, 2, generator=gen)
        xi[7] = xi[3]
        disp = 0.002 * torch.randn(B * 300, 2, generator=gen)
        disp[7], disp[307] = disp[3], disp[303]
        pos = xi.repeat(B, 1) + disp
        about = torch.tensor([3, 7])
    else:
        raise KeyError(name)
    return xi, pos, about


@pytest.mark.parametrize("name", ["small", "one_far", "lattice", "cluster_kk", "coincident"])
def test_select_then_sort_equals_full_search(dev, name):
    from mmpde_amd import ops

    xi, pos, about = _case(name)
    N = xi.shape[0]
    assert 150 <= N <= 400 and N > ops.KNN_CAND
    qry = xi.repeat(B, 1)
    xd, pd, qd = xi.to(dev), pos.to(dev), qry.to(dev)
    cand = ops.knn_candidates(xd)
    assert cand is not None
    cand_h = cand.cpu().long().numpy()

    # ---- graph (fp32 keys, kk = KG + 1, the moved point itself is the query)
    miss_g = torch.full((B * N,), 255, dtype=torch.uint8, device=dev)
    nbr, deg = ops.knn_graph_moved(pd, xd, cand, B, KG, scratch=miss_g, count_degenerate=True)
    full, fdeg = ops.knn_graph_nbr(pd, B, KG, count_degenerate=True)
    assert torch.equal(nbr, full)
    assert int(deg.item()) == int(fdeg.item())
    # ---- query (fp64 order checked on the fp32 sort, kk = KQ, queries at xi)
    miss_q = torch.full((B * N,), 255, dtype=torch.uint8, device=dev)
    ties = torch.zeros((1,), dtype=torch.int32, device=dev)
    fties = torch.zeros((1,), dtype=torch.int32, device=dev)
    idx = ops.knn_query_moved(pd, qd, xd, cand, B, KQ, scratch=miss_q, ties=ties)
    assert torch.equal(idx, ops.knn_query(pd, qd, B, KQ, ties=fties))
    assert int(ties.item()) == int(fties.item())

    assert int((miss_g > 1).sum()) == 0 and int((miss_q > 1).sum()) == 0      # every flag was written
    tg = (miss_g.cpu() == 0).reshape(B, N).numpy()
    tq = (miss_q.cpu() == 0).reshape(B, N).numpy()
    m_g = [_m_bounds(pos[b * N:(b + 1) * N], pos[b * N:(b + 1) * N], cand_h, KG + 1) for b in range(B)]
    m_q = [_m_bounds(pos[b * N:(b + 1) * N], xi, cand_h, KQ) for b in range(B)]
    lo_g, hi_g = (np.stack([m[i] for m in m_g]) for i in (0, 1))
    lo_q, hi_q = (np.stack([m[i] for m in m_q]) for i in (0, 1))
    print(f"{name}: table answered graph {tg.mean():.3f} query {tq.mean():.3f}; "
          f"m graph [{lo_g.min()}, {hi_g.max()}] query [{lo_q.min()}, {hi_q.max()}]; "
          f"ties {int(ties.item())} degenerate {int(deg.item())}")
    ag, aq = about if isinstance(about, tuple) else (about, about)
    # the queries the case is about were answered by the table, not the fallback
    if about is None:
        assert tg.mean() > 0.9 and tq.mean() > 0.9
    else:
        ag, aq = ag.numpy(), aq.numpy()
        assert tg[:, ag].all() and tq[:, aq].all()
    if name in ("small", "coincident"):
        assert hi_g.max() <= 64 and hi_q.max() <= 64              # the 64-wide sort everywhere
    if name == "one_far":
        assert ((lo_g > 64) & tg).any() and ((lo_q > 64) & tq).any()   # the 128-wide sort
    if name == "lattice":
        mid = 8 * 16 + 8                                          # an interior point: 37 within d2 <= 10 h^2
        assert tg[:, mid].all() and tq[:, mid].all()
        assert (hi_g[:, mid] > KG + 1).all() and (hi_q[:, mid] > KQ).all()   # ties at the threshold
        assert int(ties.item()) > 0                               # and at rank kk (query)
    if name == "cluster_kk":
        assert (hi_g[:, ag] == KG + 1).all() and (hi_q[:, aq] == KQ).all()   # m == kk
    if name == "small":
        # the oracle (C reimplementation of torch_cluster / sklearn's orders)
        _, ref, rdeg = refcpu.knn_graph(pos, KG, B)
        assert torch.equal(nbr.cpu().long(), ref) and int(deg.item()) == rdeg
        ref_q = refcpu.knn_query(pos, qry, B, KQ)
        assert torch.equal(idx.cpu().long().reshape(ref_q.shape), ref_q)
