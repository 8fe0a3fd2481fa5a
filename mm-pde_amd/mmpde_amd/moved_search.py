"""The rollout's neighbour searches on the moved mesh, and what they own.

Roles: 'graph' (the moved mesh's kNN-n or radius graph, main2), 'query' (kNN-30
of the fixed grid onto the moved mesh, side2), Burgers' 'query1' (kNN-30 of the
moved mesh onto the fixed grid, main2).  Each goes through the mesh's cell bins
('binned'), from its candidate table with the full search behind it ('table',
while ops.KnnTablePolicy finds that the table pays) or as the plain full search
('full'); a radius graph as the index-order scan ('radius') or through the bins
('radius-binned').  Every way gives the same tables bit for bit.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib as L
from . import ops


class Choice(NamedTuple):
    modes: dict     # role -> 'binned' | 'table' | 'full' | 'radius' | 'radius-binned'
    bins: bool      # the step bins the moved mesh (once, for every search that reads the bins)
    record: bool    # the step computes the moved mesh's displacement record (ops.knn_moved_cells)


def choose(radius_graph: bool, knn_binned: bool, radius_binned, n_per: int, tables: dict,
           answers: dict) -> Choice:
    """The way of every search of one step, from flags and sizes alone.
    tables: role -> whether its candidate table exists, for the roles the
    engine has; answers: role -> KnnTablePolicy.use_table's answer, read only
    for a role whose table exists while knn_binned is off.  radius_binned None:
    through the bins whenever the step bins the mesh anyway or n_per >=
    ops.RADIUS_BINNED_MIN_POINTS; True / False force it."""
    modes = {}
    for role, have in tables.items():
        if role == "graph" and radius_graph:
            rb = (knn_binned or n_per >= ops.RADIUS_BINNED_MIN_POINTS) if radius_binned is None \
                else bool(radius_binned)
            modes[role] = "radius-binned" if rb else "radius"
        elif knn_binned:
            modes[role] = "binned"
        else:
            modes[role] = "table" if have and answers[role] else "full"
    return Choice(modes, bool(knn_binned) or modes["graph"] == "radius-binned",
                  "table" in (modes["graph"], modes["query"]))


class MovedMeshSearch:
    """The searches' buffers, policy and ties counter, and a method per stage.
    knn_binned: every kNN search through cell bins of the moved mesh, no table
    consulted (the default without a table, N > 4096; csrc/knn.hip
    knn_binned_kernel); radius_binned: `choose`.  Both are settable before the
    first step and before enable_graph."""

    def __init__(self, kind, gc, xi, grid, grid_rep, batches: int):
        self.B, self.N = B, N = batches, grid.shape[0]
        self.xi, self.grid, self.grid_rep, self.k = xi, grid, grid_rep, gc.n
        dev = self.device = grid.device
        self.radius_graph = gc.e == "radius"
        self.radius_r = gc.radius() if self.radius_graph else None
        self.radius_binned = None
        # The graph from the 128 nearest of each xi point, the query from the
        # 128 nearest xi points of each grid point (exact: csrc/knn_cand.hip
        # knn_cand_kernel, full search where its bound fails).  Burgers' grid
        # is in 'ij' order and xi in 'xy' order, so the query table is built
        # for the grid's own order.  A radius graph has no kNN-n search: no
        # graph table, skip threshold or policy role.
        ref = None if grid is xi else grid
        cand_g = None if self.radius_graph else ops.knn_candidates(xi)
        cand_q = cand_g if ref is None and cand_g is not None else ops.knn_candidates(xi, ref=ref)
        self.cand = {"graph": cand_g, "query": cand_q}
        # trajectories whose typical displacement exceeds these go straight
        # to the full search (about half the lookups would fail; read once)
        self.skip = {"graph": ops.knn_skip_threshold(xi, cand_g, gc.n + 1, moved_queries=True),
                     "query": ops.knn_skip_threshold(xi, cand_q, 30, ref=grid)}
        # the miss flags, per role: the query runs on side2 beside the graph
        nb = max(L.lib().mmpde_knn_graph_cand_scratch_bytes(B, N), 1)
        self.scratch = {r: torch.empty((nb,), dtype=torch.uint8, device=dev) for r in ("graph", "query")}
        # kNN-30 queries whose sorted fp64 distances hold an exact tie (sklearn's
        # order unpinned there): cumulative
        self.ties = torch.zeros((1,), dtype=torch.int32, device=dev)
        # the moved mesh's per-step displacement record, shared by graph and query
        self.cells = torch.empty((L.lib().mmpde_knn_moved_cells_bytes(B) // 4,), dtype=torch.float32,
                                 device=dev)
        if kind == "burgers":
            # a table of the 128 grid points nearest each xi point, and a record
            # of the unmoved grid (all zero; rebuilt every step, which also
            # zeroes its miss counters)
            self.cand["query1"] = ops.knn_candidates(grid, ref=xi)
            self.skip["query1"] = ops.knn_skip_threshold(grid, self.cand["query1"], 30, ref=xi,
                                                         moved_queries=True)
            self.cells_1 = torch.empty_like(self.cells)
            self.scratch["query1"] = torch.empty((nb,), dtype=torch.uint8, device=dev)
        # table vs full search per role, from the share the table answered at
        # an earlier step (the cost model, no sync)
        self.policy = ops.KnnTablePolicy(dev, B, N, [r for r in self.cand
                                                     if not (r == "graph" and self.radius_graph)])
        self.knn_binned = cand_q is None and N >= ops.KNN_BINNED_MIN_POINTS
        self.bins = None      # the moved mesh's bins, rebuilt every step
        self.bins_1 = None    # query1: the fixed grid's bins, built once
        if self.knn_binned:
            self._ensure_bins()
        self.choice = None    # the last step's

    def _ensure_bins(self):
        if self.bins is None:
            nb = L.lib().mmpde_knn_bins_bytes(self.B, self.N)
            self.bins = torch.empty((nb,), dtype=torch.uint8, device=self.device)
        if "query1" in self.cand and self.knn_binned and self.bins_1 is None:
            self.bins_1 = ops.knn_bins(self.grid_rep, self.B)

    def _choose(self, answers) -> Choice:
        return choose(self.radius_graph, self.knn_binned, self.radius_binned, self.N,
                      {r: c is not None for r, c in self.cand.items()}, answers)

    def begin_step(self, mesh) -> None:
        """Ends main1: the step's choice, then what it needs of the moved mesh,
        once for side2 and main2 alike: the bins, and the displacement record
        when a table is consulted this step."""
        ask = not self.knn_binned
        ch = self.choice = self._choose({r: ask and c is not None and self.policy.use_table(r)
                                         for r, c in self.cand.items()})
        if ch.bins:
            self._ensure_bins()
            ops.knn_bins(mesh, self.B, out=self.bins)
        if ch.record:
            ops.knn_moved_cells(mesh, self.xi, self.B, out=self.cells)

    def knn(self, role, mesh):
        """idx2 ('query', side2), idx1 ('query1', main2), or the kNN graph's nbr_m."""
        mode, B, graph = self.choice.modes[role], self.B, role == "graph"
        if role == "query1":   # the fixed grid's points, searched from the moved mesh
            src, qry, fixed, ref, bins = self.grid_rep, mesh, self.grid, self.xi, self.bins_1
        else:
            src, qry, fixed, ref, bins = mesh, self.grid_rep, self.xi, self.grid, self.bins
        if mode == "table":
            cells = self.cells if role != "query1" else ops.knn_moved_cells(src, fixed, B, out=self.cells_1)
            if graph:
                out = ops.knn_graph_moved(src, fixed, self.cand[role], B, self.k, self.scratch[role],
                                          cells=cells, skip_above=self.skip[role])
            else:
                out = ops.knn_query_moved(src, qry, fixed, self.cand[role], B, 30, self.scratch[role], ref=ref,
                                          cells=cells, skip_above=self.skip[role], ties=self.ties)
            self.policy.after_table(role, cells, 0 if graph else 1)   # on the table call's stream
            return out
        how = dict(method="binned", bins=bins) if mode == "binned" else {}
        if graph:
            return ops.knn_graph_nbr(src, B, self.k, **how)
        return ops.knn_query(src, qry, B, 30, ties=self.ties, **how)

    def graph(self, mesh):
        """main2: (nbr_m, deg_m); deg_m None for a kNN graph."""
        if not self.radius_graph:
            return self.knn("graph", mesh), None
        how = dict(method="binned", bins=self.bins) if self.choice.modes["graph"] == "radius-binned" else {}
        return ops.radius_graph_nbr(mesh, self.B, self.radius_r, 32, **how)   # torch_cluster's default 32

    def modes(self) -> dict:
        """role -> the way the next step's search goes as things stand (a role
        on a policy probe counts as 'full' until the probe's share is known)."""
        return self._choose({r: self.policy.mode(r) == "table" for r in self.policy.state}).modes

    def table_share(self):
        if self.cand["query"] is None:
            return None
        torch.cuda.synchronize(self.device)
        used = {r: m == "table" for r, m in self.choice.modes.items()} if self.choice else {}
        s = ops.knn_table_share(self.cells, self.B, self.N).mean(0).tolist()
        s = [s[0] if used.get("graph") else None, s[1] if used.get("query") else None]
        if "query1" in self.cand:
            s.append(ops.knn_table_share(self.cells_1, self.B, self.N)[:, 1].mean().item()
                     if used.get("query1") else None)
        return tuple(s)

    def query_ties(self) -> int:
        torch.cuda.synchronize(self.device)
        return int(self.ties.item())
