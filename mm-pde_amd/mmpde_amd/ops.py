"""Tensor-level wrappers over the C-ABI (one function per entry point).

Every function launches on the current torch stream of the input's device and
returns new device tensors; nothing here synchronises or falls back to CPU.
"""
from __future__ import annotations

import collections
import ctypes
import math

import os

import torch

from . import _lib as L
from . import rows

# kNN kernels search one trajectory's points from LDS (csrc/knn.hip): the whole
# set staged at once up to 16384 points, streamed in tiles of KNN_TILE_POINTS
# above that, up to KNN_MAX_POINTS per trajectory (include/mmpde_hip.h
# mmpde_knn_graph / mmpde_knn_query).  The reference's benchmarked grids are
# 2521 (cy) and 48 x 48 = 2304 (burgers); burgers at the PDE's own default
# 96 x 96 (PDEs.py:27) and at its data's native 192 x 192 (mmpde.py:171) fit.
KNN_MAX_POINTS = 65536
KNN_TILE_POINTS = 4096  # kTile in csrc/knn.hip


def _knn_points_check(n_per: int, k: int, what: str):
    if n_per > KNN_MAX_POINTS:
        raise ValueError(f"{what}: {n_per} points per trajectory; the HIP kNN kernels take at "
                         f"most {KNN_MAX_POINTS} (run --base_resolution <= 256 x 256)")
    if k > 63:
        raise ValueError(f"{what}: k = {k}; the HIP kNN kernels take k <= 63")


# Trajectories of at least this many points are searched through cell bins by
# the rollout when no candidate table exists (knn_bins; csrc/knn.hip
# knn_binned_kernel): the binned search beat the full one at every measured
# size from 4225 points up (profiles/knn_binned_times.txt).
KNN_BINNED_MIN_POINTS = 4097
KNN_METHODS = ("full", "binned")


def knn_bins_grid(n_per: int) -> int:
    """Cells per axis of the grid knn_bins lays over a trajectory of n_per
    points (mmpde_knn_bins_grid; host arithmetic)."""
    return int(L.lib().mmpde_knn_bins_grid(int(n_per)))


def knn_bins(src: torch.Tensor, batches: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """Cell bins of src [batches * n_per, 2] for knn_graph_nbr / knn_query with
    method="binned": every trajectory's points sorted into a uniform grid over
    its own bounding box (mmpde_knn_bin).  One binning serves any number of
    searches of the same points.  out: a uint8 workspace to reuse (at least
    mmpde_knn_bins_bytes(batches, n_per) bytes), else allocated."""
    L.require_device(src)
    src = L.f32c(src).reshape(-1, 2)
    n = src.shape[0]
    if batches < 1 or n % batches or n == 0:
        raise ValueError("src rows must split into equal batch segments")
    n_per = n // batches
    _knn_points_check(n_per, 1, "knn_bins")
    need = L.lib().mmpde_knn_bins_bytes(batches, n_per)
    if out is None:
        out = torch.empty((need,), dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() < need:
        raise ValueError(f"knn_bins: out must be a contiguous uint8 device tensor of >= {need} bytes")
    L.check(L.lib().mmpde_knn_bin(L.ptr(src), batches, n_per, L.ptr(out), out.numel(),
                                  L.stream(src.device)), "mmpde_knn_bin")
    return out


def _knn_method(method, bins, stats, src, batches, n_per):
    """Validated (bins, stats) of a search with `method`; bins built when absent."""
    if method not in KNN_METHODS:
        raise ValueError(f"knn method {method!r}; one of {KNN_METHODS}")
    if method == "full":
        if bins is not None or stats is not None:
            raise ValueError('bins / stats belong to method="binned"')
        return None, None
    if stats is not None and (stats.dtype != torch.int64 or stats.numel() < 2 or not stats.is_cuda
                              or not stats.is_contiguous()):
        raise ValueError("stats must be an int64[2] device counter")
    if bins is None:
        bins = knn_bins(src, batches)
    elif (bins.dtype != torch.uint8 or not bins.is_cuda or not bins.is_contiguous()
          or bins.numel() < L.lib().mmpde_knn_bins_bytes(batches, n_per)):
        raise ValueError("bins must come from knn_bins of the same source points")
    return bins, stats


def knn_graph_nbr(pos: torch.Tensor, batches: int, k: int, count_degenerate: bool = False,
                  method: str = "full", bins: torch.Tensor | None = None,
                  stats: torch.Tensor | None = None):
    """torch_cluster.knn_graph(pos, k, batch, loop=False) for `batches` equal
    contiguous segments (reference data_creator_2d.py:260, dmm_model.py:228).
    Returns nbr [n, k] int32 (global source indices, (d2, index) order)
    [, degenerate count tensor].  method "binned": the same table from the cell
    bins of pos (bins = knn_bins(pos, batches), built here when None); stats:
    optional int64[2] device counter, += (points examined, queries whose
    candidate list overflowed)."""
    L.require_device(pos)
    pos = L.f32c(pos).reshape(-1, 2)
    n = pos.shape[0]
    if n % batches:
        raise ValueError("pos rows must split into equal batch segments")
    _knn_points_check(n // batches, k, "knn_graph")
    bins, stats = _knn_method(method, bins, stats, pos, batches, n // batches)
    nbr = torch.empty((n, k), dtype=torch.int32, device=pos.device)
    deg = torch.zeros((1,), dtype=torch.int32, device=pos.device) if count_degenerate else None
    if method == "binned":
        L.check(L.lib().mmpde_knn_graph_binned(L.ptr(pos), L.ptr(bins), batches, n // batches, k, L.ptr(nbr),
                                               L.ptr(deg), L.ptr(stats), L.stream(pos.device)),
                "mmpde_knn_graph_binned")
    else:
        L.check(L.lib().mmpde_knn_graph(L.ptr(pos), batches, n // batches, k, L.ptr(nbr),
                                        L.ptr(deg), L.stream(pos.device)), "mmpde_knn_graph")
    return (nbr, deg) if count_degenerate else nbr


KNN_CAND = 128  # candidates per point in mmpde_knn_candidates' table


def knn_candidates(xi: torch.Tensor, ref: torch.Tensor | None = None):
    """Static candidate table of knn_graph_moved / knn_query_moved for fixed
    points xi [N, 2] and reference points ref [N, 2] (default xi; for a query,
    the fixed query points): [N, 128] int32, the 128 nearest of ref_p in xi in
    (d2, index) order, or None where the candidate path does not apply (N
    outside [128, 4096])."""
    L.require_device(xi, ref)
    xi = L.f32c(xi).reshape(-1, 2)
    N = xi.shape[0]
    if N < KNN_CAND or N > 4096:
        return None
    if ref is not None:
        ref = L.f32c(ref).reshape(-1, 2)
        if ref.shape[0] != N:
            raise ValueError("ref must hold one reference point per xi point")
    cand = torch.empty((N, KNN_CAND), dtype=torch.int32, device=xi.device)
    L.check(L.lib().mmpde_knn_candidates(L.ptr(xi), L.ptr(ref), N, L.ptr(cand), L.stream(xi.device)),
            "mmpde_knn_candidates")
    return cand


def knn_skip_threshold(xi: torch.Tensor, cand, kk: int, ref: torch.Tensor | None = None,
                       moved_queries: bool = False) -> float:
    """The skip_above of knn_graph_moved / knn_query_moved for a table cand =
    knn_candidates(xi, ref) and kk = k + 1 (graph) or k (query): the median of
    R128 - R_kk over the reference points, halved for queries that move with
    the mesh (the graph) (mmpde_knn_skip_threshold).  Reads one float back to
    the host: call once per table, not per step."""
    if cand is None:
        return 0.0
    L.require_device(xi, cand, ref)
    xi = L.f32c(xi).reshape(-1, 2)
    ref = None if ref is None else L.f32c(ref).reshape(-1, 2)
    out = torch.empty((1,), dtype=torch.float32, device=xi.device)
    L.check(L.lib().mmpde_knn_skip_threshold(L.ptr(xi), L.ptr(ref), xi.shape[0], L.ptr(cand), kk,
                                             int(moved_queries), L.ptr(out), L.stream(xi.device)),
            "mmpde_knn_skip_threshold")
    return float(out.item())


def knn_moved_cells(pos: torch.Tensor, xi: torch.Tensor, batches: int,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """Per-trajectory displacement record of moved points pos [batches * N, 2]
    (every trajectory moved from xi [N, 2]): the largest |pos_j - xi_j| per cell
    of a 16 x 16 grid over xi's box (mmpde_knn_moved_cells).  One per moved mesh,
    shared by knn_graph_moved and knn_query_moved."""
    L.require_device(pos, xi)
    pos = L.f32c(pos).reshape(-1, 2)
    xi = L.f32c(xi).reshape(-1, 2)
    N = xi.shape[0]
    if pos.shape[0] != batches * N:
        raise ValueError("pos must hold `batches` meshes of xi's size")
    nf = L.lib().mmpde_knn_moved_cells_bytes(batches) // 4
    if out is None or out.numel() < nf:
        out = torch.empty((nf,), dtype=torch.float32, device=pos.device)
    L.check(L.lib().mmpde_knn_moved_cells(L.ptr(pos), L.ptr(xi), batches, N, L.ptr(out),
                                          L.stream(pos.device)), "mmpde_knn_moved_cells")
    return out


def knn_table_share(cells: torch.Tensor, batches: int, n_per: int) -> torch.Tensor:
    """[batches, 2] float: per trajectory, the share of the graph (column 0) and
    query (column 1) lookups the candidate tables answered since `cells` was
    computed (knn_moved_cells), from the record's miss counters (diagnostics)."""
    L.require_device(cells)
    miss = torch.empty((batches, 2), dtype=torch.int32, device=cells.device)
    L.check(L.lib().mmpde_knn_table_misses(L.ptr(cells), batches, L.ptr(miss),
                                           L.stream(cells.device)), "mmpde_knn_table_misses")
    return 1.0 - miss.float() / n_per


def _capturing() -> bool:
    """A hipGraph capture is in progress on the current stream."""
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class KnnTablePolicy:
    """Per-role choice between the candidate table (knn_graph_moved /
    knn_query_moved) and the plain full search for a rollout, from a cost model
    and the share f of lookups the table answered at an earlier step.

    Cost model (tools/knn_cand_time.py, cy B=16 on MI355X): the table path costs
    about T_cand + (1 - f) T_full -- the candidate kernel (37-44 us when every
    lookup passes) plus the full search of the lookups it could not answer --
    against T_full (61-80 us) for the full search, so it pays only while f >
    T_cand / T_full ~ 0.6; MIN_SHARE = 0.7 leaves room for the sorts the failed
    lookups also pay.  f is read back without a sync: the per-trajectory miss
    counters are copied to pinned host memory behind an event after a table
    call and consumed at a later step.  A role starts on the table (checked
    every CHECK_EVERY calls); below MIN_SHARE it runs the full search -- no
    candidate or cell kernels -- and after PROBE_EVERY calls makes ONE table
    call (a probe), staying on the full search until the probe's share is
    known.  Either path gives the same indices bit for bit."""

    MIN_SHARE = 0.7
    PROBE_EVERY = 64
    CHECK_EVERY = 4

    def __init__(self, device, batches: int, n_per: int, roles):
        self.device = torch.device(device)
        self.B, self.N = batches, n_per
        self.state = {r: {"mode": "table", "wait": 0, "since": 0, "pending": None, "share": None}
                      for r in roles}
        self.enabled = True

    def _resolve(self, st):
        pend = st["pending"]
        if pend is None or not pend[0].query():
            return
        st["pending"] = None
        share = 1.0 - float(pend[1].sum()) / (self.B * self.N)
        st["share"] = share
        if share >= self.MIN_SHARE:
            if st["mode"] != "table":
                st["mode"], st["since"] = "table", 0
        else:
            st["mode"], st["wait"] = "full", self.PROBE_EVERY

    def use_table(self, role) -> bool:
        if not self.enabled:
            return True
        st = self.state[role]
        self._resolve(st)
        if st["mode"] == "full":
            st["wait"] -= 1
            # no probe inside a hipGraph capture: its read-back cannot be queued
            # there (after_table), so the probe would never resolve
            if st["wait"] < 0 and not _capturing():
                st["mode"], st["since"] = "probe", 0
                return True                          # the probe call
            return False
        if st["mode"] == "probe":                    # probe made, its share not known yet
            return False
        return True

    def mode(self, role) -> str:
        return self.state[role]["mode"]

    def after_table(self, role, cells: torch.Tensor, column: int) -> None:
        """Queue the read-back of the miss counters of the table call just made
        with `cells` (on the current stream, after that call): at a probe and
        every CHECK_EVERY table calls."""
        st = self.state[role]
        st["since"] += 1
        if st["pending"] is not None or (st["mode"] == "table" and (st["since"] - 1) % self.CHECK_EVERY):
            return
        if _capturing():
            if st["mode"] == "probe":                # cannot read back: retry after capture
                st["mode"], st["wait"] = "full", self.PROBE_EVERY
            return
        miss = torch.empty((self.B, 2), dtype=torch.int32, device=self.device)
        L.check(L.lib().mmpde_knn_table_misses(L.ptr(cells), self.B, L.ptr(miss), L.stream(self.device)),
                "mmpde_knn_table_misses")
        host = torch.empty((self.B,), dtype=torch.int32, pin_memory=True)
        host.copy_(miss[:, column], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        st["pending"] = (ev, host)


def _cand_scratch(scratch, batches, N, device):
    need = L.lib().mmpde_knn_graph_cand_scratch_bytes(batches, N)
    if scratch is None or scratch.numel() * scratch.element_size() < need:
        scratch = torch.empty((max(need, 1),), dtype=torch.uint8, device=device)
    return scratch


def knn_graph_moved(pos: torch.Tensor, xi: torch.Tensor, cand, batches: int, k: int,
                    scratch: torch.Tensor | None = None, count_degenerate: bool = False,
                    cells: torch.Tensor | None = None, skip_above: float = 0.0):
    """knn_graph_nbr of moved points pos [batches * N, 2] (every trajectory's
    mesh moved from the same xi [N, 2]), bit for bit, answered from the
    candidate table `cand` (knn_candidates(xi)) where a distance bound proves
    it complete and by the full search elsewhere (reference
    data_creator_2d.py:260 on the DMM's moved mesh).  cells: knn_moved_cells(pos,
    xi, batches) if already computed; skip_above > 0: trajectories moved
    further go straight to the full search (knn_skip_threshold)."""
    if cand is None:
        return knn_graph_nbr(pos, batches, k, count_degenerate)
    L.require_device(pos)
    pos = L.f32c(pos).reshape(-1, 2)
    xi = L.f32c(xi).reshape(-1, 2)
    n = pos.shape[0]
    N = xi.shape[0]
    if n != batches * N or cand.shape != (N, KNN_CAND):
        raise ValueError("pos must hold `batches` meshes of xi's size; cand from knn_candidates(xi)")
    _knn_points_check(N, k, "knn_graph")
    if cells is None:
        cells = knn_moved_cells(pos, xi, batches)
    scratch = _cand_scratch(scratch, batches, N, pos.device)
    nbr = torch.empty((n, k), dtype=torch.int32, device=pos.device)
    deg = torch.zeros((1,), dtype=torch.int32, device=pos.device) if count_degenerate else None
    L.check(L.lib().mmpde_knn_graph_cand(L.ptr(pos), L.ptr(xi), L.ptr(cells), float(skip_above),
                                         batches, N, k,
                                         L.ptr(cand), L.ptr(nbr), L.ptr(deg), L.ptr(scratch),
                                         L.stream(pos.device)), "mmpde_knn_graph_cand")
    return (nbr, deg) if count_degenerate else nbr


RADIUS_METHODS = ("scan", "binned")
# Trajectories of at least this many points get the rollout's moved-mesh radius
# graph through cell bins even when the step does not build them anyway
# (csrc/knn_bins.hip radius_binned_kernel): the smallest measured size from which
# binning plus the binned search stayed below the index-order scan at every
# larger size, in both repeats (profiles/radius_times.txt).
RADIUS_BINNED_MIN_POINTS = 9216


def radius_graph_nbr(pos: torch.Tensor, batches: int, r: float, max_num_neighbors: int = 32,
                     method: str = "scan", bins: torch.Tensor | None = None,
                     stats: torch.Tensor | None = None):
    """torch_cluster.radius_graph(pos, r, batch, loop=False, max_num_neighbors) for
    `batches` equal contiguous segments (reference data_creator_2d.py:257-258),
    CUDA semantics (first max_num_neighbors + 1 in index order within r, self
    dropped).  Returns (nbr int32 [n, max_num_neighbors + 1] global sources,
    padded with -1; degree int32 [n]).  method "binned": the same tables from
    the cell bins of pos (bins = knn_bins(pos, batches), built here when None;
    at most 65536 points per trajectory and 63 neighbours); stats: optional
    int64[2] device counter, += (points examined, queries that took the
    index-order scan)."""
    if method not in RADIUS_METHODS:
        raise ValueError(f"radius method {method!r}; one of {RADIUS_METHODS}")
    L.require_device(pos)
    pos = L.f32c(pos).reshape(-1, 2)
    n = pos.shape[0]
    if n % batches:
        raise ValueError("pos rows must split into equal batch segments")
    n_per = n // batches
    if method == "scan":
        if bins is not None or stats is not None:
            raise ValueError('bins / stats belong to method="binned"')
    else:
        if n_per > KNN_MAX_POINTS:
            raise ValueError(f"radius_graph binned: {n_per} points per trajectory; at most {KNN_MAX_POINTS}")
        if not 1 <= max_num_neighbors <= 63:
            raise ValueError(f"radius_graph binned: max_num_neighbors = {max_num_neighbors}; 1..63")
        if not r > 0:
            raise ValueError(f"radius_graph binned: r = {r}; must be positive")
        bins, stats = _knn_method("binned", bins, stats, pos, batches, n_per)
    w = max_num_neighbors + 1
    nbr = torch.empty((n, w), dtype=torch.int32, device=pos.device)
    deg = torch.empty((n,), dtype=torch.int32, device=pos.device)
    if method == "binned":
        L.check(L.lib().mmpde_radius_graph_binned(L.ptr(pos), L.ptr(bins), batches, n_per, float(r),
                                                  max_num_neighbors, L.ptr(nbr), L.ptr(deg), L.ptr(stats),
                                                  L.stream(pos.device)), "mmpde_radius_graph_binned")
    else:
        L.check(L.lib().mmpde_radius_graph(L.ptr(pos), batches, n_per, float(r),
                                           max_num_neighbors, L.ptr(nbr), L.ptr(deg),
                                           L.stream(pos.device)), "mmpde_radius_graph")
    return nbr, deg


def edge_index_from_nbr(nbr: torch.Tensor, degree: torch.Tensor | None = None) -> torch.Tensor:
    """PyG edge_index int64 [2, E] (row 0 source, row 1 target) of a target-major
    table; with `degree`, row i contributes its first degree[i] entries."""
    if degree is not None:
        n, k = nbr.shape
        keep = torch.arange(k, device=nbr.device)[None, :] < degree[:, None].long()
        tgt = torch.arange(n, device=nbr.device)[:, None].expand(n, k)
        return torch.stack((nbr.long()[keep], tgt[keep]))
    """PyG edge_index int64 [2, n*k] (row 0 source, row 1 target)."""
    L.require_device(nbr)
    n, k = nbr.shape
    ei = torch.empty((2, n * k), dtype=torch.int64, device=nbr.device)
    L.check(L.lib().mmpde_edge_index_from_nbr(L.ptr(nbr.contiguous()), n, k, L.ptr(ei),
                                              L.stream(nbr.device)), "mmpde_edge_index_from_nbr")
    return ei


def nbr_from_edge_index(edge_index: torch.Tensor, n: int) -> torch.Tensor:
    """Recover the fixed-degree target-major table from a PyG edge_index whose
    targets are grouped (the layout knn_graph produces).  Raises on ragged
    degree (use nbr_table_from_edge_index)."""
    e = edge_index.shape[1]
    if e % n:
        raise ValueError("edge_index has ragged in-degree; fixed-degree kernels need k*n edges")
    k = e // n
    tgt = torch.arange(n, device=edge_index.device).repeat_interleave(k)
    if not bool(torch.equal(edge_index[1], tgt)):
        raise ValueError("edge_index targets are not grouped as knn_graph emits them")
    return edge_index[0].reshape(n, k).to(torch.int32).contiguous()


def nbr_table_from_edge_index(edge_index: torch.Tensor, n: int):
    """Any PyG edge_index -> (nbr int32 [n, k], degree int32 [n] or None).  A
    grouped fixed-degree graph gives degree None; otherwise the in-edges of every
    target (stable order) fill its row, padded with -1, k = max in-degree."""
    e = edge_index.shape[1]
    if e % n == 0:
        k = e // n
        tgt = torch.arange(n, device=edge_index.device).repeat_interleave(k)
        if bool(torch.equal(edge_index[1], tgt)):
            src = edge_index[0]
            if e and (int(src.min()) < 0 or int(src.max()) >= n):
                raise ValueError("edge_index holds nodes outside [0, n)")
            return src.reshape(n, k).to(torch.int32).contiguous(), None
    src, tgt = edge_index[0].long(), edge_index[1].long()
    if e and (int(src.min()) < 0 or int(src.max()) >= n or int(tgt.min()) < 0 or int(tgt.max()) >= n):
        raise ValueError("edge_index holds nodes outside [0, n)")
    order = torch.argsort(tgt, stable=True)
    src, tgt = src[order], tgt[order]
    deg = torch.bincount(tgt, minlength=n)
    k = max(int(deg.max().item()) if e else 0, 1)
    start = torch.cumsum(deg, 0) - deg
    slot = torch.arange(e, device=edge_index.device) - start[tgt]
    nbr = torch.full((n, k), -1, dtype=torch.int32, device=edge_index.device)
    nbr[tgt, slot] = src.to(torch.int32)
    return nbr, deg.to(torch.int32)


def _ties(ties):
    if ties is not None and (ties.dtype != torch.int32 or ties.numel() < 1 or not ties.is_cuda):
        raise ValueError("ties must be an int32 device counter")
    return ties


def knn_query(src: torch.Tensor, qry: torch.Tensor, batches: int, k: int,
              ties: torch.Tensor | None = None, method: str = "full",
              bins: torch.Tensor | None = None, stats: torch.Tensor | None = None) -> torch.Tensor:
    """Per-trajectory sklearn NearestNeighbors(k).fit(src_b).kneighbors(qry_b):
    LOCAL indices int32 [batches * n_qry, k], fp64-distance order
    (reference data_creator_2d.py:66-78).  ties: optional int32 [1] device
    counter, += the queries with an exact fp64 distance tie among their first
    k (or at rank k): where sklearn's order is its KD-tree's, parity unpinned.
    method "binned": the same table from the cell bins of src (bins =
    knn_bins(src, batches), built here when None); stats as for knn_graph_nbr."""
    L.require_device(src, qry)
    src = L.f32c(src).reshape(-1, 2)
    qry = L.f32c(qry).reshape(-1, 2)
    ns, nq = src.shape[0] // batches, qry.shape[0] // batches
    _knn_points_check(ns, k, "knn_query")
    bins, stats = _knn_method(method, bins, stats, src, batches, ns)
    idx = torch.empty((batches * nq, k), dtype=torch.int32, device=src.device)
    if method == "binned":
        L.check(L.lib().mmpde_knn_query_binned(L.ptr(src), L.ptr(bins), L.ptr(qry), batches, ns, nq, k,
                                               L.ptr(idx), L.ptr(_ties(ties)), L.ptr(stats),
                                               L.stream(src.device)), "mmpde_knn_query_binned")
    else:
        L.check(L.lib().mmpde_knn_query(L.ptr(src), L.ptr(qry), batches, ns, nq, k, L.ptr(idx),
                                        L.ptr(_ties(ties)), L.stream(src.device)), "mmpde_knn_query")
    return idx


def knn_query_moved(src: torch.Tensor, qry: torch.Tensor, xi: torch.Tensor, cand, batches: int,
                    k: int, scratch: torch.Tensor | None = None, ref: torch.Tensor | None = None,
                    cells: torch.Tensor | None = None, skip_above: float = 0.0,
                    ties: torch.Tensor | None = None) -> torch.Tensor:
    """knn_query of qry onto moved points src (every trajectory's mesh moved
    from the same xi [N, 2]; n_src = n_qry = N), bit for bit, answered from the
    candidate table `cand` = knn_candidates(xi, ref) (ref: the fixed points the
    queries sit at or near, default xi) where a distance bound proves it
    complete and by the full search elsewhere (reference data_creator_2d.py:66-78
    onto the DMM's moved mesh).  cells: knn_moved_cells(src, xi, batches) if
    already computed; skip_above as for knn_graph_moved; ties as for knn_query."""
    if cand is None:
        return knn_query(src, qry, batches, k, ties)
    L.require_device(src, qry, ref)
    src = L.f32c(src).reshape(-1, 2)
    qry = L.f32c(qry).reshape(-1, 2)
    xi = L.f32c(xi).reshape(-1, 2)
    N = xi.shape[0]
    if src.shape[0] != batches * N or qry.shape[0] != batches * N or cand.shape != (N, KNN_CAND):
        raise ValueError("src and qry must hold `batches` point sets of xi's size; "
                         "cand from knn_candidates(xi, ref)")
    if ref is not None:
        ref = L.f32c(ref).reshape(-1, 2)
        if ref.shape[0] != N:
            raise ValueError("ref must hold one reference point per xi point")
    _knn_points_check(N, k, "knn_query")
    if cells is None:
        cells = knn_moved_cells(src, xi, batches)
    scratch = _cand_scratch(scratch, batches, N, src.device)
    idx = torch.empty((batches * N, k), dtype=torch.int32, device=src.device)
    L.check(L.lib().mmpde_knn_query_cand(L.ptr(src), L.ptr(qry), L.ptr(xi), L.ptr(ref),
                                         L.ptr(cells), float(skip_above), batches, N, k,
                                         L.ptr(cand), L.ptr(idx), L.ptr(_ties(ties)),
                                         L.ptr(scratch), L.stream(src.device)),
            "mmpde_knn_query_cand")
    return idx


_SKINNY_WS = {}


def _skinny_workspace(device, nbytes: int) -> torch.Tensor:
    """Split-K scratch of mmpde_linear_skinny_ws: zeroed once, then reused (each
    call leaves its ticket counters at zero).  One per device and stream: calls
    on one stream are ordered, so they may share it."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _SKINNY_WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.zeros((max(nbytes, 4) // 4 + 1024,), dtype=torch.float32, device=device)
        _SKINNY_WS[key] = ws
    return ws


def linear_skinny(x: torch.Tensor, w: torch.Tensor, b=None, act: int = L.ACT_NONE,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """act(x @ w.T + b) for a few rows (M = trajectories)."""
    L.require_device(x, w)
    x = L.f32c(x)
    w = L.f32c(w)
    m, k = x.shape
    n = w.shape[0]
    y = out if out is not None else torch.empty((m, n), dtype=torch.float32, device=x.device)
    lib = L.lib()
    wsb = lib.mmpde_linear_skinny_workspace_bytes(m, n, k)
    ws = _skinny_workspace(x.device, wsb)
    L.check(lib.mmpde_linear_skinny_ws(L.ptr(x), k, m, k, L.ptr(w), k,
                                       L.ptr(L.f32c(b)) if b is not None else None, n, act,
                                       L.ptr(y), n, L.ptr(ws), wsb, L.stream(x.device)),
            "mmpde_linear_skinny")
    return y


def linear_rows(x: torch.Tensor, w: torch.Tensor, b=None, act: int = L.ACT_NONE) -> torch.Tensor:
    """act(x @ w.T + b) for any number of rows (x [..., k]): linear_skinny on
    blocks of at most 4096 rows (the skinny kernel's row limit)."""
    lead = x.shape[:-1]
    x2 = L.f32c(x).reshape(-1, x.shape[-1])
    y = torch.empty((x2.shape[0], w.shape[0]), dtype=torch.float32, device=x2.device)
    for r0 in range(0, x2.shape[0], 4096):
        linear_skinny(x2[r0:r0 + 4096], w, b, act, out=y[r0:r0 + 4096])
    return y.reshape(*lead, w.shape[0])


def resample_bilinear(u: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
    """F.interpolate(u[:, None], size=(oh, ow), mode='bilinear',
    align_corners=True)[:, 0] of u [..., h, w] (data_creator_2d.py:102-103)."""
    L.require_device(u)
    h, w = u.shape[-2:]
    x = L.f32c(u).reshape(-1, h, w)
    y = torch.empty((x.shape[0], oh, ow), dtype=torch.float32, device=x.device)
    L.check(L.lib().mmpde_resample_bilinear(L.ptr(x), x.shape[0], h, w, oh, ow, L.ptr(y),
                                            L.stream(x.device)), "mmpde_resample_bilinear")
    return y.reshape(*u.shape[:-2], oh, ow)


def conv2d(x: torch.Tensor, w: torch.Tensor, b, stride: int, pad: int, act: int,
           residual=None, circular: bool = False, res_after_act: bool = False) -> torch.Tensor:
    """act(conv2d(x, w, b, stride, pad) [+ residual]), NCHW fp32; circular:
    padding_mode='circular'; res_after_act: residual + act(conv2d(...))."""
    L.require_device(x, w)
    x = L.f32c(x)
    bt, cin, h, wd = x.shape
    cout, _, ks, _ = w.shape
    oh = (h + 2 * pad - ks) // stride + 1
    ow = (wd + 2 * pad - ks) // stride + 1
    y = torch.empty((bt, cout, oh, ow), dtype=torch.float32, device=x.device)
    res = L.f32c(residual) if residual is not None else None
    # w and b are held until the launch: f32c copies a misaligned or strided
    # tensor, and a copy freed before the next one is made is that one's memory
    w = L.f32c(w)
    b = L.f32c(b) if b is not None else None
    L.check(L.lib().mmpde_conv2d_ex(L.ptr(x), bt, cin, h, wd, L.ptr(w), L.ptr(b), cout, ks, stride,
                                    pad, L.PAD_CIRCULAR if circular else L.PAD_ZEROS, L.ptr(res),
                                    int(res_after_act), act, L.ptr(y), L.stream(x.device)),
            "mmpde_conv2d_ex")
    return y


def conv2d_grad_weight(x: torch.Tensor, dy: torch.Tensor, ks: int, pad: int, circular: bool,
                       bias: bool = True):
    """(dw [cout, cin, ks, ks], db [cout] or None) of a stride-1 conv2d with
    output size = input size (mmpde_conv2d_grad_weight; deterministic)."""
    L.require_device(x, dy)
    x, dy = L.f32c(x), L.f32c(dy)
    bt, cin, h, wd = x.shape
    cout = dy.shape[1]
    if dy.shape != (bt, cout, h, wd):
        raise ValueError("dy must be [batches, cout, h, w] of x's batches and plane")
    dw = torch.empty((cout, cin, ks, ks), dtype=torch.float32, device=x.device)
    db = torch.empty((cout,), dtype=torch.float32, device=x.device) if bias else None
    L.check(L.lib().mmpde_conv2d_grad_weight(L.ptr(x), bt, cin, h, wd, L.ptr(dy), cout, ks, pad,
                                             L.PAD_CIRCULAR if circular else L.PAD_ZEROS, L.ptr(dw), L.ptr(db),
                                             L.stream(x.device)), "mmpde_conv2d_grad_weight")
    return dw, db


class LinearRows(torch.autograd.Function):
    """y = x W^T + b over many rows: the train-mode Linears of GNN_Layer_FS_2D /
    MP_PDE_Solver_2D (gnn_2d.py:53-69,99-114) and ItpNet (interpolate.py:79-93)
    on the HIP row GEMMs (rows.py, csrc/rgemm.hip: exact fp32 MFMA): forward
    mmpde_rgemm (NT), dX = dY W mmpde_rgemm (NN), dW = dY^T X and db over the
    rows in fixed row chunks (mmpde_rgemm_tn), or for a skinny map (the Conv1d
    head's windows, the embedding's first Linear) mmpde_rows_grad_weight.  No
    library GEMM; deterministic for a given shape."""

    @staticmethod
    def forward(ctx, x, w, b):
        L.require_device(x, w, b)
        x, wc = L.f32c(x), L.f32c(w)
        ctx.save_for_backward(x, wc)
        ctx.has_bias = b is not None
        return rows.linear_fwd(x, wc, L.f32c(b) if b is not None else None)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = L.f32c(dy)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = rows.linear_bwd_input(dy, w)
        n, k = x.shape
        nout = w.shape[0]
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if not (want_b or ctx.needs_input_grad[1]):
            return gx, None, None          # frozen weight and bias: dX only
        if n >= 4096 and rows_grad_fits(k, nout):
            # skinny map (head windows, embedding): dW and db in one row pass
            gw, gb = rows_grad_weight(x, dy, k if ctx.needs_input_grad[1] else 0, want_b)
            return gx, gw, gb
        gw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        gb = torch.empty((nout,), dtype=torch.float32, device=x.device) if want_b else None
        rows.linear_bwd_weight(dy, x, gw, gb)
        return gx, gw, gb


def rows_grad_fits(k: int, nout: int) -> bool:
    """Shapes mmpde_rows_grad_weight takes with the weight gradient."""
    return 0 < k <= 64 and nout <= 128 and k * nout + nout <= 1280


class HeadTrain(torch.autograd.Function):
    """output_mlp(h[:, None]) of MP_PDE_Solver_2D at time_window 1 (gnn_2d.py:
    108-114: Conv1d(1, 4, 16, 3) -> ReLU -> Conv1d(4, 8, 12, 3) -> ReLU ->
    Conv1d(8, 1, 8, 2)) in train mode: y [n, 1] from h [n, 128] on
    mmpde_head_train_forward, dL/dh and the six weight / bias gradients on
    mmpde_head_train_backward (one lane per node, fixed summation orders)."""

    @staticmethod
    def forward(ctx, h, w1, b1, w2, b2, w3, b3):
        L.require_device(h, w1, b1, w2, b2, w3, b3)
        h = L.f32c(h)
        ws = [L.f32c(t) for t in (w1, b1, w2, b2, w3, b3)]
        n = h.shape[0]
        y = torch.empty((n, 1), dtype=torch.float32, device=h.device)
        L.check(L.lib().mmpde_head_train_forward(L.ptr(h), h.stride(0), n, *[L.ptr(t) for t in ws], L.ptr(y),
                                                 L.stream(h.device)), "mmpde_head_train_forward")
        ctx.save_for_backward(h, *ws)
        ctx.shapes = [tuple(t.shape) for t in (w1, b1, w2, b2, w3, b3)]
        return y

    @staticmethod
    def backward(ctx, dy):
        h, *ws = ctx.saved_tensors
        dy = L.f32c(dy)
        n = h.shape[0]
        dev = h.device
        dh = torch.empty_like(h)
        grads = torch.empty((HEAD_TRAIN_GRADS,), dtype=torch.float32, device=dev)
        nb = L.lib().mmpde_head_train_workspace_bytes(n)
        wk = torch.empty((nb // 4,), dtype=torch.float32, device=dev)
        L.check(L.lib().mmpde_head_train_backward(L.ptr(h), h.stride(0), n, *[L.ptr(t) for t in ws], L.ptr(dy),
                                                  L.ptr(dh), dh.stride(0), L.ptr(grads), L.ptr(wk), nb,
                                                  L.stream(dev)), "mmpde_head_train_backward")
        out, o = [], 0
        for shp in ctx.shapes:
            k = 1
            for d in shp:
                k *= d
            out.append(grads[o:o + k].view(shp))
            o += k
        gh = dh if ctx.needs_input_grad[0] else None
        return (gh, *[g if ctx.needs_input_grad[1 + j] else None for j, g in enumerate(out)])


HEAD_TRAIN_GRADS = 525  # include/mmpde_hip.h MMPDE_HEAD_TRAIN_GRADS


def head_train_fits(output_mlp, h: torch.Tensor) -> bool:
    """The Conv1d head HeadTrain implements (gnn_2d.py:108-114 at time_window 1).
    MMPDE_HEAD_FUSED=0 keeps the unfold + LinearRows form (A/B runs)."""
    if os.environ.get("MMPDE_HEAD_FUSED", "1") == "0":
        return False
    try:
        convs = [output_mlp[i] for i in (0, 2, 4)]
    except (IndexError, TypeError):
        return False
    if len(output_mlp) != 5 or not all(isinstance(c, torch.nn.Conv1d) for c in convs):
        return False
    want = [((4, 1, 16), 3), ((8, 4, 12), 3), ((1, 8, 8), 2)]
    for c, (shape, st) in zip(convs, want):
        if (tuple(c.weight.shape) != shape or c.stride[0] != st or c.padding[0] != 0 or c.dilation[0] != 1
                or c.groups != 1 or c.bias is None or c.padding_mode != "zeros"):
            return False
    return (isinstance(output_mlp[1], torch.nn.ReLU) and isinstance(output_mlp[3], torch.nn.ReLU)
            and h.dim() == 2 and h.shape[1] == 128 and h.is_cuda and h.dtype == torch.float32)


def rows_grad_weight(x: torch.Tensor, dy: torch.Tensor, k: int, bias: bool):
    """(dW = dy^T x [nout, k] or None when k = 0, db = sum_rows dy or None) on
    mmpde_rows_grad_weight (fixed summation order)."""
    rows, nout = dy.shape
    dy = L.f32c(dy)
    x = L.f32c(x) if k else None
    dev = dy.device
    gw = torch.empty((nout, k), dtype=torch.float32, device=dev) if k else None
    gb = torch.empty((nout,), dtype=torch.float32, device=dev) if bias else None
    nb = L.lib().mmpde_rows_grad_weight_workspace_bytes(rows, k, nout)
    ws = torch.empty((nb // 4,), dtype=torch.float32, device=dev)
    L.check(L.lib().mmpde_rows_grad_weight(L.ptr(x), x.stride(0) if k else 0, rows, k, L.ptr(dy), dy.stride(0),
                                           nout, L.ptr(gw), L.ptr(gb), L.ptr(ws), nb, L.stream(dev)),
            "mmpde_rows_grad_weight")
    return gw, gb


class BatchNormRows(torch.autograd.Function):
    """nn.BatchNorm1d in train mode over [n, C] rows of x + res (the residual
    add of GNN_Layer_FS_2D, norm(h + update), gnn_2d.py:69, and the
    embedding's BatchNorm1d, gnn_2d.py:101,105) on
    mmpde_batch_norm_rows_train / _backward: batch statistics, running
    statistics update in place, normalisation; gradients for x, res, weight
    and bias.  Deterministic."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, eps, factor, running_mean, running_var):
        n, C = x.shape
        dev = x.device
        y = torch.empty_like(x)
        stats = torch.empty((4 * C,), dtype=torch.float32, device=dev)
        nb = L.lib().mmpde_batch_norm_rows_workspace_bytes(n, C) + 12 * C
        ws = torch.empty((nb // 4,), dtype=torch.float32, device=dev)
        L.check(L.lib().mmpde_batch_norm_rows_train(
            L.ptr(x), L.ptr(res), n, C, L.ptr(weight), L.ptr(bias), float(eps), float(factor),
            L.ptr(running_mean), L.ptr(running_var), L.ptr(y), L.ptr(stats), L.ptr(ws), nb, L.stream(dev)),
            "mmpde_batch_norm_rows_train")
        ctx.save_for_backward(x, res, weight, stats)
        ctx.ws = nb
        ctx.has = (res is not None, weight is not None, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, res, weight, stats = ctx.saved_tensors
        has_res, has_w, has_b = ctx.has
        n, C = x.shape
        dev = x.device
        dy = L.f32c(dy)
        dx = torch.empty_like(x)
        dw = torch.empty((C,), dtype=torch.float32, device=dev) if has_w else None
        db = torch.empty((C,), dtype=torch.float32, device=dev) if has_b else None
        ws = torch.empty((ctx.ws // 4,), dtype=torch.float32, device=dev)
        L.check(L.lib().mmpde_batch_norm_rows_backward(
            L.ptr(x), L.ptr(res), L.ptr(dy), n, C, L.ptr(weight), L.ptr(stats), L.ptr(dx), L.ptr(dw), L.ptr(db),
            L.ptr(ws), ctx.ws, L.stream(dev)), "mmpde_batch_norm_rows_backward")
        return dx, (dx if has_res else None), dw, db, None, None, None, None


def _batch_norm_rows_segments(bn, x, res, segments: int) -> torch.Tensor:
    """batch_norm_rows' train-mode route for segments > 1 (forward only)."""
    params = (bn.weight, bn.bias) if torch.is_grad_enabled() else ()
    if any(t is not None and t.requires_grad for t in (x, res, *params)):
        raise ValueError("batch_norm_rows(segments > 1) is forward only: x and res must not require grad, and the "
                         "module's parameters only under torch.no_grad()")
    if x.dim() != 2 or x.shape[0] % segments or x.shape[1] % 4 or not 4 <= x.shape[1] <= 1024:
        raise ValueError(f"batch_norm_rows(segments={segments}): x must be [segments * n, C] with C % 4 == 0, "
                         f"C <= 1024 (got {tuple(x.shape)})")
    n, C = x.shape[0] // segments, x.shape[1]
    if n < 2:
        raise ValueError("batch_norm_rows: a train-mode segment needs more than one row")
    if res is not None and res.shape != x.shape:
        raise ValueError("batch_norm_rows: res must have x's shape")
    L.require_device(x, res)
    track = bn.track_running_stats and bn.num_batches_tracked is not None
    if track and bn.momentum is None:   # a factor per segment: the calls one after the other
        with torch.no_grad():
            return torch.cat([batch_norm_rows(bn, x[s * n:(s + 1) * n], None if res is None else res[s * n:(s + 1) * n])
                              for s in range(segments)])
    factor = 0.0
    if track:
        bn.num_batches_tracked.add_(segments)
        factor = bn.momentum
    rm = bn.running_mean if bn.track_running_stats else None
    rv = bn.running_var if bn.track_running_stats else None
    x = x.detach().float().contiguous()
    res = res.detach().float().contiguous() if res is not None else None
    w = L.f32c(bn.weight.detach()) if bn.weight is not None else None
    b = L.f32c(bn.bias.detach()) if bn.bias is not None else None
    dev = x.device
    y = torch.empty_like(x)
    stats = torch.empty((segments, 4 * C), dtype=torch.float32, device=dev)
    nb = L.lib().mmpde_batch_norm_rows_train_segments_workspace_bytes(segments, n, C)
    ws = torch.empty((nb // 4,), dtype=torch.float32, device=dev)
    L.check(L.lib().mmpde_batch_norm_rows_train_segments(
        L.ptr(x), L.ptr(res), segments, n, C, L.ptr(w), L.ptr(b), float(bn.eps), float(factor), L.ptr(rm), L.ptr(rv),
        L.ptr(y), L.ptr(stats), L.ptr(ws), nb, L.stream(dev)), "mmpde_batch_norm_rows_train_segments")
    return y


def batch_norm_rows(bn: torch.nn.BatchNorm1d, x: torch.Tensor, res: torch.Tensor | None = None,
                    segments: int = 1) -> torch.Tensor:
    """bn(x + res) for [n, C] rows: the HIP kernels in train mode (running
    statistics and num_batches_tracked advanced as nn.BatchNorm1d does), the
    module itself in eval mode.
    segments = S > 1, train mode: x (+ res) is S segments of n / S consecutive
    rows, each normalised as a batch of its own, the running statistics
    advanced S times in segment order and num_batches_tracked by S -- what S
    calls on the segments give, bit for bit -- in one
    mmpde_batch_norm_rows_train_segments call.  Forward only: raises if x or
    res requires grad, or a parameter does outside torch.no_grad(); a shape the
    kernel does not take raises too.  momentum=None (the cumulative average, another factor for
    every segment) takes the S calls one after the other instead.  In eval mode
    BatchNorm acts row by row, so segments changes nothing there."""
    if segments < 1:
        raise ValueError(f"batch_norm_rows: segments must be >= 1 (got {segments})")
    if segments > 1 and bn.training:
        return _batch_norm_rows_segments(bn, x, res, segments)
    if not bn.training or x.dim() != 2 or x.shape[1] % 4 or x.shape[1] > 1024 or x.shape[0] < 2:
        return bn(x if res is None else x + res)
    factor = 0.0
    if bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
        factor = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else bn.momentum
    rm = bn.running_mean if bn.track_running_stats else None
    rv = bn.running_var if bn.track_running_stats else None
    x = x.float().contiguous()                  # no detach: autograd inputs
    res = res.float().contiguous() if res is not None else None
    return BatchNormRows.apply(x, res, bn.weight, bn.bias, bn.eps, factor, rm, rv)


def linear_train(x: torch.Tensor, lin: torch.nn.Linear) -> torch.Tensor:
    """lin(x) for [n, k] rows in train mode through LinearRows."""
    return LinearRows.apply(x.contiguous(), lin.weight, lin.bias)


class Conv2dSame(torch.autograd.Function):
    """Differentiable stride-1 conv2d with output size = input size (odd ks,
    pad = ks // 2), zero or circular padding, on the HIP kernels: forward
    mmpde_conv2d_ex; backward dx = the same convolution of dy with the flipped,
    transposed kernel (circular indices wrap the same way), dw / db
    mmpde_conv2d_grad_weight.  Deterministic."""

    @staticmethod
    def forward(ctx, x, w, b, circular: bool):
        ks = w.shape[-1]
        if w.shape[-2] != ks or ks % 2 != 1:
            raise ValueError("Conv2dSame takes square odd kernels")
        ctx.save_for_backward(x, w)
        ctx.circular = circular
        ctx.has_bias = b is not None
        return conv2d(x, w, b, 1, ks // 2, L.ACT_NONE, circular=circular)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        ks = w.shape[-1]
        dy = L.f32c(dy)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            wt = w.flip(2, 3).transpose(0, 1).contiguous()
            gx = conv2d(dy, wt, None, 1, ks // 2, L.ACT_NONE, circular=ctx.circular)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gw, gb = conv2d_grad_weight(x, dy, ks, ks // 2, ctx.circular, bias=ctx.has_bias)
        return gx, gw, gb, None


class ItpNetPack:
    """ItpNet.packed() of a shape the specialised kernel does not serve: the
    image of mmpde_itp_net_pack, its size and the shape block (n_layers and
    widths, no pointers) that mmpde_itp_interp_net reads at the call."""
    __slots__ = ("image", "shape", "nbytes")

    def __init__(self, image: torch.Tensor, shape, nbytes: int):
        self.image, self.shape, self.nbytes = image, shape, nbytes

    @property
    def widths(self):
        return list(self.shape.widths[:self.shape.n_layers + 1])


def itp_interp(src, vals, qry, idx, batches: int, packed, addend=None, addend2=None):
    """ItpNet weights + weighted neighbour sum (interpolate.py:77-93,
    data_creator_2d.py:80-83), + addend, then + addend2 (both optional).
    packed is ItpNet.packed(mode): the bare image of the default widths
    (mmpde_itp_interp_ex) or an ItpNetPack (mmpde_itp_interp_net).
    Returns [batches * n_qry] fp32."""
    net = packed if isinstance(packed, ItpNetPack) else None
    if net is not None:
        packed = net.image
    L.require_device(src, vals, qry, idx, packed)
    src = L.f32c(src).reshape(-1, 2)
    qry = L.f32c(qry).reshape(-1, 2)
    vals = L.f32c(vals).reshape(-1)
    ns, nq = src.shape[0] // batches, qry.shape[0] // batches
    out = torch.empty((batches * nq,), dtype=torch.float32, device=src.device)
    add = L.f32c(addend).reshape(-1) if addend is not None else None
    add2 = L.f32c(addend2).reshape(-1) if addend2 is not None else None
    if net is not None:
        L.check(L.lib().mmpde_itp_interp_net(L.ptr(src), L.ptr(vals), L.ptr(qry), L.ptr(idx.contiguous()),
                                             batches, ns, nq, ctypes.byref(net.shape), L.ptr(packed),
                                             net.nbytes, L.ptr(add), L.ptr(add2), L.ptr(out),
                                             L.stream(src.device)), "mmpde_itp_interp_net")
        return out
    L.check(L.lib().mmpde_itp_interp_ex(L.ptr(src), L.ptr(vals), L.ptr(qry), L.ptr(idx.contiguous()),
                                        batches, ns, nq, L.ptr(packed), L.ptr(add), L.ptr(add2),
                                        L.ptr(out), L.stream(src.device)), "mmpde_itp_interp_ex")
    return out


def mesh_relax(mesh: torch.Tensor, xi: torch.Tensor, hess: torch.Tensor | None = None, *, batches: int,
               alpha: float = 1.0, floor: float | None = None, alpha_out=None, lam_out=None, det_out=None,
               detmin_out=None, folds_out=None, guarded_total=None):
    """The fold guard (mmpde_dmm_mesh_relax): the relaxation that ends the
    reference's moving_mesh[_tri], x = alpha x + (1 - alpha) xi
    (data_creator_2d.py:109-111,133-135), in place on mesh [batches * N, 2] (the
    full move of DMM.mesh / mesh_hess) with xi [N, 2] the fixed grid.
    floor None: every trajectory is relaxed by alpha.  floor in (0, 1): a
    trajectory whose full move would leave an eigenvalue of dx/dxi = I + alpha
    Hess phi below floor at some node is moved only as far as keeps it at floor,
    alpha_b = (1 - floor) / (-lam_b), lam_b the smallest eigenvalue of hess
    [batches * N, 3] (mesh_hess's) over the trajectory; a NaN in a trajectory's
    hess gives alpha_b = 0.  Rows of trajectories with alpha_b == 1 keep their
    bits.  guarded_total: a [batches] int32 counter, += (alpha_b < alpha).
    Returns (mesh, alpha_b [batches], lam_b [batches], detmin [batches], folds
    [batches] int32), the last two of det(I + alpha_b Hess phi) (det_out:
    [batches * N], to keep it); lam_b, detmin and folds are None without hess.
    No synchronisation; capturable."""
    L.require_device(mesh, xi, hess)
    if mesh.dtype != torch.float32 or not mesh.is_contiguous() or mesh.dim() != 2 or mesh.shape[1] != 2 \
            or mesh.data_ptr() % 8:
        raise ValueError("mesh must be a contiguous float32 [batches * N, 2] tensor (it is relaxed in place)")
    xi = L.f32c(xi).reshape(-1, 2)
    n, N = mesh.shape[0], xi.shape[0]
    if batches < 1 or n != batches * N or n == 0:
        raise ValueError("mesh rows must be batches copies of xi's")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha {alpha}: the relaxation takes 0 <= alpha <= 1")
    if floor is not None and not 0.0 < floor < 1.0:
        raise ValueError(f"floor {floor}: None (no guard) or 0 < floor < 1")
    if hess is None:
        if floor is not None:
            raise ValueError("the guard (floor) needs hess")
        if not (lam_out is None and det_out is None and detmin_out is None and folds_out is None):
            raise ValueError("lam_out, det_out, detmin_out and folds_out need hess")
    elif hess.dtype != torch.float32 or not hess.is_contiguous() or hess.numel() != 3 * n:
        raise ValueError("hess must be a contiguous float32 [batches * N, 3] tensor")

    def buf(t, shape, dtype, what):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=mesh.device)
        L.require_device(t)
        if t.dtype != dtype or not t.is_contiguous() or t.numel() != torch.Size(shape).numel():
            raise ValueError(f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)}")
        return t

    alpha_b = buf(alpha_out, (batches,), torch.float32, "alpha_out")
    lam = det = detmin = folds = None
    if hess is not None:
        lam = buf(lam_out, (batches,), torch.float32, "lam_out")
        det = buf(det_out, (n,), torch.float32, "det_out")
        detmin = buf(detmin_out, (batches,), torch.float32, "detmin_out")
        folds = buf(folds_out, (batches,), torch.int32, "folds_out")
    if guarded_total is not None:
        guarded_total = buf(guarded_total, (batches,), torch.int32, "guarded_total")
    io = L.DmmRelaxIO(L.ptr(alpha_b), L.ptr(lam), L.ptr(det), L.ptr(detmin), L.ptr(folds), L.ptr(guarded_total))
    L.check(L.lib().mmpde_dmm_mesh_relax(L.ptr(mesh), L.ptr(xi), L.ptr(hess), batches, N, float(alpha),
                                         float(floor) if floor is not None else 0.0, ctypes.byref(io),
                                         L.stream(mesh.device)), "mmpde_dmm_mesh_relax")
    return mesh, alpha_b, lam, detmin, folds


# --------------------------------------------------------------------------- random-feature phase
RfFeatures = collections.namedtuple("RfFeatures", ("s", "s_x", "s_y", "s_xx", "s_xy", "s_yy"))
RfFeatures.__doc__ = """ops.dmm_rf_features's tables, [n_grid, L'] each: the features s = DMM.forward(rf=True)'s
second_out and their derivatives in the grid row; s_xx, s_xy, s_yy are None with second_order=False."""


def dmm_rf_features(branch: torch.Tensor, grid: torch.Tensor, head_params, second_order: bool = True,
                    workspace: torch.Tensor | None = None) -> RfFeatures:
    """mmpde_dmm_rf_features: the random features of the DMM head and their
    derivatives per feature, which the reference's random-feature phase takes
    from 6 L' autograd.grad calls per batch (mesh/dmm_utils.py:883-905).
    branch [B, L] (the model's branch output), grid [n_grid, 2] (row i belongs to
    trajectory i // (n_grid // B)), head_params: the model's _lib.DmmHead.
    Deliberate difference: the reference computes so_xy and so_yx separately;
    they are equal, and the one table s_xy stands for both.  s is bit for bit
    mmpde_dmm_phi's second_out; with second_order=False the first-order tables
    keep their bits.  No synchronisation; capturable given a workspace."""
    L.require_device(branch, grid)
    branch = L.f32c(branch)
    grid = L.f32c(grid).reshape(-1, 2)
    hd = head_params
    if branch.dim() != 2 or branch.shape[1] != hd.latent:
        raise ValueError("branch must be [B, L]")
    B, ng = branch.shape[0], grid.shape[0]
    if B < 1 or ng < 1 or ng % B:
        raise ValueError("grid rows must be a multiple of the batch size")
    lib = L.lib()
    nb = lib.mmpde_dmm_rf_features_workspace_bytes(B, ng, hd.latent, hd.hidden, hd.th)
    if workspace is None:
        workspace = torch.empty((nb // 4,), dtype=torch.float32, device=grid.device)
    else:
        L.require_device(workspace)
        if workspace.numel() * workspace.element_size() < nb:
            raise ValueError("workspace is smaller than mmpde_dmm_rf_features_workspace_bytes")
    tabs = [torch.empty((ng, hd.hidden), dtype=torch.float32, device=grid.device)
            for _ in range(6 if second_order else 3)] + [None] * (0 if second_order else 3)
    out = L.DmmRfOut(*[L.ptr(t) for t in tabs])
    L.check(lib.mmpde_dmm_rf_features(L.ptr(branch), B, L.ptr(grid), ng, ctypes.byref(hd), L.ptr(workspace),
                                      ctypes.byref(out), L.stream(grid.device)), "mmpde_dmm_rf_features")
    return RfFeatures(*tabs)


Jet = collections.namedtuple("Jet", ("phi", "phi_x", "phi_y", "phi_xx", "phi_xy", "phi_yy"))
Jet.__doc__ = """The Monge-Ampere jet of the DMM head per grid row: phi and its derivatives in the row;
phi_xx, phi_xy, phi_yy are None with second_order=False."""
JetGrads = collections.namedtuple("JetGrads", ("branch", "t0_w", "t0_b", "t1_w", "t1_b", "o0_w", "o0_b", "o1_w",
                                               "o1_b"))
JetGrads.__doc__ = """ops.dmm_jet_grad's gradients: of branch [B, L] and of trunk.layers[0/1] and
out_nn.layers[0/1] weight and bias, each in its parameter's shape."""


def _jet_args(branch, grid, hd, workspace):
    L.require_device(branch, grid)
    branch = L.f32c(branch)
    grid = L.f32c(grid).reshape(-1, 2)
    if branch.dim() != 2 or branch.shape[1] != hd.latent:
        raise ValueError("branch must be [B, L]")
    B, ng = branch.shape[0], grid.shape[0]
    if B < 1 or ng < 1 or ng % B:
        raise ValueError("grid rows must be a multiple of the batch size")
    nb = L.lib().mmpde_dmm_jet_workspace_bytes(B, ng, hd.latent, hd.hidden, hd.th)
    if workspace is None:
        workspace = torch.empty((max(nb, 16) // 4,), dtype=torch.float32, device=grid.device)
    else:
        L.require_device(workspace)
        if workspace.numel() * workspace.element_size() < nb:
            raise ValueError("workspace is smaller than mmpde_dmm_jet_workspace_bytes")
    return branch, grid, B, ng, workspace


def dmm_jet(branch: torch.Tensor, grid: torch.Tensor, head_params, o1_b: torch.Tensor | None = None,
            second_order: bool = True, workspace: torch.Tensor | None = None) -> Jet:
    """mmpde_dmm_jet: phi = out_nn(cat(branch_b, trunk(grid_i))) and its first and
    second derivatives in the grid row, [n_grid] each, in closed form (no
    autograd, no [n_grid, L'] table).  branch [B, L], grid [n_grid, 2] (row i
    belongs to trajectory i // (n_grid // B)), head_params: the model's
    _lib.DmmHead, o1_b: out_nn's last bias (None: 0).  With second_order=False
    the first-order outputs keep their bits.  No synchronisation; capturable
    given a workspace."""
    hd = head_params
    branch, grid, B, ng, workspace = _jet_args(branch, grid, hd, workspace)
    outs = [torch.empty((ng,), dtype=torch.float32, device=grid.device)
            for _ in range(6 if second_order else 3)] + [None] * (0 if second_order else 3)
    out = L.DmmJetOut(*[L.ptr(t) for t in outs])
    ob = L.f32c(o1_b) if o1_b is not None else None
    L.check(L.lib().mmpde_dmm_jet(L.ptr(branch), B, L.ptr(grid), ng, ctypes.byref(hd), L.ptr(ob),
                                  L.ptr(workspace), ctypes.byref(out), L.stream(grid.device)), "mmpde_dmm_jet")
    return Jet(*outs)


def dmm_jet_grad(branch: torch.Tensor, grid: torch.Tensor, head_params, cotangents,
                 workspace: torch.Tensor | None = None) -> JetGrads:
    """mmpde_dmm_jet_grad: the gradient of sum_c <cotangents[c], jet_c> in branch
    and the head's seven tensors and last bias.  cotangents: six [n_grid]
    tensors in Jet's order, None meaning zero.  The grid rows are data: no
    gradient in them.  Sums in a fixed order: the same bits on every call."""
    hd = head_params
    branch, grid, B, ng, workspace = _jet_args(branch, grid, hd, workspace)
    cots = []
    for c in tuple(cotangents) + (None,) * (6 - len(cotangents)):
        if c is not None:
            L.require_device(c)
            c = L.f32c(c).reshape(-1)
            if c.numel() != ng:
                raise ValueError("a cotangent must have one value per grid row")
        cots.append(c)
    dev = grid.device
    Lt, Lp, th = hd.latent, hd.hidden, hd.th
    g = JetGrads(*[torch.empty(s, dtype=torch.float32, device=dev)
                   for s in ((B, Lt), (th, 2), (th,), (Lt, th), (Lt,), (Lp, 2 * Lt), (Lp,), (1, Lp), (1,))])
    cot = L.DmmJetOut(*[L.ptr(c) for c in cots])
    gr = L.DmmJetGrads(*[L.ptr(t) for t in g])
    L.check(L.lib().mmpde_dmm_jet_grad(L.ptr(branch), B, L.ptr(grid), ng, ctypes.byref(hd), None, L.ptr(workspace),
                                       ctypes.byref(cot), ctypes.byref(gr), L.stream(dev)), "mmpde_dmm_jet_grad")
    return g


def _gnn_weights(ws):
    return L.DmmGnnWeights(*[t.data_ptr() for t in ws])


class DmmGnnLayerTrain(torch.autograd.Function):
    """The update of one train-mode DMM GNN layer (GNN_Layer_FS_2D of
    dmm_model.py, hidden 4): upd = update_net_2(update_net_1(cat(h, mean of
    message_net_2(message_net_1(cat(h_i, h_j, u_i - u_j, g_i - g_j))))))
    [B N, 4], before the residual and the BatchNorm, on
    mmpde_dmm_gnn_train_forward / _backward.  h [B N, 4], u [B N], grid [N, 2],
    nbr [N, k] int32 local, rev = ops.reverse_adjacency(nbr) of the same table,
    then the eight tensors of message_net_1/2 and update_net_1/2.  Gradients for
    h and the eight tensors (u, the grid and the table are data); only the
    inputs are saved -- the backward recomputes the layer -- and nothing per
    edge outlives a call.  Deterministic."""

    @staticmethod
    def forward(ctx, h, u, grid, nbr, rev, *params):
        L.require_device(h, u, grid, nbr, *rev, *params)
        h, u, grid = L.f32c(h), L.f32c(u).reshape(-1), L.f32c(grid).reshape(-1, 2)
        ws = [L.f32c(t) for t in params]
        n, k = nbr.shape
        nt, hidden = h.shape
        if len(ws) != 8 or grid.shape[0] != n or nt % n or u.numel() != nt or nbr.dtype != torch.int32:
            raise ValueError("DmmGnnLayerTrain: h [B N, C], u [B N], grid [N, 2], nbr [N, k] int32, eight tensors")
        nbr = nbr.contiguous()
        upd = torch.empty_like(h)
        wp = _gnn_weights(ws)
        L.check(L.lib().mmpde_dmm_gnn_train_forward(L.ptr(h), L.ptr(u), L.ptr(grid), nt // n, n, L.ptr(nbr), k, hidden,
                                                    ctypes.byref(wp), L.ptr(upd), L.stream(h.device)),
                "mmpde_dmm_gnn_train_forward")
        ctx.save_for_backward(h, u, grid, nbr, rev[0], rev[1], *ws)
        ctx.shapes = [tuple(t.shape) for t in params]
        return upd

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_upd):
        h, u, grid, nbr, rev_off, rev_edge, *ws = ctx.saved_tensors
        d_upd = L.f32c(d_upd)
        n, k = nbr.shape
        nt, hidden = h.shape
        dev = h.device
        d_h = torch.empty_like(h)
        grads = torch.empty((L.DMM_GNN_TRAIN_GRADS,), dtype=torch.float32, device=dev)
        nb = L.lib().mmpde_dmm_gnn_train_workspace_bytes(nt // n, n, k)
        wk = torch.empty((nb // 4,), dtype=torch.float32, device=dev)
        wp = _gnn_weights(ws)
        L.check(L.lib().mmpde_dmm_gnn_train_backward(
            L.ptr(h), L.ptr(u), L.ptr(grid), nt // n, n, L.ptr(nbr), k, hidden, L.ptr(rev_off), L.ptr(rev_edge),
            ctypes.byref(wp), L.ptr(d_upd), L.ptr(d_h), L.ptr(grads), L.ptr(wk), L.stream(dev)),
            "mmpde_dmm_gnn_train_backward")
        out, o = [], 0
        for j, shp in enumerate(ctx.shapes):
            cnt = math.prod(shp)
            out.append(grads[o:o + cnt].view(shp) if ctx.needs_input_grad[5 + j] else None)
            o += cnt
        return (d_h if ctx.needs_input_grad[0] else None, None, None, None, None, *out)


class DmmDecodeTrain(torch.autograd.Function):
    """decoding_mlp = DenseNet[4, 128, 1] of the DMM graph branch in train mode:
    d [n, 1] = w1 tanh(w0 h + b0) + b1 on mmpde_dmm_decode_train_forward, and
    dL/dh with the four parameter gradients on _backward.  Only the inputs are
    saved; no [n, 128] table is held in either direction.  Deterministic."""

    @staticmethod
    def forward(ctx, h, w0, b0, w1, b1):
        L.require_device(h, w0, b0, w1, b1)
        h = L.f32c(h)
        ws = [L.f32c(t) for t in (w0, b0, w1, b1)]
        n, hidden = h.shape
        if tuple(ws[0].shape) != (128, hidden) or ws[1].numel() != 128 or ws[2].numel() != 128 or ws[3].numel() != 1:
            raise ValueError("DmmDecodeTrain: DenseNet[C, 128, 1] only")
        out = torch.empty((n, 1), dtype=torch.float32, device=h.device)
        L.check(L.lib().mmpde_dmm_decode_train_forward(L.ptr(h), n, hidden, *[L.ptr(t) for t in ws], L.ptr(out),
                                                       L.stream(h.device)), "mmpde_dmm_decode_train_forward")
        ctx.save_for_backward(h, *ws[:3])
        ctx.shapes = [tuple(t.shape) for t in (w0, b0, w1, b1)]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        h, w0, b0, w1 = ctx.saved_tensors
        d_out = L.f32c(d_out).reshape(-1)
        n, hidden = h.shape
        dev = h.device
        d_h = torch.empty_like(h)
        grads = torch.empty((L.DMM_DECODE_TRAIN_GRADS,), dtype=torch.float32, device=dev)
        nb = L.lib().mmpde_dmm_decode_train_workspace_bytes(n)
        wk = torch.empty((nb // 4,), dtype=torch.float32, device=dev)
        L.check(L.lib().mmpde_dmm_decode_train_backward(L.ptr(h), n, hidden, L.ptr(w0), L.ptr(b0), L.ptr(w1),
                                                        L.ptr(d_out), L.ptr(d_h), L.ptr(grads), L.ptr(wk),
                                                        L.stream(dev)), "mmpde_dmm_decode_train_backward")
        out, o = [], 0
        for j, shp in enumerate(ctx.shapes):
            cnt = math.prod(shp)
            out.append(grads[o:o + cnt].view(shp) if ctx.needs_input_grad[1 + j] else None)
            o += cnt
        return (d_h if ctx.needs_input_grad[0] else None, *out)


CONVNET_TRAIN_MAX_S = 51   # include/mmpde_hip.h MMPDE_DMM_CONVNET_TRAIN_MAX_S


def convnet_out_sizes(s: int) -> tuple[int, int]:
    """(o1, o2): the side of ConvNet's x1..x3 planes and of its last convolution's output for an s x s field."""
    o1 = (s - 1) // 2 + 1
    return o1, (o1 - 1) // 2 + 1


class ConvNetTrain(torch.autograd.Function):
    """The convolution stack of the DMM array branch's ConvNet (dmm_model.py:65-79,
    layers == 7) in train mode: f [B, o2^2] = flatten(tanh(c3(tanh(x1 +
    c2(tanh(c1(x1))))))) with x1 = tanh(c0(u)), on
    mmpde_dmm_convnet_train_forward / _backward.  u [B, s, s] (s <=
    CONVNET_TRAIN_MAX_S), then weight, bias of the four convolutions.  Gradients
    for the eight tensors; u is data.  Only the inputs are saved -- the backward
    recomputes the stack in LDS -- and its one workspace is a row of 6833 sums
    per field.  Deterministic."""

    @staticmethod
    def forward(ctx, u, *params):
        L.require_device(u, *params)
        if u.dim() != 3 or u.shape[1] != u.shape[2] or len(params) != 8:
            raise ValueError("ConvNetTrain: u [B, s, s] and the eight tensors of the four convolutions")
        shapes = [(8, 1, 5, 5), (8,), (16, 8, 5, 5), (16,), (8, 16, 5, 5), (8,), (1, 8, 5, 5), (1,)]
        if [tuple(t.shape) for t in params] != shapes:
            raise ValueError("ConvNetTrain: the convolutions of ConvNet(layers == 7) only")
        B, s = u.shape[0], u.shape[1]
        if s > CONVNET_TRAIN_MAX_S:
            raise NotImplementedError(f"ConvNetTrain: the kernels hold a field's whole state in LDS and take s <= "
                                      f"{CONVNET_TRAIN_MAX_S} (got {s})")
        u = L.f32c(u)
        ws = [L.f32c(t) for t in params]
        o2 = convnet_out_sizes(s)[1]
        f = torch.empty((B, o2 * o2), dtype=torch.float32, device=u.device)
        wp = L.DmmConvnetWeights(*[t.data_ptr() for t in ws])
        L.check(L.lib().mmpde_dmm_convnet_train_forward(L.ptr(u), B, s, ctypes.byref(wp), L.ptr(f),
                                                        L.stream(u.device)), "mmpde_dmm_convnet_train_forward")
        ctx.save_for_backward(u, *ws)
        ctx.shapes = shapes
        return f

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_f):
        u, *ws = ctx.saved_tensors
        d_f = L.f32c(d_f)
        B, s = u.shape[0], u.shape[1]
        dev = u.device
        grads = torch.empty((L.DMM_CONVNET_TRAIN_GRADS,), dtype=torch.float32, device=dev)
        nb = L.lib().mmpde_dmm_convnet_train_workspace_bytes(B)
        wk = torch.empty((nb // 4,), dtype=torch.float32, device=dev)
        wp = L.DmmConvnetWeights(*[t.data_ptr() for t in ws])
        L.check(L.lib().mmpde_dmm_convnet_train_backward(L.ptr(u), B, s, ctypes.byref(wp), L.ptr(d_f), L.ptr(grads),
                                                         L.ptr(wk), nb, L.stream(dev)),
                "mmpde_dmm_convnet_train_backward")
        out, o = [], 0
        for j, shp in enumerate(ctx.shapes):
            cnt = math.prod(shp)
            out.append(grads[o:o + cnt].view(shp) if ctx.needs_input_grad[1 + j] else None)
            o += cnt
        return (None, *out)


class FewRowsMlp(torch.autograd.Function):
    """A tanh MLP (tanh on all but the last Linear) over a few rows in train
    mode -- the DMM graph branch's output_mlp at M = B trajectories, [B, N] ->
    512 -> 256 -> L: the forward on mmpde_linear_skinny (split-K, tanh fused),
    the backward per layer dW = dZ^T X, db = sum dZ (mmpde_outer_rows), dX = dZ W
    as the skinny forward of W^T (mmpde_transpose), times tanh' of the layer
    input (mmpde_tanh_bwd), as interpolate.ResCutMlp does for the cylinder
    ``down`` MLP.  Arguments: x [M, K] (M <= 4096), then weight, bias per layer.
    The row GEMMs of LinearRows tile 32 rows at a time and leave most of the
    chip idle at M = 160 and K = 2521.  Exact fp32 products in fixed orders:
    deterministic."""

    @staticmethod
    def forward(ctx, x, *params):
        L.require_device(x, *params)
        ws, bs = params[0::2], params[1::2]
        ins = [L.f32c(x)]
        for i, (w, b) in enumerate(zip(ws, bs)):
            ins.append(linear_skinny(ins[-1], w, b, L.ACT_TANH if i + 1 < len(ws) else L.ACT_NONE))
        y = ins.pop()
        ctx.save_for_backward(*ins, *[L.f32c(w) for w in ws])
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        saved = ctx.saved_tensors
        nl = len(saved) // 2
        ins, ws = saved[:nl], saved[nl:]
        lib = L.lib()
        dev = dy.device
        st = L.stream(dev)
        grads = [None] * (2 * nl)
        g = L.f32c(dy)
        m = g.shape[0]
        for layer in range(nl - 1, -1, -1):
            w, xin = ws[layer], ins[layer]
            n, k = w.shape
            need_w, need_b = ctx.needs_input_grad[1 + 2 * layer], ctx.needs_input_grad[2 + 2 * layer]
            if need_w or need_b:
                dw = torch.empty((n, k), dtype=torch.float32, device=dev)
                db = torch.empty((n,), dtype=torch.float32, device=dev) if need_b else None
                L.check(lib.mmpde_outer_rows(L.ptr(g), n, L.ptr(xin), k, m, n, k, L.ptr(dw), k, L.ptr(db), st),
                        "mmpde_outer_rows")
                grads[2 * layer] = dw if need_w else None
                grads[2 * layer + 1] = db
            if layer == 0 and not ctx.needs_input_grad[0]:
                g = None
                break
            wt = torch.empty((k, n), dtype=torch.float32, device=dev)
            L.check(lib.mmpde_transpose(L.ptr(w), n, k, k, L.ptr(wt), n, st), "mmpde_transpose")
            dx = linear_skinny(g, wt)
            del wt          # stream-ordered: the next layer's dw and W^T may take its place
            if layer > 0:   # the layer's input is the previous layer's tanh output
                L.check(lib.mmpde_tanh_bwd(L.ptr(dx), L.ptr(xin), dx.numel(), L.ptr(dx), st), "mmpde_tanh_bwd")
            g = dx
        return (g, *grads)


class RfObjective:
    """random_feature_torch2 (mesh/dmm_utils.py:351-388) and its gradient on
    mmpde_rf_objective: f(w) = convex_rel (sum w^2)^2 + w1 loss_bound + w0 loss_in
    + w2 loss_convex for the last Linear's weight w [L'] over fixed feature tables.
    interior: RfFeatures of the sampled points x [M, 2] (second order); sides:
    the four boundary tables (s_x on x = 0 and x = 1, s_y on y = 0 and y = 1,
    [Mb, L'] each); ux, uy [bu, n, n], alpha, rhs [bu]: the sample's monitor
    fields, points i bx .. i bx + bx - 1 reading field i.
    ``obj(w)`` returns (f, g) as device tensors (f a 0-dim view); parts =
    (loss_in, loss_bound, loss_convex) and lhs [M] are those of the last call.
    Every call writes the same buffers: clone what must outlive the next call.
    Deliberate differences: one s_xy table for the reference's so_xy and so_yx;
    where the monitor's square root has no derivative (u_xi_x = u_xi_y = 0,
    autograd: NaN) the point contributes 0 to g.  Two calls on the same inputs
    give the same bits (fixed-order sums, no atomics)."""

    def __init__(self, interior: RfFeatures, sides, x, ux, uy, alpha, rhs, w0, w1, w2, convex_rel):
        from .dmm_train import unit_lattice

        tabs = [interior.s_x, interior.s_y, interior.s_xx, interior.s_xy, interior.s_yy]
        sides = list(sides)
        if len(sides) != 4 or any(t.dim() != 2 for t in sides) or any(t.shape != sides[0].shape for t in sides):
            raise ValueError("sides: four [Mb, L'] tables")
        if sides[0].shape[0] == 0:
            raise ValueError("no boundary points (Mb == 0): the reference's MSE over an empty side is NaN; "
                             "batch_size_x_rf must be at least 4")
        L.require_device(*tabs, *sides, x, ux, uy, alpha, rhs)
        sides = [L.f32c(t) for t in sides]
        tabs = [L.f32c(t) for t in tabs]
        x = L.f32c(x).reshape(-1, 2)
        M, n_feat = tabs[0].shape
        ux, uy = L.f32c(ux), L.f32c(uy)
        bu, n = ux.shape[0], ux.shape[-1]
        alpha, rhs = L.f32c(alpha).reshape(-1), L.f32c(rhs).reshape(-1)
        if any(t.shape != (M, n_feat) for t in tabs) or x.shape[0] != M or sides[0].shape[1] != n_feat:
            raise ValueError("the interior tables must be [M, L'] for x [M, 2], the sides [Mb, L']")
        if ux.shape != (bu, n, n) or uy.shape != ux.shape or alpha.numel() != bu or rhs.numel() != bu or M % bu:
            raise ValueError("ux, uy [bu, n, n], alpha, rhs [bu], bu dividing M")
        dev = x.device
        lat = unit_lattice(n, dev)
        self._keep = (tabs, sides, x, ux, uy, alpha, rhs, lat)
        self.pb = L.RfProblem(*[L.ptr(t) for t in tabs], *[L.ptr(t) for t in sides], L.ptr(x), L.ptr(ux),
                              L.ptr(uy), L.ptr(alpha), L.ptr(rhs), L.ptr(lat), M, sides[0].shape[0], n_feat, bu,
                              n, float(w0), float(w1), float(w2), float(convex_rel))
        self.n = n_feat
        nb = L.lib().mmpde_rf_objective_workspace_bytes(M, sides[0].shape[0])
        self.ws = torch.empty((nb // 4,), dtype=torch.float32, device=dev)
        self.fbuf = torch.empty((4,), dtype=torch.float32, device=dev)   # f, parts[3]
        self.g = torch.empty((n_feat,), dtype=torch.float32, device=dev)
        self.lhs = torch.empty((M,), dtype=torch.float32, device=dev)

    @property
    def parts(self):
        return self.fbuf[1:]

    def __call__(self, w: torch.Tensor):
        L.require_device(w)
        w = L.f32c(w).reshape(-1)
        if w.numel() != self.n:
            raise ValueError(f"w must have {self.n} entries")
        L.check(L.lib().mmpde_rf_objective(L.ptr(w), ctypes.byref(self.pb), L.ptr(self.ws), L.ptr(self.fbuf),
                                           L.ptr(self.g), self.fbuf.data_ptr() + 4, L.ptr(self.lhs),
                                           L.stream(w.device)), "mmpde_rf_objective")
        return self.fbuf[0], self.g


def _dense_check(H, n, *vecs):
    if n < 1 or n > L.BFGS_MAX_N:
        raise ValueError(f"n = {n}: the dense BFGS operations take 1 <= n <= {L.BFGS_MAX_N}")
    L.require_device(H, *vecs)
    if H.dtype != torch.float32 or not H.is_contiguous() or H.shape != (n, n):
        raise ValueError("H must be a contiguous float32 [n, n] tensor")
    for v in vecs:
        if v.dtype != torch.float32 or not v.is_contiguous() or v.numel() != n:
            raise ValueError("vectors must be contiguous float32 [n] tensors")


def sym_matvec(H: torch.Tensor, g: torch.Tensor, scale: float = 1.0, out: torch.Tensor | None = None):
    """out = scale * H g for H [n, n] float32, n <= 1024 (mmpde_sym_matvec): one wave
    per row, sums in a fixed order."""
    n = g.numel()
    _dense_check(H, n, g)
    if out is None:
        out = torch.empty_like(g)
    _dense_check(H, n, out)
    L.check(L.lib().mmpde_sym_matvec(L.ptr(H), L.ptr(g), n, L.ptr(out), float(scale), L.stream(g.device)),
            "mmpde_sym_matvec")
    return out


def bfgs_update(H: torch.Tensor, s: torch.Tensor, y: torch.Tensor, workspace: torch.Tensor | None = None):
    """H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T in place, rho = 1 / y.s
    (mmpde_bfgs_update), skipped on the device when y.s <= 1e-10; a symmetric H
    stays symmetric bit for bit."""
    n = s.numel()
    _dense_check(H, n, s, y)
    nb = L.lib().mmpde_bfgs_update_workspace_bytes(n)
    if workspace is None:
        workspace = torch.empty((nb // 4,), dtype=torch.float32, device=H.device)
    elif workspace.numel() * workspace.element_size() < nb:
        raise ValueError("workspace is smaller than mmpde_bfgs_update_workspace_bytes")
    L.check(L.lib().mmpde_bfgs_update(L.ptr(H), L.ptr(s), L.ptr(y), n, L.ptr(workspace), L.stream(H.device)),
            "mmpde_bfgs_update")
    return H


# --------------------------------------------------------------------------- mesh quality
MESH_QUALITY_MAX_N = 256   # include/mmpde_hip.h MMPDE_MESH_QUALITY_MAX_N

MeshQuality = collections.namedtuple(
    "MeshQuality", ("mean", "std", "range", "inverted", "area_ratio_min", "mg"))
MeshQuality.__doc__ = """ops.mesh_quality's per-trajectory result: mean, std (unbiased) and range (max - min)
of mg = monitor at the cell centre x cell area over the cells, the number of
inverted cells (int32), the smallest signed moved area / fixed-grid area, all
[batches]; mg [batches, C] or None."""


def mesh_cells_lattice(s: int) -> torch.Tensor:
    """The (s - 1)^2 quadrilaterals of the s x s lattice in flat 'xy' order, as
    the reference slices them (dmm_utils.py:1264-1267): [(s - 1)^2, 4] int32 (CPU)
    with columns (bl, br, tl, tr) = nodes (i, j), (i + 1, j), (i, j + 1),
    (i + 1, j + 1) of x.reshape(s, s), cell i (s - 1) + j."""
    if s < 2:
        raise ValueError(f"a lattice of {s} x {s} points has no cells")
    idx = torch.arange(s * s, dtype=torch.int32).reshape(s, s)
    cols = (idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:])
    return torch.stack([c.reshape(-1) for c in cols], dim=1).contiguous()


def mesh_cells_delaunay(grid: torch.Tensor) -> torch.Tensor:
    """The Delaunay triangles of the fixed grid [N, 2] (scipy, on the host, as
    the reference's evaluate_tri, dmm_utils.py:1174-1178): [T, 3] int32 (CPU),
    every triangle with its last two vertices swapped where needed so that
    (v1 - v0) x (v2 - v0) > 0 on the grid; indices checked to lie in [0, N)."""
    import numpy as np
    from scipy.spatial import Delaunay

    pts = grid.detach().cpu().numpy().astype(np.float64).reshape(-1, 2)
    tris = np.asarray(Delaunay(pts).simplices).astype(np.int64)
    if tris.ndim != 2 or tris.shape[1] != 3 or tris.shape[0] < 1:
        raise ValueError("the grid has no Delaunay triangles")
    if tris.min() < 0 or tris.max() >= pts.shape[0]:
        raise ValueError("Delaunay returned an index outside the grid")
    v = pts[tris]
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    cross = e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]
    flip = cross < 0
    tris[flip] = tris[flip][:, [0, 2, 1]]
    return torch.from_numpy(tris.astype(np.int32)).contiguous()


def _cell_table(cells: torch.Tensor, n_per: int, device) -> tuple[torch.Tensor, int]:
    """cells [C, 3 | 4] -> the device table [C, 4] int32 mmpde_mesh_quality reads
    (a triangle's fourth column repeats its third) and the arity; indices
    validated on the host (the kernels only clamp them)."""
    if cells.dim() != 2 or cells.shape[1] not in (3, 4) or cells.shape[0] < 1:
        raise ValueError("cells must be [C, 3] (triangles) or [C, 4] (quadrilaterals), C >= 1")
    arity = cells.shape[1]
    c = cells.detach().cpu().to(torch.int64)
    if int(c.min()) < 0 or int(c.max()) >= n_per:
        raise ValueError(f"cell indices must lie in [0, {n_per})")
    if arity == 3:
        c = torch.cat((c, c[:, 2:]), dim=1)
    return c.to(torch.int32).contiguous().to(device), arity


class MeshCells:
    """A validated cell table on the device (ops.mesh_quality builds one from a
    [C, 3 | 4] index tensor; build it once to reuse it across calls)."""

    def __init__(self, cells: torch.Tensor, n_per: int, device):
        self.table, self.arity = _cell_table(cells, n_per, device)
        self.n_per = n_per
        self.n_cells = self.table.shape[0]


def _monitor_lattice(n: int, batches: int, device):
    """The unit lattice repeated per trajectory [B n^2, 2] and the ones [B n^2]
    that mmpde_softmax_interp_grad takes as queries and grad_out."""
    from .dmm_train import unit_lattice

    return (unit_lattice(n, device).repeat(batches, 1).contiguous(),
            torch.ones((batches * n * n,), dtype=torch.float32, device=device))


def mesh_monitor(u: torch.Tensor, grid: torch.Tensor | None = None, *, out=None, scratch=None):
    """The monitor function of the reference's evaluate / evaluate_tri on the
    n x n unit lattice (flat 'xy' order, dmm_train.unit_lattice), per trajectory:
    alpha = sum |grad u| / (n - 1)^2, m = 1 + |grad u| / (0.01 alpha), rhs = sum m
    / (n - 1)^2 (dmm_utils.py:209-210, :1215-1217, :1248-1252).
    grid None: array data u [B, s, s], n = s, forward differences times s - 1.
    grid [N, 2]: point data u [B, N] on the fixed grid, n = floor(sqrt(N)), the
    gradient of the softmax smoother of u at the lattice points
    (mmpde_softmax_interp_grad, scale sqrt(N)).
    Returns (m [B, n, n], alpha [B], rhs [B]).  A constant field has alpha = 0 and
    gives NaN, as the reference does.  out: (m, alpha, rhs) to write into;
    scratch: point data's (queries [B n^2, 2], ones [B n^2], grad [B n^2, 2]).
    No synchronisation; with out and scratch given, no allocation (capturable)."""
    L.require_device(u, grid)
    u = L.f32c(u)
    if grid is None:
        if u.dim() != 3 or u.shape[1] != u.shape[2]:
            raise ValueError("array data must be [B, s, s]")
        B, n = u.shape[0], u.shape[1]
    else:
        grid = L.f32c(grid).reshape(-1, 2)
        if u.dim() != 2 or u.shape[1] != grid.shape[0]:
            raise ValueError("point data must be [B, N] on a grid [N, 2]")
        B, N = u.shape
        n = int(math.isqrt(N))
    if not 2 <= n <= MESH_QUALITY_MAX_N:
        raise ValueError(f"monitor lattice n = {n}: 2 <= n <= {MESH_QUALITY_MAX_N}")
    f32 = dict(dtype=torch.float32, device=u.device)
    if out is None:
        out = (torch.empty((B, n, n), **f32), torch.empty((B,), **f32), torch.empty((B,), **f32))
    m, alpha, rhs = out
    for t, numel in ((m, B * n * n), (alpha, B), (rhs, B)):
        L.require_device(t)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel:
            raise ValueError("out must be contiguous float32 (m [B, n, n], alpha [B], rhs [B])")
    st = L.stream(u.device)
    if grid is None:
        L.check(L.lib().mmpde_mesh_monitor_array(L.ptr(u), B, n, L.ptr(m), L.ptr(alpha), L.ptr(rhs), st),
                "mmpde_mesh_monitor_array")
        return m, alpha, rhs
    if scratch is None:
        qry, ones = _monitor_lattice(n, B, u.device)
        scratch = (qry, ones, torch.empty_like(qry))
    qry, ones, g = scratch
    if qry.shape != (B * n * n, 2) or ones.numel() != B * n * n or g.shape != qry.shape:
        raise ValueError("scratch must be (queries [B n^2, 2], ones [B n^2], grad [B n^2, 2])")
    L.check(L.lib().mmpde_softmax_interp_grad(L.ptr(grid), N, 1, L.ptr(u), B, L.ptr(qry), B * n * n,
                                              float(math.sqrt(N)), L.ptr(ones), L.ptr(g), st),
            "mmpde_softmax_interp_grad")
    L.check(L.lib().mmpde_mesh_monitor_grad(L.ptr(g), B, n, L.ptr(m), L.ptr(alpha), L.ptr(rhs), st),
            "mmpde_mesh_monitor_grad")
    return m, alpha, rhs


def mesh_quality(mesh: torch.Tensor, xi: torch.Tensor, cells, m: torch.Tensor, batches: int, *,
                 mg: bool | torch.Tensor = False, inverted_total: torch.Tensor | None = None, out=None,
                 workspace: torch.Tensor | None = None) -> MeshQuality:
    """The equidistribution statistics and the inverted cells of a moved mesh
    (mmpde_mesh_quality; reference dmm_utils.py:1162-1284, per trajectory and on
    the device).  mesh [batches * N, 2], xi [N, 2] the fixed grid, cells a
    [C, 4] (mesh_cells_lattice) or [C, 3] (mesh_cells_delaunay) index tensor or
    a MeshCells, m [batches, n, n] from mesh_monitor.  Per cell mg = m(centre) x
    area: a quadrilateral's area is the reference's product of the diagonals /
    2, its centre the vertices' mean; a triangle's area |cross| / 2, its centre
    the centroid; m(centre) the softmax smoother over all n^2 lattice points
    with scale n.  A cell is inverted when its signed area, oriented so that the
    fixed-grid cell is positive, is <= 0 or NaN.  A trajectory's results do not
    depend on the other trajectories.
    mg: True (or a [batches, C] tensor) to keep the per-cell values;
    inverted_total: a [batches] int32 counter, += inverted; out: (mean, std,
    range, inverted, area_ratio_min) to write into.  No synchronisation; with a
    MeshCells, out and workspace (or mg) given, no allocation (capturable)."""
    L.require_device(mesh, xi, m)
    mesh = L.f32c(mesh).reshape(-1, 2)
    xi = L.f32c(xi).reshape(-1, 2)
    m = L.f32c(m)
    N = xi.shape[0]
    if batches < 1 or mesh.shape[0] != batches * N or N == 0:
        raise ValueError("mesh rows must be batches copies of xi's")
    if m.dim() != 3 or m.shape[0] != batches or m.shape[1] != m.shape[2]:
        raise ValueError("m must be [batches, n, n]")
    n = m.shape[1]
    if not isinstance(cells, MeshCells):
        cells = MeshCells(cells, N, mesh.device)
    if cells.n_per != N or cells.table.device != mesh.device:
        raise ValueError("the cell table was built for another grid or device")
    C = cells.n_cells
    f32 = dict(dtype=torch.float32, device=mesh.device)
    i32 = dict(dtype=torch.int32, device=mesh.device)
    if out is None:
        out = (torch.empty((batches,), **f32), torch.empty((batches,), **f32), torch.empty((batches,), **f32),
               torch.empty((batches,), **i32), torch.empty((batches,), **f32))
    for t, dt in zip(out, (torch.float32,) * 3 + (torch.int32, torch.float32)):
        L.require_device(t)
        if t.dtype != dt or not t.is_contiguous() or t.numel() != batches:
            raise ValueError("out must be contiguous [batches] tensors (float32; inverted int32)")
    mean, std, rng, inverted, ratio = out
    if inverted_total is not None:
        L.require_device(inverted_total)
        if inverted_total.dtype != torch.int32 or not inverted_total.is_contiguous() \
                or inverted_total.numel() != batches:
            raise ValueError("inverted_total must be a contiguous int32 [batches] tensor")
    if mg is True:
        mg = torch.empty((batches, C), **f32)
    elif mg is False:
        mg = None
    if mg is not None:
        L.require_device(mg)
        if mg.dtype != torch.float32 or not mg.is_contiguous() or mg.numel() != batches * C:
            raise ValueError("mg must be a contiguous float32 [batches, C] tensor")
    else:
        nb = L.lib().mmpde_mesh_quality_workspace_bytes(batches, C)
        if workspace is None:
            workspace = torch.empty((nb // 4,), **f32)
        L.require_device(workspace)
        if workspace.numel() * workspace.element_size() < nb or workspace.data_ptr() % 16:
            raise ValueError(f"workspace must hold {nb} bytes, 16-B aligned")
    io = L.MeshQualityIO(L.ptr(mean), L.ptr(std), L.ptr(rng), L.ptr(inverted), L.ptr(ratio),
                         L.ptr(inverted_total), L.ptr(mg))
    L.check(L.lib().mmpde_mesh_quality(L.ptr(mesh), L.ptr(xi), batches, N, L.ptr(cells.table), C, cells.arity,
                                       L.ptr(m), n, ctypes.byref(io), L.ptr(workspace),
                                       L.stream(mesh.device)), "mmpde_mesh_quality")
    return MeshQuality(mean, std, rng, inverted, ratio, mg)


def reverse_adjacency(nbr: torch.Tensor, degree: torch.Tensor | None = None,
                      n_src: int | None = None, check: bool = True, slot_pos: bool = False):
    """Source-major view of a target-major table, for the source-side gradient of
    the edge stage (mmpde_gnn_edge_source_sum): rev_edge int64 = the live slot
    ids i*k+e grouped by source j (stable: target order within a source),
    rev_off int64 [n_src+1] = the group offsets (n_src defaults to the number of
    targets).  Device tables: mmpde_reverse_adjacency (no host round trip
    unless `check`, which reads back the count of sources outside [0, n_src)
    and raises on any; the engine's own kNN tables pass check=False;
    slot_pos=True adds the int32 [nt*k] position of every slot in that order,
    for mmpde_gnn_edge_backward_sorted).  Host tables (tests): the same lists
    from a stable argsort."""
    nt, k = nbr.shape
    n = nt if n_src is None else n_src
    if nbr.is_cuda:
        dev = nbr.device
        nbr = nbr.to(torch.int32).contiguous()
        deg = degree.to(torch.int32).contiguous() if degree is not None else None
        rev_off = torch.empty((n + 1,), dtype=torch.int64, device=dev)
        rev_edge = torch.empty((max(nt * k, 1),), dtype=torch.int64, device=dev)
        sb = L.lib().mmpde_reverse_adjacency_scratch_bytes(nt, k, n)
        scratch = torch.empty(((sb + 255) // 256 * 64,), dtype=torch.float32, device=dev).view(torch.uint8)
        bad = torch.empty((1,), dtype=torch.int32, device=dev)
        pos = torch.empty((max(nt * k, 1),), dtype=torch.int32, device=dev) if slot_pos else None
        L.check(L.lib().mmpde_reverse_adjacency(L.ptr(nbr), nt, k, L.ptr(deg), n, L.ptr(rev_off),
                                                L.ptr(rev_edge), L.ptr(pos), L.ptr(scratch), scratch.numel(),
                                                L.ptr(bad), L.stream(dev)), "mmpde_reverse_adjacency")
        if check and int(bad.item()):
            raise ValueError("neighbour table holds sources outside [0, n)")
        return (rev_off, rev_edge, pos) if slot_pos else (rev_off, rev_edge)
    if slot_pos:
        raise ValueError("slot_pos: device tables only")
    src = nbr.reshape(-1).long()
    slot = torch.arange(nt * k, device=nbr.device)
    if degree is not None:
        live = (torch.arange(k, device=nbr.device)[None, :] < degree[:, None].long()).reshape(-1)
        src, slot = src[live], slot[live]
    if src.numel() and (int(src.min()) < 0 or int(src.max()) >= n):
        raise ValueError("neighbour table holds sources outside [0, n)")
    order = torch.argsort(src, stable=True)
    rev_edge = slot[order].contiguous()
    rev_off = torch.zeros((n + 1,), dtype=torch.int64, device=nbr.device)
    rev_off[1:] = torch.cumsum(torch.bincount(src, minlength=n), 0)
    return rev_off, rev_edge


class GatherRows(torch.autograd.Function):
    """rows[idx] for a flat index list, whose backward is the fixed-order
    segmented sum mmpde_segment_sum over the reverse index lists (torch's
    scatter-add backward of a gather accumulates with atomics, in no fixed
    order).  rows [n, w] fp32, idx int [m] -> [m, w]."""

    @staticmethod
    def forward(ctx, rows, idx, check=False):
        L.require_device(rows, idx)
        ctx.n = rows.shape[0]
        ctx.idx = idx
        ctx.check = check      # idx from the engine's kNN kernels: in range
        return rows[idx.long()]

    @staticmethod
    def backward(ctx, g):
        g = L.f32c(g)
        n, w = ctx.n, g.shape[1]
        rev_off, rev_edge = reverse_adjacency(ctx.idx.reshape(-1, 1), n_src=n, check=ctx.check)
        out = torch.empty((n, w), dtype=torch.float32, device=g.device)
        L.check(L.lib().mmpde_segment_sum(L.ptr(g), w, L.ptr(rev_off), L.ptr(rev_edge), n,
                                          L.ptr(out), L.stream(g.device)), "mmpde_segment_sum")
        return out, None, None
