"""Autoregressive MM-PDE rollout engine (the benchmarked hot path).

One step is the forward of train_helper_2d.py:174-185 (test_timestep_losses),
composed directly on the C-ABI with every buffer preallocated:

    pred = interpolate_pred(itp, model_b(graph_moved), graph_moved, data) + model(graph_uni)

cylinder (DMM graph mode):
    mesh   = DMM.mesh(u, grid)                      # x = xi + d(phi)/d(xi)
    nbr_m  = knn_graph(mesh, k=35)                  # moved-mesh graph (every step)
    out_b  = model_b(u, (t, mesh), nbr_m)
    idx    = knn_query(src=mesh, qry=grid, k=30)    # sklearn replacement
    pred   = itp_interp(mesh, out_b, grid, idx, '2') + res_cut(u) + model(u, (t, grid), nbr_u)
Burgers (DMM array mode) additionally interpolates u onto the moved mesh first
(ItpNet mode '1'); the reference's interpolation of the *labels* onto the
moved mesh (data_creator_2d.py:208-209) feeds only graph.y, which no step
reads, so the rollout (which has no labels) does not compute it.

With connect_edge='radius' (graph_creator.e, data_creator_2d.py:195,226,257-258)
both graphs are radius graphs instead (radius_graph(mesh, r=gc.radius(), 32
neighbours): ragged tables nbr_u / deg_u, nbr_m / deg_m).

The fixed-grid GNN runs on a side stream beside the moving-mesh chain.

Rollout: the prediction becomes the next step's input (u <- pred, t index + 1),
which the reference itself never does (it only evaluates one-step losses,
SURVEY.md §3); ``step`` is that one-step forward.  What depends only on the
fixed grid and the weights is built once at construction: the fixed-grid graph
(``nbr_u``) and the DMM head's grid side (trunk(xi), Q, J; ``dmm_cache``).
Changing weights after construction needs a new engine.

A DMM fed its own predictions can fold the mesh (det(dx/dxi) <= 0 at a node),
after which the moved-mesh graph and the interpolation are built on tangled
points.  ``mesh_check = True`` makes the DMM stage report that
(``mesh_report()``) without changing the step.  ``mesh_guard = delta`` corrects
it: a trajectory whose move would leave an eigenvalue of dx/dxi below delta at
some node is moved only as far as keeps it at delta (the reference's
relaxation x = alpha x + (1 - alpha) xi with alpha chosen per trajectory,
``DMM.mesh_guarded``); trajectories that do not fold keep their mesh bit for
bit.  The damping is uniform over a trajectory, and phi is not smoothed.

Both judge the continuous map at the nodes.  ``mesh_quality = True`` adds the
discrete view of the mesh the step used (after the guard / relaxation), per
trajectory and on a side stream, without changing the step: the reference's
equidistribution measure (evaluate / evaluate_tri, dmm_utils.py:1162-1284:
monitor function at each moved cell's centre times the cell's area; mean, std
and max - min over the cells) and the number of inverted cells (signed area
against the same cell of the fixed grid), ``mesh_quality_report()``.  The cells
are the lattice quadrilaterals (Burgers) or the fixed grid's Delaunay triangles
(cylinder); the monitor lattice is the unit square, as in the reference.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from . import _lib as L
from . import ops
from .moved_search import MovedMeshSearch


# default of MMPDERollout.priorities (set_priorities)
PRIORITIES = False


class MMPDERollout:
    def __init__(self, kind, model, model_b, itp, dmm, graph_creator, batches: int, device,
                 moving_mesh: bool = True):
        self.kind = kind
        self.model, self.model_b, self.itp, self.dmm = model, model_b, itp, dmm
        self.gc = graph_creator
        self.B = batches
        self.device = torch.device(device)
        self.moving_mesh = moving_mesh
        self.trace_hook = None   # callable() -> _lib.GnnTrace | None, one per GNN forward
        # run the fixed-grid model beside the moving-mesh chain (False: one stream,
        # e.g. to time single kernels without a concurrent neighbour)
        self.overlap = True
        # stream priorities (set_priorities): the moving-mesh chain and the
        # kNN-30 query at high priority, the fixed-grid model at low priority
        self.priorities = PRIORITIES
        # the fold monitor: the DMM step also computes det(dx/dxi) = det(I + Hess phi)
        # at every node and counts the nodes where it is not positive (the moved
        # mesh has folded there; mesh_report()).  The mesh, and so the step, keep
        # their bits.  Settable before the first step and before enable_graph.
        self.mesh_check = False
        gc = graph_creator
        # the fold guard (DMM.mesh_guarded): mesh_alpha is the alpha of the
        # reference's relaxation x = alpha x + (1 - alpha) xi (1: the full move);
        # mesh_guard None, or the floor delta in (0, 1) of the smallest
        # eigenvalue of dx/dxi, which a trajectory's move is cut back to keep
        # (0.1 is DMM.mesh_guarded's default, not a measured optimum).  Read from
        # the graph creator; settable like mesh_check.  mesh_guard implies the
        # Hessian path of mesh_check.
        self.mesh_guard = getattr(gc, "mesh_guard", None)
        self.mesh_alpha = getattr(gc, "mesh_alpha", 1.0)
        # the mesh-quality stage (the mesh_quality property): its cell table,
        # buffers and stream are built on the first such step (_ensure_mesh_quality)
        self._mesh_quality = False
        self.mesh_q = None
        self.grid = gc.uniform_grid(self.device).contiguous()           # [N, 2]
        self.N = N = self.grid.shape[0]
        self.n = n = batches * N
        self.grid_rep = self.grid.repeat(batches, 1).contiguous()        # [B*N, 2]
        # connect_edge (reference data_creator_2d.py:257-260): 'knn' graphs of
        # gc.n neighbours, or 'radius' graphs (gc.radius(), at most 32
        # neighbours): ragged [n, 33] tables with in-degrees, for the fixed grid
        # (built once) and the moved mesh (every step)
        if gc.e not in ("knn", "radius"):
            raise ValueError(f"connect_edge {gc.e!r}: knn | radius")
        self.radius_graph = gc.e == "radius"
        self.nbr_u, self.deg_u = gc.fixed_graph(self.grid, batches)
        self.deg_m = None
        self.search = None
        self.t = gc.time_grid()
        f32 = dict(dtype=torch.float32, device=self.device)
        self.out_u = torch.empty((n, 1), **f32)
        self.out_b = torch.empty((n, 1), **f32)
        self.ws_gnn = torch.empty((L.lib().mmpde_gnn_workspace_bytes(n) // 4,), **f32)
        if moving_mesh:
            hd = dmm.device_params()[1]
            self.ws_dmm = torch.empty(
                (L.lib().mmpde_dmm_workspace_bytes(batches, N, hd.latent, hd.hidden) // 4,), **f32)
            self.mesh = torch.empty((n, 2), **f32)
            if kind == "burgers":
                s = int(round(N ** 0.5))
                self.s = s
                self.xi = gc.xi_grid_xy(s, s, self.device)
            else:
                self.xi = self.grid
            for mode in ("1", "2") if kind == "burgers" else ("2",):
                itp.packed(mode)
            # the DMM head's grid side depends on xi and the weights only
            self.dmm_cache = dmm.head_cache(self.xi, workspace=self.ws_dmm)
            # the fold monitor (mesh_check): its table K = dJ/dxi and its buffers
            # are built on the first checked step, a default engine holds none
            self.hess_cache = None
            self.mesh_hess = self.mesh_det = self.mesh_detmin = None
            self.mesh_folds = self.mesh_folds_total = None
            # the fold guard's [B] extras (mesh_guard / mesh_alpha), likewise
            self.mesh_alpha_b = self.mesh_lam = self.mesh_guarded_total = None
            self.mesh_det_after = self.mesh_detmin_after = self.mesh_folds_after = None
            # the per-step neighbour searches on the moved mesh: their tables,
            # bins, policy and the choice among them (moved_search.py)
            self.search = MovedMeshSearch(kind, gc, self.xi, self.grid, self.grid_rep, batches)
            # the fixed-grid model depends on u only: it runs on a side stream,
            # with its own workspace, beside the moving-mesh chain
            self.ws_gnn_u = torch.empty_like(self.ws_gnn)
            # the kNN-30 query onto the fixed grid and res_cut need only the mesh
            # and u: a second side stream runs them beside the moved-mesh graph
            # and model_b
            self.set_priorities(self.priorities)

        # hipGraph replay of the step (enable_graph): static input / time /
        # output buffers, one graph per stage, replayed on the stage's stream
        self._graphs = None
        self._g_u = self._g_t = self._g_out = None

    def set_priorities(self, on: bool) -> None:
        """on: the moving-mesh chain (DMM, kNN graph, model_b) runs on a
        high-priority stream and the kNN-30 query / res_cut on another, the
        fixed-grid model(u) on a low-priority one, so that the chain's small
        kernels take the SIMDs the fixed-grid GNN's kernels free before that
        GNN's next launch does (the chain gates model_b).  off: default
        priorities, the chain on the caller's stream.  Which stream runs a
        kernel does not change its result."""
        if not self.moving_mesh:
            return
        self.priorities = bool(on)
        hi, lo = (-8, 8) if on else (0, 0)   # torch clamps to the device's range
        self.side = torch.cuda.Stream(self.device, priority=lo)
        self.side2 = torch.cuda.Stream(self.device, priority=hi)
        self.main_hi = torch.cuda.Stream(self.device, priority=hi) if on else None
        self._graphs = None

    def _trace(self):
        return self.trace_hook() if self.trace_hook is not None else None

    def _nodes(self, u, xy, nbr, step_idx, deg=None):
        """The GNN's node inputs with (x, y) positions and one t for every node
        (mmpde_gnn_scales.pos_xy): no (t, x, y) array is filled per step.  Graph
        capture passes the device slot holding t."""
        if isinstance(step_idx, torch.Tensor):
            return _Nodes(u, xy, nbr, self.N, t_slot=step_idx, deg=deg)
        return _Nodes(u, xy, nbr, self.N, t=float(self.t[step_idx]), deg=deg)

    # ------------------------------------------------------------ the stages
    # The moving-mesh step is five stages on three streams (every kernel is one
    # of the C-ABI's; each stage runs on the caller's current stream):
    #   side   model(u) on the fixed grid                       needs u
    #   main1  DMM mesh, per-trajectory displacement record     needs u
    #          (knn_binned: the moved mesh's cell bins instead; a binned
    #          radius graph: the bins as well)
    #   side2  kNN-30 query onto the fixed grid, res_cut(u)     needs main1
    #   main2  moved-mesh kNN-35 or radius graph (Burgers: u onto the moved
    #          mesh), model_b
    #   final  interpolation + res_cut + model(u) in one kernel  needs all
    def _st_side(self, u_flat, step_idx):
        nodes_u = self._nodes(u_flat, self.grid_rep, self.nbr_u, step_idx, self.deg_u)
        self.model(nodes_u, out=self.out_u, workspace=self.ws_gnn_u, trace=self._trace())

    def _ensure_mesh_check(self):
        """The monitor's table and buffers (once): K = dJ/dxi of the fixed grid,
        a workspace with room for the det scratch, Hess phi, det and the counts."""
        if self.hess_cache is not None:
            return
        hd = self.dmm.device_params()[1]
        f32 = dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.hess_cache = self.dmm.hess_cache(self.xi, workspace=self.ws_dmm)
        nb = L.lib().mmpde_dmm_hess_workspace_bytes(self.B, self.N, hd.latent, hd.hidden)
        self.ws_dmm_hess = torch.empty((nb // 4,), **f32)
        self.mesh_hess = torch.empty((self.n, 3), **f32)
        self.mesh_det = torch.empty((self.n,), **f32)
        self.mesh_detmin = torch.empty((self.B,), **f32)
        self.mesh_folds = torch.zeros((self.B,), **i32)
        self.mesh_folds_total = torch.zeros((self.B,), **i32)

    def _ensure_mesh_guard(self):
        """The guard's buffers (once): the monitor's, when the guard is on, and
        the per-trajectory step, eigenvalue, counts and the det after the guard."""
        if self.mesh_guard is not None:
            self._ensure_mesh_check()
        if self.mesh_alpha_b is not None and (self.mesh_guard is None or self.mesh_lam is not None):
            return
        f32 = dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        if self.mesh_alpha_b is None:
            self.mesh_alpha_b = torch.ones((self.B,), **f32)
            self.mesh_guarded_total = torch.zeros((self.B,), **i32)
        if self.mesh_guard is not None:
            self.mesh_lam = torch.zeros((self.B,), **f32)
            self.mesh_det_after = torch.empty((self.n,), **f32)
            self.mesh_detmin_after = torch.empty((self.B,), **f32)
            self.mesh_folds_after = torch.zeros((self.B,), **i32)

    # mesh_quality: settable before the first step and before enable_graph, like
    # mesh_check.  The step then also runs the monitor and cell-quality kernels on
    # the final mesh (ops.mesh_monitor, ops.mesh_quality) on a side stream; they
    # read u and self.mesh and write their own buffers only.
    @property
    def mesh_quality(self) -> bool:
        return self._mesh_quality

    @mesh_quality.setter
    def mesh_quality(self, on) -> None:
        on = bool(on)
        if on:
            if not self.moving_mesh:
                raise ValueError("mesh_quality needs a moving mesh")
            pde = self.gc.pde
            if self.kind == "burgers" and (float(pde.Lx) != 1.0 or float(pde.Ly) != 1.0):
                raise ValueError(f"mesh_quality: the monitor lattice is the unit square (dmm_utils.py:1238-1240), "
                                 f"the domain is {pde.Lx} x {pde.Ly}")
        if on != self._mesh_quality:
            self._graphs = None   # the captured stages are those of the other setting
        self._mesh_quality = on

    def _ensure_mesh_quality(self):
        """The quality stage's cell table, buffers and stream (once): the lattice
        quadrilaterals (Burgers) or the fixed grid's Delaunay triangles (cylinder,
        scipy on the host), the monitor field and the per-trajectory outputs."""
        if self.mesh_q is not None:
            return
        B, N = self.B, self.N
        f32 = dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        q = SimpleNamespace(steps=0)
        if self.kind == "burgers":
            q.cells = ops.MeshCells(ops.mesh_cells_lattice(self.s), N, self.device)
            q.n = self.s
            q.scratch = None
        else:
            q.cells = ops.MeshCells(ops.mesh_cells_delaunay(self.grid), N, self.device)
            q.n = math.isqrt(N)
            qry, ones = ops._monitor_lattice(q.n, B, self.device)
            q.scratch = (qry, ones, torch.empty_like(qry))
        q.m = torch.empty((B, q.n, q.n), **f32)
        q.alpha, q.rhs = torch.empty((B,), **f32), torch.empty((B,), **f32)
        q.mean, q.std, q.range = (torch.empty((B,), **f32) for _ in range(3))
        q.inverted = torch.zeros((B,), **i32)
        q.area_ratio_min = torch.empty((B,), **f32)
        q.inverted_total = torch.zeros((B,), **i32)
        q.ws = torch.empty((L.lib().mmpde_mesh_quality_workspace_bytes(B, q.cells.n_cells) // 4,), **f32)
        q.stream = torch.cuda.Stream(self.device)
        self.mesh_q = q

    def _st_quality(self, u):
        q = self.mesh_q
        if self.kind == "burgers":
            ops.mesh_monitor(u.reshape(self.B, self.s, self.s), out=(q.m, q.alpha, q.rhs))
        else:
            ops.mesh_monitor(u.reshape(self.B, self.N), self.grid, out=(q.m, q.alpha, q.rhs), scratch=q.scratch)
        ops.mesh_quality(self.mesh, self.xi, q.cells, q.m, self.B, inverted_total=q.inverted_total,
                         out=(q.mean, q.std, q.range, q.inverted, q.area_ratio_min), workspace=q.ws)

    def _st_main1(self, u):
        B = self.B
        if self.mesh_guard is not None:
            # the Hessian path, then the relaxation with the step chosen per
            # trajectory, before anything reads the mesh
            self._ensure_mesh_guard()
            self.dmm.mesh_guarded(u, self.xi, floor=self.mesh_guard, alpha=self.mesh_alpha, out=self.mesh,
                                  hess_out=self.mesh_hess, det_out=self.mesh_det_after,
                                  workspace=self.ws_dmm_hess, head_cache=self.dmm_cache,
                                  hess_cache=self.hess_cache, folds_total=self.mesh_folds_total,
                                  guarded_total=self.mesh_guarded_total, alpha_out=self.mesh_alpha_b,
                                  lam_out=self.mesh_lam, detmin_out=self.mesh_detmin_after,
                                  folds_out=self.mesh_folds_after, det_before_out=self.mesh_det,
                                  detmin_before_out=self.mesh_detmin, folds_before_out=self.mesh_folds)
        elif self.mesh_check:
            # the same mesh bits, with Hess phi, det and the fold counts beside them
            self._ensure_mesh_check()
            self.dmm.mesh_hess(u, self.xi, out=self.mesh, hess_out=self.mesh_hess, det_out=self.mesh_det,
                               workspace=self.ws_dmm_hess, head_cache=self.dmm_cache,
                               hess_cache=self.hess_cache, folds_total=self.mesh_folds_total,
                               detmin_out=self.mesh_detmin, folds_out=self.mesh_folds)
        else:
            self.dmm.mesh(u, self.xi, out=self.mesh, workspace=self.ws_dmm, head_cache=self.dmm_cache)
        if self.mesh_guard is None and self.mesh_alpha != 1.0:
            # the plain relaxation (the monitor, when on, reports the full move)
            self._ensure_mesh_guard()
            ops.mesh_relax(self.mesh, self.xi, batches=B, alpha=self.mesh_alpha, alpha_out=self.mesh_alpha_b)
        self.search.begin_step(self.mesh)

    def _st_side2(self, u):
        B, N = self.B, self.N
        self.idx2 = self.search.knn("query", self.mesh)
        if self.kind == "burgers":
            self._res = self.itp.res_cut(u.reshape(B, 1, self.s, self.s)).reshape(-1)
        else:
            self._res = self.itp.res_cut(u.reshape(B, N)).reshape(-1)

    def _st_main2(self, u_flat, step_idx):
        mesh = self.mesh
        self.nbr_m, self.deg_m = self.search.graph(mesh)
        if self.kind == "burgers":
            self.idx1 = self.search.knn("query1", mesh)
            u_m = ops.itp_interp(self.grid_rep, u_flat, mesh, self.idx1, self.B, self.itp.packed("1"))
        else:
            u_m = u_flat
        nodes_m = self._nodes(u_m, mesh, self.nbr_m, step_idx, self.deg_m)
        self.model_b(nodes_m, out=self.out_b, workspace=self.ws_gnn, trace=self._trace())

    def _st_final(self):
        # interpolate_pred(...) + model(graph_uniform) (train_helper_2d.py:178-185):
        # (interp + res_cut) + out_u in the interpolation kernel's epilogue
        return ops.itp_interp(self.mesh, self.out_b, self.grid_rep, self.idx2, self.B, self.itp.packed("2"),
                              addend=self._res, addend2=self.out_u.reshape(-1))

    # ------------------------------------------------------------ hipGraph
    def enable_graph(self, u_like: torch.Tensor, serial: bool = False) -> None:
        """Capture the step for replay: one hipGraph per stage (see the stage
        list above), each captured on the stream it replays on, with its own
        memory pool (two stages that replay concurrently never share scratch).
        `graph_step` replays them with the eager step's cross-stream waits, so
        the side streams' stages still run beside the main chain (a single
        graph of the whole step replays its branches one after the other).
        The step must have run eagerly once before (weight images packed, DMM
        head cache built).  Inputs are copied into static buffers; the time
        value is read from a one-element device slot, so the graphs serve every
        step index.  serial: every stage captured and replayed on one stream (the
        measurement baseline of the side streams' overlap)."""
        if self.trace_hook is not None:
            raise ValueError("graph replay records no per-kernel events; clear trace_hook")
        if self.moving_mesh and self.mesh_check:
            self._ensure_mesh_check()   # allocations and the K table stay out of the capture
        if self.moving_mesh and (self.mesh_guard is not None or self.mesh_alpha != 1.0):
            self._ensure_mesh_guard()
        if self.moving_mesh and self._mesh_quality:
            self._ensure_mesh_quality()   # the cell table, buffers and stream likewise
        self._g_u = torch.empty_like(u_like).contiguous()
        self._g_u.copy_(u_like)
        self._g_t = torch.zeros((1,), dtype=torch.float32, device=self.device)
        u, t = self._g_u, self._g_t
        u_flat = u.reshape(-1)
        torch.cuda.synchronize(self.device)
        cap = torch.cuda.Stream(self.device)
        graphs = {}

        def capture(name, stream, fn):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                out = fn()
            torch.cuda.synchronize(self.device)
            graphs[name] = g
            return out

        if not self.moving_mesh:
            self._g_out = capture("main", cap, lambda: self.model(
                self._nodes(u_flat, self.grid_rep, self.nbr_u, t, self.deg_u), out=self.out_u,
                workspace=self.ws_gnn).reshape(u.shape))
        else:
            capture("side", cap if serial else self.side, lambda: self._st_side(u_flat, t))
            capture("main1", cap, lambda: self._st_main1(u))
            if self._mesh_quality:
                capture("quality", cap if serial else self.mesh_q.stream, lambda: self._st_quality(u))
            capture("side2", cap if serial else self.side2, lambda: self._st_side2(u))
            capture("main2", cap, lambda: self._st_main2(u_flat, t))
            self._g_out = capture("final", cap, self._st_final).reshape(u.shape)
        self._graphs = graphs
        self._graph_serial = serial

    def graph_step(self, u: torch.Tensor, step_idx: int) -> torch.Tensor:
        """`step` by replaying the captured graphs.  Returns the static output
        buffer (overwritten by the next replay; clone to keep it)."""
        if self._graphs is None:
            raise RuntimeError("enable_graph() first")
        if u.data_ptr() != self._g_u.data_ptr():
            self._g_u.copy_(u.reshape(self._g_u.shape))
        self._g_t.fill_(float(self.t[step_idx]))
        g = self._graphs
        if not self.moving_mesh:
            g["main"].replay()
            return self._g_out
        if self._graph_serial:
            for name in ("side", "main1", "quality", "side2", "main2", "final"):
                if name in g:
                    g[name].replay()
            if "quality" in g:
                self.mesh_q.steps += 1
            return self._g_out
        cur = torch.cuda.current_stream(self.device)
        self.side.wait_stream(cur)
        with torch.cuda.stream(self.side):
            g["side"].replay()
        g["main1"].replay()
        if "quality" in g:   # beside everything that follows: it only reads u and the mesh
            sq = self.mesh_q.stream
            sq.wait_stream(cur)
            with torch.cuda.stream(sq):
                g["quality"].replay()
            self.mesh_q.steps += 1
        self.side2.wait_stream(cur)
        with torch.cuda.stream(self.side2):
            g["side2"].replay()
        g["main2"].replay()
        cur.wait_stream(self.side)
        cur.wait_stream(self.side2)
        if "quality" in g:
            cur.wait_stream(sq)   # the next step's DMM stage overwrites the mesh
        g["final"].replay()
        return self._g_out

    def step(self, u: torch.Tensor, step_idx) -> torch.Tensor:
        """u: [B, N] (cylinder) or [B, s, s] (Burgers) on the device -> pred, same shape.
        step_idx: time index (int), or during graph capture the device slot holding t."""
        u = u.contiguous()
        u_flat = u.reshape(-1)
        if not self.moving_mesh:
            return self.model(self._nodes(u_flat, self.grid_rep, self.nbr_u, step_idx, self.deg_u), out=self.out_u,
                              workspace=self.ws_gnn, trace=self._trace()).reshape(u.shape)
        cur = torch.cuda.current_stream(self.device)
        side = self.side if self.overlap else cur
        main = self.main_hi if self.overlap and self.main_hi is not None else cur
        if main is not cur:   # the chain first: its first kernel is queued before model(u)'s
            main.wait_stream(cur)
            u.record_stream(main)
        side.wait_stream(cur)
        if main is not cur:
            with torch.cuda.stream(main):
                self._st_main1(u)
        with torch.cuda.stream(side):
            u.record_stream(side)
            self._st_side(u_flat, step_idx)
        if main is cur:
            self._st_main1(u)
        if self._mesh_quality:
            # the mesh is final: the quality stage beside everything that follows
            self._ensure_mesh_quality()
            sq = self.mesh_q.stream if self.overlap else main
            if sq is not main:
                sq.wait_stream(main)
            with torch.cuda.stream(sq):
                u.record_stream(sq)
                self._st_quality(u)
            self.mesh_q.steps += 1
        side2 = self.side2 if self.overlap else cur
        side2.wait_stream(main)
        with torch.cuda.stream(side2):
            u.record_stream(side2)
            self._st_side2(u)
            self.idx2.record_stream(cur)
            self._res.record_stream(cur)
        with torch.cuda.stream(main):
            self._st_main2(u_flat, step_idx)
        if main is not cur:
            cur.wait_stream(main)
        cur.wait_stream(side)
        cur.wait_stream(side2)
        if self._mesh_quality and sq is not cur:
            cur.wait_stream(sq)   # the next step's DMM stage overwrites the mesh
        return self._st_final().reshape(u.shape)

    # The search object's flags and tables under the engine's names: knn_binned
    # and radius_binned are settable before the first step and before enable_graph.
    knn_binned = property(lambda self: self.search.knn_binned,
                          lambda self, on: setattr(self.search, "knn_binned", on))
    radius_binned = property(lambda self: self.search.radius_binned,
                             lambda self, on: setattr(self.search, "radius_binned", on))
    knn_cand = property(lambda self: self.search.cand["graph"])
    knn_cand_q = property(lambda self: self.search.cand["query"])

    def knn_table_share(self):
        """(graph, query[, burgers mode-'1' query]): the share of the last step's
        moved-mesh kNN lookups the candidate tables answered (the rest went to
        the full search); None for a search the policy ran without the table
        that step (ops.KnnTablePolicy).  Diagnostics: synchronises the device."""
        return self.search.table_share() if self.moving_mesh else None

    def knn_modes(self):
        """Per neighbour search of the step: 'binned' (knn_binned), else 'table'
        or 'full' (ops.KnnTablePolicy); a radius graph's role is 'radius-binned'
        or 'radius' (radius_binned).  moved_search.choose."""
        return self.search.modes() if self.moving_mesh else {}

    def knn_query_ties(self) -> int:
        """Queries of the kNN-30 searches (reference data_creator_2d.py:75-76)
        since construction whose sorted fp64 distances held an exact tie inside
        the first 30 or at rank 30: the only inputs on which sklearn's order (its
        KD-tree traversal) may differ from the engine's (distance, index) order,
        i.e. where parity with the reference is unpinned.  Synchronises."""
        return self.search.query_ties() if self.moving_mesh else 0

    def mesh_report(self):
        """The fold monitor's record (mesh_check = True): per trajectory, the
        last step's number of folded nodes (det(dx/dxi) <= 0 or NaN: the moved
        mesh is not a mesh there) and its smallest det, and the folded nodes
        summed over every checked step since construction.  The monitor only
        reports; the step does not change.  None before the first checked step.
        With the fold guard on (mesh_guard) these describe the full move, before
        the guard, and the record adds per trajectory the step taken (alpha),
        the smallest eigenvalue of Hess phi (lam_min), the folded nodes and the
        smallest det of the relaxed mesh (folds_after, detmin_after) and the
        number of steps since construction on which the guard cut the move
        (guarded_total).  Synchronises."""
        if not self.moving_mesh or self.hess_cache is None:
            return None
        torch.cuda.synchronize(self.device)
        rep = {"folds": self.mesh_folds.tolist(), "detmin": self.mesh_detmin.tolist(),
               "folds_total": self.mesh_folds_total.tolist()}
        if self.mesh_guard is not None and self.mesh_lam is not None:
            rep.update(alpha=self.mesh_alpha_b.tolist(), lam_min=self.mesh_lam.tolist(),
                       folds_after=self.mesh_folds_after.tolist(),
                       detmin_after=self.mesh_detmin_after.tolist(),
                       guarded_total=self.mesh_guarded_total.tolist())
        return rep

    def mesh_quality_report(self):
        """The quality stage's record of the last step (mesh_quality = True), per
        trajectory: mean, std and range (max - min) over the cells of the monitor
        function at the moved cell's centre times the cell's area (the
        reference's evaluate / evaluate_tri figures, for the mesh the step used),
        the monitor's rhs and alpha, the number of inverted cells (signed area
        <= 0 or NaN against the same cell of the fixed grid), the smallest signed
        moved area / fixed area, and the inverted cells summed over every such
        step since construction.  A constant u has alpha = 0 and NaN statistics,
        as in the reference.  None before the first such step.  Synchronises."""
        q = self.mesh_q
        if q is None or q.steps == 0:
            return None
        torch.cuda.synchronize(self.device)
        return {k: getattr(q, k).tolist() for k in ("mean", "std", "range", "rhs", "alpha", "inverted",
                                                    "area_ratio_min", "inverted_total")}

    def rollout(self, u0: torch.Tensor, start_step: int, n_steps: int):
        """Feed each prediction back as the next input; returns the final state."""
        u = u0
        for s in range(start_step, start_step + n_steps):
            u = self.step(u, s)
        return u


class _Nodes:
    """The graph fields the solver reads (x, pos, nbr, seg_n = nodes per
    trajectory); pos [n, 2] = (x, y) with t (host float) or t_slot (device
    scalar) for every node, or the reference's [n, 3] (t, x, y)."""
    __slots__ = ("x", "pos", "nbr", "deg", "edge_index", "seg_n", "t", "t_slot")

    def __init__(self, x, pos, nbr, seg_n=None, t=None, t_slot=None, deg=None):
        self.x = x.reshape(-1, 1)
        self.pos = pos
        self.nbr = nbr
        self.deg = deg   # in-degrees of a ragged table (radius graph), else None
        self.edge_index = None
        self.seg_n = seg_n
        self.t = t
        self.t_slot = t_slot
