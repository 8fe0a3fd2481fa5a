"""GraphCreator_FS_2D on the HIP kernels (drop-in for reference
data_creator_2d.py:18-305).

Same constructor and method signatures as the reference; every method that
the MM-PDE step calls (create_graph, interpolate, interpolate_pred,
moving_mesh, moving_mesh_tri) runs on device kernels:

* kNN graphs: mmpde_knn_graph (torch_cluster.knn_graph replacement).  The graph
  of the *fixed* grid is a pure function of the grid and B, so it is built once
  and cached (the reference rebuilds it every call, train_helper_2d.py:177);
  the moved-mesh graph is rebuilt every call, as in the reference.
* interpolation: mmpde_knn_query (sklearn replacement, no host round trip) +
  mmpde_itp_interp (ItpNet weights and weighted sum in one kernel).
* moving mesh: DMM.mesh (analytic d(phi)/d(xi), no autograd graph).

Only the torch plumbing (reshapes, the (t, x, y) position tensor) uses torch
ops; there is no CPU or eager compute fallback.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import ops
from .graph import Data


class GraphCreator_FS_2D(nn.Module):  # noqa: N801 - reference name
    def __init__(self, pde, neighbors: int = 2, connect_edge: str = "knn",
                 time_window: int = 10, t_resolution: int = 100):
        super().__init__()
        self.pde = pde
        self.n = neighbors
        self.e = connect_edge
        self.tw = time_window
        self.t_res = t_resolution
        assert isinstance(self.n, int)
        assert isinstance(self.tw, int)
        self._fixed_graph_cache = {}
        # "full" or "binned" (ops.knn_graph_nbr / ops.knn_query): how create_graph's
        # moved-mesh graph and the kNN-30 queries of interpolate / interpolate_pred
        # search; the same tables either way
        self.knn_method = "full"
        # "scan" or "binned" (ops.radius_graph_nbr): how create_graph's moved-mesh
        # radius graph searches; the same tables either way
        self.radius_method = "scan"
        # the relaxation that ends the reference's moving_mesh[_tri], x = alpha x +
        # (1 - alpha) xi (data_creator_2d.py:109-111,133-135, alpha = 1 hard-coded
        # there): mesh_alpha is that alpha; mesh_guard None, or a floor in (0, 1)
        # for the smallest eigenvalue of dx/dxi: a trajectory whose move would
        # fold is then moved only as far as keeps it (DMM.mesh_guarded; eval mode).
        # At the defaults moving_mesh[_tri] is DMM.mesh, the same bits.
        self.mesh_alpha = 1.0
        self.mesh_guard = None

    # ------------------------------------------------------------------ grids
    def _is_array(self):
        return len(self.pde.grid_size) == 3

    def time_grid(self):
        """t = linspace(tmin, tmax, nt) computed on the host in fp32 exactly as
        data_creator_2d.py:185,220."""
        return torch.linspace(self.pde.tmin, self.pde.tmax, self.pde.grid_size[0])

    def uniform_grid(self, device, nx=None, ny=None):
        """Array mode: meshgrid(linspace, linspace) 'ij' flattened (data_creator_2d.py:187-194);
        cylinder: pde.ori_grid.  Returns [N, 2] fp32 on `device` -- the same tensor
        for the same grid parameters (cached), so that the fixed-grid graph cache
        below hits by identity without comparing contents on the host."""
        if self._is_array():
            nx = self.pde.grid_size[1] if nx is None else nx
            ny = self.pde.grid_size[2] if ny is None else ny
            key = ("ij", str(device), nx, ny, float(self.pde.Lx), float(self.pde.Ly))
        else:
            og = self.pde.ori_grid
            key = ("ori", str(device), id(og), og._version, tuple(og.shape))
        cache = self.__dict__.setdefault("_uniform_grid_cache", {})
        hit = cache.get(key)
        if hit is not None and (key[0] == "ij" or hit[0] is self.pde.ori_grid):
            return hit[1]
        if self._is_array():
            x = torch.linspace(0, self.pde.Lx, nx)
            y = torch.linspace(0, self.pde.Ly, ny)
            gx, gy = torch.meshgrid(x, y, indexing="ij")
            g = torch.stack((gx, gy), 2).float().reshape(-1, 2).to(device)
        else:
            g = self.pde.ori_grid.float().reshape(-1, 2).to(device)
            if g.data_ptr() == self.pde.ori_grid.data_ptr():
                g = g.clone()   # own storage: a caller's in-place edit of ori_grid misses the cache
        # the pde's grid object is kept with the entry, so its id cannot be reused
        cache[key] = (self.pde.ori_grid if key[0] == "ori" else None, g)
        return g

    def xi_grid_xy(self, n_grid_x, n_grid_y, device):
        """The DMM xi grid of moving_mesh (data_creator_2d.py:94-96): numpy
        linspace in float64, np.meshgrid 'xy' order, then cast to fp32."""
        gx = np.linspace(0, self.pde.Lx, n_grid_x)
        gy = np.linspace(0, self.pde.Ly, n_grid_y)
        g = torch.tensor(np.array(np.meshgrid(gx, gy)), dtype=torch.float)
        return g.reshape(2, -1).permute(1, 0).contiguous().to(device)

    def radius(self) -> float:
        """connect_edge='radius' cut-off, data_creator_2d.py:187-195 / :221-226:
        neighbors * |(dx, dy)| + 1e-4 of the uniform linspace grid (cylinder:
        nx = ny = int(sqrt(N))), computed in fp32 as the reference does."""
        if self._is_array():
            _, nx, ny = self.pde.grid_size
        else:
            nx = ny = int(np.sqrt(self.pde.grid_size[1]))
        x = torch.linspace(0, self.pde.Lx, nx)
        y = torch.linspace(0, self.pde.Ly, ny)
        dx, dy = x[1] - x[0], y[1] - y[0]
        return float(self.n * torch.sqrt(dx ** 2 + dy ** 2) + 0.0001)

    def fixed_graph_nbr(self, grid: torch.Tensor, batches: int) -> torch.Tensor:
        """kNN-k table of `batches` copies of the fixed grid (cached).  Keyed on
        the grid tensor's identity and version: the cache holds the tensor, so
        its storage cannot be freed and reused by another grid while the entry
        lives, and an in-place change bumps the version (no host copy, no
        device sync per call; create_graph passes the cached uniform_grid)."""
        key = (grid.data_ptr(), grid._version, tuple(grid.shape), str(grid.device), batches, self.n)
        hit = self._fixed_graph_cache.get(key)
        if hit is None or hit[0] is not grid:
            hit = (grid, ops.knn_graph_nbr(grid.repeat(batches, 1), batches, self.n))
            self._fixed_graph_cache = {key: hit}
        return hit[1]

    def fixed_graph(self, grid: torch.Tensor, batches: int):
        """(nbr, deg) of `batches` copies of the fixed grid for this creator's
        connect_edge: the kNN-k table of fixed_graph_nbr with deg None, or the
        radius graph's ragged [n, 33] table and in-degrees (radius(), 32
        neighbours; cached like fixed_graph_nbr)."""
        if self.e == "knn":
            return self.fixed_graph_nbr(grid, batches), None
        if self.e != "radius":
            raise ValueError(f"connect_edge {self.e!r}: knn | radius")
        r = self.radius()
        key = (grid.data_ptr(), grid._version, tuple(grid.shape), str(grid.device), batches, r)
        cache = self.__dict__.setdefault("_fixed_radius_cache", {})
        hit = cache.get(key)
        if hit is None or hit[0] is not grid:
            hit = (grid, ops.radius_graph_nbr(grid.repeat(batches, 1), batches, r, 32))
            self._fixed_radius_cache = {key: hit}
        return hit[1]

    # ------------------------------------------------------------------ data
    def create_data(self, datapoints, steps):
        """data_creator_2d.py:139-154: input window u[step-tw:step] and target
        u[step:step+tw] of every trajectory (stacked once, not cat'ed in a loop)."""
        data = torch.stack([dp[s - self.tw:s] for dp, s in zip(datapoints, steps)])
        labels = torch.stack([dp[s:s + self.tw] for dp, s in zip(datapoints, steps)])
        return data, labels

    # ------------------------------------------------------------------ mesh
    def _mesh(self, mesh_model, u, xi):
        """DMM.mesh, or with mesh_alpha / mesh_guard set the relaxed / guarded mesh."""
        if self.mesh_guard is None and self.mesh_alpha == 1.0:
            return mesh_model.mesh(u, xi)
        return mesh_model.mesh_guarded(u, xi, floor=self.mesh_guard, alpha=self.mesh_alpha)[0]

    def moving_mesh(self, u, mesh_model, n_grid_x, n_grid_y):
        """data_creator_2d.py:88-113 (Burgers, DMM array mode).  u [B, nx, ny].
        Returns (x1, x2), each [B*nx*ny, 1]."""
        mx, my = self.pde.movingmesh_grid_size[-2], self.pde.movingmesh_grid_size[-1]
        if mx != n_grid_x or my != n_grid_y:   # data_creator_2d.py:102-103
            u = ops.resample_bilinear(u, mx, my)
        xi = self.xi_grid_xy(n_grid_x, n_grid_y, u.device)
        mesh = self._mesh(mesh_model, u, xi)
        return mesh[:, 0:1], mesh[:, 1:2]

    def moving_mesh_tri(self, u, mesh_model, grid_x, grid_y):
        """data_creator_2d.py:115-137 (cylinder, DMM graph mode).  grid_x/grid_y are
        the fixed grid repeated per trajectory ([B, N]); all trajectories share it."""
        xi = torch.stack((grid_x[0], grid_y[0]), -1)
        mesh = self._mesh(mesh_model, u, xi)
        return mesh[:, 0:1], mesh[:, 1:2]

    # ------------------------------------------------------------------ interpolation
    def interpolate(self, itp_model, u, init_x, init_y, x, y, mode):
        """data_creator_2d.py:46-85: per trajectory, the 30 nearest source points
        (fp64 distance order) of every query, ItpNet weights, weighted sum of
        the source values.  Returns [nu * n_query]."""
        nu = u.shape[0]
        src = torch.cat((init_x, init_y), -1).reshape(-1, 2)
        qry = torch.cat((x, y), -1).reshape(-1, 2)
        idx = ops.knn_query(src, qry, nu, 30, method=self.knn_method)
        if itp_model.training:
            return self._interpolate_autograd(itp_model, u, src, qry, idx, nu, mode)
        return ops.itp_interp(src, u.reshape(-1), qry, idx, nu, itp_model.packed(mode))

    @staticmethod
    def _interpolate_autograd(itp_model, u, src, qry, idx, nu, mode, addend=None):
        """Training path of data_creator_2d.py:70-83: the HIP kNN-30 indices, then
        the neighbour gather, ItpNet weights and weighted sum as device torch ops,
        differentiable in the ItpNet parameters and in the values `u`."""
        ns, nq = src.shape[0] // nu, qry.shape[0] // nu
        gidx = idx.long().reshape(nu, nq * 30)
        pts = src.reshape(nu, ns, 2)
        nb = torch.gather(pts, 1, gidx[..., None].expand(nu, nq * 30, 2)).reshape(nu, nq, 30, 2)
        flat = (gidx + ns * torch.arange(nu, device=gidx.device)[:, None]).reshape(-1)
        lab = ops.GatherRows.apply(u.reshape(nu * ns, 1).float(), flat).reshape(nu, nq, 30)
        w = itp_model.weights(nb, qry.reshape(nu, nq, 1, 2), mode)
        out = torch.sum(w * lab, dim=-1).reshape(-1)
        return out if addend is None else out + addend

    # ------------------------------------------------------------------ graph
    def _graph(self, u_nodes, mesh, t_nodes, labels_nodes, nbr, B, n, deg=None):
        pos = torch.cat((t_nodes[:, None], mesh), 1).contiguous()
        batch = torch.arange(B, device=mesh.device).repeat_interleave(n)
        g = Data(x=u_nodes, edge_index=None)
        g.y = labels_nodes
        g.pos = pos
        g.batch = batch
        g.nbr = nbr
        g.nbr_checked = True   # from the engine's kNN / radius kernels: sources in range
        g.deg = deg
        g.seg_n = n
        return g

    def create_graph(self, itp_model, data, labels, steps, device, mesh_model=None):
        """data_creator_2d.py:157-267 (connect_edge 'knn' or 'radius')."""
        if self.e not in ("knn", "radius"):
            raise ValueError(f"connect_edge {self.e!r}: knn | radius")
        data = data.to(device)
        labels = labels.to(device)
        B = data.shape[0]
        t = self.time_grid()
        if self._is_array():
            nt, nx, ny = self.pde.grid_size
            n = nx * ny
            grid = self.uniform_grid(device, nx, ny)
            if mesh_model is not None:
                ori_nx, ori_ny = data.shape[-2], data.shape[-1]
                mm_nx, mm_ny = self.pde.movingmesh_grid_size[-2:]
                u_mm = data.reshape(-1, ori_nx, ori_ny)[:, ::int(ori_nx / mm_nx),
                                                        ::int(ori_ny / mm_ny)]
                mx, my = self.moving_mesh(u_mm.contiguous(), mesh_model, nx, ny)
                mesh = torch.cat((mx, my), -1)
                ori = self.uniform_grid(device, ori_nx, ori_ny).repeat(B, 1)
                data = self.interpolate(itp_model, data.reshape(-1, ori_nx, ori_ny),
                                        ori[:, 0:1], ori[:, 1:2], mx, my, "1"
                                        ).reshape(-1, self.tw, nx, ny)
                labels = self.interpolate(itp_model, labels.reshape(-1, ori_nx, ori_ny),
                                          ori[:, 0:1], ori[:, 1:2], mx, my, "1"
                                          ).reshape(-1, self.tw, nx, ny)
            else:
                mesh = grid.repeat(B, 1)
        else:
            n = self.pde.ori_grid_size[1]
            grid = self.uniform_grid(device)
            if mesh_model is not None:
                gx = grid[:, 0][None].expand(B, n)
                gy = grid[:, 1][None].expand(B, n)
                mx, my = self.moving_mesh_tri(data.reshape(-1, n), mesh_model, gx, gy)
                mesh = torch.cat((mx, my), -1)
            else:
                mesh = grid.repeat(B, 1)
        # node tensors (data_creator_2d.py:242-254): u [B*n, tw], labels, t[step]
        u_nodes = data.reshape(B, self.tw, n).permute(0, 2, 1).reshape(B * n, self.tw)
        y_nodes = labels.reshape(B, self.tw, n).permute(0, 2, 1).reshape(B * n, self.tw)
        # steps[b] for the B trajectories only: training_itp passes 128 x batch_size
        # steps for a batch of batch_size (train_helper_2d.py:44,47; the reference
        # loops b over the data, data_creator_2d.py:243-254)
        # a pageable host->device copy waits for the stream to drain: stage the B
        # times in pinned memory and copy asynchronously (no sync per graph)
        t_b = t[list(steps)[:B]]
        if torch.device(device).type == "cuda":
            t_b = t_b.pin_memory().to(device, non_blocking=True)
        t_nodes = t_b.to(device).repeat_interleave(n)
        deg = None
        if self.e == "radius":   # torch_cluster default max_num_neighbors = 32
            nbr, deg = ops.radius_graph_nbr(mesh.contiguous(), B, self.radius(), 32,
                                            method=self.radius_method)
        elif mesh_model is None:
            nbr = self.fixed_graph_nbr(grid, B)
        else:
            nbr = ops.knn_graph_nbr(mesh, B, self.n, method=self.knn_method)
        return self._graph(u_nodes.contiguous(), mesh.contiguous(), t_nodes, y_nodes, nbr, B, n,
                           deg)

    def interpolate_pred(self, itp_model, pred, graph, data, device):
        """data_creator_2d.py:270-305: moved-mesh prediction -> fixed grid (kNN-30 of
        each fixed point among the moved points + ItpNet mode '2') plus
        res_cut(data)."""
        data = data.to(device)
        if self._is_array():
            ori_nx, ori_ny = self.pde.ori_grid_size[1], self.pde.ori_grid_size[2]
            nx, ny = self.pde.grid_size[1], self.pde.grid_size[2]
            nu = pred.shape[0] // (nx * ny)
            qry = self.uniform_grid(device, ori_nx, ori_ny).repeat(nu, 1)
            res = itp_model.res_cut(data.reshape(-1, 1, ori_nx, ori_ny)).reshape(-1)
            n_src = nx * ny
        else:
            n = self.pde.ori_grid_size[1]
            nu = pred.shape[0] // n
            qry = self.uniform_grid(device).repeat(nu, 1)
            res = itp_model.res_cut(data.reshape(-1, n)).reshape(-1)
            n_src = n
        src = graph.pos[:, 1:3].contiguous()
        idx = ops.knn_query(src, qry, nu, 30, method=self.knn_method)
        if itp_model.training:
            out = self._interpolate_autograd(itp_model, pred, src, qry, idx, nu, "2",
                                             addend=res)
        else:
            out = ops.itp_interp(src, pred.reshape(-1), qry, idx, nu, itp_model.packed("2"),
                                 addend=res)
        assert src.shape[0] == nu * n_src
        return out.reshape(-1, 1)
