"""DMM mesh mover on the HIP kernels (drop-in for reference mesh/dmm_model.py).

Module tree and ``state_dict`` keys match the reference (including the unused
``DenseNet.fc0``, which also keeps the default-init RNG stream aligned), so
the reference checkpoints ``cy_checkpoint`` / ``burgers_checkpoint``
(``model_state_dict``) load unchanged.  Unlike the reference, nothing is
hard-wired to ``device="cuda"`` at construction (dmm_model.py:27-28).

The MM-PDE step never needs phi itself, only the moved mesh
x = xi + d(phi)/d(xi) that GraphCreator_FS_2D.moving_mesh[_tri] obtains with
two autograd.grad calls (data_creator_2d.py:106-107,130-131).  ``DMM.mesh``
returns exactly that through an analytic vector-Jacobian product
(mmpde_dmm_mesh_graph / mmpde_dmm_mesh_array; derivation in dmm.hip).
``DMM.mesh_hess`` returns the same mesh together with the mesh map's Jacobian
dx/dxi = I + Hess phi, its determinant and per-trajectory fold counts
(mmpde_dmm_mesh_*_hess: the reference's phixx, phixy, phiyy of
mesh/dmm_utils.py:507-552, in eval mode and without autograd).
``DMM.forward`` (phi, and rf=True's second output) runs the branch and the
head on the same kernels (mmpde_dmm_branch_*, mmpde_dmm_phi); ``DenseNet`` /
``ConvNet`` forwards run on the skinny-linear and conv kernels.

In ``train()`` mode (DMM training, reference mesh/dmm_utils.py:391-1095,
SURVEY.md §8(f) row 4: ``mmpde_amd.dmm_train``) every forward is the
reference's computation as differentiable device torch ops -- BatchNorm on
batch statistics, twice differentiable in the grid (the Monge-Ampere loss
takes d2 phi / d xi2 through autograd) -- with the fixed grid's kNN-35 graph
from the HIP kernel and the mean aggregation over its fixed in-degree.
``DMM.mesh_fields`` is the moved mesh of K fields, each a batch of its own to
the BatchNorms, in either mode and without autograd (DMM training's per-epoch
evaluation, K fields per call).
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from . import _lib as L
from .gnn_2d import BatchNorm
from . import ops
from .ops import knn_graph_nbr




class DenseNet(nn.Module):
    """Reference dmm_model.py:9-45 (normalize=False): Linear layers with tanh on
    all but the last.  ``fc0`` is unused by the reference forward but is a
    parameter there, so it is kept for state_dict / RNG parity."""

    def __init__(self, layers, width=32, normalize=False):
        super().__init__()
        if normalize:
            raise NotImplementedError("DenseNet(normalize=True) is not used by MM-PDE")
        self.n_layers = len(layers) - 1
        assert self.n_layers >= 1
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(layers[:-1], layers[1:]))
        self.normalize = normalize
        self.width = width
        self.fc0 = nn.Linear(4, width)

    def forward(self, x):
        """dmm_model.py:31-45 (normalize=False): (out, x) with x the last hidden
        activation (the input of the last Linear)."""
        if self.training:   # differentiable torch ops (DMM training)
            for i, l in enumerate(self.layers):
                if i != self.n_layers - 1:
                    x = torch.tanh(l(x))
                else:
                    out = l(x)
            return out, x
        for i, l in enumerate(self.layers):
            if i != self.n_layers - 1:
                x = ops.linear_rows(x, l.weight, l.bias, L.ACT_TANH)
            else:
                out = ops.linear_rows(x, l.weight, l.bias, L.ACT_NONE)
        return out, x


class ConvNet(nn.Module):
    """Reference dmm_model.py:48-81 (layers == 7, the only configuration it builds).
    eval(): the conv and skinny-linear kernels.  train(): differentiable torch
    ops in ``forward``; ``forward_train_hip`` is the same function on the
    training kernels (DMM.hip_branch_train selects it)."""

    def __init__(self, s, layers):
        super().__init__()
        if layers != 7:
            raise NotImplementedError("ConvNet is only defined for layers == 7")
        self.layers = nn.ModuleList([
            nn.Conv2d(1, 8, 5, stride=2, padding=2), nn.Conv2d(8, 16, 5, padding=2),
            nn.Conv2d(16, 8, 5, padding=2), nn.Conv2d(8, 1, 5, stride=2, padding=2)])
        self.fc1 = None
        self.fc2 = nn.Linear(int(((s + 1) / 2 + 1) / 2) ** 2, 1024)
        self.fc3 = nn.Linear(1024, 512)
        self.s = s

    def forward(self, x):
        """dmm_model.py:65-81: x [B, 1, s, s] -> [B, 512]."""
        c = self.layers
        if self.training:   # differentiable torch ops (DMM training)
            x1 = torch.tanh(c[0](x))
            x3 = torch.tanh(x1 + c[2](torch.tanh(c[1](x1))))
            f = torch.flatten(torch.tanh(c[3](x3)), 1)
            return self.fc3(torch.tanh(self.fc2(f)))
        x1 = ops.conv2d(x, c[0].weight, c[0].bias, 2, 2, L.ACT_TANH)
        x2 = ops.conv2d(x1, c[1].weight, c[1].bias, 1, 2, L.ACT_TANH)
        x3 = ops.conv2d(x2, c[2].weight, c[2].bias, 1, 2, L.ACT_TANH, residual=x1)
        x4 = ops.conv2d(x3, c[3].weight, c[3].bias, 2, 2, L.ACT_TANH)
        f = torch.flatten(x4, 1)
        f = ops.linear_rows(f, self.fc2.weight, self.fc2.bias, L.ACT_TANH)
        return ops.linear_rows(f, self.fc3.weight, self.fc3.bias, L.ACT_NONE)

    def forward_train_hip(self, u):
        """The train()-mode forward on kernels, u [B, s, s] -> [B, 512]: the four
        convolutions, forward and backward, on ops.ConvNetTrain (one workgroup
        per field, s <= ops.CONVNET_TRAIN_MAX_S, else NotImplementedError), fc2 /
        fc3 on the few-row skinny kernels (ops.FewRowsMlp; above 4096 fields on
        ops.linear_train, fc2's K zero-padded to a multiple of 8 as in
        ItpNet.weights).  First order in the twelve tensors, none in u; no
        library convolution or GEMM, the same bits on every run."""
        s = u.shape[-1]
        if u.dim() != 3 or u.shape[1] != s or s != self.s:
            raise ValueError(f"ConvNet.forward_train_hip: u must be [B, {self.s}, {self.s}]")
        if s > ops.CONVNET_TRAIN_MAX_S:
            raise NotImplementedError(f"hip_branch_train: the array branch kernels take s <= {ops.CONVNET_TRAIN_MAX_S} "
                                      f"(got {s})")
        L.require_device(u)
        c = self.layers
        f = ops.ConvNetTrain.apply(u, c[0].weight, c[0].bias, c[1].weight, c[1].bias, c[2].weight, c[2].bias,
                                   c[3].weight, c[3].bias)
        if f.shape[1] != self.fc2.in_features:
            raise ValueError(f"ConvNet: fc2 takes {self.fc2.in_features} inputs, the convolutions give {f.shape[1]}")
        if u.shape[0] <= 4096:
            return ops.FewRowsMlp.apply(f, self.fc2.weight, self.fc2.bias, self.fc3.weight, self.fc3.bias)
        padk = -f.shape[1] % 8
        if padk:   # x and W alike: the extra products are exact zeros
            f = torch.nn.functional.pad(f, (0, padk)).contiguous()
            h = ops.LinearRows.apply(f, torch.nn.functional.pad(self.fc2.weight, (0, padk)), self.fc2.bias)
        else:
            h = ops.linear_train(f, self.fc2)
        return ops.linear_train(torch.tanh(h), self.fc3)


class GNN_Layer_FS_2D(nn.Module):  # noqa: N801 - reference name
    """The DMM branch's tanh GNN layer (reference dmm_model.py:94-142)."""

    def __init__(self, in_features, out_features, hidden_features):
        super().__init__()
        self.message_net_1 = nn.Sequential(nn.Linear(2 * in_features + 3, hidden_features),
                                           nn.Tanh())
        self.message_net_2 = nn.Sequential(nn.Linear(hidden_features, out_features), nn.Tanh())
        self.update_net_1 = nn.Sequential(nn.Linear(in_features + hidden_features,
                                                    hidden_features), nn.Tanh())
        self.update_net_2 = nn.Sequential(nn.Linear(hidden_features, out_features), nn.Tanh())
        self.norm = BatchNorm(hidden_features)

    def forward(self, x, u, pos_x, pos_y, nbr):
        """Training-mode layer (dmm_model.py:126-142) as differentiable torch ops:
        tanh messages cat(x_i, x_j, u_i - u_j, dx, dy) over the target-major
        neighbour table nbr [n, k] (every row k sources: PyG's mean is the mean
        over them), update x + U2 tanh(U1 cat(x, m)), BatchNorm.  The eval
        forward runs inside mmpde_dmm_mesh_graph."""
        n, k = nbr.shape
        j = nbr.reshape(-1).long()
        i = torch.arange(n, device=x.device).repeat_interleave(k)
        m = torch.cat((x[i], x[j], u[i] - u[j], pos_x[i] - pos_x[j], pos_y[i] - pos_y[j]), dim=-1)
        m = self.message_net_2(self.message_net_1(m)).reshape(n, k, -1).mean(1)
        return self.norm(x + self.update_net_2(self.update_net_1(torch.cat((x, m), dim=-1))))


class _HeadJet(torch.autograd.Function):
    """DMM.jet's kernel pair: mmpde_dmm_jet forward, mmpde_dmm_jet_grad backward.
    Differentiable, first order, in branch and the head's tensors; the grid rows
    are data.  Only the inputs are saved: the backward recomputes the head."""

    @staticmethod
    def forward(ctx, branch, grid, second_order, dims, t0_w, t0_b, t1_w, t1_b, o0_w, o0_b, o1_w, o1_b):
        head = [L.f32c(t) for t in (t0_w, t0_b, t1_w, t1_b, o0_w, o0_b, o1_w)]
        hd = _head_struct(head, dims)
        out = ops.dmm_jet(branch, grid, hd, o1_b, second_order)
        ctx.save_for_backward(branch, grid, *head)
        ctx.dims = dims
        ctx.has_bias = o1_b is not None
        ctx.set_materialize_grads(False)   # an unused output's cotangent stays None: a null pointer, zero
        res = tuple(t.reshape(-1, 1) for t in out if t is not None)
        return res

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *cots):
        branch, grid, *head = ctx.saved_tensors
        hd = _head_struct(head, ctx.dims)
        g = ops.dmm_jet_grad(branch, grid, hd, cots)
        # phi's bias reaches the loss through phi alone: no gradient (not a zero one) when phi is unused, as on
        # the autograd route, so that an optimiser with weight decay leaves it alone
        return (g.branch, None, None, None, g.t0_w, g.t0_b, g.t1_w, g.t1_b, g.o0_w, g.o0_b, g.o1_w,
                g.o1_b if ctx.has_bias and cots[0] is not None else None)


def _head_struct(fh, dims):
    """_lib.DmmHead over the seven float32 head tensors fh (kept alive by the caller); dims = (th, L, L')."""
    th, latent, hidden = dims
    return L.DmmHead(fh[0].data_ptr(), fh[1].data_ptr(), fh[2].data_ptr(), fh[3].data_ptr(), th, latent,
                     fh[4].data_ptr(), fh[5].data_ptr(), fh[6].data_ptr(), hidden)


class DMM(nn.Module):
    """Reference dmm_model.py:145-219."""

    def __init__(self, branch_layer, trunk_layer, grid=None, out_layer=None, s=None,
                 mode="array"):
        super().__init__()
        self.mode = mode
        self.ori_grid = grid
        if mode == "array":
            self.branch = ConvNet(s, branch_layer)
            self.trunk = DenseNet(trunk_layer)
            self.out_nn = DenseNet(out_layer)
        elif mode == "graph":
            self.hidden_features = branch_layer[0]
            self.hidden_layer = branch_layer[1]
            self.gnn_layers = nn.ModuleList(
                GNN_Layer_FS_2D(in_features=self.hidden_features,
                                hidden_features=self.hidden_features,
                                out_features=self.hidden_features)
                for _ in range(self.hidden_layer))
            self.embedding_mlp = nn.Sequential(
                nn.Linear(3, self.hidden_features), nn.BatchNorm1d(self.hidden_features),
                nn.Tanh(), nn.Linear(self.hidden_features, self.hidden_features),
                nn.BatchNorm1d(self.hidden_features))
            self.decoding_mlp = DenseNet([self.hidden_features, 128, 1])
            self.output_mlp = nn.Sequential(
                nn.Linear(grid.shape[0], 512), nn.Tanh(), nn.Linear(512, 256), nn.Tanh(),
                nn.Linear(256, trunk_layer[-1]))
            self.trunk = DenseNet(trunk_layer)
            self.out_nn = DenseNet(out_layer)
        else:
            raise ValueError(mode)
        self._pack_key = None
        self._pack = None
        self._grid_cache = {}
        self._rev_cache = {}
        # train() mode, either branch: run _branch_train on the HIP kernels (a plain attribute, not in state_dict)
        self.hip_branch_train = False

    def forward(self, u, grid, rf=False):
        """dmm_model.py:185-219: phi = out_nn(cat(branch(u), trunk(grid))), the
        branch of trajectory b repeated over its grid.shape[0] / B rows of grid.
        u: graph [B, N] (values on self.ori_grid), array [B, s, s]; grid [B*m, 2].
        Returns phi [B*m, 1], or (phi, second_out [B*m, L'], ones [B*m*L', 1])
        with rf=True."""
        L.require_device(u, grid)
        if self.training:
            return self._forward_train(u, grid, rf)
        bp, hd = self.device_params()
        u = L.f32c(u)
        grid = L.f32c(grid).reshape(-1, 2)
        B, ng = u.shape[0], grid.shape[0]
        if ng % B:
            raise ValueError("grid rows must be a multiple of the batch size")
        lib = L.lib()
        st = L.stream(u.device)
        branch = self.branch_features(u)
        nb = lib.mmpde_dmm_phi_workspace_bytes(B, ng, hd.latent, hd.hidden, hd.th)
        ws2 = torch.empty((nb // 4,), dtype=torch.float32, device=u.device)
        phi = torch.empty((ng, 1), dtype=torch.float32, device=u.device)
        second = (torch.empty((ng, hd.hidden), dtype=torch.float32, device=u.device)
                  if rf else None)
        ob = self.out_nn.layers[1].bias
        L.check(lib.mmpde_dmm_phi(L.ptr(branch), B, L.ptr(grid), ng, ctypes.byref(hd),
                                  L.ptr(L.f32c(ob)) if ob is not None else None, L.ptr(ws2),
                                  L.ptr(phi), L.ptr(second), st), "mmpde_dmm_phi")
        if not rf:
            return phi
        return phi, second, torch.ones_like(second).reshape(-1, 1)

    def _forward_train(self, u, grid, rf=False):
        """dmm_model.py:185-219 in train() mode: differentiable in the weights and
        in `grid` (to any order), BatchNorm on batch statistics."""
        B = u.shape[0]
        if grid.shape[0] % B:
            raise ValueError("grid rows must be a multiple of the batch size")
        branch = self._branch_train(u)
        rep = grid.shape[0] // B
        branch = branch[:, None, :].expand(B, rep, branch.shape[-1]).reshape(-1, branch.shape[-1])
        trunk, _ = self.trunk(grid)
        out, second = self.out_nn(torch.cat((branch, trunk.reshape(-1, branch.shape[-1])), dim=-1))
        if not rf:
            return out
        return out, second, torch.ones_like(second).reshape(-1, 1)

    def _branch_train(self, u, nbr=None):
        """The branch of _forward_train [B, L] (dmm_model.py:188,197-210 in train()
        mode): the graph branch's BatchNorms use batch statistics and advance
        their running statistics once per call.  nbr: graph mode only, an [N, k]
        int32 local neighbour table used instead of the kNN-35 table of
        self.ori_grid.  With hip_branch_train the branch runs forward and
        backward on the HIP kernels: the graph branch on _branch_train_hip, the
        array branch on ConvNet.forward_train_hip (s <=
        ops.CONVNET_TRAIN_MAX_S, else NotImplementedError).  Flag off: the torch
        ops, bit for bit."""
        B = u.shape[0]
        if self.mode == "array":
            if nbr is not None:
                raise ValueError("nbr is a graph-mode argument")
            if self.hip_branch_train:
                return self.branch.forward_train_hip(u)
            return self.branch(u.unsqueeze(1))
        else:
            og = torch.as_tensor(self.ori_grid).to(u.device, torch.float32).reshape(-1, 2)
            N = og.shape[0]
            og = og.contiguous()
            nbr = self.grid_nbr(og) if nbr is None else self._local_nbr(nbr, N, u.device)   # [N, 35] local
            if self.hip_branch_train:
                return self._branch_train_hip(u, og, nbr)
            gnbr = (nbr[None].long() + N * torch.arange(B, device=u.device)[:, None, None])
            gnbr = gnbr.reshape(B * N, -1)
            x = u.reshape(-1, 1)
            pos = og[None].expand(B, N, 2).reshape(-1, 2)
            pos_x, pos_y = pos[:, :1], pos[:, 1:]
            h = self.embedding_mlp(torch.cat((x, pos_x, pos_y), -1))
            for layer in self.gnn_layers:
                h = layer(h, x, pos_x, pos_y, gnbr)
            h, _ = self.decoding_mlp(h)
            return self.output_mlp(h.reshape(B, -1))

    def _branch_train_hip(self, u, og, nbr, segments=1):
        """_branch_train's graph branch on kernels, forward and backward: the
        embedding on the row kernels (ops.linear_train, ops.batch_norm_rows),
        every GNN layer's update on ops.DmmGnnLayerTrain with its residual and
        BatchNorm on ops.batch_norm_rows, the decoder on ops.DmmDecodeTrain,
        output_mlp on the few-row skinny kernels (ops.FewRowsMlp; above 4096
        trajectories on ops.linear_train).  The same modules' BatchNorms advance
        in the same order as on the torch route; no per-edge tensor and no
        library GEMM.  segments = B (mesh_fields; forward only, under
        torch.no_grad()): every BatchNorm takes each trajectory's N rows as a batch
        of its own and advances B times, in trajectory order, as B calls of one
        trajectory each would (ops.batch_norm_rows(segments=)); nothing else in
        the sequence mixes trajectories."""
        if self.hidden_features != 4:
            raise NotImplementedError("hip_branch_train: the graph branch kernels take hidden_features == 4 only "
                                      f"(got {self.hidden_features})")
        L.require_device(u)
        B, N = u.shape[0], og.shape[0]
        rev = self._nbr_rev(nbr)
        uf = u.float().reshape(-1)
        e = self.embedding_mlp
        x3 = torch.cat((uf[:, None], og.repeat(B, 1)), -1)
        h = ops.batch_norm_rows(e[1], ops.linear_train(x3, e[0]), segments=segments)
        h = ops.batch_norm_rows(e[4], ops.linear_train(torch.tanh(h), e[3]), segments=segments)
        for g in self.gnn_layers:
            upd = ops.DmmGnnLayerTrain.apply(
                h, uf, og, nbr, rev, g.message_net_1[0].weight, g.message_net_1[0].bias, g.message_net_2[0].weight,
                g.message_net_2[0].bias, g.update_net_1[0].weight, g.update_net_1[0].bias, g.update_net_2[0].weight,
                g.update_net_2[0].bias)
            h = ops.batch_norm_rows(g.norm.module, upd, res=h, segments=segments)
        d = self.decoding_mlp.layers
        dec = ops.DmmDecodeTrain.apply(h, d[0].weight, d[0].bias, d[1].weight, d[1].bias)
        o = self.output_mlp
        x = dec.reshape(B, N)
        if B <= 4096:     # a few rows of K = N: the split-K skinny kernels (the row GEMMs take the shape, slowly)
            return ops.FewRowsMlp.apply(x, o[0].weight, o[0].bias, o[2].weight, o[2].bias, o[4].weight, o[4].bias)
        x = torch.tanh(ops.linear_train(x, o[0]))
        x = torch.tanh(ops.linear_train(x, o[2]))
        return ops.linear_train(x, o[4])

    def _nbr_rev(self, nbr: torch.Tensor):
        """ops.reverse_adjacency of a local table, built (and range-checked) once per table."""
        key = (nbr.data_ptr(), nbr._version, tuple(nbr.shape), str(nbr.device))
        hit = self._rev_cache.get(key)
        if hit is None:
            hit = (nbr, ops.reverse_adjacency(nbr))   # holds the table: its storage cannot be reused meanwhile
            self._rev_cache = {key: hit}
        return hit[1]

    # ----------------------------------------------------------------- packing
    def _check(self):
        if self.training:
            raise NotImplementedError("the HIP head is eval-mode: call .eval() (train() "
                                      "mode runs DMM.forward as torch ops)")
        tl = self.trunk.layers
        ol = self.out_nn.layers
        if len(tl) != 2 or len(ol) != 2 or ol[1].out_features != 1:
            raise NotImplementedError("trunk DenseNet[2, th, L] / out_nn DenseNet[2L, L', 1] only")
        if self.mode == "graph" and (self.hidden_features != 4 or self.hidden_layer > 3):
            raise NotImplementedError("graph branch: hidden 4, <= 3 layers (cy checkpoint)")

    def _tensors(self):
        tl, ol = self.trunk.layers, self.out_nn.layers
        head = [tl[0].weight, tl[0].bias, tl[1].weight, tl[1].bias, ol[0].weight, ol[0].bias,
                ol[1].weight]
        if self.mode == "graph":
            e = self.embedding_mlp
            br = [e[0].weight, e[0].bias, e[1].weight, e[1].bias, e[1].running_mean,
                  e[1].running_var, e[3].weight, e[3].bias, e[4].weight, e[4].bias,
                  e[4].running_mean, e[4].running_var]
            for g in self.gnn_layers:
                br += [g.message_net_1[0].weight, g.message_net_1[0].bias,
                       g.message_net_2[0].weight, g.message_net_2[0].bias,
                       g.update_net_1[0].weight, g.update_net_1[0].bias,
                       g.update_net_2[0].weight, g.update_net_2[0].bias,
                       g.norm.module.weight, g.norm.module.bias, g.norm.module.running_mean,
                       g.norm.module.running_var]
            d, o = self.decoding_mlp.layers, self.output_mlp
            br += [d[0].weight, d[0].bias, d[1].weight, d[1].bias, o[0].weight, o[0].bias,
                   o[2].weight, o[2].bias, o[4].weight, o[4].bias]
        else:
            b = self.branch
            br = [b.layers[0].weight, b.layers[0].bias, b.layers[1].weight, b.layers[1].bias,
                  b.layers[2].weight, b.layers[2].bias, b.layers[3].weight, b.layers[3].bias,
                  b.fc2.weight, b.fc2.bias, b.fc3.weight, b.fc3.bias]
        return head, br

    def device_params(self):
        self._check()
        head, br = self._tensors()
        key = tuple((t.data_ptr(), t._version) for t in head + br)
        if key == self._pack_key:
            return self._pack[0]
        fh = [L.f32c(t) for t in head]
        fb = [L.f32c(t) for t in br]
        tl, ol = self.trunk.layers, self.out_nn.layers
        hd = L.DmmHead(fh[0].data_ptr(), fh[1].data_ptr(), fh[2].data_ptr(), fh[3].data_ptr(),
                       tl[0].out_features, tl[1].out_features, fh[4].data_ptr(),
                       fh[5].data_ptr(), fh[6].data_ptr(), ol[0].out_features)
        if self.mode == "graph":
            p = [t.data_ptr() for t in fb]
            nl = self.hidden_layer
            per = [p[12 + 12 * i: 24 + 12 * i] for i in range(nl)]
            arrs = []
            for fld in range(12):
                vals = [per[i][fld] if i < nl else None for i in range(3)]
                arrs.append(L._P3(*vals))
            tail = p[12 + 12 * nl:]
            bn_eps = float(self.embedding_mlp[1].eps)
            bp = L.DmmGraphBranch(*p[:12], *arrs, nl, *tail, bn_eps)
        else:
            bp = L.DmmArrayBranch(*[t.data_ptr() for t in fb], self.branch.s)
        self._pack = ((bp, hd), fh + fb)
        self._pack_key = key
        return self._pack[0]

    def _head_params(self):
        """The head alone as a _lib.DmmHead (with the float32 tensors it points
        to), in either mode: the head has no BatchNorm, so it is the same
        function in train() and eval()."""
        tl, ol = self.trunk.layers, self.out_nn.layers
        if len(tl) != 2 or len(ol) != 2 or ol[1].out_features != 1:
            raise NotImplementedError("trunk DenseNet[2, th, L] / out_nn DenseNet[2L, L', 1] only")
        fh = [L.f32c(t) for t in self._tensors()[0]]
        hd = L.DmmHead(fh[0].data_ptr(), fh[1].data_ptr(), fh[2].data_ptr(), fh[3].data_ptr(),
                       tl[0].out_features, tl[1].out_features, fh[4].data_ptr(),
                       fh[5].data_ptr(), fh[6].data_ptr(), ol[0].out_features)
        return hd, fh

    def rf_features(self, u: torch.Tensor, grid: torch.Tensor, second_order: bool = True,
                    branch: torch.Tensor | None = None):
        """The random features of forward(u, grid, rf=True) -- second_out, the tanh
        layer under out_nn's last Linear -- and their derivatives in grid, per
        feature (ops.dmm_rf_features): what the reference's random-feature phase
        builds with 6 L' autograd.grad calls (mesh/dmm_utils.py:883-905).
        u, grid as for forward; branch: the branch output [B, L] to use instead
        of computing it from u.  In eval() the branch is branch_features(u); in
        train() it comes from the torch ops of the train()-mode forward, so the
        graph branch's BatchNorms use batch statistics and advance their running
        statistics once per call, as the reference's model(u, x_, rf=True) does.
        Nothing is differentiable here.  Deliberate difference: one table s_xy
        for the reference's so_xy and so_yx (they are equal).
        Returns ops.RfFeatures(s, s_x, s_y, s_xx, s_xy, s_yy), [rows, L'] each,
        the last three None with second_order=False."""
        L.require_device(u, grid)
        with torch.no_grad():
            if branch is None:
                branch = self._branch_train(u) if self.training else self.branch_features(u)
            hd, keep = self._head_params()
            out = ops.dmm_rf_features(branch, grid, hd, second_order)
        del keep
        return out

    def jet(self, u: torch.Tensor, grid: torch.Tensor, second_order: bool = True,
            branch: torch.Tensor | None = None):
        """phi = forward(u, grid) and its derivatives in the grid row -- the jet
        (phi, phi_x, phi_y, phi_xx, phi_xy, phi_yy) the Monge-Ampere loss is made
        of -- from the head's closed form (ops.dmm_jet) instead of autograd
        through out_nn: what the reference's Adam and LBFGS phases obtain with
        autograd.grad(create_graph=True) twice (mesh/dmm_utils.py:507-552).
        u, grid as for forward; branch: the branch output [B, L] to use instead
        of computing it from u.  In train() the branch comes from the torch ops
        of the train()-mode forward (_branch_train): it stays differentiable and
        the graph branch's BatchNorms advance their running statistics once per
        call; in eval() it is branch_features(u).  The outputs are differentiable,
        first order, in the branch and in the head's parameters (trunk, out_nn);
        not in grid, which must not require grad.
        Returns ops.Jet of six [rows, 1] tensors, the last three None with
        second_order=False."""
        L.require_device(u, grid)
        if grid.requires_grad:
            raise ValueError("DMM.jet is not differentiable in grid: pass the rows detached (the derivatives in "
                             "the row are the jet's outputs)")
        self._head_params()   # NotImplementedError for a head the kernels do not take
        if branch is None:
            branch = self._branch_train(u) if self.training else self.branch_features(u)
        tl, ol = self.trunk.layers, self.out_nn.layers
        dims = (tl[0].out_features, tl[1].out_features, ol[0].out_features)
        out = _HeadJet.apply(branch, grid, bool(second_order), dims, *self._tensors()[0], ol[1].bias)
        return ops.Jet(*out, *([None] * (6 - len(out))))

    def grid_nbr(self, grid: torch.Tensor, k: int = 35) -> torch.Tensor:
        """kNN-35 table of the fixed grid (reference dmm_model.py:222-234 builds it
        every call on B identical copies; it depends only on the grid, so it is
        built once per grid here).  LOCAL indices [N, k] int32."""
        # the entry holds the grid tensor itself, so its storage cannot be freed
        # and reused by another grid while the entry lives: (address, version,
        # shape) then identifies the content
        key = (grid.data_ptr(), grid._version, tuple(grid.shape), str(grid.device), k)
        hit = self._grid_cache.get(key)
        if hit is None:
            hit = (grid, knn_graph_nbr(grid, 1, k))
            self._grid_cache = {key: hit}
        return hit[1]

    # ----------------------------------------------------------------- the API
    @staticmethod
    def _local_nbr(nbr: torch.Tensor, n: int, device) -> torch.Tensor:
        """A caller's [N, k] int32 LOCAL neighbour table, checked for the kernels."""
        L.require_device(nbr)
        if nbr.dtype != torch.int32 or nbr.dim() != 2 or nbr.shape[0] != n or nbr.device != device:
            raise ValueError("nbr must be an [N, k] int32 table of local indices on u's device")
        return nbr.contiguous()

    @staticmethod
    def _workspace(workspace, B, n, hd, device) -> torch.Tensor:
        """The caller's workspace, checked against mmpde_dmm_workspace_bytes, or a new one."""
        nb = L.lib().mmpde_dmm_workspace_bytes(B, n, hd.latent, hd.hidden)
        if workspace is None:
            return torch.empty((nb // 4,), dtype=torch.float32, device=device)
        L.require_device(workspace)
        if workspace.numel() * workspace.element_size() < nb:
            raise ValueError("workspace is smaller than mmpde_dmm_workspace_bytes")
        return workspace

    def branch_features(self, u: torch.Tensor, nbr: torch.Tensor | None = None,
                        workspace: torch.Tensor | None = None) -> torch.Tensor:
        """The branch of forward (dmm_model.py:188,197-210) alone.
        u: graph mode [B, N] (values on self.ori_grid), array mode [B, s, s];
        nbr: graph mode only, an [N, k] int32 local neighbour table of any k used
        instead of the kNN-35 table of self.ori_grid.  Returns [B, L] fp32."""
        L.require_device(u)
        if self.training:
            raise NotImplementedError("branch_features is eval-mode: call .eval()")
        bp, hd = self.device_params()
        u = L.f32c(u)
        B = u.shape[0]
        lib = L.lib()
        st = L.stream(u.device)
        branch = torch.empty((B, hd.latent), dtype=torch.float32, device=u.device)
        if self.mode == "graph":
            og = L.f32c(torch.as_tensor(self.ori_grid).to(u.device)).reshape(-1, 2)
            N = og.shape[0]
            nbr = self.grid_nbr(og) if nbr is None else self._local_nbr(nbr, N, u.device)
            workspace = self._workspace(workspace, B, N, hd, u.device)
            L.check(lib.mmpde_dmm_branch_graph(L.ptr(u), L.ptr(og), B, N, L.ptr(nbr), nbr.shape[1],
                                               ctypes.byref(bp), ctypes.byref(hd), L.ptr(workspace),
                                               L.ptr(branch), st), "mmpde_dmm_branch_graph")
        else:
            if nbr is not None:
                raise ValueError("nbr is a graph-mode argument")
            s = self.branch.s
            workspace = self._workspace(workspace, B, s * s, hd, u.device)
            L.check(lib.mmpde_dmm_branch_array(L.ptr(u), B, ctypes.byref(bp), ctypes.byref(hd),
                                               L.ptr(workspace), L.ptr(branch), st),
                    "mmpde_dmm_branch_array")
        return branch

    def head_cache(self, xi: torch.Tensor, workspace: torch.Tensor | None = None) -> torch.Tensor:
        """The grid side of the head (trunk(xi), Q, J = dQ/dxi): a function of xi
        and the weights only, prepared once for a rollout over a fixed grid and
        passed to mesh(..., head_cache=).  Recompute it after changing weights."""
        L.require_device(xi)
        _, hd = self.device_params()
        xi = L.f32c(xi).reshape(-1, 2)
        N = xi.shape[0]
        if workspace is None:
            nb = L.lib().mmpde_dmm_workspace_bytes(1, N, hd.latent, hd.hidden)
            workspace = torch.empty((nb // 4,), dtype=torch.float32, device=xi.device)
        cache = torch.empty((L.lib().mmpde_dmm_head_cache_bytes(N, hd.hidden) // 4,),
                            dtype=torch.float32, device=xi.device)
        L.check(L.lib().mmpde_dmm_head_prepare(L.ptr(xi), N, ctypes.byref(hd), L.ptr(workspace),
                                               L.ptr(cache), L.stream(xi.device)),
                "mmpde_dmm_head_prepare")
        return cache

    def mesh(self, u: torch.Tensor, xi: torch.Tensor, out: torch.Tensor | None = None,
             workspace: torch.Tensor | None = None,
             head_cache: torch.Tensor | None = None,
             nbr: torch.Tensor | None = None) -> torch.Tensor:
        """Moved mesh x = xi + d(phi)/d(xi) for every trajectory.
        u: graph mode [B, N] (values on the fixed grid), array mode [B, s, s];
        xi: [N, 2] grid shared by all trajectories (graph: self.ori_grid;
        array: the np.meshgrid 'xy' grid of data_creator_2d.py:94-100);
        head_cache: head_cache(xi) of the same xi and weights, or None;
        nbr: graph mode only, an [N, k] int32 local neighbour table of any k used
        instead of the kNN-35 table of xi.
        Returns [B*N, 2] fp32."""
        L.require_device(u, xi)
        bp, hd = self.device_params()
        u = L.f32c(u)
        xi = L.f32c(xi).reshape(-1, 2)
        B, N = u.shape[0], xi.shape[0]
        if workspace is None:
            ne = N if self.mode == "graph" else max(N, self.branch.s ** 2)  # array: xi may be coarser
            nb = L.lib().mmpde_dmm_workspace_bytes(B, ne, hd.latent, hd.hidden)
            workspace = torch.empty((nb // 4,), dtype=torch.float32, device=u.device)
        if out is None:
            out = torch.empty((B * N, 2), dtype=torch.float32, device=u.device)
        if head_cache is not None:
            L.require_device(head_cache)
            if head_cache.numel() * 4 < L.lib().mmpde_dmm_head_cache_bytes(N, hd.hidden):
                raise ValueError("head_cache is smaller than mmpde_dmm_head_cache_bytes")
        hc = L.ptr(head_cache) if head_cache is not None else None
        st = L.stream(u.device)
        if self.mode == "graph":
            nbr = self.grid_nbr(xi) if nbr is None else self._local_nbr(nbr, N, u.device)
            L.check(L.lib().mmpde_dmm_mesh_graph_cached(
                L.ptr(u), L.ptr(xi), B, N, L.ptr(nbr), nbr.shape[1], ctypes.byref(bp),
                ctypes.byref(hd), hc, L.ptr(workspace), L.ptr(out), st), "mmpde_dmm_mesh_graph")
        else:
            if nbr is not None:
                raise ValueError("nbr is a graph-mode argument")
            L.check(L.lib().mmpde_dmm_mesh_array_cached(
                L.ptr(u), L.ptr(xi), B, N, ctypes.byref(bp), ctypes.byref(hd), hc,
                L.ptr(workspace), L.ptr(out), st), "mmpde_dmm_mesh_array")
        return out

    def mesh_fields(self, u: torch.Tensor, xi: torch.Tensor) -> torch.Tensor:
        """The moved mesh xi + grad(phi) of each of the K fields of u, every field
        treated as a batch of its own: what K calls with one field each give
        (the reference's per-epoch evaluation, mesh/dmm_utils.py:1162-1284, which
        runs the model in whatever mode training left it in).  u, xi as for
        mesh; returns [K * N, 2] fp32, under torch.no_grad().
        eval(): mesh(u, xi).
        train(): the branch on the training kernels -- array mode
        ConvNet.forward_train_hip for s <= ops.CONVNET_TRAIN_MAX_S and the torch
        ConvNet above (no BatchNorm there: a batch of K is K batches of one);
        graph mode _branch_train_hip's sequence on self.ori_grid with every
        BatchNorm over K row segments (ops.batch_norm_rows(segments=K)): each
        field normalised with its own statistics, the running statistics
        advanced K times in field order and num_batches_tracked by K.  Graph
        mode needs hidden_features == 4 (NotImplementedError otherwise).  grad(phi)
        is the head's closed form (ops.dmm_jet, first order) at xi repeated K
        times; the head has no BatchNorm."""
        L.require_device(u, xi)
        if not self.training:
            with torch.no_grad():
                return self.mesh(u, xi)
        xi = L.f32c(xi).reshape(-1, 2)
        K = u.shape[0]
        with torch.no_grad():
            if self.mode == "array":
                if self.branch.s <= ops.CONVNET_TRAIN_MAX_S:
                    branch = self.branch.forward_train_hip(L.f32c(u))
                else:
                    branch = self.branch(u.float().unsqueeze(1))
            else:
                if self.hidden_features != 4:
                    raise NotImplementedError("mesh_fields: the graph branch kernels take hidden_features == 4 only "
                                              f"(got {self.hidden_features})")
                og = torch.as_tensor(self.ori_grid).to(u.device, torch.float32).reshape(-1, 2).contiguous()
                branch = self._branch_train_hip(u, og, self.grid_nbr(og), segments=K)
            hd, keep = self._head_params()
            rows = xi.repeat(K, 1)
            jet = ops.dmm_jet(branch, rows, hd, self.out_nn.layers[1].bias, second_order=False)
            del keep
            return rows + torch.stack((jet.phi_x, jet.phi_y), dim=-1)

    # ----------------------------------------------------------------- the mesh Jacobian
    def hess_cache(self, xi: torch.Tensor, workspace: torch.Tensor | None = None) -> torch.Tensor:
        """K = dJ/dxi [N, L', 3], the table of xi and the weights that the Hessian
        needs beside head_cache's Q and J: prepared once for a rollout over a
        fixed grid and passed to mesh_hess(..., hess_cache=).  Recompute it after
        changing weights."""
        L.require_device(xi)
        _, hd = self.device_params()
        xi = L.f32c(xi).reshape(-1, 2)
        N = xi.shape[0]
        nb = L.lib().mmpde_dmm_workspace_bytes(1, N, hd.latent, hd.hidden)
        if workspace is None:
            workspace = torch.empty((nb // 4,), dtype=torch.float32, device=xi.device)
        else:
            L.require_device(workspace)
            if workspace.numel() * workspace.element_size() < nb:
                raise ValueError("workspace is smaller than mmpde_dmm_workspace_bytes")
        cache = torch.empty((L.lib().mmpde_dmm_hess_cache_bytes(N, hd.hidden) // 4,),
                            dtype=torch.float32, device=xi.device)
        L.check(L.lib().mmpde_dmm_hess_prepare(L.ptr(xi), N, ctypes.byref(hd), L.ptr(workspace),
                                               L.ptr(cache), L.stream(xi.device)),
                "mmpde_dmm_hess_prepare")
        return cache

    def mesh_hess(self, u: torch.Tensor, xi: torch.Tensor, out: torch.Tensor | None = None,
                  hess_out: torch.Tensor | None = None, det_out: torch.Tensor | None = None,
                  workspace: torch.Tensor | None = None,
                  head_cache: torch.Tensor | None = None,
                  hess_cache: torch.Tensor | None = None,
                  nbr: torch.Tensor | None = None, folds_total: torch.Tensor | None = None,
                  detmin_out: torch.Tensor | None = None, folds_out: torch.Tensor | None = None):
        """mesh(u, xi) together with the mesh map's Jacobian dx/dxi = I + Hess phi
        (reference mesh/dmm_utils.py:507-552's phixx, phixy, phiyy and determinant,
        without autograd and in eval mode).  Arguments as for mesh; hess_cache:
        hess_cache(xi) of the same xi and weights, or None; folds_total: a [B]
        int32 counter the call adds this call's folds to (never reset here).
        Returns (mesh [B*N, 2], hess [B*N, 3] = (phi_11, phi_12, phi_22),
        det [B*N], detmin [B], folds [B] int32): det <= 0 (or NaN) at a node means
        the moved mesh has folded there; folds counts those nodes per trajectory.
        The mesh is bit for bit that of mesh()."""
        L.require_device(u, xi)
        bp, hd = self.device_params()
        u = L.f32c(u)
        xi = L.f32c(xi).reshape(-1, 2)
        B, N = u.shape[0], xi.shape[0]
        lib = L.lib()
        ne = N if self.mode == "graph" else max(N, self.branch.s ** 2)  # array: xi may be coarser
        nb = lib.mmpde_dmm_hess_workspace_bytes(B, ne, hd.latent, hd.hidden)
        if workspace is None:
            workspace = torch.empty((nb // 4,), dtype=torch.float32, device=u.device)
        else:
            L.require_device(workspace)
            if workspace.numel() * workspace.element_size() < nb:
                raise ValueError("workspace is smaller than mmpde_dmm_hess_workspace_bytes")
        for name, cache, need in (("head_cache", head_cache, lib.mmpde_dmm_head_cache_bytes(N, hd.hidden)),
                                  ("hess_cache", hess_cache, lib.mmpde_dmm_hess_cache_bytes(N, hd.hidden))):
            if cache is not None:
                L.require_device(cache)
                if cache.dtype != torch.float32 or not cache.is_contiguous() or cache.numel() * 4 < need:
                    raise ValueError(f"{name} is smaller than mmpde_dmm_{name}_bytes")

        def buf(t, shape, dtype, what):
            if t is None:
                return torch.empty(shape, dtype=dtype, device=u.device)
            L.require_device(t)
            if t.dtype != dtype or not t.is_contiguous() or t.numel() != torch.Size(shape).numel():
                raise ValueError(f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)}")
            return t

        out = buf(out, (B * N, 2), torch.float32, "out")
        hess_out = buf(hess_out, (B * N, 3), torch.float32, "hess_out")
        det_out = buf(det_out, (B * N,), torch.float32, "det_out")
        detmin = buf(detmin_out, (B,), torch.float32, "detmin_out")
        folds = buf(folds_out, (B,), torch.int32, "folds_out")
        if folds_total is not None:
            folds_total = buf(folds_total, (B,), torch.int32, "folds_total")
        io = L.DmmHessIO(L.ptr(head_cache), L.ptr(hess_cache), L.ptr(hess_out), L.ptr(det_out),
                         L.ptr(detmin), L.ptr(folds), L.ptr(folds_total))
        st = L.stream(u.device)
        if self.mode == "graph":
            nbr = self.grid_nbr(xi) if nbr is None else self._local_nbr(nbr, N, u.device)
            L.check(lib.mmpde_dmm_mesh_graph_hess(
                L.ptr(u), L.ptr(xi), B, N, L.ptr(nbr), nbr.shape[1], ctypes.byref(bp),
                ctypes.byref(hd), ctypes.byref(io), L.ptr(workspace), L.ptr(out), st),
                "mmpde_dmm_mesh_graph_hess")
        else:
            if nbr is not None:
                raise ValueError("nbr is a graph-mode argument")
            L.check(lib.mmpde_dmm_mesh_array_hess(
                L.ptr(u), L.ptr(xi), B, N, ctypes.byref(bp), ctypes.byref(hd), ctypes.byref(io),
                L.ptr(workspace), L.ptr(out), st), "mmpde_dmm_mesh_array_hess")
        return out, hess_out, det_out, detmin, folds

    # ----------------------------------------------------------------- the fold guard
    def mesh_guarded(self, u: torch.Tensor, xi: torch.Tensor, floor: float | None = 0.1, alpha: float = 1.0,
                     out: torch.Tensor | None = None, hess_out: torch.Tensor | None = None,
                     det_out: torch.Tensor | None = None, workspace: torch.Tensor | None = None,
                     head_cache: torch.Tensor | None = None, hess_cache: torch.Tensor | None = None,
                     nbr: torch.Tensor | None = None, folds_total: torch.Tensor | None = None,
                     guarded_total: torch.Tensor | None = None, alpha_out: torch.Tensor | None = None,
                     lam_out: torch.Tensor | None = None, detmin_out: torch.Tensor | None = None,
                     folds_out: torch.Tensor | None = None, det_before_out: torch.Tensor | None = None,
                     detmin_before_out: torch.Tensor | None = None,
                     folds_before_out: torch.Tensor | None = None):
        """mesh_hess(u, xi) followed by the reference's relaxation x = alpha x +
        (1 - alpha) xi (data_creator_2d.py:109-111,133-135; alpha = 1 there) with
        the step chosen per trajectory (ops.mesh_relax): a trajectory whose full
        move leaves an eigenvalue of dx/dxi = I + alpha Hess phi below `floor` at
        some node is moved only as far as keeps it at floor; the others move by
        `alpha` (at alpha = 1 their rows are mesh()'s bit for bit).  floor is a
        parameter in (0, 1) (0.1: a default, not a measured optimum); the
        damping is uniform over a trajectory.  floor None: mesh() and the plain
        relaxation by alpha, no Hessian.  Eval mode, no autograd.  Buffers as for
        mesh_hess; workspace: mmpde_dmm_hess_workspace_bytes (floor None:
        mmpde_dmm_workspace_bytes); guarded_total: a [B] int32 counter, +=
        (alpha_b < alpha); the *_before_out buffers take mesh_hess's det, detmin
        and folds of the full move.
        Returns (mesh [B*N, 2], alpha_b [B], lam_b [B] = the smallest eigenvalue of
        Hess phi per trajectory, hess [B*N, 3], det_after [B*N], detmin_after [B],
        folds_after [B] int32, folds_before [B] int32); floor None: the last six
        are None."""
        if self.training:
            raise NotImplementedError("mesh_guarded is eval-mode: call .eval()")
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"alpha {alpha}: the relaxation takes 0 <= alpha <= 1")
        if floor is not None and not 0.0 < floor < 1.0:
            raise ValueError(f"floor {floor}: None (no guard) or 0 < floor < 1")
        B = u.shape[0]
        with torch.no_grad():
            if floor is None:
                out = self.mesh(u, xi, out=out, workspace=workspace, head_cache=head_cache, nbr=nbr)
                _, alpha_b, _, _, _ = ops.mesh_relax(out, xi, batches=B, alpha=alpha, alpha_out=alpha_out,
                                                     guarded_total=guarded_total)
                return out, alpha_b, None, None, None, None, None, None
            out, hess, _, _, folds_before = self.mesh_hess(
                u, xi, out=out, hess_out=hess_out, det_out=det_before_out, workspace=workspace,
                head_cache=head_cache, hess_cache=hess_cache, nbr=nbr, folds_total=folds_total,
                detmin_out=detmin_before_out, folds_out=folds_before_out)
            if det_out is None:
                det_out = torch.empty((out.shape[0],), dtype=torch.float32, device=out.device)
            _, alpha_b, lam, detmin, folds = ops.mesh_relax(
                out, xi, hess, batches=B, alpha=alpha, floor=floor, alpha_out=alpha_out, lam_out=lam_out,
                det_out=det_out, detmin_out=detmin_out, folds_out=folds_out, guarded_total=guarded_total)
        return out, alpha_b, lam, hess, det_out, detmin, folds, folds_before
