"""Inputs and float64 references of the DMM shape tests (test_gpu_dmm_shapes.py
on the device, test_dmm_shape_cases.py on the CPU alone).

Graph models are DMM(mode="graph", grid=..., branch_layer=[4, nl],
trunk_layer=[2, th, L], out_layer=[2 L, L', 1]) under a fixed seed, every
BatchNorm's buffers and affine parameters randomised (running_var in [0.5, 2],
running_mean and bias in +-0.5, weight in [0.5, 1.5]), on a grid of random
points of the unit square, with a random neighbour table randint(0, N) [N, k]
(self loops and repeats allowed; entries 0 and N - 1 forced in).  Branch cases
double the Linear weights of gnn_layers.*, decoding_mlp and output_mlp (the
tanh layers then leave their linear regime); mesh cases keep the default init.

Every case is built once (lru_cache) and never modified; its references are
float64 evaluations of oracle/refcpu.py on the float64 casts of the state
dict, u and the grids.
"""
import functools

import numpy as np
import torch

from oracle import refcpu

DEFAULT_HEAD = (16, 512, 512)        # (th, L, L')
BRANCH_BAR = 1e-5                    # of max|ref|
MESH_BAR = 2e-5                      # of max|disp_ref|, + 2^-23 max|xi|
PHI_BAR = 2e-5                       # of max|ref|

# (n_per, k, nl, B), smallest first
GRAPH_BRANCH_CASES = (
    # k = 1..65 at n_per = 129: one, two and three trips of the edge loop, ragged last quad
    [(129, k, 3, 2) for k in (1, 3, 4, 31, 32, 33)] +
    # n_per with k = 35: k + 1, the 128-target block edge
    [(36, 35, 3, 2), (127, 35, 3, 2), (128, 35, 3, 2)] +
    # layers and batch at n_per = 129
    [(129, 35, 0, 2), (129, 35, 1, 2), (129, 35, 2, 2), (129, 35, 3, 1), (129, 35, 3, 2)] +
    [(129, 64, 3, 2), (129, 65, 3, 2), (129, 35, 3, 65)] +
    # second trip of the 512-thread staging loop; 2340: the staging alone fits 64 KiB, with the
    # kernel's static weights it does not; 4388: largest LDS size; 4389: first global-kernel
    # size, with B = 3 a workgroup's 64 nodes span two trajectories
    [(513, 35, 3, 2), (2340, 35, 3, 2), (4388, 35, 3, 2), (4389, 35, 3, 2), (4389, 35, 3, 3)])
ARRAY_BRANCH_CASES = [(5, 3), (6, 3), (7, 3), (33, 1), (33, 3), (33, 65), (48, 3)]      # (s, B)
# (n_per, B, head) in graph mode with k = 5, nl = 1
GRAPH_MESH_CASES = (
    [(130, 3, h) for h in ((1, 8, 128), (7, 64, 1024), DEFAULT_HEAD, (64, 512, 512))] +
    [(n, 3, DEFAULT_HEAD) for n in (6, 129, 131)] +
    [(130, b, DEFAULT_HEAD) for b in (1, 32, 33, 65)])
ARRAY_MESH_CASES = [(33, 3), (33, 33)]                                                  # (s, B)
# One changed slot moves the branch by 1e-4 to 1e-3 of its maximum on most
# draws, and by far less where the replaced source happens to resemble the
# original.  test_dmm_shape_cases.py asks for 5 bars; the graph branch cases
# whose first draw gave less than 10 bars take the first later draw with 10.
SEED_SALT = {(129, 35, 1, 2): 3, (129, 35, 3, 1): 1, (129, 65, 3, 2): 2, (129, 35, 3, 65): 2,
             (4388, 35, 3, 2): 1, (4389, 35, 3, 2): 3, (4389, 35, 3, 3): 2}


class Case:
    """mode, dmm (CPU, eval), sd (float32 state dict), u, and per mode: graph
    grid [N, 2], nbr [N, k] int32, ei [2, B N k] global edge index, nl; array
    s and xi (the s x s meshgrid 'xy' grid of data_creator_2d.py:94-100)."""


def _randomise_bn(dmm, g):
    for m in dmm.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            n = m.num_features
            with torch.no_grad():
                m.running_var.copy_(0.5 + 1.5 * torch.rand(n, generator=g))
                m.running_mean.copy_(torch.rand(n, generator=g) - 0.5)
                m.weight.copy_(0.5 + torch.rand(n, generator=g))
                m.bias.copy_(torch.rand(n, generator=g) - 0.5)


def edge_index(nbr, batches):
    """The global source -> target edge index of `batches` copies of a local table."""
    n, k = nbr.shape
    src = nbr.long()[None] + n * torch.arange(batches)[:, None, None]
    tgt = torch.arange(batches * n).repeat_interleave(k)
    return torch.stack([src.reshape(-1), tgt])


@functools.lru_cache(maxsize=None)
def graph_case(n_per, k, nl, B, head=DEFAULT_HEAD, branch_x2=True):
    from mmpde_amd import DMM

    th, L, Lp = head
    seed = 7 + 1000003 * n_per + 10007 * k + 101 * nl + 11 * B + th + Lp + 7919 * SEED_SALT.get((n_per, k, nl, B), 0)
    g = torch.Generator().manual_seed(seed)
    c = Case()
    c.mode, c.nl, c.B, c.head = "graph", nl, B, head
    c.grid = torch.rand(n_per, 2, generator=g)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        c.dmm = DMM(mode="graph", grid=c.grid, branch_layer=[4, nl], trunk_layer=[2, th, L],
                    out_layer=[2 * L, Lp, 1])
    _randomise_bn(c.dmm, g)
    if branch_x2:
        with torch.no_grad():
            for part in (c.dmm.gnn_layers, c.dmm.decoding_mlp.layers, c.dmm.output_mlp):
                for m in part.modules():
                    if isinstance(m, torch.nn.Linear):
                        m.weight.mul_(2.0)
    c.dmm.eval()
    c.sd = {n: t.detach().clone() for n, t in c.dmm.state_dict().items()}
    c.nbr = torch.randint(0, n_per, (n_per, k), generator=g, dtype=torch.int32)
    c.nbr[0, 0] = n_per - 1
    c.nbr[n_per - 1, k - 1] = 0
    c.ei = edge_index(c.nbr, B)
    c.u = torch.randn(B, n_per, generator=g)
    c.xi = c.grid
    return c


@functools.lru_cache(maxsize=None)
def array_case(s, B, head=DEFAULT_HEAD):
    from mmpde_amd import DMM

    th, L, Lp = head
    seed = 13 + 1009 * s + 11 * B + th + Lp
    g = torch.Generator().manual_seed(seed)
    c = Case()
    c.mode, c.s, c.B, c.head = "array", s, B, head
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        c.dmm = DMM(s=s, mode="array", branch_layer=7, trunk_layer=[2, th, L], out_layer=[2 * L, Lp, 1])
    c.dmm.eval()
    c.sd = {n: t.detach().clone() for n, t in c.dmm.state_dict().items()}
    c.u = torch.randn(B, s, s, generator=g)
    lin = np.linspace(0, 1, s)
    c.xi = torch.tensor(np.array(np.meshgrid(lin, lin)), dtype=torch.float).reshape(2, -1).permute(1, 0).contiguous()
    return c


# --------------------------------------------------------------------------- references
def branch_ref(c, dtype=torch.float64, ei=None, u=None):
    """[B, L] of refcpu in `dtype` (ei / u: a mutated edge index / input)."""
    cast = (lambda t: t.to(dtype) if t.is_floating_point() else t)
    sd = {k: cast(v) for k, v in c.sd.items()}
    u = cast(c.u if u is None else u)
    with torch.no_grad():
        if c.mode == "array":
            return refcpu.convnet(sd, "branch", u.unsqueeze(1))
        return refcpu.dmm_branch(sd, "graph", u, ori_grid=cast(c.grid), hidden_layer=c.nl,
                                 grid_edge_index=c.ei if ei is None else ei)


def disp_ref(c, dtype=torch.float64, sd=None):
    """mesh - xi [B N, 2] through refcpu's autograd in `dtype` (sd: a mutated
    float32 state dict)."""
    cast = (lambda t: t.to(dtype) if t.is_floating_point() else t)
    sd = {k: cast(v) for k, v in (c.sd if sd is None else sd).items()}
    u, xi = cast(c.u), cast(c.xi)
    if c.mode == "graph":
        gx, gy = xi[None, :, 0].repeat(c.B, 1), xi[None, :, 1].repeat(c.B, 1)
        x1, x2 = refcpu.moving_mesh_tri(sd, u, gx, gy, xi, grid_edge_index=c.ei, hidden_layer=c.nl)
        return torch.cat((x1 - gx.reshape(-1, 1), x2 - gy.reshape(-1, 1)), dim=-1)
    # data_creator_2d.py:104-107 on the given xi
    rows = xi.repeat(c.B, 1).clone().requires_grad_(True)
    with torch.enable_grad():
        phi = refcpu.dmm_forward(sd, "array", u, rows)
        x = torch.autograd.grad(phi, rows, grad_outputs=torch.ones_like(phi))[0] + rows
    return (x - rows).detach()


def mesh_bar(c, ref):
    """2e-5 of the displacement + the rounding of the stored fp32 coordinate."""
    return MESH_BAR * ref.abs().max().item() + 2.0 ** -23 * c.xi.abs().max().item()


def phi_ref(c, grid, dtype=torch.float64):
    """(phi [B m, 1], second_out [B m, L']) of refcpu in `dtype` on grid [B m, 2]."""
    cast = (lambda t: t.to(dtype) if t.is_floating_point() else t)
    sd = {k: cast(v) for k, v in c.sd.items()}
    with torch.no_grad():
        br = branch_ref(c, dtype)
        rep = grid.shape[0] // c.B
        br = br[:, None, :].repeat(1, rep, 1).reshape(-1, br.shape[-1])
        trunk, _ = refcpu.densenet(sd, "trunk", cast(grid), 2)
        phi, second = refcpu.densenet(sd, "out_nn", torch.cat((br, trunk), dim=-1), 2)
        full = refcpu.dmm_forward(sd, c.mode, cast(c.u), cast(grid))
    assert (full - phi).abs().max().item() <= 1e-5 * phi.abs().max().item()
    return full, second


# --------------------------------------------------------------------------- mutations (self-check)
def mutated_last_slot(c):
    """The edge index with the last slot of the last row of the last trajectory changed."""
    n, k = c.nbr.shape
    ei = c.ei.clone()
    e = c.B * n * k - 1
    assert int(ei[1, e]) == c.B * n - 1
    old = int(ei[0, e]) - (c.B - 1) * n
    ei[0, e] = (c.B - 1) * n + (old + 1 + n // 2) % n
    return ei


def mutated_last_block(c):
    """The edge index with the last slot of every row of the last trajectory's
    trailing partial 128-row block changed."""
    n, k = c.nbr.shape
    ei = c.ei.clone()
    first = (n - 1) // 128 * 128
    rows = torch.arange(first, n)
    e = ((c.B - 1) * n + rows) * k + (k - 1)
    old = ei[0, e] - (c.B - 1) * n
    ei[0, e] = (c.B - 1) * n + (old + 1 + n // 2) % n
    return ei


def mutated_last_pixel(c):
    """u with the last pixel of the last trajectory zeroed (array branch)."""
    u = c.u.clone()
    u[-1, -1, -1] = 0.0
    return u


def mutated_head(c, which):
    sd = dict(c.sd)
    if which == "w_o":
        w = sd["out_nn.layers.1.weight"].clone()
        w[0, -1] = 0.0
        sd["out_nn.layers.1.weight"] = w
    else:
        w = sd["trunk.layers.0.weight"].clone()
        w[-1, :] = 0.0
        sd["trunk.layers.0.weight"] = w
    return sd
