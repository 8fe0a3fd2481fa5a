"""Inputs and float64 references of the GNN stage shape tests
(test_gpu_node_shapes.py on the device, test_gnn_stage_cases.py on the CPU
alone): the fused eval forward (embed kernel, edge stage, node kernels, fused
head) at the row counts around its 32-row tile (two 16-row blocks), time
windows 1 .. 16, depths 0 .. 3, ragged tables, non-unit 1/Lx, 1/Ly, 1/tmax
and trajectory segments.

Models are MP_PDE_Solver_2D(pde, time_window=tw) under a fixed seed with
every BatchNorm randomised (synth._randomise_bn), gnn_layers cut to `depth`
layers.  The pde object and the oracle's PDEConst carry the case's own Lx, Ly
and tmax (dt stays the cylinder default 0.1).  Graphs: u randn [n, tw];
pos = (t, x, y) with a different t in (0, tmax) in every row (or one t for all,
const_t) and (x, y) uniform in [0, Lx) x [0, Ly); nbr int32 [n, k] uniform in
the row's segment (self loops and repeats allowed); ragged cases add deg with
deg[0] = 0, deg[n - 1] = k and every padding slot set to -1.

Every case is built once (lru_cache) and never modified; references are
oracle/refcpu.mp_pde_solver on the casts of the state dict and the inputs.

The two floors are the largest errors of the float32 CPU oracle against the
float64 one over CASES (row_rel_err of the compared hidden state; max|out -
out64| / max|out64|), rounded up to one digit.  Measured: 6.17e-7 and 3.41e-7
on one x86 host (the same with 1, 4 and 16 threads), 6.17e-7 and 3.47e-7 on
another vendor's: the fp32 BLAS sums in an order of the host's choosing, hence
one digit and not two.  They are the yardstick of the device tests: a HIP
arithmetic may be 4 x the fp32 oracle's error (the rule of
test_gpu_precision.py), the floor never comes from a kernel.
"""
import collections
import functools

import torch

from oracle import refcpu

FP32_FLOOR_H = 7e-7
FP32_FLOOR_OUT = 4e-7
FACTOR = 4.0                         # HIP arithmetic vs the fp32 oracle (test_gpu_precision.py)
MIN_ROW_MAG = 0.1                    # every compared float64 row has max|h| above it

UNIT = (1.0, 1.0, 2.9)               # (Lx, Ly, tmax) of both reference PDEs
SCALES = [(2.0, 0.5, 2.9), (3.0, 0.7, 1.7)]      # the second: 1/L no power of two

Case = collections.namedtuple("Case", "n tw depth k ragged scales seg_n", defaults=(5, False, UNIT, 0))

MAIN = [Case(n, tw, depth) for depth in (1, 2, 3) for tw in (1, 2, 16) for n in (1, 15, 16, 17, 31, 32, 33, 65)]
RAGGED = [Case(n, tw, 2, ragged=True) for n in (17, 33, 65) for tw in (1, 3)] + [Case(65, 3, 2, k=35, ragged=True)]
NONUNIT = [Case(33, tw, 2, scales=s) for s in SCALES for tw in (1, 3)]
# segments on tile boundaries, and straddling tiles
SEGMENTS = [Case(96, 1, 2, seg_n=32), Case(111, 1, 2, seg_n=37)]
DEPTH0 = [Case(1, 1, 0), Case(33, 1, 0)]     # the C API takes no layers at tw = 1 only
CASES = MAIN + RAGGED + NONUNIT + SEGMENTS + DEPTH0
# one t for every row: the (x, y) + t and (x, y) + t_slot position forms
CONST_T = [Case(33, 1, 2), Case(17, 3, 2, ragged=True), Case(33, 16, 3)]


def case_id(c):
    s = f"n{c.n}-tw{c.tw}-d{c.depth}-k{c.k}"
    if c.ragged:
        s += "-ragged"
    if c.scales != UNIT:
        s += "-L" + "x".join(f"{v:g}" for v in c.scales)
    if c.seg_n:
        s += f"-seg{c.seg_n}"
    return s


@functools.lru_cache(maxsize=None)
def solver(tw, depth, Lx=1.0, Ly=1.0, tmax=2.9):
    """The CPU eval model of a case (callers that move it copy it first)."""
    from mmpde_amd.gnn_2d import MP_PDE_Solver_2D
    from mmpde_amd.pdes import cy
    from mmpde_amd.synth import _randomise_bn, cy_synth_mesh

    grid = cy_synth_mesh()
    pde = cy(ori_grid=grid)
    pde.grid_size = [30, grid.shape[0]]
    pde.Lx, pde.Ly, pde.tmax = Lx, Ly, tmax      # dt stays 2.9 / 29, as PDEConst's
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(40 + tw)
        model = MP_PDE_Solver_2D(pde=pde, time_window=tw, eq_variables={})
    _randomise_bn(model, torch.Generator().manual_seed(41 + tw))
    model.gnn_layers = model.gnn_layers[:depth]
    model.hidden_layer = depth
    return model.eval()


def oracle_pde(c):
    """refcpu.PDEConst with the case's Lx, Ly, tmax."""
    pde = refcpu.PDEConst("cy", [30, 2521])
    pde.Lx, pde.Ly, pde.tmax = c.scales
    return pde


class Graph:
    """u [n, tw], pos [n, 3], nbr [n, k] int32, deg [n] int32 or None,
    edge_index [2, E] int64 (source, target) over the live slots, seg_n."""


@functools.lru_cache(maxsize=None)
def graph(c, const_t=False):
    Lx, Ly, tmax = c.scales
    seed = 1 + 1000003 * c.n + 10007 * c.tw + 101 * c.depth + 11 * c.k + 7 * c.ragged + c.seg_n \
        + int(1000 * (Lx + 3 * Ly + 7 * tmax))
    g = torch.Generator().manual_seed(seed)
    n, k = c.n, c.k
    d = Graph()
    d.u = torch.randn(n, c.tw, generator=g)
    # one t per stratum of (0, tmax), shuffled: distinct in every row
    t = tmax * (torch.randperm(n, generator=g) + 0.25 + 0.5 * torch.rand(n, generator=g)) / n
    if const_t:
        t = torch.full((n,), 0.37 * tmax)
    xy = torch.rand(n, 2, generator=g) * torch.tensor([Lx, Ly])
    d.pos = torch.cat((t[:, None], xy), 1).float()
    seg = c.seg_n or n
    assert n % seg == 0
    d.seg_n = c.seg_n
    d.nbr = (torch.randint(0, seg, (n, k), generator=g) + (torch.arange(n) // seg * seg)[:, None]).to(torch.int32)
    d.deg = None
    live = torch.ones((n, k), dtype=torch.bool)
    if c.ragged:
        d.deg = torch.randint(0, k + 1, (n,), generator=g, dtype=torch.int32)
        d.deg[0], d.deg[n - 1] = 0, k
        live = torch.arange(k)[None, :] < d.deg[:, None]
        d.nbr[~live] = -1
    tgt = torch.arange(n)[:, None].expand(n, k)
    d.edge_index = torch.stack([d.nbr.long()[live], tgt[live]])
    return d


def _reference(c, dtype):
    cast = (lambda t: t.to(dtype) if t.is_floating_point() else t)
    sd = {name: cast(t.detach().cpu()) for name, t in solver(c.tw, c.depth, *c.scales).state_dict().items()}
    d = graph(c)
    with torch.no_grad():
        out, hs = refcpu.mp_pde_solver(sd, oracle_pde(c), cast(d.u), cast(d.pos), d.edge_index,
                                       time_window=c.tw, hidden_layer=c.depth, return_hidden=True)
    return out, hs


@functools.lru_cache(maxsize=None)
def reference(c, dtype=torch.float64):
    """(out [n, tw], [h_0 .. h_depth]) of the oracle in `dtype`: h_0 the
    embedding, h_depth what the forward hands out as h_last."""
    return _reference(c, dtype)


def row_rel_err(h, h64):
    """(max, rms) over the rows of max_c |h - h64| / max_c |h64|."""
    h64 = h64.double()
    r = (h.detach().double().cpu() - h64).abs().amax(1) / h64.abs().amax(1)
    return r.max().item(), r.pow(2).mean().sqrt().item()


def out_rel_err(out, out64):
    """max|out - out64| / max|out64|."""
    out64 = out64.double()
    return (out.detach().double().cpu() - out64).abs().max().item() / out64.abs().max().item()
