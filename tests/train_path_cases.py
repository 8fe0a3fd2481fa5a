"""Inputs, float64 references and judging of the GNN training kernels' shape
tests (test_gpu_edge_bwd_shapes.py and test_gpu_train_path_shapes.py on the
device, test_train_path_cases.py on the CPU alone): the edge backward and the
source sums of csrc/edge_bwd.hip, the Conv1d head of csrc/head_train.hip, and
the skinny weight gradient and the reverse adjacency of csrc/train_rows.hip,
at their tile, grid and list edges.

Float tensors travel as flat fp32 buffers: an input sits inside NaN, an output
inside SENT, and every float the call does not own must come back bitwise as
it was (the helpers of dense_cases.py where they fit).

Lattice inputs.  The backward kernels use the pre-activations only through
their signs, and a float32 sign that differs from the float64 one at |z| of a
rounding error moves a gradient by O(1e-3) of its scale.  So every operand
that feeds a ReLU is drawn from a dyadic lattice on which the pre-activation
is exact in float32 in any summation order (and through the fp16 hi + lo
split of the edge stage): edge a, b multiples of 2^-12 in [-1, 1], W2 and b2
multiples of 2^-3 in [-1, 1] (z2 a multiple of 2^-15 below 2^8: 23 bits); head
h multiples of 2^-6, its weights and biases multiples of 2^-3 (z1 a multiple
of 2^-9, z2 of 2^-12).  The incoming gradients stay real (randn).  Exact zeros
occur and are wanted: torch's ReLU gradient at 0 is 0 and the kernels test
`> 0`.  test_train_path_cases.py asserts the exactness for every case.
"""
import functools
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

import dense_cases as D

SENT, NAN = D.SENT, D.NAN
FRONT, BACK = 4, 8                       # floats of fence in front of / behind a contiguous tensor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mm-pde_amd", "csrc")
FALLBACK_GRID = 256                      # mmpde_gnn_edge_backward_partials without a device
H = 128


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def lattice(g, shape, bits):
    """Multiples of 2^-bits in [-1, 1]."""
    return torch.randint(-2 ** bits, 2 ** bits + 1, shape, generator=g).float() / 2.0 ** bits


def fenced_in(v, front=FRONT):
    flat = torch.full((front + v.numel() + BACK,), NAN, dtype=torch.float32)
    flat[front:front + v.numel()] = v.reshape(-1).float()
    return flat


def fenced_out(numel, front=FRONT):
    return torch.full((front + numel + BACK,), SENT, dtype=torch.float32)


def inside(flat, numel, front=FRONT):
    return flat[front:front + numel]


def fence_intact(flat, numel, front=FRONT, fill=SENT):
    """Every float outside [front, front + numel) is bitwise the fill."""
    want = torch.full_like(flat, fill).view(torch.int32)
    got = flat.view(torch.int32)
    return torch.equal(got[:front], want[:front]) and torch.equal(got[front + numel:], want[front + numel:])


def errs(got, ref):
    """(max, rms) of |got - ref|."""
    d = (got.double() - ref).abs()
    return (d.max().item(), d.pow(2).mean().sqrt().item()) if d.numel() else (0.0, 0.0)


# --------------------------------------------------------------------------- A. edge backward
EDGE_BAR = 2e-5                          # of max|ref|: the edge-stage bar of test_gpu_edge_shapes.py
BT, FT, FKMAX, STAGE_THREADS = 16, 32, 64, 512   # edge_bwd.hip: tile rows of the two kernels, slot limit
FIXED, RAGGED_LAST0, RAGGED_LASTK = 0, 1, 2
RAGGED_NAME = {FIXED: "fixed", RAGGED_LAST0: "ragged-last0", RAGGED_LASTK: "ragged-lastk"}
LIST_LENGTHS = (0, 1, 2, 31, 32, 33, 64, 65)     # in-degrees of the lists case, besides the hub

EDGE_TILE = [(1, 3), (15, 3), (16, 3), (17, 3), (31, 3), (32, 3), (33, 3)]
EDGE_FEW = [(144, 3)]                    # with (16, 3) and (33, 3): 1, 2, 3, 5 and 9 partials
EDGE_SLOTS = [(40, 1), (40, 2), (40, 16), (40, 17)]
EDGE_LIMIT = [(64, 63), (64, 64), (50, 65)]
EDGE_LISTS = (203, 9)


def edge_multi(grid):
    """More fp16x3 tiles than workgroups: some get two, others one; the last tile partial."""
    return [(32 * grid + 45, 3), (32 * grid + 45, 2)]


def edge_shapes(grid):
    """(n, k, lists) of every shape."""
    s = EDGE_TILE + EDGE_FEW + EDGE_SLOTS + EDGE_LIMIT + edge_multi(grid)
    return [(n, k, False) for n, k in s] + [EDGE_LISTS + (True,)]


EDGE_VARIANTS = {
    # variant -> (entry, edge_gemm, mask?) of each of its entry points
    "f32": [("backward", "f32", False), ("ex", "f32", False), ("sorted", "f32", False)],
    "f32+mask": [("sorted", "f32", True)],
    "f16x3": [("ex", "f16x3", False), ("sorted", "f16x3", False)],
    "f16x3+mask": [("sorted", "f16x3", True)],
}


def edge_variant_runs(variant, k):
    return variant in ("f32", "f16x3") or k <= FKMAX


def edge_deg(n, k, ragged, g):
    """Ragged: random degrees with a whole tile of zeros (32 rows from n = 64,
    16 rows below), a full row, and row n - 1 of degree 0 or k."""
    if ragged == FIXED:
        return torch.full((n,), k, dtype=torch.int32)
    deg = torch.randint(0, k + 1, (n,), generator=g, dtype=torch.int32)
    zero = range(32, 64) if n > 64 else range(0, 32) if n == 64 else range(16, 32) if n > 32 else \
        range(0, 16) if n > 16 else range(0)        # never row n - 1
    if n >= 3 and n - 2 not in zero:
        deg[n - 2] = k
    deg[list(zero)] = 0
    deg[n - 1] = 0 if ragged == RAGGED_LAST0 else k
    return deg


def _list_sources(n, k, live, g):
    """nbr of the lists case: source 7 is named by slot 0 of every row (the
    hub), sources 10 .. 16 by exactly 1, 2, 31, 32, 33, 64, 65 live slots,
    source 9 by none, every other slot by a source from 20 on."""
    nbr = torch.randint(20, n, (n, k), generator=g, dtype=torch.int32)
    nbr[:, 0] = 7
    free = torch.nonzero(live[:, 1:].reshape(-1)).reshape(-1)
    free = free[torch.randperm(free.numel(), generator=g)]
    at = 0
    flat = nbr[:, 1:].reshape(-1).clone()
    for j, length in enumerate(LIST_LENGTHS[1:]):
        flat[free[at:at + length]] = 10 + j
        at += length
    assert at <= free.numel()
    nbr[:, 1:] = flat.reshape(n, k - 1)
    return nbr


def _edge_forward(a, b, w2, b2, idx, live, deg):
    """The edge stage with z1 as a node of the graph: (z1, z2, mean)."""
    z1 = a[:, None, :] + b[idx]
    z2 = torch.relu(z1) @ w2.t() + b2
    m = torch.relu(z2) * live[..., None].to(a.dtype)
    return z1, z2, m.sum(1) / deg.clamp(min=1).to(a.dtype)[:, None]


def edge_grads(c, dtype):
    """mean, d/da, d/db, d/dW2, d/db2 and the per-edge rows d/dz1 [n k, 128] by autograd in dtype."""
    leaves = [c[x].to(dtype).clone().requires_grad_() for x in ("a", "b", "w2", "b2")]
    z1, z2, mean = _edge_forward(*leaves, c["nbr_alt"].long(), c["live"], c["deg"])
    z1.retain_grad()
    (mean * c["g"].to(dtype)).sum().backward()
    out = dict(mean=mean.detach(), z1=z1.detach(), z2=z2.detach(), gz1=z1.grad.reshape(-1, H))
    out.update({name: t.grad for name, t in zip(("ga", "gb", "gw2", "gb2"), leaves)})
    return out


def pack_mask(z2pos, live):
    """[n k][4] words (as int32 bits): bit c % 32 of word c / 32 where z2[c] > 0; padding slots all ones."""
    bits = z2pos.reshape(-1, 4, 32).numpy().astype(np.uint64)
    words = (bits << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    words[~live.reshape(-1).numpy()] = 0xFFFFFFFF
    return torch.from_numpy(words.view(np.int32).copy())


def reverse_lists(src, live, n_src):
    """The host construction of the reverse adjacency of slots q with sources
    src[q] (int64): (rev_off [n_src + 1], rev_edge [slots] -- the live slots by
    a stable sort on the source, then the dead ones ascending --, slot_pos)."""
    q_live = torch.nonzero(live).reshape(-1)
    order = torch.sort(src[q_live], stable=True).indices
    rev_edge = torch.cat([q_live[order], torch.nonzero(~live).reshape(-1)])
    counts = torch.bincount(src[q_live], minlength=n_src)
    rev_off = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    slot_pos = torch.empty(live.numel(), dtype=torch.int32)
    slot_pos[rev_edge] = torch.arange(live.numel(), dtype=torch.int32)
    return rev_off, rev_edge, slot_pos


@functools.lru_cache(maxsize=None)
def edge_case(n, k, ragged, lists=False):
    """One case, built once and never modified: lattice a, b, W2, b2, a real
    grad_mean g, the two nbr copies (padding -1 / arbitrary in-range), deg,
    the mask words of the float64 z2, the host reverse lists, the float64
    gradients (`ref`) and the float32 CPU evaluation (`cpu32`)."""
    g = torch.Generator().manual_seed(7_000_000 + 1000 * n + 10 * k + ragged + 5 * lists)
    c = dict(n=n, k=k, ragged=ragged, lists=lists,
             name=f"{n}x{k}-{RAGGED_NAME[ragged]}" + ("-lists" if lists else ""))
    c["a"], c["b"] = lattice(g, (n, H), 12), lattice(g, (n, H), 12)
    c["w2"], c["b2"] = lattice(g, (H, H), 3), lattice(g, (H,), 3)
    c["g"] = torch.randn(n, H, generator=g)
    c["deg"] = edge_deg(n, k, ragged, g)
    c["live"] = torch.arange(k)[None, :] < c["deg"][:, None]
    nbr = _list_sources(n, k, c["live"], g) if lists else torch.randint(0, n, (n, k), generator=g, dtype=torch.int32)
    c["nbr_alt"] = nbr
    c["nbr"] = nbr.clone()
    c["nbr"][~c["live"]] = -1
    c["ref"] = edge_grads(c, torch.float64)
    c["cpu32"] = edge_grads(c, torch.float32)
    c["mask"] = pack_mask(c["ref"]["z2"] > 0, c["live"])
    c["rev_off"], c["rev_edge"], c["slot_pos"] = reverse_lists(nbr.reshape(-1).long(), c["live"].reshape(-1), n)
    return c


def split_scale(mx):
    """f16x3.hpp split_scale."""
    eb = (np.float32(mx).view(np.uint32) >> 23) & 0xff
    if eb in (0, 255):
        return 1.0
    return 2.0 ** (min(max(267 - int(eb), 127 - 40), 127 + 40) - 127)


def edge_z2_split(c):
    """z2 in float32 as edge_bwd_f16_kernel forms it: relu(z1) scaled by the
    launch's power of two and split into fp16 hi + lo, both times W2 (whose
    lattice values are exact in fp16, so its lo plane is zero)."""
    z1 = c["a"][:, None, :] + c["b"][c["nbr_alt"].long()]
    sz = split_scale(c["a"].abs().max().item() + c["b"].abs().max().item())
    x = torch.relu(z1) * sz
    hi = x.half()
    lo = (x - hi.float()).half()
    assert torch.isfinite(hi).all() and torch.equal(hi.float() + lo.float(), x), "the split must be exact"
    assert torch.equal(c["w2"].half().float(), c["w2"])
    z2 = (hi.float() @ c["w2"].t() + lo.float() @ c["w2"].t()) / sz + c["b2"]
    return z2, int((lo != 0).sum()), lo.numel()


def edge_regime(n, k, grid):
    """What a shape makes the kernels do."""
    t16, t32 = -(-n // BT), -(-n // FT)
    return dict(g_f32=min(grid, t16), g_f16=min(grid, t32), tiles_f32=t16, tiles_f16=t32,
                stage_passes=-(-FT * k // STAGE_THREADS), f16_kernel=k <= FKMAX,
                maxabs_capped=-(-n * (H // 4) // 256) > 1024)


# --------------------------------------------------------------------------- B. head
HEAD_Y_BAR, HEAD_GRAD_BAR = 2e-5, 5e-5   # test_head_train_vs_fp64's
HEAD_N = (1, 63, 64, 65, 128, 4097)
HEAD_LD = ((128, 128), (132, 136), (256, 128))
HEAD_SHAPES = [(16, 4, 1), (4,), (12, 8, 4), (8,), (8, 8, 1), (1,)]     # w1 b1 w2 b2 w3 b3 (elements: K, Cout, Cin)
HEAD_LAYOUT = ("w1", "b1", "w2", "b2", "w3", "b3")                        # include/mmpde_hip.h: dW1 | db1 | ...
HEAD_SIZES = (64, 4, 384, 8, 64, 1)
HEAD_GRADS = 525


def head_table():
    """(n, ldh, lddh, tied): every n at (128, 128), the strided forms at n = 65
    and 4097, and one case with an all-zero h row and a zero b1 component."""
    t = [(n, 128, 128, False) for n in HEAD_N]
    t += [(n, ldh, lddh, False) for n in (65, 4097) for ldh, lddh in HEAD_LD[1:]]
    return t + [(65, 132, 136, True)]


def head_name(p):
    return f"n{p[0]}-ld{p[1]}x{p[2]}" + ("-tied" if p[3] else "")


def head_forward(h, w, dtype):
    """(z1, z2, y) of the Conv1d head in dtype; w in torch's layouts."""
    w1, b1, w2, b2, w3, b3 = (t.to(dtype) for t in w)
    z1 = F.conv1d(h.to(dtype)[:, None, :], w1, b1, stride=3)
    z2 = F.conv1d(torch.relu(z1), w2, b2, stride=3)
    y = F.conv1d(torch.relu(z2), w3, b3, stride=2)
    assert y.shape[1:] == (1, 1)
    return z1, z2, y.reshape(-1)


@functools.lru_cache(maxsize=None)
def head_case(n, ldh, lddh, tied):
    g = torch.Generator().manual_seed(8_000_000 + 10 * n + ldh + lddh + tied)
    c = dict(n=n, ldh=ldh, lddh=lddh, tied=tied, name=head_name((n, ldh, lddh, tied)))
    h = lattice(g, (n, H), 6)
    w = [lattice(g, s, 3) for s in ((4, 1, 16), (4,), (8, 4, 12), (8,), (1, 8, 8), (1,))]
    if tied:
        h[n // 2] = 0.0
        w[1][2] = 0.0                    # z1[n // 2, 2, :] = b1[2] = 0: a whole channel of the row ties
    c["h"], c["w"], c["dy"] = h, w, torch.randn(n, generator=g)
    b = D.Bufs(0)
    b.inp("h", h, ld=ldh)
    b.out("dh", n, H, ld=lddh)
    c["bufs"], c["at"] = b.t, b.at
    leaves = [h.double().requires_grad_()] + [t.double().requires_grad_() for t in w]
    z1, z2, y = head_forward(leaves[0], leaves[1:], torch.float64)
    (y * c["dy"].double()).sum().backward()
    c["ref"] = dict(z1=z1.detach(), z2=z2.detach(), y=y.detach(), dh=leaves[0].grad,
                    grads=torch.cat([t.grad.reshape(-1) for t in leaves[1:]]))
    return c


def head_parts(grads):
    """name -> the slice of the 525 gradients, by the header's layout."""
    out, o = {}, 0
    for name, size in zip(HEAD_LAYOUT, HEAD_SIZES):
        out[name] = grads[o:o + size]
        o += size
    assert o == HEAD_GRADS
    return out


# --------------------------------------------------------------------------- C. skinny weight gradient
RGW_BAR = 2e-5
RGW_CAP = 1280
COLS_K = (16, 20, 48, 64)
COLS_NOUT = (1, 2, 4, 8)
PART_K = (0, 1, 3, 4, 5, 8, 12, 16, 17, 20, 63, 64)
PART_NOUT = (1, 3, 16, 64, 65, 100, 128)


def cols_R(k):
    return 64 // (k // 4)


def cols_rows(k):
    r = cols_R(k)
    return (1, 4 * r - 1, 4 * r, 4 * r + 1, 16 * r + 1, 64 * r + 3)


def part_rows(n_out):
    rg = 256 // n_out
    return (1, max(rg - 1, 1), rg, rg + 1, 8 * rg + 1, 3 * 8 * rg + 1)


def rgw_route(k, n_out, ldx, x_front):
    """The instantiation mmpde_rows_grad_weight launches (train_rows.hip's dispatch)."""
    vec = k % 4 == 0 and ldx % 4 == 0 and x_front % 4 == 0
    if vec and 16 <= k <= 64 and k % 4 == 0 and n_out in (1, 2, 4, 8):
        return f"cols<{n_out}>"
    kb = 0 if k == 0 else 4 if k <= 4 else 16 if k <= 16 else 64
    return "partial<0>" if kb == 0 else f"partial<{kb},{'vec' if vec else 'scalar'}>"


RGW_ROUTES = [f"cols<{n}>" for n in COLS_NOUT] + ["partial<0>"] + \
    [f"partial<{kb},{v}>" for kb in (4, 16, 64) for v in ("vec", "scalar")]

# (k, n_out) of the partial kernel's cases; "odd" = an odd ldx
PART_PAIRS = [(0, 1), (0, 65), (0, 128), (1, 3), (1, 128), (3, 16), (3, 100), (4, 64), (4, 65), (4, 128), (4, 3),
              (5, 1), (5, 100), (5, 128), (8, 3), (8, 65), (8, 128), (9, 128), (12, 16), (12, 64), (16, 3),
              (16, 16), (16, 64), (16, 65), (17, 1), (17, 64), (19, 64), (20, 3), (20, 16), (63, 1), (63, 3),
              (63, 16), (64, 3), (64, 16)]


def rgw_table(cus):
    """dicts (k, n_out, rows, ldx, ldy, db, x_front) of every case."""
    t = []

    def add(k, n_out, rows, ldx_pad=0, ldy_pad=0, db=True, x_front=4, tag=""):
        p = dict(k=k, n_out=n_out, rows=rows, ldx=k + ldx_pad, ldy=n_out + ldy_pad, db=db, x_front=x_front)
        p["route"] = rgw_route(k, n_out, p["ldx"], x_front)
        p["name"] = f"k{k}-o{n_out}-r{rows}-ldx{p['ldx']}-ldy{p['ldy']}" + ("" if db else "-nodb") + \
            ("-xoff1" if x_front % 4 else "") + tag
        t.append(p)

    forms = [(lp, yp, db) for lp in (0, 4) for yp in (0, 3) for db in (True, False)]
    for ki, k in enumerate(COLS_K):
        for ni, n_out in enumerate(COLS_NOUT):
            i = 4 * ki + ni
            for j in (0, 3):
                lp, yp, db = forms[(2 * i + j) % 8]
                add(k, n_out, cols_rows(k)[(i + j) % 6], lp, yp, db)
        # the same shape with x one float off its alignment: the partial kernel
        add(k, COLS_NOUT[ki], cols_rows(k)[4], 0, 0, True)
        add(k, COLS_NOUT[ki], cols_rows(k)[4], 0, 0, True, x_front=5)
    seen = {}
    for i, (k, n_out) in enumerate(PART_PAIRS):
        odd = 1 if k == 20 else (i % 2) * (1 if k % 4 == 0 and k else 0)
        turn = seen[n_out] = seen.get(n_out, -1) + 1
        for j in ((0, 2, 4), (1, 3, 5))[turn % 2]:       # each n_out meets all six row counts
            add(k, n_out, part_rows(n_out)[j], odd + (4 if (i + j) % 3 == 0 and k else 0),
                3 if (i + j) % 2 else 0, True)
    add(10, 128, 17, db=False, tag="-cap")                      # k n_out = 1280 without the bias
    add(4, 128, 16 * 4 * cus + 17, tag="-blockcap")             # past the 4 CUs workgroups
    for k, n_out, ldx_pad in ((4, 16, 0), (16, 16, 0), (63, 3, 0), (5, 65, 2), (64, 16, 0), (17, 1, 0)):
        add(k, n_out, part_rows(n_out)[4], ldx_pad, 0, db=False)     # dw alone
    return t


def rgw_blocks(p, cus):
    """(G0, G) of the launch: the workgroups asked for and those with rows."""
    rows, k, n_out = p["rows"], p["k"], p["n_out"]
    per_block = 32 * cols_R(k) if p["route"].startswith("cols") else (256 // n_out) * 8
    g0 = max(1, min(4 * cus, -(-rows // per_block)))
    per = -(-rows // g0)
    return g0, -(-rows // per)


@functools.lru_cache(maxsize=None)
def rgw_case(key):
    p = dict(key)
    shape_name = p["name"].replace("-xoff1", "")          # the offset twin of a case holds the same values
    g = torch.Generator().manual_seed(9_000_000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(shape_name)))
    rows, k, n_out = p["rows"], p["k"], p["n_out"]
    x = torch.randn(rows, max(k, 1), generator=g)[:, :k]
    dy = torch.randn(rows, n_out, generator=g)
    b = D.Bufs(0)
    if k:
        b.inp("x", x, ld=p["ldx"], front=p["x_front"])
        b.out("dw", n_out, k)
    b.inp("dy", dy, ld=p["ldy"])
    if p["db"]:
        b.out("db", 1, n_out)
    c = dict(p, bufs=b.t, at=b.at, x=x, dy=dy)
    c["ref"] = dict(dw=dy.double().t() @ x.double(), db=dy.double().sum(0))
    c["cpu32"] = dict(dw=(dy.t() @ x).double(), db=dy.sum(0).double())
    return c


def rgw_key(p):
    return tuple(sorted(p.items()))


# --------------------------------------------------------------------------- C. reverse adjacency
INT_SENT = -7777
# (name, n_tgt, k, n_src, pattern); patterns: "mixed" (ragged deg, a few live entries out of range),
# "dead" (all degrees 0), "one" (every slot names source 5 or 0, deg NULL), "inner" (sources 0 and n_src - 1 never)
REV = [("src1", 300, 3, 1, "mixed"), ("src2", 300, 3, 2, "mixed"), ("src255", 255, 3, 255, "mixed"),
       ("src256", 256, 3, 256, "mixed"), ("src257", 257, 3, 257, "mixed"),
       ("src65535", 10000, 7, 65535, "mixed"), ("src65536", 10000, 7, 65536, "mixed"),
       ("src65537", 10000, 7, 65537, "mixed"),
       ("tgt1000-src7", 1000, 1, 7, "mixed"), ("tgt3-src70000", 3, 5, 70000, "mixed"),
       ("slots255", 255, 1, 40, "mixed"), ("slots256", 64, 4, 40, "mixed"), ("slots257", 257, 1, 40, "mixed"),
       ("all-dead", 100, 4, 256, "dead"), ("one-source", 70, 5, 9, "one"), ("one-group", 33, 3, 1, "one"),
       ("inner-sources", 200, 6, 256, "inner"), ("src256-full", 256, 2, 256, "inner")]


@functools.lru_cache(maxsize=None)
def rev_case(idx):
    name, n_tgt, k, n_src, pattern = REV[idx]
    g = torch.Generator().manual_seed(9_500_000 + idx)
    slots = n_tgt * k
    c = dict(name=name, n_tgt=n_tgt, k=k, n_src=n_src, pattern=pattern, slots=slots)
    lo, hi = (1, n_src - 1) if pattern == "inner" else (0, n_src)
    nbr = torch.randint(lo, hi, (n_tgt, k), generator=g, dtype=torch.int32)
    deg = torch.randint(0, k + 1, (n_tgt,), generator=g, dtype=torch.int32)
    if pattern == "dead":
        deg.zero_()
    if pattern == "one":
        nbr.fill_(min(5, n_src - 1))
        deg = None
    live = (torch.arange(k)[None, :] < deg[:, None]) if deg is not None else torch.ones(n_tgt, k, dtype=torch.bool)
    if pattern in ("mixed", "dead"):
        # dead slots hold anything (never read); a few live ones are out of range and counted
        junk = torch.tensor([-1, n_src, n_src + 5, -2 ** 31, 2 ** 31 - 1, 0], dtype=torch.int64)
        pick = torch.randint(0, junk.numel(), (n_tgt, k), generator=g)
        nbr = torch.where(live, nbr, junk[pick].to(torch.int32))
        if pattern == "mixed":
            q = torch.nonzero(live.reshape(-1)).reshape(-1)
            bad = q[torch.randperm(q.numel(), generator=g)[:min(5, q.numel() // 4)]]
            flat = nbr.reshape(-1)
            flat[bad] = junk[torch.arange(bad.numel()) % 5].to(torch.int32)
    c["nbr"], c["deg"], c["live"] = nbr, deg, live
    flat, lv = nbr.reshape(-1).long(), live.reshape(-1)
    ok = lv & (flat >= 0) & (flat < n_src)
    c["bad"] = int((lv & ~ok).sum())
    c["rev_off"], c["rev_edge"], c["slot_pos"] = reverse_lists(flat.clamp(0, n_src - 1), ok, n_src)
    c["n_live"] = int(ok.sum())
    return c


def key_bits(n_src):
    """train_rows.hip key_bits: the radix passes cover keys 0 .. n_src."""
    b = 1
    while b < 31 and (1 << b) <= n_src:
        b += 1
    return b


# --------------------------------------------------------------------------- source predicates
def require_lines(text, entry):
    """The MMPDE_REQUIRE conditions inside the definition of entry point `entry`."""
    m = re.search(r'extern "C" \w+ ' + re.escape(entry) + r"\(", text)
    assert m, entry
    body = text[m.end():]
    end = re.search(r"^}", body, re.M).start()
    return re.findall(r"MMPDE_REQUIRE\((.*?)\);", body[:end], re.S)
