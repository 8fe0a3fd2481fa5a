"""Dump GNN outputs to a file, to compare two library builds bit for bit
(profiling aid): one forward (cy, B=16, f16x3 and f32), the edge stage
mmpde_gnn_edge_mean_ex in its four variants (F32, F32 + mask, F16X3 + mask,
F16X3 without mask: wave kernel + edge_finish_kernel), fixed-degree and ragged,
at a partial tile, a last partial round, k past the 36-slot unroll and several
tiles per workgroup (means and mask words), and one small forward with two
trajectory segments and ragged degrees (the node stage's side-block path).
    python tools/gnn_out_dump.py OUT.pt [--lib PATH/libmmpde_hip.so]
--lib loads another build of the library (same ABI) instead of the tree's;
compare two dumps with torch.equal on every tensor."""
import argparse
import math
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "mm-pde_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch  # noqa: E402

from mmpde_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("out")
ap.add_argument("--lib", help="libmmpde_hip.so to load instead of the tree's")
args = ap.parse_args()
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)  # before the first call loads it

from mmpde_amd.gnn_2d import EdgeGraph, _edge_mean_fwd  # noqa: E402
from mmpde_amd.rollout import _Nodes  # noqa: E402
from mmpde_amd.synth import build_models  # noqa: E402
from oracle import refcpu  # noqa: E402

dev = torch.device("cuda:0")
outs = {}

# ---- the full forward
pde, model, _, _, _, gc = build_models("cy", moving_mesh=False, seed=0)
B = 16
pts = pde.ori_grid
n = B * pts.shape[0]
torch.manual_seed(7)
pos = torch.cat((torch.full((n, 1), float(gc.time_grid()[5])), pts.repeat(B, 1)), 1)
u = torch.randn(n, 1)
_, nbr, _ = refcpu.knn_graph(pts.repeat(B, 1), 35, B)
model.to(dev)
for mode in ("f16x3", "f32"):
    model.edge_gemm = mode
    outs[mode] = model(_Nodes(u.to(dev), pos.to(dev), nbr.int().to(dev), seg_n=pts.shape[0])).cpu()


# ---- the edge stage alone
def edge_inputs(n, k, ragged, seed):
    """The inputs of tests/test_gpu_edge_shapes.py (_inputs, _pad): padding entries are -1."""
    g = torch.Generator().manual_seed(seed)
    a = 0.5 * torch.randn(n, 128, generator=g)
    b = 0.5 * torch.randn(n, 128, generator=g)
    w2 = torch.randn(128, 128, generator=g) / math.sqrt(128)
    b2 = 0.1 * torch.randn(128, generator=g)
    nbr = torch.randint(0, n, (n, k), generator=g, dtype=torch.int32)
    if ragged:
        deg = torch.randint(0, k + 1, (n,), generator=g, dtype=torch.int32)
        deg[:3] = 0
        if n >= 32:
            deg[16:32] = 0
        deg[3] = k
    else:
        deg = torch.full((n,), k, dtype=torch.int32)
    nbr[torch.arange(k)[None, :] >= deg[:, None]] = -1
    return dict(a=a, b=b, w2=w2, b2=b2, nbr=nbr, deg=deg)


EDGE_SHAPES = [(17, 5), (37, 35), (100, 37), (203, 9)]
EDGE_VARIANTS = [("f32", "f32", False), ("f32+mask", "f32", True), ("f16x3+mask", "f16x3", True),
                 ("f16x3-wave", "f16x3", False)]
for (en, ek) in EDGE_SHAPES:
    for ragged in (False, True):
        c = edge_inputs(en, ek, ragged, 1000 * en + 10 * ek + ragged)
        a, b, w2, b2 = (c[x].to(dev) for x in ("a", "b", "w2", "b2"))
        graph = EdgeGraph(c["nbr"].to(dev), c["deg"].to(dev) if ragged else None)
        for name, mode, keep in EDGE_VARIANTS:
            mean, mask = _edge_mean_fwd(a, b, w2, b2, graph, mode, keep_mask=keep)
            assert (mask is not None) == keep
            tag = f"edge/{name}/{en}x{ek}/{'ragged' if ragged else 'fixed'}"
            outs[tag + "/mean"] = mean.cpu()
            if keep:
                outs[tag + "/mask"] = mask.cpu()

# ---- two segments smaller than n, ragged degrees: the node stage adds side
# blocks (f16x3) per segment and divides by the degrees
seg, nseg, k = 37, 2, 35
n = seg * nseg
g = torch.Generator().manual_seed(11)
spts = pts[:seg]
pos = torch.cat((torch.full((n, 1), float(gc.time_grid()[5])), spts.repeat(nseg, 1)), 1)
u = torch.randn(n, 1, generator=g)
nbr = (torch.randint(0, seg, (n, k), generator=g) + seg * (torch.arange(n) // seg)[:, None]).int()
deg = torch.randint(0, k + 1, (n,), generator=g, dtype=torch.int32)
deg[:3] = 0
deg[3] = k
for mode in ("f16x3", "f32"):
    model.edge_gemm = mode
    data = SimpleNamespace(x=u.to(dev), pos=pos.to(dev), nbr=nbr.to(dev), deg=deg.to(dev), edge_index=None,
                           seg_n=seg)
    outs[f"segments/{mode}"] = model(data).cpu()

torch.save(outs, args.out)
print("saved", len(outs), "tensors;", {k: float(v.abs().sum()) for k, v in outs.items() if "/" not in k})
