"""Full kNN searches on large trajectories (profiling aid): hipEvent means of
mmpde_knn_graph (k = 35) and mmpde_knn_query (k = 30, one query per source
point) on s x s Burgers lattices, one JSON line per (s, B).  s = 128 is the
largest set knn_large_kernel takes; above it the tiled kernel runs, whose
yardstick is the 128 x 128 time scaled by (n / 16384)^2.
    python tools/knn_tiled_time.py [--lib OTHER_LIBMMPDE_HIP_SO] [--random] [--gnn] [--reps R] s:B [s:B ...]
--lib times another build of the library (e.g. the parent commit's) through
the same bindings; --random takes s * s uniform random points instead of the
lattice (no query overflows its candidate list: the two passes alone); --gnn
adds the 192 x 192 GNN-only forward (B = 1)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "mm-pde_amd"))
import torch  # noqa: E402

from mmpde_amd import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib")
ap.add_argument("--random", action="store_true")
ap.add_argument("--gnn", action="store_true")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("shapes", nargs="*")
args = ap.parse_args()
if args.lib:
    L.LIB_PATH = os.path.abspath(args.lib)

from mmpde_amd import ops  # noqa: E402
from mmpde_amd.synth import build_models, burgers_grid_points, fields  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


dev = torch.device("cuda:0")
for shape in args.shapes:
    s, B = (int(x) for x in shape.split(":"))
    grid = burgers_grid_points(s)
    n = grid.shape[0]
    gen = torch.Generator().manual_seed(s)
    # every trajectory a differently moved lattice, queried from the fixed one
    if args.random:
        pos, qry = torch.rand(B * n, 2, generator=gen).to(dev), torch.rand(B * n, 2, generator=gen).to(dev)
    else:
        pos = (grid.repeat(B, 1) + (0.1 / s) * torch.randn(B * n, 2, generator=gen)).to(dev)
        qry = grid.repeat(B, 1).to(dev)
    rec = {"lib": args.lib or "tree", "points": "random" if args.random else "lattice", "s": s, "n": n,
           "B": B, "reps": args.reps}
    for rep in range(2):                                        # twice: the run-to-run spread
        rec[f"graph_us_{rep}"] = round(timed(lambda: ops.knn_graph_nbr(pos, B, 35), args.reps), 1)
        rec[f"query_us_{rep}"] = round(timed(lambda: ops.knn_query(pos, qry, B, 30), args.reps), 1)
    print(json.dumps(rec), flush=True)

if args.gnn:
    pde, model, _, _, _, gc = build_models("burgers", moving_mesh=False, seed=4)
    res = [31, 192, 192]
    pde.grid_size = pde.movingmesh_grid_size = pde.ori_grid_size = res
    u = fields(burgers_grid_points(192), 1, 31, seed=5).reshape(1, 31, 192, 192)
    data, labels = gc.create_data(u, [7])
    model.to(dev)
    graph = gc.create_graph(None, data, labels, [7], dev, None)
    with torch.no_grad():
        t = timed(lambda: model(graph), 5)
    print(json.dumps({"gnn_forward_192x192_B1_us": round(t, 1)}), flush=True)
