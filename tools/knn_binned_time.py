"""Cell-binned against full kNN searches (profiling aid): hipEvent means of the
binned path (mmpde_knn_bin + the search; the binning alone too) alternated
with the full search (mmpde_knn_graph k = 35, mmpde_knn_query k = 30, one
query per source point) on s x s lattices moved by 0.1 h noise, one JSON line
per (s, B), every measurement twice.
    python tools/knn_binned_time.py [--parent-lib LIBMMPDE_HIP_SO] [--random] [--engine] [--reps R] s:B [s:B ...]
--parent-lib: the full search runs from another build of the library (the
parent commit's), bound here for those two entry points only; otherwise this
tree's method="full".  --random: s * s uniform random points instead of the
moved lattice.  --engine adds the 4500-point cylinder engine's time per step
at B = 4 with knn_binned off and on."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "mm-pde_amd"))
import torch  # noqa: E402

from mmpde_amd import _lib as L  # noqa: E402
from mmpde_amd import ops  # noqa: E402
from mmpde_amd.synth import build_models, burgers_grid_points, fields, generate_cy_mesh  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib")
ap.add_argument("--random", action="store_true")
ap.add_argument("--engine", action="store_true")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("shapes", nargs="*")
args = ap.parse_args()

parent = None
if args.parent_lib:
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name in ("mmpde_knn_graph", "mmpde_knn_query"):
        f = getattr(parent, name)
        f.restype, f.argtypes = L._SIGS[name]


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
    if args.random:
        pos, qry = torch.rand(B * n, 2, generator=gen).to(dev), torch.rand(B * n, 2, generator=gen).to(dev)
    else:
        pos = (grid.repeat(B, 1) + (0.1 / (s - 1)) * torch.randn(B * n, 2, generator=gen)).to(dev)
        qry = grid.repeat(B, 1).to(dev)
    ws = torch.empty((L.lib().mmpde_knn_bins_bytes(B, n),), dtype=torch.uint8, device=dev)
    nbr = torch.empty((B * n, 35), dtype=torch.int32, device=dev)
    idx = torch.empty((B * n, 30), dtype=torch.int32, device=dev)

    def full_graph():
        if parent is None:
            return ops.knn_graph_nbr(pos, B, 35)
        L.check(parent.mmpde_knn_graph(L.ptr(pos), B, n, 35, L.ptr(nbr), None, L.stream(dev)), "parent graph")
        return nbr

    def full_query():
        if parent is None:
            return ops.knn_query(pos, qry, B, 30)
        L.check(parent.mmpde_knn_query(L.ptr(pos), L.ptr(qry), B, n, n, 30, L.ptr(idx), None, L.stream(dev)),
                "parent query")
        return idx

    def binned_graph():
        return ops.knn_graph_nbr(pos, B, 35, method="binned", bins=ops.knn_bins(pos, B, out=ws))

    def binned_query():
        return ops.knn_query(pos, qry, B, 30, method="binned", bins=ops.knn_bins(pos, B, out=ws))

    st = torch.zeros((2,), dtype=torch.int64, device=dev)
    same_g = torch.equal(ops.knn_graph_nbr(pos, B, 35, method="binned", stats=st), full_graph())
    same_q = torch.equal(ops.knn_query(pos, qry, B, 30, method="binned", stats=st), full_query())
    rec = {"full": "parent" if parent is not None else "tree", "points": "random" if args.random else "lattice",
           "s": s, "n": n, "B": B, "reps": args.reps, "equal": bool(same_g and same_q),
           "examined_per_query": round(int(st[0].item()) / (2 * B * n), 1), "overflowed": int(st[1].item())}
    for rep in range(2):                                        # twice: the run-to-run spread
        rec[f"bin_us_{rep}"] = round(timed(lambda: ops.knn_bins(pos, B, out=ws), args.reps), 1)
        rec[f"graph_binned_us_{rep}"] = round(timed(binned_graph, args.reps), 1)
        rec[f"graph_full_us_{rep}"] = round(timed(full_graph, args.reps), 1)
        rec[f"query_binned_us_{rep}"] = round(timed(binned_query, args.reps), 1)
        rec[f"query_full_us_{rep}"] = round(timed(full_query, args.reps), 1)
    print(json.dumps(rec), flush=True)

if args.engine:
    from mmpde_amd.rollout import MMPDERollout

    B = 4
    pde, model, model_b, itp, dmm, gc = build_models("cy", grid=generate_cy_mesh(n=4500))
    u0 = fields(pde.ori_grid, B, 30)[:, 3].to(dev).contiguous()
    for m in (model, model_b, itp, dmm):
        m.to(dev)
    eng = MMPDERollout("cy", model, model_b, itp, dmm, gc, B, dev)
    rec = {"engine": "cy 4500 points", "B": B, "reps": args.reps}
    for rep in range(2):
        for on in (False, True):
            eng.knn_binned = on
            rec[f"step_us_binned_{'on' if on else 'off'}_{rep}"] = round(timed(lambda: eng.step(u0, 5), args.reps), 1)
    print(json.dumps(rec), flush=True)
