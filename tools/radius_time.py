"""Cell-binned against index-order radius graphs (profiling aid): hipEvent means
of mmpde_radius_graph_binned (with mmpde_knn_bin in the timed call, and with
the bins given; the binning alone too) alternated with mmpde_radius_graph in
one process, one JSON line per (s, B, points, neighbors), every measurement
twice.  The scan kernel is the same in either build, so one build serves both.
    python tools/radius_time.py [--reps R] [--engine] [--out FILE] [s:B ...]
Points: an s x s lattice, each trajectory moved by 0.1 h noise, and s * s
uniform random points.  r follows the reference rule (data_creator_2d.py:195):
neighbors * sqrt(dx^2 + dy^2) + 1e-4 of the side's linspace, for neighbors = 2
and, at every shape once, neighbors = 35 (the reference's default: the radius
covers the domain, every query takes the binned entry's fallback).
--engine adds step times (hipEvents around R steps after 5): the cylinder
rollout at B = 16 with connect_edge 'radius' (neighbors = 2) next to the
kNN-35 step of the same construction, and the 4500-point cylinder mesh at
B = 4 with radius_binned off and on.  --out appends the lines to FILE."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "mm-pde_amd"))
import torch  # noqa: E402

from mmpde_amd import _lib as L  # noqa: E402
from mmpde_amd import ops  # noqa: E402
from mmpde_amd.synth import build_models, burgers_grid_points, fields, generate_cy_mesh  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--engine", action="store_true")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out")
ap.add_argument("shapes", nargs="*")
args = ap.parse_args()


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def reference_r(s, neighbors):
    x = torch.linspace(0, 1, s)
    dx = x[1] - x[0]
    return float(neighbors * torch.sqrt(dx ** 2 + dx ** 2) + 0.0001)


dev = torch.device("cuda:0")
for shape in args.shapes:
    s, B = (int(x) for x in shape.split(":"))
    grid = burgers_grid_points(s)
    n = grid.shape[0]
    gen = torch.Generator().manual_seed(s)
    sets = {"lattice": (grid.repeat(B, 1) + (0.1 / (s - 1)) * torch.randn(B * n, 2, generator=gen)).to(dev),
            "random": torch.rand(B * n, 2, generator=gen).to(dev)}
    ws = torch.empty((L.lib().mmpde_knn_bins_bytes(B, n),), dtype=torch.uint8, device=dev)
    for points, neighbors in (("lattice", 2), ("random", 2), ("lattice", 35)):
        pos, r = sets[points], reference_r(s, neighbors)

        def scan():
            return ops.radius_graph_nbr(pos, B, r, 32)

        def binned():
            return ops.radius_graph_nbr(pos, B, r, 32, method="binned", bins=ops.knn_bins(pos, B, out=ws))

        def binned_given():
            return ops.radius_graph_nbr(pos, B, r, 32, method="binned", bins=ws)

        st = torch.zeros((2,), dtype=torch.int64, device=dev)
        got = ops.radius_graph_nbr(pos, B, r, 32, method="binned", stats=st)
        want = scan()
        rec = {"points": points, "neighbors": neighbors, "s": s, "n": n, "B": B, "reps": args.reps,
               "equal": bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])),
               "mean_degree": round(want[1].float().mean().item(), 1),
               "examined_per_query": round(int(st[0].item()) / (B * n), 1),
               "scan_share": round(int(st[1].item()) / (B * n), 3)}
        for rep in range(2):                                        # twice: the run-to-run spread
            rec[f"bin_us_{rep}"] = round(timed(lambda: ops.knn_bins(pos, B, out=ws), args.reps), 1)
            rec[f"binned_us_{rep}"] = round(timed(binned, args.reps), 1)
            rec[f"scan_us_{rep}"] = round(timed(scan, args.reps), 1)
            rec[f"binned_given_bins_us_{rep}"] = round(timed(binned_given, args.reps), 1)
        emit(rec)

if args.engine:
    from mmpde_amd.rollout import MMPDERollout

    def engine(B, grid, edge, neighbors):
        pde, model, model_b, itp, dmm, gc = build_models("cy", grid=grid)
        gc.e, gc.n = edge, neighbors
        u0 = fields(pde.ori_grid, B, 30)[:, 3].to(dev).contiguous()
        for m in (model, model_b, itp, dmm):
            m.to(dev)
        return MMPDERollout("cy", model, model_b, itp, dmm, gc, B, dev), u0

    rec = {"engine": "cy 2521 points", "B": 16, "reps": args.reps}
    engs = {"radius_2": engine(16, None, "radius", 2), "knn_35": engine(16, None, "knn", 35)}
    for rep in range(2):
        for name, (eng, u0) in engs.items():
            rec[f"step_us_{name}_{rep}"] = round(timed(lambda: eng.step(u0, 5), args.reps, warm=5), 1)
    rec["modes_radius_2"] = engs["radius_2"][0].knn_modes()
    emit(rec)
    del engs

    eng, u0 = engine(4, generate_cy_mesh(n=4500), "radius", 2)
    rec = {"engine": "cy 4500 points, radius neighbors = 2", "B": 4, "reps": args.reps}
    for rep in range(2):
        for on in (False, True):
            eng.radius_binned = on
            rec[f"step_us_radius_binned_{'on' if on else 'off'}_{rep}"] = round(
                timed(lambda: eng.step(u0, 5), args.reps, warm=5), 1)
    emit(rec)
