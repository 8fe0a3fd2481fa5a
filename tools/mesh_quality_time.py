"""The mesh-quality stage's cost (profiling aid): the rollout step with
mesh_quality off and on, and the stage's two calls alone (ops.mesh_monitor,
ops.mesh_quality on the engine's own buffers), for the cylinder at B = 16
(5022 Delaunay triangles, 50 x 50 monitor lattice) and Burgers at B = 32 (2209
quadrilaterals, 48 x 48).  hipEvent means over R calls after a warm-up, the two
engines alternated in one process, every measurement three times (the
run-to-run spread), one JSON line per engine kind.
    python tools/mesh_quality_time.py [--reps R] [--out FILE]
--out appends the lines to FILE."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "mm-pde_amd"))
import torch  # noqa: E402

from mmpde_amd import ops  # noqa: E402
from mmpde_amd.rollout import MMPDERollout  # noqa: E402
from mmpde_amd.synth import build_models, burgers_grid_points, fields  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out")
args = ap.parse_args()


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


dev = torch.device("cuda:0")
for kind, B in (("cy", 16), ("burgers", 32)):
    pde, model, model_b, itp, dmm, gc = build_models(kind)
    if kind == "cy":
        u0 = fields(pde.ori_grid, B, 30)[:, 3]
    else:
        u0 = fields(burgers_grid_points(), B, 31).reshape(B, 31, 48, 48)[:, 3]
    u0 = u0.to(dev).contiguous()
    for m in (model, model_b, itp, dmm):
        m.to(dev)
    model.edge_gemm = model_b.edge_gemm = "f16x3"    # the benchmark's edge arithmetic (bench.py --edge-gemm)
    engs = {k: MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev)
            for k in ("off", "on", "graph_off", "graph_on")}
    engs["on"].mesh_quality = engs["graph_on"].mesh_quality = True
    for k, e in engs.items():
        # tables, workspaces and buffers; the kNN table policy's read-back of the
        # first step is consumed by the second (it cannot be queried inside a capture)
        e.step(u0, 5)
        torch.cuda.synchronize()
        e.step(u0, 5)
        if k.startswith("graph"):
            e.enable_graph(u0)
    gengs = {k[6:]: engs.pop(k) for k in ("graph_off", "graph_on")}
    e = engs["on"]
    q = e.mesh_q
    mon = (q.m, q.alpha, q.rhs)
    if kind == "cy":
        u2 = u0.reshape(B, e.N)
        calls = {"monitor": lambda: ops.mesh_monitor(u2, e.grid, out=mon, scratch=q.scratch)}
    else:
        calls = {"monitor": lambda: ops.mesh_monitor(u0, out=mon)}
    outs = (q.mean, q.std, q.range, q.inverted, q.area_ratio_min)
    calls["cells"] = lambda: ops.mesh_quality(e.mesh, e.xi, q.cells, q.m, B, out=outs, workspace=q.ws)
    rec = {"kind": kind, "B": B, "N": e.N, "cells": q.cells.n_cells, "n": q.n, "reps": args.reps}
    for rep in range(3):
        for name, fn in calls.items():
            rec[f"{name}_us_{rep}"] = round(timed(fn, args.reps), 1)
    for rep in range(3):
        for k, eng in engs.items():
            rec[f"step_us_{k}_{rep}"] = round(timed(lambda: eng.step(u0, 5), args.reps), 1)
    # the same two steps as hipGraph replays (enable_graph / graph_step): the eager
    # step is bound by the host's launches, the replay by the device
    for rep in range(3):
        for k, eng in gengs.items():
            rec[f"graph_step_us_{k}_{rep}"] = round(timed(lambda: eng.graph_step(u0, 5), args.reps), 1)
    r = e.mesh_quality_report()
    rec.update(mean=[round(x, 6) for x in r["mean"][:2]], inverted=r["inverted"][:2])
    emit(rec)
    del engs, gengs, e, q
