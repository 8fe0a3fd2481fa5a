"""Wall time of one per-epoch mesh evaluation of DMM training --
dmm_train.evaluate (burgers, 48 x 48 fields) and evaluate_tri (cy, the
2521-point mesh) -- on the per-field route (batch=None: one model call, a few
dozen torch launches and three host reads per field) and on the batched route
(batch=K: DMM.mesh_fields, ops.mesh_monitor, ops.mesh_quality per K fields, one
host read per call).  The per-field route is bound by the host, so the figure is
the host clock around a device synchronise, not device events.  Routes
alternated in one process, each measured twice after one warm-up call;
build_models weights, synthetic fields, the model in train() mode (as the
training loop leaves it).  One JSON line per (kind, fields, K): ms per call and
per field of both routes, and the peak device memory the batched call allocates
above what is resident before it.
    python tools/dmm_eval_time.py [--kinds burgers,cy] [--out FILE]
--out appends the lines to FILE (default profiles/dmm_eval_times.txt)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "mm-pde_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmpde_amd import dmm_train as T  # noqa: E402
from mmpde_amd.synth import build_models, burgers_grid_points, fields  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kinds", default="burgers,cy")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dmm_eval_times.txt"))
args = ap.parse_args()

# kind -> [(fields, (K, ...))]
CONFIGS = {"burgers": [(160, (32, 160)), (640, (32, 160))], "cy": [(150, (10, 50))]}


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


dev = torch.device("cuda:0")
for kind in args.kinds.split(","):
    pde, _, _, _, dmm, _ = build_models(kind, seed=3)
    dmm.to(dev).train()
    for F, batches in CONFIGS[kind]:
        if kind == "cy":
            u = fields(pde.ori_grid, 1, F, seed=5)[0].float().to(dev)            # [F, N]
            grid = pde.ori_grid.float()

            def call(batch):
                np.random.seed(3)
                return T.evaluate_tri(dmm, u, grid, dev, batch=batch)
        else:
            u = fields(burgers_grid_points(), 1, F, seed=5)[0].reshape(F, 48, 48).float().to(dev)

            def call(batch):
                np.random.seed(3)
                return T.evaluate(dmm, u, dev, batch=batch)

        routes = (None,) + tuple(batches)
        ms = {r: [] for r in routes}
        value = {}
        for r in routes:                                  # warm-up: kernels loaded, lattices and tables built
            value[r] = call(r)
        for _ in range(2):
            for r in routes:
                ms[r].append(wall_ms(lambda: call(r))[0])
        for K in batches:
            rec = {"kind": kind, "fields": F, "K": K, "points": int(u[0].numel()),
                   "per_field_ms_per_call": [round(v, 2) for v in ms[None]],
                   "per_field_ms_per_field": [round(v / F, 4) for v in ms[None]],
                   "batched_ms_per_call": [round(v, 2) for v in ms[K]],
                   "batched_ms_per_field": [round(v / F, 4) for v in ms[K]],
                   "speedup": round(min(ms[None]) / min(ms[K]), 1),
                   "batched_peak_MB": round(peak_mb(lambda: call(K)), 1),
                   "per_field_value": value[None], "batched_value": value[K]}
            emit(rec)
        del u
        torch.cuda.empty_cache()
    del dmm
