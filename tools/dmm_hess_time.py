"""DMM.mesh against DMM.mesh_hess, and the rollout step with the fold monitor
off and on (profiling aid): hipEvent means over R calls after a warm-up, the
variants alternated in one process, every measurement twice (the run-to-run
spread), one JSON line per shape.
    python tools/dmm_hess_time.py [--reps R] [--out FILE]
Shapes: the cylinder DMM (graph mode) at B = 16, N = 2521 and the Burgers DMM
(array mode) at B = 32, 48 x 48; each with both caches (the rollout's call) and
with none (the grid side recomputed inside the call).  The step: the same two
engines' MMPDERollout.step with mesh_check off and on.  --out appends the lines
to FILE."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "mm-pde_amd"))
import torch  # noqa: E402

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
        u0 = fields(pde.ori_grid, B, 30)[:, 3].to(dev).contiguous()
    else:
        u0 = fields(burgers_grid_points(), B, 31).reshape(B, 31, 48, 48)[:, 3].to(dev).contiguous()
    for m in (model, model_b, itp, dmm):
        m.to(dev)
    engs = {False: MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev),
            True: MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev)}
    engs[True].mesh_check = True
    eng = engs[True]
    eng.step(u0, 5)          # builds the monitor's table, workspace and buffers
    xi, N = eng.xi, eng.N
    hc, kc, ws = eng.dmm_cache, eng.hess_cache, eng.ws_dmm_hess
    out = dict(out=eng.mesh, hess_out=eng.mesh_hess, det_out=eng.mesh_det, detmin_out=eng.mesh_detmin,
               folds_out=eng.mesh_folds, workspace=ws)
    calls = {
        "mesh_cached": lambda: dmm.mesh(u0, xi, out=eng.mesh, workspace=ws, head_cache=hc),
        "mesh_hess_cached": lambda: dmm.mesh_hess(u0, xi, head_cache=hc, hess_cache=kc, **out),
        "mesh_nocache": lambda: dmm.mesh(u0, xi, out=eng.mesh, workspace=ws),
        "mesh_hess_nocache": lambda: dmm.mesh_hess(u0, xi, **out),
    }
    rec = {"kind": kind, "B": B, "N": N, "reps": args.reps,
           "cache_MB": {"Q_J": round(hc.numel() * 4 / 1e6, 1), "K": round(kc.numel() * 4 / 1e6, 1)}}
    for rep in range(2):
        for name, fn in calls.items():
            rec[f"{name}_us_{rep}"] = round(timed(fn, args.reps), 1)
    for rep in range(3):
        for on in (False, True):
            rec[f"step_us_check_{'on' if on else 'off'}_{rep}"] = round(
                timed(lambda: engs[on].step(u0, 5), args.reps), 1)
    rec["folds"] = eng.mesh_report()["folds"]
    emit(rec)
    del engs, eng
