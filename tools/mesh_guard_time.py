"""The fold guard's cost (profiling aid): the relax entry alone and the rollout
step with the guard off, with the monitor (mesh_check) and with the guard
(mesh_guard = 0.1), on unguarded data (the synthetic models as they are) and on
guarded data (the DMM head scaled until the mesh folds: w_o x 64, branch half x
8).  hipEvent means over R calls after a warm-up, the variants alternated in one
process, every measurement three times (the run-to-run spread), one JSON line
per data set.
    python tools/mesh_guard_time.py [--reps R] [--out FILE]
Shape: the cylinder DMM (graph mode) at B = 16, N = 2521.  relax_*: ops.mesh_relax
on the engine's own buffers (mesh, Hess phi), with every output the rollout
asks for; mesh_hess / mesh_guarded: the DMM stage's two calls.  --out appends
the lines to FILE."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "mm-pde_amd"))
import torch  # noqa: E402

from mmpde_amd import ops  # noqa: E402
from mmpde_amd.rollout import MMPDERollout  # noqa: E402
from mmpde_amd.synth import build_models, fields  # noqa: E402

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
B, FLOOR = 16, 0.1
for data, scale in (("unguarded", None), ("guarded", (64.0, 8.0))):
    pde, model, model_b, itp, dmm, gc = build_models("cy")
    if scale is not None:
        lat = dmm.trunk.layers[1].out_features
        with torch.no_grad():
            dmm.out_nn.layers[1].weight.mul_(scale[0])
            dmm.out_nn.layers[0].weight[:, :lat].mul_(scale[1])
    u0 = fields(pde.ori_grid, B, 30)[:, 3].to(dev).contiguous()
    for m in (model, model_b, itp, dmm):
        m.to(dev)
    engs = {k: MMPDERollout("cy", model, model_b, itp, dmm, gc, B, dev) for k in ("off", "check", "guard")}
    engs["check"].mesh_check = True
    engs["guard"].mesh_guard = FLOOR
    for e in engs.values():
        e.step(u0, 5)            # tables, workspaces and buffers
    g = engs["guard"]
    xi, N = g.xi, g.N
    full = g.mesh.clone()        # relax works in place: every timed call starts from some mesh; the cost does not depend on it
    hess_kw = dict(out=g.mesh, hess_out=g.mesh_hess, det_out=g.mesh_det, detmin_out=g.mesh_detmin,
                   folds_out=g.mesh_folds, workspace=g.ws_dmm_hess, head_cache=g.dmm_cache, hess_cache=g.hess_cache)
    relax_kw = dict(alpha_out=g.mesh_alpha_b, lam_out=g.mesh_lam, det_out=g.mesh_det_after,
                    detmin_out=g.mesh_detmin_after, folds_out=g.mesh_folds_after,
                    guarded_total=g.mesh_guarded_total)
    calls = {
        "mesh_hess": lambda: dmm.mesh_hess(u0, xi, **hess_kw),
        "mesh_guarded": lambda: dmm.mesh_guarded(
            u0, xi, floor=FLOOR, out=g.mesh, hess_out=g.mesh_hess, workspace=g.ws_dmm_hess,
            head_cache=g.dmm_cache, hess_cache=g.hess_cache, det_before_out=g.mesh_det,
            detmin_before_out=g.mesh_detmin, folds_before_out=g.mesh_folds, **relax_kw),
        "relax_guard": lambda: ops.mesh_relax(full, xi, g.mesh_hess, batches=B, floor=FLOOR, **relax_kw),
        "relax_plain_half": lambda: ops.mesh_relax(full, xi, batches=B, alpha=0.5, alpha_out=g.mesh_alpha_b),
        "relax_plain_one": lambda: ops.mesh_relax(full, xi, batches=B, alpha=1.0, alpha_out=g.mesh_alpha_b),
    }
    rec = {"data": data, "kind": "cy", "B": B, "N": N, "reps": args.reps, "floor": FLOOR}
    for rep in range(3):
        for name, fn in calls.items():
            rec[f"{name}_us_{rep}"] = round(timed(fn, args.reps), 1)
    for rep in range(3):
        for k, e in engs.items():
            rec[f"step_us_{k}_{rep}"] = round(timed(lambda: e.step(u0, 5), args.reps), 1)
    g.step(u0, 5)
    rep_ = g.mesh_report()
    rec.update(folds=rep_["folds"], folds_after=rep_["folds_after"], alpha=[round(a, 4) for a in rep_["alpha"]])
    emit(rec)
    del engs, g
