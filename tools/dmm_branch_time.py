"""One draw of DMM training's objective + backward at the reference's Adam shape
(--batch_size_x_adam 120 x --batch_size_u_adam 160: 19 200 interior rows and four
sides of 30 rows per field), with the train-mode branch on torch ops
(hip_branch off) and on the HIP kernels (hip_branch on), for jet=False and
jet=True: hipEvent means over R draws after 3 warm-ups, the routes alternated in
one process, every measurement twice (the run-to-run spread), and the peak
device memory each route allocates above what is resident before the call; then
one train-mode DMM.rf_features call on the interior rows, off and on, and the
kernels' workspaces.  Synthetic fields, one sample drawn once and reused; cy
(graph branch: the GNN layer and decoder kernels) and burgers (array branch: the
ConvNet kernels), one JSON line each.
    python tools/dmm_branch_time.py [--reps R] [--bx 120] [--bu 160] [--kinds cy,burgers] [--out FILE]
--out appends the lines to FILE (default profiles/dmm_branch_times.txt)."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "mm-pde_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmpde_amd import _lib as L  # noqa: E402
from mmpde_amd import dmm_train as T  # noqa: E402
from mmpde_amd.synth import build_models, burgers_grid_points, fields  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--bx", type=int, default=120)
ap.add_argument("--bu", type=int, default=160)
ap.add_argument("--kinds", default="cy,burgers")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dmm_branch_times.txt"))
args = ap.parse_args()


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
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
    return a.elapsed_time(b) / reps


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
    Tn = 6
    if kind == "cy":
        g = torch.Generator().manual_seed(5)
        u = fields(pde.ori_grid, 1, Tn, seed=5)[0]
        mesh = pde.ori_grid[None] + 1e-3 * torch.randn(Tn, *pde.ori_grid.shape, generator=g)
        all_u = torch.cat((mesh.clamp(0, 1), u[..., None]), -1).float()
    else:
        all_u = fields(burgers_grid_points(), 1, Tn, seed=5)[0].reshape(Tn, 48, 48)
    targs = SimpleNamespace(experiment=kind, bound_constraint="soft", loss_weight0=1.0, loss_weight1=1000.0,
                            loss_weight2=1.0, loss_convex=True)
    np.random.seed(3)
    sample = T._sample(targs, all_u, args.bx, args.bu, dev)

    def draw(jet, hip):
        dmm.hip_branch_train = hip
        dmm.zero_grad(set_to_none=True)
        loss = T.objective(dmm, targs, sample, args.bx, False, dev, jet=jet)[0]
        loss.backward()
        return loss

    def name(jet, hip):
        return f"{'jet' if jet else 'autograd'}_{'hip' if hip else 'torch'}"

    routes = [(jet, hip) for jet in (False, True) for hip in (False, True)]
    tl, ol = dmm.trunk.layers, dmm.out_nn.layers
    rec = {"kind": kind, "bx": args.bx, "bu": args.bu, "rows": args.bx * args.bu,
           "head": [tl[0].out_features, tl[1].out_features, ol[0].out_features], "reps": args.reps}
    for jet, hip in routes:
        rec[f"loss_{name(jet, hip)}"] = draw(jet, hip).item()
    for rep in range(2):
        for jet, hip in routes:
            rec[f"{name(jet, hip)}_ms_{rep}"] = round(timed(lambda: draw(jet, hip), args.reps), 3)
    for jet, hip in routes:
        rec[f"{name(jet, hip)}_peak_MB"] = round(peak_mb(lambda: draw(jet, hip)), 1)
    # one train-mode rf_features call (the branch under no_grad, then the feature tables) on the interior rows
    x = sample[5]
    for rep in range(2):
        for hip in (False, True):
            dmm.hip_branch_train = hip
            rec[f"rf_features_{'hip' if hip else 'torch'}_ms_{rep}"] = round(
                timed(lambda: dmm.rf_features(sample[0], x, second_order=False), args.reps), 3)
    if kind == "cy":
        n = pde.ori_grid.shape[0]
        rec["layer_workspace_MB"] = round(L.lib().mmpde_dmm_gnn_train_workspace_bytes(args.bu, n, 35) / 2 ** 20, 1)
        rec["decoder_workspace_MB"] = round(L.lib().mmpde_dmm_decode_train_workspace_bytes(args.bu * n) / 2 ** 20, 2)
    else:
        rec["convnet_workspace_MB"] = round(L.lib().mmpde_dmm_convnet_train_workspace_bytes(args.bu) / 2 ** 20, 2)
    dmm.hip_branch_train = False
    emit(rec)
    del dmm, sample
    torch.cuda.empty_cache()
