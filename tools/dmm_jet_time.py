"""One draw of DMM training's objective + backward at the reference's Adam shape
(--batch_size_x_adam 120 x --batch_size_u_adam 160: 19 200 interior rows and four
sides of 30 rows per field), on the autograd route (jet=False) and on the jet
kernels (jet=True): hipEvent means over R calls after a warm-up, the two routes
alternated in one process, every measurement twice (the run-to-run spread), and
the peak device memory each route allocates above what is resident before the
call; then mmpde_dmm_jet and mmpde_dmm_jet_grad alone on the interior rows (the
branch given, the wrapper's output allocations included).  Synthetic fields, one
sample drawn once and reused; cy (graph branch) and burgers (array branch), one
JSON line each.
    python tools/dmm_jet_time.py [--reps R] [--bx 120] [--bu 160] [--out FILE]
--out appends the lines to FILE."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "mm-pde_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmpde_amd import _lib as L  # noqa: E402
from mmpde_amd import dmm_train as T  # noqa: E402
from mmpde_amd.synth import build_models, burgers_grid_points, fields  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--bx", type=int, default=120)
ap.add_argument("--bu", type=int, default=160)
ap.add_argument("--out")
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
    return a.elapsed_time(b) / reps


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


dev = torch.device("cuda:0")
for kind in ("cy", "burgers"):
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

    def draw(jet):
        dmm.zero_grad(set_to_none=True)
        loss = T.objective(dmm, targs, sample, args.bx, False, dev, jet=jet)[0]
        loss.backward()
        return loss

    tl, ol = dmm.trunk.layers, dmm.out_nn.layers
    rec = {"kind": kind, "bx": args.bx, "bu": args.bu, "rows": args.bx * args.bu,
           "head": [tl[0].out_features, tl[1].out_features, ol[0].out_features], "reps": args.reps,
           "loss_autograd": draw(False).item(), "loss_jet": draw(True).item()}
    for rep in range(2):
        for jet in (False, True):
            rec[f"{'jet' if jet else 'autograd'}_ms_{rep}"] = round(timed(lambda: draw(jet), args.reps), 3)
    for jet in (False, True):
        rec[f"{'jet' if jet else 'autograd'}_peak_MB"] = round(peak_mb(lambda: draw(jet)), 1)
    # the two kernel calls alone on the interior rows, the branch given
    from mmpde_amd import ops
    with torch.no_grad():
        branch = dmm._branch_train(sample[0]).float().contiguous()
    hd, keep = dmm._head_params()
    x = sample[5]
    cots = [torch.randn(x.shape[0], device=dev) for _ in range(6)]
    bias = ol[1].bias.detach()
    rec["jet_call_us"] = round(1e3 * timed(lambda: ops.dmm_jet(branch, x, hd, bias), 50), 1)
    rec["jet_grad_call_us"] = round(1e3 * timed(lambda: ops.dmm_jet_grad(branch, x, hd, cots), 50), 1)
    rec["jet_workspace_MB"] = round(L.lib().mmpde_dmm_jet_workspace_bytes(branch.shape[0], x.shape[0], hd.latent,
                                                                          hd.hidden, hd.th) / 2 ** 20, 1)
    del keep
    emit(rec)
    del dmm, sample
    torch.cuda.empty_cache()
