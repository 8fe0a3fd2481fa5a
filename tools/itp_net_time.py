"""The cost of the shape-generic ItpNet interpolation (profiling aid):
itp_interp_kernel (the specialised 62 -> 128 -> 64 -> 30 kernel) beside
itp_net_kernel at [128, 64] (packed(generic=True)), [64, 32], [256, 256] and
[256, 256, 256, 256], at the cylinder rollout's shape, B = 16 trajectories of
2521 nodes (40 336 queries, n_src 2521): the moved mesh is the fixed mesh
jittered by 0.004, the neighbour table the product's kNN-30 query.  hipEvent
means over R calls after a warm-up, the kernels alternated in one process,
every measurement three times (the run-to-run spread), one JSON line.
    python tools/itp_net_time.py [--reps R] [--out FILE]
--out appends the line to FILE (profiles/itp_net_times.txt)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "mm-pde_amd"))
import torch  # noqa: E402

from mmpde_amd import ops  # noqa: E402
from mmpde_amd.interpolate import ItpNet  # noqa: E402
from mmpde_amd.synth import cy_synth_mesh, fields  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out")
args = ap.parse_args()


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
B = 16
grid = cy_synth_mesh()
N = grid.shape[0]
g = torch.Generator().manual_seed(3)
qry = grid.repeat(B, 1).to(dev)
src = (grid.repeat(B, 1) + 0.004 * torch.randn(B * N, 2, generator=g)).clamp(0, 1).to(dev)
vals = fields(grid, B, 30)[:, 3].reshape(-1).to(dev).contiguous()
idx = ops.knn_query(src, qry, B, 30)

torch.manual_seed(0)
packs = {"specialised": ItpNet(N, None, [128, 64], [128, 64], []).to(dev).packed("2")}
for hidden in ([128, 64], [64, 32], [256, 256], [256, 256, 256, 256]):
    net = ItpNet(N, None, [128, 64], hidden, []).to(dev)
    packs["generic " + "x".join(map(str, hidden))] = net.packed("2", generic=True)
calls = {k: (lambda p=p: ops.itp_interp(src, vals, qry, idx, B, p)) for k, p in packs.items()}

rec = {"B": B, "n_src": N, "queries": B * N, "reps": args.reps}
for rep in range(3):
    for name, fn in calls.items():
        rec.setdefault(name + " us", []).append(round(timed(fn, args.reps), 1))
spec, gen = rec["specialised us"], rec["generic 128x64 us"]
rec["generic/specialised at 128x64"] = [round(b / a, 3) for a, b in zip(spec, gen)]
line = json.dumps(rec)
print(line, flush=True)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
