"""Row-GEMM timing (csrc/rgemm.hip via ops.LinearRows) against torch's library
GEMM at the train-mode GNN shapes (cy B=16: n = 40336 rows): forward
y = x W^T + b, input gradient dX = dY W, weight gradient dW = dY^T X (+ db).
HIP events on the current stream around 20 back-to-back calls.

    python tools/rgemm_bench.py
    python tools/rgemm_bench.py --layer     # the mmpde_rgemm launches of GnnLayerTrain

--layer: the seven launches of one train-mode GNN layer (gnn_2d.py
GnnLayerTrain, forward and backward; 6s is the ncols = 4 sibling of the sixth)
with the production part tables, the median of 9 timings of 20 calls each.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-pde_amd")]

import torch  # noqa: E402


def timed(fn, reps=20):
    """Microseconds per call of `reps` back-to-back calls (the host's issue time
    overlaps the device work when the kernels are the longer part)."""
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def layer_launches(n, dev):
    """name -> callable of each mmpde_rgemm launch of GnnLayerTrain at n rows."""
    from mmpde_amd import _lib as L
    from mmpde_amd import rows
    P, NT, NN = rows._p, L.RGEMM_NT, L.RGEMM_NN
    st = L.stream(dev)
    t = {k: torch.randn(n, 128, device=dev) for k in ("h", "mean", "v", "upd", "dx", "dv", "da", "db", "o0", "o1")}
    ext, dext = torch.randn(n, 4, device=dev), torch.zeros(n, 4, device=dev)
    W1, U1, nwp = (torch.randn(128, 260, device=dev) / 16 for _ in range(3))
    U2 = torch.randn(128, 128, device=dev) / 11
    b = torch.randn(128, device=dev)
    full = (128, 128)

    def part(out, **k):
        return dict(out=P(t[out]), ldo=128, ncols=128, **k)

    return {
        "1": lambda: rows.rgemm(n, 64, NT, (P(W1), P(W1, 64)), 260, (P(t["h"]), P(t["h"], 64)), full,
                                [part("o0", bias=P(b), ns=4, xw=P(W1, 256)),
                                 part("o1", wk=128, ns=3, xw=P(W1, 256), xscale=-1.0)],
                                xs=P(ext), ldxs=4, ldxw=260, stream=st),
        "2": lambda: rows.rgemm(n, 128, NT, (P(U1), P(U1, 128)), 260, (P(t["h"]), P(t["mean"])), full,
                                [part("o0", bias=P(b), ns=1, xw=P(U1, 256))], relu=True, xs=P(ext, 3), ldxs=4,
                                ldxw=260, stream=st),
        "3": lambda: rows.rgemm(n, 64, NT, (P(U2), P(U2, 64)), 128, (P(t["v"]), P(t["v"], 64)), full,
                                [part("o0", bias=P(b))], relu=True, stream=st),
        "4": lambda: rows.rgemm(n, 64, NN, (P(U2), P(U2, 64 * 128)), 128, (P(t["dx"]), P(t["dx"], 64)), full,
                                [part("o0", omask=P(t["v"]), ldom=128)], amask=(P(t["upd"]), P(t["upd"], 64)),
                                stream=st),
        "5": lambda: rows.rgemm(n, 64, NN, (P(U1), P(U1, 64 * 260)), 260, (P(t["dv"]), P(t["dv"], 64)), full,
                                [part("o0", wc=0, acc=True), part("o1", wc=128)], stream=st),
        "6": lambda: rows.rgemm(n, 128, NN, (P(W1), P(W1, 128)), 260, (P(t["da"]), P(t["db"])), full,
                                [part("o0", wc=0, acc=True)], stream=st),
        "6s": lambda: rows.rgemm(n, 128, NN, (P(W1, 256), P(nwp, 256)), 260, (P(t["da"]), P(t["db"])), full,
                                 [dict(out=P(dext), ldo=4, ncols=4)], stream=st),
        "7": lambda: rows.rgemm(n, 64, NN, (P(U1, 256), P(U1, 64 * 260 + 256)), 260,
                                (P(t["dv"]), P(t["dv"], 64)), full, [dict(out=P(dext, 3), ldo=4, ncols=1, acc=True)],
                                stream=st),
    }


def layer(n=40336):
    dev = torch.device("cuda:0")
    res = {}
    for name, fn in layer_launches(n, dev).items():
        ts = sorted(timed(fn) for _ in range(9))
        res[name] = {"median_us": round(ts[4], 2), "min_us": round(ts[0], 2), "max_us": round(ts[-1], 2)}
    print(json.dumps({"n": n, "launches": res}), flush=True)


def main():
    if "--layer" in sys.argv[1:]:
        return layer()
    from mmpde_amd import rows
    dev = torch.device("cuda:0")
    out = []
    for n, k, nout in ((40336, 128, 128), (40336, 256, 128), (40336, 128, 256), (40336, 62, 128),
                       (40336, 128, 64), (40336, 64, 30)):
        x = torch.randn(n, k, device=dev)
        w = torch.randn(nout, k, device=dev)
        b = torch.randn(nout, device=dev)
        dy = torch.randn(n, nout, device=dev)
        dw = torch.empty(nout, k, device=dev)
        db = torch.empty(nout, device=dev)
        r = {"n": n, "k": k, "nout": nout,
             "fwd_us": timed(lambda: rows.linear_fwd(x, w, b)),
             "fwd_torch_us": timed(lambda: torch.addmm(b, x, w.t())),
             "dx_us": timed(lambda: rows.linear_bwd_input(dy, w)),
             "dx_torch_us": timed(lambda: dy @ w),
             "dw_us": timed(lambda: rows.linear_bwd_weight(dy, x, dw, db)),
             "dw_torch_us": timed(lambda: (dy.t() @ x, dy.sum(0)))}
        flop = 2 * n * k * nout
        r["fwd_tflops"] = flop / r["fwd_us"] / 1e6
        out.append(r)
        print(json.dumps({q: (round(v, 2) if isinstance(v, float) else v) for q, v in r.items()}), flush=True)


if __name__ == "__main__":
    main()
