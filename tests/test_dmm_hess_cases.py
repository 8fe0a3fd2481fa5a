"""CPU-only self-check of the inputs of test_gpu_dmm_hess.py, on the float64
reference alone (as test_dmm_shape_cases.py does for the mesh):

  * the autograd Hessian is symmetric, and the float32 CPU oracle meets the H
    bar (2e-5 of max|H_ref|) on every case;
  * zeroing out_nn.layers.1.weight[0, L' - 1] or the last trunk hidden unit
    (dmm_shape_cases.mutated_head) moves H_ref by at least 5 bars, or the bar
    could not see a kernel that drops one unit;
  * every fold case has a trajectory with folds and one with a different count,
    an unfolded node, and at most 1 % of its nodes within the sign margin
    m = delta (2 + 4 max|H_ref|), delta = the H bar, of det = 0.

Measured (float64, CPU): unscaled cases max|H| 0.0105 - 0.0654, det in
[0.90, 1.07], fp32 oracle 5.8e-7 - 2.1e-6 of max|H|; the mutations move H_ref
by 67 bars at the least (w_o, n_per = 6; 435 - 7405 bars elsewhere) and the
trunk unit by 230 bars at the least (B = 65; 1206 - 50000 bars elsewhere).
Fold cases: graph-130-B3 folds 11 / 13 / 15 nodes (max|H| 0.663, min|det| 1.28e-4, m 6.2e-5), graph-130-B33 4 - 6 nodes per trajectory (161 in
all, max|H| 1.056, min|det| 2.9e-4, m 1.3e-4), array-33-B3 0 / 0 / 26 nodes
(max|H| 0.873, min|det| 2.7e-3, m 9.6e-5); no node within the margin.
"""
import pytest
import torch

import dmm_hess_cases as H
import dmm_shape_cases as C

FACTOR = 5.0


def _ids(cases):
    return ["-".join(str(x) for x in (c if not isinstance(c[-1], tuple) else c[:-1] + c[-1])) for c in cases]


def _hess_check(c, tag):
    ref, asym = H.hess_ref(c, key="base")
    scale = ref.abs().max().item()
    bar = H.h_bar(ref)
    det = H.det_of(ref)
    assert ref.dtype == torch.float64 and ref.shape == (c.B * c.xi.shape[0], 3)
    assert scale > 1e-3, (tag, scale)
    assert asym <= 1e-15, (tag, asym)
    assert bool((det > 0.5).all()), "an unscaled case folds"
    cpu32 = (H.hess_ref(c, torch.float32)[0].double() - ref).abs().max().item()
    msg = [f"{tag}: max|H| {scale:.3e} det in [{det.min().item():.3f}, {det.max().item():.3f}] asym {asym:.1e} "
           f"fp32 CPU oracle {cpu32 / scale:.2e} of max|H|"]
    diffs = {}
    for which in ("w_o", "trunk"):
        diffs[which] = (H.hess_ref(c, sd=C.mutated_head(c, which))[0] - ref).abs().max().item()
        msg.append(f"{which} {diffs[which] / bar:.0f} bars")
    print(", ".join(msg))
    assert cpu32 <= bar / 8, msg     # the bar is at least 8 x the oracle's own error
    for which, d in diffs.items():
        assert d >= FACTOR * bar, (which, msg)


@pytest.mark.parametrize("n_per,B,head", C.GRAPH_MESH_CASES, ids=_ids(C.GRAPH_MESH_CASES))
def test_graph_hess_bar_sees_head_mutations(n_per, B, head):
    _hess_check(C.graph_case(n_per, 5, 1, B, head, False), f"graph hess n_per={n_per} B={B} head={head}")


@pytest.mark.parametrize("s,B", C.ARRAY_MESH_CASES, ids=_ids(C.ARRAY_MESH_CASES))
def test_array_hess_bar_sees_head_mutations(s, B):
    _hess_check(C.array_case(s, B), f"array hess s={s} B={B}")


@pytest.mark.parametrize("name", [f[0] for f in H.FOLD_CASES])
def test_fold_case_folds_differently_per_trajectory(name):
    c, sd = H.fold_case(name)
    ref, asym = H.hess_ref(c, sd=sd, key=name)
    det = H.det_of(ref).reshape(c.B, -1)
    m = H.sign_margin(ref)
    folds = (~(det > 0)).sum(1)
    near = int((det.abs() <= m).sum())
    cpu32 = H.hess_ref(c, torch.float32, sd=sd)[0].double()
    err32 = (cpu32 - ref).abs().max().item()
    det32 = H.det_of(cpu32).reshape(c.B, -1)
    print(f"{name}: max|H| {ref.abs().max().item():.3f} min det {det.min().item():.3e} min|det| "
          f"{det.abs().min().item():.2e} margin {m:.2e} within it {near} folds {folds.tolist()} "
          f"fp32 CPU oracle {err32 / ref.abs().max().item():.2e} of max|H|")
    assert asym <= 1e-14
    assert int(folds.max()) > 0 and len(set(folds.tolist())) >= 2, "no fold, or the same count everywhere"
    assert bool((det > 0).any()), "every node folded"
    assert near <= 0.01 * det.numel()
    assert err32 <= H.h_bar(ref)
    outside = det.abs() > m
    assert torch.equal((det32 > 0)[outside], (det > 0)[outside]), "the fp32 oracle disagrees on a sign"


def test_wo_alone_folds_every_trajectory_alike():
    """Why the branch half is scaled too: w_o x 16 alone folds 59 nodes in every
    trajectory (the case then could not see a trajectory-index error)."""
    c = H.base_case("graph", 130, 3)
    det = H.det_of(H.hess_ref(c, sd=H.fold_sd(c, 16.0, 1.0))[0]).reshape(c.B, -1)
    folds = (~(det > 0)).sum(1).tolist()
    print(f"w_o x 16 alone: folds {folds}")
    assert max(folds) > 0 and len(set(folds)) == 1, folds
