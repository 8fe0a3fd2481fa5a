"""CPU-only self-check of the inputs of test_gpu_dmm_shapes.py: on the float64
reference alone, a small error of the kind a kernel makes at an edge must move
the compared quantity by at least 5 x the case's bar, or the bar could not see
it.  Also: the float32 CPU oracle itself meets every bar.

Mutations
    graph branch  one slot of the last row of the last trajectory's table
                  changed; n_per >= 4388 also the last slot of every row of that
                  trajectory's trailing partial 128-row block; with no GNN layer
                  (nothing reads the table) the last node's u zeroed
    array branch  the last pixel of the last trajectory zeroed
    mesh          out_nn.layers.1.weight[0, L' - 1] zeroed; the last row of
                  trunk.layers.0.weight zeroed
"""
import pytest
import torch

import dmm_shape_cases as C

FACTOR = 5.0


def _rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


def _ids(cases):
    return ["-".join(str(x) for x in (c if not isinstance(c[-1], tuple) else c[:-1] + c[-1])) for c in cases]


@pytest.mark.parametrize("n_per,k,nl,B", C.GRAPH_BRANCH_CASES, ids=_ids(C.GRAPH_BRANCH_CASES))
def test_graph_branch_bar_sees_one_slot(n_per, k, nl, B):
    c = C.graph_case(n_per, k, nl, B)
    ref = C.branch_ref(c)
    assert ref.shape == (B, c.head[1]) and ref.dtype == torch.float64
    tbl = c.nbr.long()
    assert (tbl == 0).any() and (tbl == n_per - 1).any() and int(tbl.min()) >= 0 and int(tbl.max()) < n_per
    muts = [("last slot", C.mutated_last_slot(c))]
    if n_per >= 4388:
        muts.append(("last block", C.mutated_last_block(c)))
    cpu32 = _rel(C.branch_ref(c, torch.float32).double(), ref)
    msg = [f"graph branch n_per={n_per} k={k} nl={nl} B={B}: max|ref| {ref.abs().max().item():.3e} "
           f"fp32 CPU oracle {cpu32:.2e}"]
    for what, ei in muts:
        assert int((ei != c.ei).sum()) >= 1
        msg.append(f"{what} {_rel(C.branch_ref(c, ei=ei), ref):.2e}")
    print(", ".join(msg))
    assert cpu32 <= C.BRANCH_BAR, msg
    if nl == 0:
        # no GNN layer reads the table: the last node's input instead
        u = c.u.clone()
        u[-1, -1] = 0.0
        d = _rel(C.branch_ref(c, u=u), ref)
        print(f"last node's u zeroed {d:.2e}")
        assert d >= FACTOR * C.BRANCH_BAR, msg
        return
    for what, ei in muts:
        assert _rel(C.branch_ref(c, ei=ei), ref) >= FACTOR * C.BRANCH_BAR, (what, msg)


@pytest.mark.parametrize("s,B", C.ARRAY_BRANCH_CASES, ids=_ids(C.ARRAY_BRANCH_CASES))
def test_array_branch_bar_sees_one_pixel(s, B):
    c = C.array_case(s, B)
    ref = C.branch_ref(c)
    assert ref.shape == (B, 512) and ref.dtype == torch.float64
    cpu32 = _rel(C.branch_ref(c, torch.float32).double(), ref)
    mut = _rel(C.branch_ref(c, u=C.mutated_last_pixel(c)), ref)
    print(f"array branch s={s} B={B}: max|ref| {ref.abs().max().item():.3e} fp32 CPU oracle {cpu32:.2e} "
          f"last pixel {mut:.2e}")
    assert cpu32 <= C.BRANCH_BAR
    assert mut >= FACTOR * C.BRANCH_BAR


def _mesh_check(c, tag):
    ref = C.disp_ref(c)
    bar = C.mesh_bar(c, ref)
    scale = ref.abs().max().item()
    assert ref.dtype == torch.float64 and scale > 1e-3, (tag, scale)
    cpu32 = (C.disp_ref(c, torch.float32).double() - ref).abs().max().item()
    msg = [f"{tag}: max|disp| {scale:.3e} bar {bar:.3e} fp32 CPU oracle {cpu32:.3e} ({cpu32 / scale:.2e} of max|disp|)"]
    diffs = {}
    for which in ("w_o", "trunk"):
        diffs[which] = (C.disp_ref(c, sd=C.mutated_head(c, which)) - ref).abs().max().item()
        msg.append(f"{which} {diffs[which]:.3e} ({diffs[which] / bar:.0f} bars)")
    print(", ".join(msg))
    assert cpu32 <= bar, msg
    for which, d in diffs.items():
        assert d >= FACTOR * bar, (which, msg)


@pytest.mark.parametrize("n_per,B,head", C.GRAPH_MESH_CASES, ids=_ids(C.GRAPH_MESH_CASES))
def test_graph_mesh_bar_sees_head_mutations(n_per, B, head):
    _mesh_check(C.graph_case(n_per, 5, 1, B, head, False), f"graph mesh n_per={n_per} B={B} head={head}")


@pytest.mark.parametrize("s,B", C.ARRAY_MESH_CASES, ids=_ids(C.ARRAY_MESH_CASES))
def test_array_mesh_bar_sees_head_mutations(s, B):
    _mesh_check(C.array_case(s, B), f"array mesh s={s} B={B}")
