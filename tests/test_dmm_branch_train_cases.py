"""CPU-only self-check of the inputs and bars of test_gpu_dmm_branch_train.py:
the float32 CPU restatement of the train-mode graph branch stays within a
quarter of every bar against the float64 one, no gradient tensor hides under
the bar's absolute floor, and the hub tables have the in-degrees they claim."""
import pytest
import torch

import dmm_branch_train_cases as C

IDS = [C.key_id(k) for k in C.KEYS]


@pytest.mark.parametrize("key", C.KEYS, ids=IDS)
def test_fp32_restatement_within_a_quarter_of_the_bars(key):
    _, nbr, u, cot = C.inputs(key)
    ref = C.reference(key)
    got = C.run(C.model(key), C.restate, u, nbr, cot)
    m = C.measure(got, ref)
    print(C.key_id(key), {k: f"{v:.2e}" for k, v in C.worst(m).items()})
    C.check(m, C.key_id(key), fraction=0.25)


@pytest.mark.parametrize("key", C.KEYS, ids=IDS)
def test_no_gradient_hides_under_the_floor(key):
    ref = C.reference(key)
    G = C.g_max(ref)
    used = {n for n, g in ref.grads.items() if g is not None}
    nl = key[0][2]
    assert {"embedding_mlp.0.weight", "decoding_mlp.layers.0.weight", "output_mlp.4.bias"} <= used
    assert sum(n.startswith("gnn_layers.") for n in used) == 10 * nl     # 8 Linear tensors + the BatchNorm's 2
    for n in used:
        g = ref.grads[n]
        if n in C.ZERO_GRADS:
            assert g.abs().max().item() <= 1e-12 * G, n                 # zero, in float64
        else:
            assert g.abs().max().item() >= 1e-3 * G, (n, g.abs().max().item(), G)


def test_hub_tables_have_the_claimed_in_degrees():
    n = C.HUB_BASE[0]
    _, hub0, _, _ = C.inputs((C.HUB_BASE, "hub0"))
    _, hub5, _, _ = C.inputs((C.HUB_BASE, "hub5"))
    _, base, _, _ = C.inputs((C.HUB_BASE, None))
    deg = lambda t: torch.bincount(t.reshape(-1).long(), minlength=n)  # noqa: E731
    assert int(deg(hub0)[0]) >= n > 64 and bool((hub0[:, 0] == 0).all())
    assert int(deg(hub5)[5]) == 0 and int(deg(base)[5]) > 0
    for t in (hub0, hub5):
        assert t.dtype == torch.int32 and t.shape == base.shape and int(t.min()) >= 0 and int(t.max()) < n
