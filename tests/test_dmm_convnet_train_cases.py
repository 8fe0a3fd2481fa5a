"""CPU-only self-check of the inputs and bars of test_gpu_dmm_convnet_train.py:
refcpu.convnet in float32 stays within a quarter of every bar against float64,
the reference is not small, no gradient tensor hides under the bar's absolute
floor, and zeroing one tap of any of the four convolution weights moves the
forward and some gradient by at least ten bars (at s <= 2, where the stack is
one value per field, the gradient alone: dmm_convnet_train_cases.taps)."""
import pytest

import dmm_convnet_train_cases as C

IDS = [C.case_id(c) for c in C.CASES]


def test_the_case_list_holds_what_the_kernels_can_get_wrong():
    assert {(1, 2), (2, 2), (5, 1), (5, 3), (6, 3), (7, 3), (8, 2), (9, 2), (33, 1), (33, 3), (33, 65), (48, 3),
            (48, 65), (C.MAX_S, 2)} <= set(C.CASES)
    o1 = {C.out_sizes(s)[0] for s, _ in C.CASES}
    assert any(o % 3 == 1 for o in o1) and any(o % 3 == 2 for o in o1) and any(o % 3 == 0 for o in o1)
    assert {o % 4 for o in o1} == {0, 1, 2, 3}
    assert any(2 * o * o > 512 for o in o1) and any(o < 4 for o in o1)
    assert C.MAX_S >= 48


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_fp32_reference_within_a_quarter_of_the_bars(c):
    ref = C.reference(c)
    m = C.measure(C.run_ref(c, dtype=C.torch.float32), ref)
    print(C.case_id(c), {k: f"{v:.2e}" for k, v in C.worst(m).items()}, f"max|ref| {ref.branch.abs().max().item():.3f}")
    C.check(m, C.case_id(c), fraction=0.25)


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_reference_is_not_small_and_no_gradient_hides_under_the_floor(c):
    ref = C.reference(c)
    s, B = c
    assert ref.branch.shape == (B, 512) and ref.branch.abs().max().item() >= 0.1
    assert ref.grads["fc2.weight"].shape == (1024, C.out_sizes(s)[1] ** 2)
    G = C.g_max(ref)
    for n in C.NAMES:
        assert ref.grads[n].abs().max().item() >= 1e-3 * G, (n, ref.grads[n].abs().max().item(), G)


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_one_zeroed_tap_moves_forward_and_a_gradient_by_ten_bars(c):
    ref = C.reference(c)
    for mut in C.taps(c[0]):
        m = C.measure(C.run_ref(c, mutate=mut), ref)
        fwd, grad = m["forward"][0] / C.BRANCH_BAR, C.worst(m)["grads"] / C.GRAD_BAR
        print(f"{C.case_id(c)} {mut}: forward {fwd:.1f} bars, worst gradient {grad:.1f} bars")
        assert grad >= 10 and (fwd >= 10 or C.out_sizes(c[0])[0] == 1), (mut, fwd, grad)   # o1 = 1: see C.taps
