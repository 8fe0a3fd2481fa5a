"""Inputs, float64 references and bars of the train-mode array branch tests
(test_gpu_dmm_convnet_train.py on the device, test_dmm_convnet_train_cases.py
on the CPU alone).

Models and inputs u are dmm_shape_cases.array_case(s, B)'s.  The reference is
oracle/refcpu.convnet on the float64 cast of the case's state dict with
requires_grad leaves: the branch [B, 512] and the gradient of sum(branch * cot)
for a seeded random cot in all twelve branch tensors (four convolutions, fc2,
fc3).

Bars (the project's own, none measured on the kernels): the forward at
BRANCH_BAR = 1e-5 of max|ref|; every gradient tensor at err / max(max|ref|,
1e-5 g_max) <= 2e-5 with g_max the largest gradient entry of the case -- the
bar tests/dense_cases.py gives convolution gradients (the graph branch's 2e-3
exists for the jet's cancellation and would hide a wrong tap here).
"""
import functools

import torch

from dmm_shape_cases import BRANCH_BAR, array_case
from oracle import refcpu

MAX_S = 51      # ops.CONVNET_TRAIN_MAX_S (test_abi_dmm_convnet_train.py holds the three copies equal)

# (s, B); o1 = (s - 1) // 2 + 1 is the side of x1..x3, o2 = (o1 - 1) // 2 + 1 that of the last convolution
CASES = (
    # o1 = o2 = 1: every tap but the centre one (and, at s = 2, its neighbours in u) is padding
    (1, 2), (2, 2),
    # o1 = 3, 3, 4, 4, 5 and o2 = 2, 2, 2, 2, 3: odd and even sides, u's last row and column read by the last
    # stride-2 output (s odd) or not (s even), x3's likewise (o1 odd / even); fewer rows than the four row parts of
    # a weight gradient (o1 = 3)
    (5, 1), (5, 3), (6, 3), (7, 3), (8, 2), (9, 2),
    # o1 = 11: a last strip of 2 outputs and a last chunk of 3 in the stride-1 kernels; o2 = 6 even
    (21, 2),
    # o1 = 17 (a last strip of 2, a last chunk of 1, and the first convolution's 2 o1^2 items take a second trip of
    # the 512 threads); 65 fields: one past a wave, and past 64 rows in the gradient reduction
    (33, 1), (33, 3), (33, 65),
    # the reference's resolution: o1 = 24, every strip and chunk full
    (48, 3), (48, 65),
    # the largest s the LDS holds: o1 = 26, o2 = 13
    (MAX_S, 2))
GRAD_BAR = 2e-5
GRAD_FLOOR = 1e-5          # of g_max, the absolute part of a tensor's bar
# A case takes the first later cotangent seed that meets test_dmm_convnet_train_cases.py where its first one does
# not: (1, 2) left layers.1.weight's gradient at 5.4e-4 g_max; at (6, 3) the one-entry gradient of layers.3.bias
# cancelled so far that torch's own float32 stood at 0.32 of its bar (6.4e-6).
SEED_SALT = {(1, 2): 1, (6, 3): 2}
CONVS = tuple(f"layers.{i}.{t}" for i in range(4) for t in ("weight", "bias"))
NAMES = CONVS + ("fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")


def case_id(c):
    return f"{c[0]}-{c[1]}"


def out_sizes(s):
    o1 = (s - 1) // 2 + 1
    return o1, (o1 - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def inputs(c):
    """(case, u [B, s, s], cot [B, L]) on the CPU, float32."""
    s, B = c
    case = array_case(s, B)
    seed = 41 + 1013 * s + 17 * B + 7919 * SEED_SALT.get(c, 0)
    cot = torch.randn(B, case.head[1], generator=torch.Generator().manual_seed(seed))
    return case, case.u, cot


def branch_sd(c, dtype, mutate=None):
    """The branch's twelve tensors {name: leaf} in dtype (mutate: (name, index) of one entry set to zero)."""
    sd = {}
    for n in NAMES:
        t = inputs(c)[0].sd["branch." + n].detach().to(dtype).clone()
        if mutate is not None and mutate[0] == n:
            t[mutate[1]] = 0.0
        sd[n] = t.requires_grad_(True)
    return sd


class Result:
    """branch [B, L] and grads {name: tensor} over NAMES."""


def run_ref(c, dtype=torch.float64, mutate=None):
    """refcpu.convnet in dtype on the CPU and the backward of sum(branch * cot)."""
    _, u, cot = inputs(c)
    sd = branch_sd(c, dtype, mutate)
    out = refcpu.convnet({"branch." + n: t for n, t in sd.items()}, "branch", u.to(dtype).unsqueeze(1))
    gs = torch.autograd.grad((out * cot.to(dtype)).sum(), [sd[n] for n in NAMES])
    r = Result()
    r.branch = out.detach()
    r.grads = {n: g.detach() for n, g in zip(NAMES, gs)}
    return r


@functools.lru_cache(maxsize=None)
def reference(c):
    return run_ref(c)


def g_max(ref):
    return max(g.abs().max().item() for g in ref.grads.values())


def measure(got, ref):
    """{quantity: (error in units of its bar's base, bar)} of a Result against the reference."""
    d = lambda a, b: (a.detach().double().cpu() - b.double()).abs().max().item()  # noqa: E731
    out = {"forward": (d(got.branch, ref.branch) / ref.branch.abs().max().item(), BRANCH_BAR)}
    G = g_max(ref)
    for n, g in ref.grads.items():
        assert got.grads[n] is not None and got.grads[n].shape == g.shape, n
        out["grad " + n] = (d(got.grads[n], g) / max(g.abs().max().item(), GRAD_FLOOR * G), GRAD_BAR)
    return out


def worst(m):
    return dict(forward=m["forward"][0], grads=max(v for k, (v, _) in m.items() if k.startswith("grad ")))


def check(m, what, fraction=1.0):
    bad = {k: v for k, (v, bar) in m.items() if not v <= fraction * bar}
    assert not bad, (what, bad)


def taps(s):
    """One tap of each convolution weight for the mutation self-check: the corner taps, which only the first or
    last outputs read; with o1 = 1 (s <= 2) every tap but the centre one reads padding alone, so the centre.
    There the whole stack is one value per field under fc2's bias, and one tap of 200 moves the branch by less than
    a bar (0.008 to 86 bars over the four taps): those two cases are held to the gradient half of the check."""
    if out_sizes(s)[0] == 1:
        return (("layers.0.weight", (7, 0, 2, 2)), ("layers.1.weight", (15, 7, 2, 2)),
                ("layers.2.weight", (7, 15, 2, 2)), ("layers.3.weight", (0, 7, 2, 2)))
    return (("layers.0.weight", (7, 0, 4, 4)), ("layers.1.weight", (15, 7, 4, 4)),
            ("layers.2.weight", (7, 15, 0, 0)), ("layers.3.weight", (0, 7, 4, 4)))


def model(c, device="cpu"):
    """A fresh float32 copy of the case's model in train() mode."""
    import copy

    return copy.deepcopy(inputs(c)[0].dmm).to(device).train()


def run_model(dmm, fn, u, cot):
    """One train-mode call of fn(dmm, u) -> branch and the backward of sum(branch * cot) into the branch's tensors."""
    dmm.train()
    dmm.zero_grad(set_to_none=True)
    out = fn(dmm, u)
    (out * cot).sum().backward()
    r = Result()
    r.branch = out.detach()
    r.grads = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in dmm.branch.named_parameters()}
    dmm.zero_grad(set_to_none=True)
    return r
