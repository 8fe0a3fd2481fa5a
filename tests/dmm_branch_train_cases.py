"""Inputs, float64 references and bars of the train-mode graph branch tests
(test_gpu_dmm_branch_train.py on the device, test_dmm_branch_train_cases.py on
the CPU alone).

Models, grids, inputs u and neighbour tables are dmm_shape_cases.graph_case's
(BatchNorm affine parameters randomised, the branch Linear weights doubled).
The reference is a deepcopy of the case's model in float64 and train() mode on
the CPU, driven by `restate`: DMM._branch_train written out over the case's
table with the module's own submodules (plain torch in train mode).  It gives
the branch [B, L], the gradient of sum(branch * cot) for a seeded random cot in
every parameter, and the BatchNorm buffers after the one call.

Bars (the project's own): the forward at BRANCH_BAR = 1e-5 of max|ref|; every
gradient tensor at err / max(max|ref|, 1e-5 g_max) <= 2e-3 with g_max the
largest gradient entry of the case (the jet tests' measure); running statistics
at 1e-5 of max|ref|; the two biases whose gradient is exactly zero (each feeds
a batch-statistics BatchNorm directly) at max|g| <= 1e-4 g_max.
"""
import copy
import functools

import torch

from dmm_shape_cases import BRANCH_BAR, graph_case

# (n_per, k, nl, B)
CASES = (
    # one edge, a ragged quad, a full quad, a second trip of the edge loop
    (129, 1, 3, 2), (129, 3, 3, 2), (129, 4, 3, 2), (129, 33, 3, 2),
    # k + 1 nodes, the 128-target block edge
    (36, 35, 3, 2), (128, 35, 3, 2),
    # the number of layers
    (129, 35, 0, 2), (129, 35, 1, 2),
    # batch sizes, one past a wave of trajectories
    (129, 35, 3, 1), (129, 35, 3, 65),
    # the second trip of the staging loop; past the LDS staging
    (513, 35, 3, 2), (4389, 35, 3, 3))
HUB_BASE = (129, 35, 3, 2)
# hub0: column 0 reads node 0 in every row (in-degree >= 129); hub5: node 5 is read by nobody
HUBS = ("hub0", "hub5")
KEYS = tuple((c, None) for c in CASES) + tuple((HUB_BASE, h) for h in HUBS)
GRAD_BAR = 2e-3
GRAD_FLOOR = 1e-5          # of g_max, the absolute part of a tensor's bar
STAT_BAR = 1e-5
ZERO_BAR = 1e-4            # of g_max
ZERO_GRADS = ("embedding_mlp.0.bias", "embedding_mlp.3.bias")
# a case whose tensors do not all reach 1e-3 g_max takes another cotangent seed
SEED_SALT = {}


def key_id(key):
    c, hub = key
    return "-".join(str(v) for v in c) + (f"-{hub}" if hub else "")


def hub_table(nbr, hub):
    nbr = nbr.clone()
    if hub == "hub0":
        nbr[:, 0] = 0
    elif hub == "hub5":
        nbr[nbr == 5] = 6
    else:
        raise ValueError(hub)
    return nbr


@functools.lru_cache(maxsize=None)
def inputs(key):
    """(case, nbr [N, k] int32, u [B, N], cot [B, L]) on the CPU, float32."""
    c, hub = key
    case = graph_case(*c)
    nbr = case.nbr if hub is None else hub_table(case.nbr, hub)
    seed = 31 + 1009 * c[0] + 101 * c[1] + 11 * c[2] + c[3] + 7919 * SEED_SALT.get(key, 0) + (HUBS.index(hub) + 1
                                                                                            if hub else 0)
    cot = torch.randn(c[3], case.head[1], generator=torch.Generator().manual_seed(seed))
    return case, nbr, case.u, cot


def restate(dmm, u, nbr):
    """DMM._branch_train in graph mode over the table nbr, on the module's own submodules."""
    B = u.shape[0]
    og = torch.as_tensor(dmm.ori_grid).to(u.device, u.dtype).reshape(-1, 2)
    N = og.shape[0]
    gnbr = (nbr[None].long() + N * torch.arange(B, device=u.device)[:, None, None]).reshape(B * N, -1)
    x = u.reshape(-1, 1)
    pos = og[None].expand(B, N, 2).reshape(-1, 2)
    pos_x, pos_y = pos[:, :1], pos[:, 1:]
    h = dmm.embedding_mlp(torch.cat((x, pos_x, pos_y), -1))
    for layer in dmm.gnn_layers:
        h = layer(h, x, pos_x, pos_y, gnbr)
    h, _ = dmm.decoding_mlp(h)
    return dmm.output_mlp(h.reshape(B, -1))


class Result:
    """branch [B, L], grads {name: tensor or None}, stats {buffer name: tensor}."""


def run(dmm, fn, u, nbr, cot):
    """One train-mode call of fn(dmm, u, nbr) -> branch and the backward of sum(branch * cot)."""
    dmm.train()
    dmm.zero_grad(set_to_none=True)
    r = Result()
    out = fn(dmm, u, nbr)
    (out * cot).sum().backward()
    r.branch = out.detach()
    r.grads = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in dmm.named_parameters()}
    r.stats = {n: b.detach().clone() for n, b in dmm.named_buffers()}
    dmm.zero_grad(set_to_none=True)
    return r


def model(key, dtype=torch.float32, device="cpu"):
    """A fresh copy of the case's model in train() mode."""
    return copy.deepcopy(inputs(key)[0].dmm).to(device=device, dtype=dtype).train()


@functools.lru_cache(maxsize=None)
def reference(key):
    _, nbr, u, cot = inputs(key)
    return run(model(key, torch.float64), restate, u.double(), nbr, cot.double())


def g_max(ref):
    return max(g.abs().max().item() for g in ref.grads.values() if g is not None)


def measure(got, ref):
    """{quantity: (error in units of its bar's base, bar)} of a Result against the reference."""
    out = {}
    d = lambda a, b: (a.detach().double().cpu() - b.double()).abs().max().item()  # noqa: E731
    out["forward"] = (d(got.branch, ref.branch) / ref.branch.abs().max().item(), BRANCH_BAR)
    G = g_max(ref)
    for n, g in ref.grads.items():
        if g is None:
            assert got.grads[n] is None or not bool(got.grads[n].any()), n
            continue
        assert got.grads[n] is not None, n
        if n in ZERO_GRADS:
            out["grad " + n] = (got.grads[n].abs().max().item() / G, ZERO_BAR)
        else:
            out["grad " + n] = (d(got.grads[n], g) / max(g.abs().max().item(), GRAD_FLOOR * G), GRAD_BAR)
    for n, b in ref.stats.items():
        if n.endswith("num_batches_tracked"):
            assert int(got.stats[n]) == int(b), n
        else:
            out["stat " + n] = (d(got.stats[n], b) / b.abs().max().item(), STAT_BAR)
    return out


def worst(m):
    """The worst forward / gradient / zero-gradient / statistics figures of a measure, for the tables."""
    pick = lambda f: max((v for k, (v, _) in m.items() if f(k)), default=0.0)  # noqa: E731
    zero = tuple("grad " + n for n in ZERO_GRADS)
    return dict(forward=m["forward"][0], grads=pick(lambda k: k.startswith("grad ") and k not in zero),
                zero=pick(lambda k: k in zero), stats=pick(lambda k: k.startswith("stat ")))


def check(m, what, fraction=1.0):
    bad = {k: v for k, (v, bar) in m.items() if not v <= fraction * bar}
    assert not bad, (what, bad)
