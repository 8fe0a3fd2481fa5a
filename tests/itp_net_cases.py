"""Cases and the float64 reference of the shape-generic ItpNet interpolation
(mmpde_itp_interp_net, itp_net.hip; reference interpolate.py:5-30,77-93 with the
weighted sum of data_creator_2d.py:80-83), for any number of Linears.  Used by
test_itp_net_cases.py on the CPU alone and by test_gpu_itp_net.py on the device.

Inputs as in test_gpu_itp_shapes.py: coordinates uniform in the unit square,
vals normal, idx uniform LOCAL in [0, n_src) per trajectory.  The nets are
ItpNet modules (layers1 = layers2 = the hidden widths, so modes '1' and '2' are
two nets of one shape with different weights) built under a seeded generator
with torch.nn.Linear's default initialisation.

Bar: the project's 2e-5 max|ref| + 1e-6 (test_itp_interp_matches_oracle).  A
case is usable only if max|ref| >= MIN_SCALE = 0.25 (the absolute term is then
at most a fifth of the bar) and, where the net has a hidden layer, if zeroing
the outgoing weights of the last hidden unit moves the float64 result by at
least MUTATION_BARS = 10 bars (the bar sees one wrong unit); the input seed of
a case is the first of 1, 2, 3, ... for which both hold in float64 on the CPU
(INPUT_SEED lists the cases that need another seed than 1), and
test_itp_net_cases.py asserts both for every case.
"""
import functools

import torch

NB = 30
HIDDEN = ([], [1], [16], [17], [64, 32], [96, 40], [128, 64], [255, 33], [256, 256], [32, 48, 16],
          [40, 24, 56, 8], [256, 256, 256, 256])
SHAPES = ((1, 30, 1), (1, 30, 17), (3, 45, 33), (2, 37, 100))   # (B, n_src, n_qry)
MODES = ("1", "2")
MIN_SCALE = 0.25
MUTATION_BARS = 10.0
NET_SEED = 11

# (hidden, (B, n_src, n_qry), mode) -> input seed, where seed 1 misses a
# condition above (found in float64 on the CPU by find_seed; all at n_qry = 1,
# where max|ref| of a single query can fall to 0.01 .. 0.1)
INPUT_SEED = {
    ((64, 32), (1, 30, 1), "2"): 2,
    ((128, 64), (1, 30, 1), "2"): 2,
    ((255, 33), (1, 30, 1), "1"): 2,
    ((255, 33), (1, 30, 1), "2"): 3,
    ((256, 256), (1, 30, 1), "1"): 2,
    ((256, 256, 256, 256), (1, 30, 1), "1"): 3,
}


def hid(hidden):
    return "x".join(map(str, hidden)) or "none"


def bar(scale):
    return 2e-5 * scale + 1e-6


@functools.lru_cache(maxsize=None)
def module(hidden):
    """The ItpNet whose modes '1' / '2' are 62 -> hidden -> 30 (a 4-point
    cylinder-style module: its res_cut network is not used here)."""
    from mmpde_amd.interpolate import ItpNet

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(NET_SEED + 7919 * len(hidden) + sum((i + 1) * w for i, w in enumerate(hidden)))
        m = ItpNet(4, None, list(hidden), list(hidden), [])
    return m.eval()


def weights(hidden, mode):
    mods = module(tuple(hidden)).layers if mode == "1" else module(tuple(hidden)).layers2
    return [(m.weight.detach().cpu().clone(), m.bias.detach().cpu().clone()) for m in mods]


def interp_ref(c, wb, dtype, drop_unit=False):
    """sum_e W[q, e] vals[b, idx[b, q, e]], W = the tanh MLP (linear last layer)
    of x = (the 30 neighbours' coordinates, the query's): [B n_qry] in `dtype`.
    drop_unit: the last hidden unit's outgoing weights zeroed."""
    idx = c["idx"].long()
    b = torch.arange(c["B"])[:, None, None]
    x = torch.cat((c["src"].to(dtype)[b, idx].reshape(c["B"], c["n_qry"], 2 * NB), c["qry"].to(dtype)), -1)
    for i, (w, bias) in enumerate(wb):
        w = w.to(dtype)
        if drop_unit and i == len(wb) - 1:
            w = w.clone()
            w[:, -1] = 0
        x = x @ w.t() + bias.to(dtype)
        if i != len(wb) - 1:
            x = torch.tanh(x)
    return (x * c["vals"].to(dtype)[b, idx]).sum(-1).reshape(-1)


def inputs(B, n_src, n_qry, seed):
    g = torch.Generator().manual_seed(seed + 1000003 * B + 1009 * n_src + 31 * n_qry)
    return dict(B=B, n_src=n_src, n_qry=n_qry,
                src=torch.rand(B, n_src, 2, generator=g), qry=torch.rand(B, n_qry, 2, generator=g),
                vals=torch.randn(B, n_src, generator=g),
                idx=torch.randint(0, n_src, (B, n_qry, NB), generator=g, dtype=torch.int32),
                addend=torch.randn(B * n_qry, generator=g), addend2=torch.randn(B * n_qry, generator=g))


def usable(c, wb):
    """(max|ref|, the mutation's shift in bars or None without a hidden layer)."""
    ref = interp_ref(c, wb, torch.float64)
    scale = ref.abs().max().item()
    if len(wb) == 1:
        return scale, None
    moved = (interp_ref(c, wb, torch.float64, drop_unit=True) - ref).abs().max().item()
    return scale, moved / bar(scale)


def find_seed(hidden, shape, mode, tries=40):
    """The first input seed that meets both conditions (how INPUT_SEED was filled)."""
    wb = weights(hidden, mode)
    for seed in range(1, tries + 1):
        scale, bars = usable(inputs(*shape, seed), wb)
        if scale >= MIN_SCALE and (bars is None or bars >= MUTATION_BARS):
            return seed
    raise AssertionError(f"no usable input seed for {hidden} {shape} mode {mode}")


@functools.lru_cache(maxsize=None)
def case(hidden, shape, mode):
    """Inputs, weights, the float64 reference and the CPU fp32 evaluation of one
    case (built once, never modified).  hidden: a tuple."""
    c = inputs(*shape, INPUT_SEED.get((hidden, shape, mode), 1))
    c["wb"] = weights(hidden, mode)
    c["ref"] = interp_ref(c, c["wb"], torch.float64)
    c["cpu32"] = interp_ref(c, c["wb"], torch.float32).double()
    return c


def all_cases():
    return [(tuple(h), s, m) for h in HIDDEN for s in SHAPES for m in MODES]


def case_id(hidden, shape, mode):
    return f"{hid(hidden)}-{shape[0]}x{shape[1]}x{shape[2]}-m{mode}"
