"""The fused ItpNet interpolation (itp_interp_kernel, itp.hip; interpolate.py:77-93
with the weighted sum of data_creator_2d.py:80-83) against a plain float64
evaluation on a given neighbour table, at the shapes where the kernel takes
another path: fewer than 16 queries, partial 16-query tiles, n_qry != n_src
both ways, the smallest n_src = 30, fewer tiles than workgroups, and a second
trip of the grid-stride loop (16 C + 1 tiles on 2 C workgroups of 8 waves, C =
compute units) that holds only a partial tile.

idx is uniform in [0, n_src) per trajectory (LOCAL indices), coordinates are
uniform in the unit square, the weights are build_models("cy")'s ItpNet in
modes '1' and '2'.  Bar: 2e-5 max|ref| + 1e-6 (test_itp_interp_matches_oracle);
the same function in torch fp32 on the CPU is printed beside the kernel's error.

out is 64 floats longer than B n_qry and sentinel-filled: the tail must come
back bit for bit.  The addend / addend2 epilogue is compared bit for bit with
fp32 sums of the plain launch in the order the header documents, (addend +
interp) + addend2; mmpde_itp_interp equals mmpde_itp_interp_ex without
addend2; a second launch gives the same bits.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

NB = 30
PAD = 64
SENTINEL = -54321.125
SMALL = [(1, 30, 1), (1, 30, 15), (1, 30, 16), (1, 30, 17), (3, 45, 33), (2, 100, 7), (2, 7 + 30, 100)]


@functools.lru_cache(maxsize=None)
def _itp():
    from mmpde_amd.synth import build_models

    return build_models("cy")[3]


@functools.lru_cache(maxsize=None)
def _case(B, n_src, n_qry, mode):
    """Inputs, the float64 reference and the CPU fp32 evaluation (built once, never modified)."""
    g = torch.Generator().manual_seed(7 + 1000003 * B + 1009 * n_src + n_qry + int(mode))
    c = dict(B=B, n_src=n_src, n_qry=n_qry,
             src=torch.rand(B, n_src, 2, generator=g), qry=torch.rand(B, n_qry, 2, generator=g),
             vals=torch.randn(B, n_src, generator=g),
             idx=torch.randint(0, n_src, (B, n_qry, NB), generator=g, dtype=torch.int32),
             addend=torch.randn(B * n_qry, generator=g), addend2=torch.randn(B * n_qry, generator=g))
    mods = _itp().layers if mode == "1" else _itp().layers2
    wb = [(m.weight.detach().cpu(), m.bias.detach().cpu()) for m in mods]
    c["ref"] = _interp_ref(c, wb, torch.float64)
    c["cpu32"] = _interp_ref(c, wb, torch.float32).double()
    return c


def _interp_ref(c, wb, dtype):
    """sum_e W[q, e] vals[b, idx[b, q, e]], W = Linear(tanh(Linear(tanh(Linear(x))))) of
    x = (the 30 neighbours' coordinates, the query's): [B n_qry] in `dtype`."""
    idx = c["idx"].long()
    b = torch.arange(c["B"])[:, None, None]
    x = torch.cat((c["src"].to(dtype)[b, idx].reshape(c["B"], c["n_qry"], 2 * NB), c["qry"].to(dtype)), -1)
    for i, (w, bias) in enumerate(wb):
        x = x @ w.to(dtype).t() + bias.to(dtype)
        if i != len(wb) - 1:
            x = torch.tanh(x)
    return (x * c["vals"].to(dtype)[b, idx]).sum(-1).reshape(-1)


def _launch(c, mode, dev, addend=None, addend2=None, ex=True):
    """One launch into a guarded out buffer: [B n_qry] after the guard checks."""
    from mmpde_amd import _lib as L

    itp = _itp().to(dev)
    packed = itp.packed(mode)
    total = c["B"] * c["n_qry"]
    src, qry, vals, idx = (c[x].to(dev).contiguous() for x in ("src", "qry", "vals", "idx"))
    out = torch.full((total + PAD,), float("nan"), dtype=torch.float32, device=dev)
    out[total:] = SENTINEL
    bits = out.view(torch.int32).clone()
    args = (L.ptr(src), L.ptr(vals), L.ptr(qry), L.ptr(idx), c["B"], c["n_src"], c["n_qry"], L.ptr(packed))
    if ex:
        L.check(L.lib().mmpde_itp_interp_ex(*args, L.ptr(addend), L.ptr(addend2), L.ptr(out), L.stream(dev)),
                "mmpde_itp_interp_ex")
    else:
        assert addend2 is None
        L.check(L.lib().mmpde_itp_interp(*args, L.ptr(addend), L.ptr(out), L.stream(dev)), "mmpde_itp_interp")
    torch.cuda.synchronize()
    assert torch.isfinite(out[:total]).all()
    assert torch.equal(out.view(torch.int32)[total:], bits[total:])
    return out[:total]


def _check(c, mode, dev, tag):
    ref = c["ref"]
    base = _launch(c, mode, dev)
    scale = ref.abs().max().item()
    err = (base.double().cpu() - ref).abs().max().item()
    floor = (c["cpu32"] - ref).abs().max().item()
    print(f"{tag}: max|ref| {scale:.3e} max|err| {err:.3e} ({err / scale:.2e} of max|ref|), torch fp32 on the CPU "
          f"{floor:.3e} ({floor / scale:.2e})")
    assert err <= 2e-5 * scale + 1e-6
    assert torch.equal(_launch(c, mode, dev), base)
    a1, a2 = c["addend"].to(dev), c["addend2"].to(dev)
    assert torch.equal(_launch(c, mode, dev, addend=a1), a1 + base)
    assert torch.equal(_launch(c, mode, dev, addend=a1, addend2=a2), (a1 + base) + a2)
    assert torch.equal(_launch(c, mode, dev, addend2=a2), base + a2)
    assert torch.equal(_launch(c, mode, dev, ex=False), base)
    assert torch.equal(_launch(c, mode, dev, addend=a1, ex=False), a1 + base)


@pytest.mark.parametrize("mode", ["1", "2"])
@pytest.mark.parametrize("B,n_src,n_qry", SMALL, ids=[f"{b}x{s}x{q}" for b, s, q in SMALL])
def test_itp_interp_shapes(dev, B, n_src, n_qry, mode):
    _check(_case(B, n_src, n_qry, mode), mode, dev, f"itp mode {mode} B={B} n_src={n_src} n_qry={n_qry}")


@pytest.mark.parametrize("mode", ["1", "2"])
def test_itp_interp_second_trip(dev, mode):
    """16 C + 1 query tiles: every wave of the 2 C workgroups takes one tile, and
    the first wave of the first workgroup comes round again for the last,
    partial one."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    n_qry = 16 * 16 * cus + 5
    tiles = (n_qry + 15) // 16
    blocks = min(2 * cus, tiles)
    trips = -(-tiles // (8 * blocks))
    print(f"{cus} compute units: n_qry {n_qry}, {tiles} tiles on {blocks} workgroups of 8 waves, {trips} trips")
    assert trips == 2 and tiles - 8 * blocks == 1
    _check(_case(1, NB, n_qry, mode), mode, dev, f"itp mode {mode} B=1 n_src={NB} n_qry={n_qry}")
