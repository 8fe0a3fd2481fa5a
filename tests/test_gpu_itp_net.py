"""The shape-generic fused ItpNet interpolation (itp_net_kernel, itp_net.hip;
mmpde_itp_net_pack / mmpde_itp_interp_net) against the float64 evaluation of
itp_net_cases.py: every hidden-width list of the issue (0 to 4 hidden layers,
widths 1 to 256, the three instantiations of the kernel and every padded /
unpadded tile edge) at four query shapes, in both modes of the module.

Bar: 2e-5 max|ref| + 1e-6; torch fp32 on the CPU is printed beside the kernel's
error.  out is 64 floats longer than B n_qry and sentinel-filled: the tail must
come back bit for bit.  A second launch repeats the bits; addend / addend2 are
fp32 device sums of the plain launch in the header's order (addend + interp) +
addend2, bit for bit; trajectory 1 of the B = 3 case launched alone has the bits
it has in the batch.  [128, 64] runs the generic kernel (packed(generic=True))
and is compared with itp_interp_kernel on the same inputs.  The second trip of
the grid-stride loop is computed from the launch geometry of mmpde_hip.h.

On the parent commit every test here fails: ItpNet.packed() has no ``generic``
argument and raises NotImplementedError for other widths, and the library has
no mmpde_itp_net_* exports.
"""
import ctypes

import pytest
import torch

import itp_net_cases as C

pytestmark = pytest.mark.gpu

PAD = 64
SENTINEL = -54321.125
CASES = C.all_cases()
IDS = [C.case_id(*k) for k in CASES]


def _pack(hidden, mode, dev):
    """The generic pack of the case's net (an ops.ItpNetPack), also at the default widths."""
    from mmpde_amd import ops

    pack = C.module(hidden).to(dev).packed(mode, generic=True)
    assert isinstance(pack, ops.ItpNetPack) and pack.widths == [62] + list(hidden) + [30]
    return pack


def _launch(c, pack, dev, addend=None, addend2=None, image=None):
    """One launch into a guarded out buffer: [B n_qry] after the guard checks."""
    from mmpde_amd import _lib as L

    total = c["B"] * c["n_qry"]
    src, qry, vals, idx = (c[x].to(dev).contiguous() for x in ("src", "qry", "vals", "idx"))
    out = torch.full((total + PAD,), float("nan"), dtype=torch.float32, device=dev)
    out[total:] = SENTINEL
    bits = out.view(torch.int32).clone()
    image = pack.image if image is None else image
    L.check(L.lib().mmpde_itp_interp_net(L.ptr(src), L.ptr(vals), L.ptr(qry), L.ptr(idx), c["B"], c["n_src"],
                                         c["n_qry"], ctypes.byref(pack.shape), L.ptr(image), pack.nbytes,
                                         L.ptr(addend), L.ptr(addend2), L.ptr(out), L.stream(dev)),
            "mmpde_itp_interp_net")
    torch.cuda.synchronize()
    assert torch.isfinite(out[:total]).all()
    assert torch.equal(out.view(torch.int32)[total:], bits[total:])
    return out[:total]


def _check(c, pack, dev, tag):
    ref = c["ref"]
    base = _launch(c, pack, dev)
    scale = ref.abs().max().item()
    err = (base.double().cpu() - ref).abs().max().item()
    floor = (c["cpu32"] - ref).abs().max().item()
    print(f"{tag}: max|ref| {scale:.3e} max|err| {err:.3e} ({err / scale:.2e} of max|ref|, "
          f"{err / C.bar(scale):.3f} bar), torch fp32 on the CPU {floor:.3e} ({floor / scale:.2e})")
    assert scale >= C.MIN_SCALE
    assert err <= C.bar(scale)
    assert torch.equal(_launch(c, pack, dev), base)
    a1, a2 = c["addend"].to(dev), c["addend2"].to(dev)
    assert torch.equal(_launch(c, pack, dev, addend=a1), a1 + base)
    assert torch.equal(_launch(c, pack, dev, addend=a1, addend2=a2), (a1 + base) + a2)
    assert torch.equal(_launch(c, pack, dev, addend2=a2), base + a2)
    return base


@pytest.mark.parametrize("hidden,shape,mode", CASES, ids=IDS)
def test_itp_net_shapes(dev, hidden, shape, mode):
    c = C.case(hidden, shape, mode)
    pack = _pack(hidden, mode, dev)
    base = _check(c, pack, dev, C.case_id(hidden, shape, mode))
    if c["B"] == 3:
        # trajectory 1 alone: a query's result depends on its own column only
        one = dict(B=1, n_src=c["n_src"], n_qry=c["n_qry"],
                   **{k: c[k][1:2] for k in ("src", "qry", "vals", "idx")})
        assert torch.equal(_launch(one, pack, dev), base[c["n_qry"]:2 * c["n_qry"]])


def test_itp_net_through_ops_dispatch(dev):
    """ops.itp_interp takes the pack object (mmpde_itp_interp_net) and gives the raw entry's bits."""
    from mmpde_amd import ops

    hidden, shape, mode = (96, 40), (3, 45, 33), "2"
    c = C.case(hidden, shape, mode)
    itp = C.module(hidden).to(dev)
    pack = itp.packed(mode)                      # not the default widths: generic without asking
    assert isinstance(pack, ops.ItpNetPack) and itp.packed(mode) is pack
    a1, a2 = c["addend"].to(dev), c["addend2"].to(dev)
    args = (c["src"].to(dev), c["vals"].to(dev), c["qry"].to(dev), c["idx"].to(dev), c["B"], pack)
    assert torch.equal(ops.itp_interp(*args), _launch(c, pack, dev))
    assert torch.equal(ops.itp_interp(*args, addend=a1, addend2=a2), _launch(c, pack, dev, addend=a1, addend2=a2))


def test_itp_net_limits_raise(dev):
    from mmpde_amd.interpolate import ItpNet

    for hidden in ([257], [8, 8, 8, 8, 8], [64, 300]):
        itp = ItpNet(4, None, hidden, [128, 64], []).to(dev)
        with pytest.raises(NotImplementedError, match="at most 4 hidden layers of width 1 to 256"):
            itp.packed("1")
        assert isinstance(itp.packed("2"), torch.Tensor)   # the other mode's default net is served


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("shape", C.SHAPES, ids=[f"{b}x{s}x{q}" for b, s, q in C.SHAPES])
def test_itp_net_default_widths_against_specialised_kernel(dev, shape, mode):
    """[128, 64] on the generic kernel and on itp_interp_kernel, same inputs:
    within the bar of each other (both are within it of float64); the print
    says whether the bits agree."""
    from mmpde_amd import _lib as L

    hidden = (128, 64)
    c = C.case(hidden, shape, mode)
    gen = _launch(c, _pack(hidden, mode, dev), dev)
    image = C.module(hidden).to(dev).packed(mode)
    assert isinstance(image, torch.Tensor) and image.numel() * 4 == L.lib().mmpde_itp_pack_bytes()
    src, qry, vals, idx = (c[x].to(dev).contiguous() for x in ("src", "qry", "vals", "idx"))
    spec = torch.empty_like(gen)
    L.check(L.lib().mmpde_itp_interp_ex(L.ptr(src), L.ptr(vals), L.ptr(qry), L.ptr(idx), c["B"], c["n_src"],
                                        c["n_qry"], L.ptr(image), None, None, L.ptr(spec), L.stream(dev)),
            "mmpde_itp_interp_ex")
    torch.cuda.synchronize()
    diff = (gen.double() - spec.double()).abs().max().item()
    scale = c["ref"].abs().max().item()
    print(f"[128, 64] mode {mode} {shape}: generic vs specialised max|diff| {diff:.3e} "
          f"({diff / C.bar(scale):.3f} bar), bitwise equal: {torch.equal(gen, spec)}")
    assert diff <= C.bar(scale)


@pytest.mark.parametrize("mode", C.MODES)
def test_itp_net_second_trip(dev, mode):
    """The smallest n_qry at which some wave takes a second tile (mmpde_hip.h: G =
    min(ceil(tiles / 4), 4 C) workgroups of 4 waves, wave w of workgroup g takes
    tiles (4 r + w) G + g): 16 C + 1 tiles, the last one a single query, taken
    by wave 0 of workgroup 0 on its second trip."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    def geometry(n):
        tiles = (n + 15) // 16
        blocks = min(-(-tiles // 4), 4 * cus)
        return tiles, blocks, -(-tiles // (4 * blocks))

    n_qry = 16 * 16 * cus + 1
    tiles, blocks, trips = geometry(n_qry)
    print(f"{cus} compute units: n_qry {n_qry}, {tiles} tiles on {blocks} workgroups of 4 waves, {trips} trips")
    assert trips == 2 and tiles - 4 * blocks == 1 and n_qry % 16 == 1
    assert geometry(n_qry - 1)[2] == 1   # one query fewer: every wave takes one tile
    hidden = (17,)
    c = C.case(hidden, (1, C.NB, n_qry), mode)
    _check(c, _pack(hidden, mode, dev), dev, f"17 second trip mode {mode} n_qry={n_qry}")


@pytest.mark.parametrize("hidden", [(), (1,), (17,), (255, 33), (40, 24, 56, 8)], ids=C.hid)
def test_itp_net_pack_writes_every_element(dev, hidden):
    """A 0xFF-filled buffer that is then packed equals a zeroed one that is then
    packed, bit for bit, and gives the same result bits."""
    from mmpde_amd import _lib as L

    mode = "1"
    pack = _pack(hidden, mode, dev)
    itp = C.module(hidden).to(dev)
    net = L.ItpNetShape.from_buffer_copy(pack.shape)
    for i, m in enumerate(itp.layers):
        net.w[i], net.b[i] = m.weight.data_ptr(), m.bias.data_ptr()
    assert L.lib().mmpde_itp_net_pack_bytes(ctypes.byref(net)) == pack.nbytes == pack.image.numel() * 4
    imgs = []
    for fill in (-1, 0):
        buf = torch.full((pack.nbytes // 4,), fill, dtype=torch.int32, device=dev)
        L.check(L.lib().mmpde_itp_net_pack(ctypes.byref(net), L.ptr(buf), pack.nbytes, L.stream(dev)),
                "mmpde_itp_net_pack")
        imgs.append(buf)
    torch.cuda.synchronize()
    assert torch.equal(imgs[0], imgs[1]) and torch.equal(imgs[0], pack.image.view(torch.int32))
    c = C.case(hidden, (3, 45, 33), mode)
    assert torch.equal(_launch(c, pack, dev, image=imgs[0].view(torch.float32)), _launch(c, pack, dev))
