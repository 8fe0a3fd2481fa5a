"""An ItpNet with other widths than the reference's defaults through the product
path: build_models("cy" | "burgers") with itp replaced by a seeded
ItpNet(..., [96, 40], [48, 24], [1, 4, 16, 4, 1]) (three Linears per mode, which
the oracle evaluates; modes '1' and '2' of different shapes), at B = 2:

- GraphCreator_FS_2D.interpolate modes '1' / '2' and interpolate_pred against
  oracle/refcpu.py (bars of test_gpu_api.py: 2e-5 of max|ref| + 1e-7);
- one MMPDERollout.step against the oracle's step, composed as
  test_gpu_parity.py's test_mmpde_step_matches_oracle, bar 2.5e-5 max|ref|;
- two fed-back steps through enable_graph / graph_step, bit for bit the eager ones;
- an engine with the default widths in the same process still takes the
  specialised entry (a bare image of mmpde_itp_pack_bytes() bytes) and keeps its
  bits after the other engine ran.

On the parent commit ItpNet.packed() raises NotImplementedError for these widths.
"""
import pytest
import torch

from oracle import refcpu

pytestmark = pytest.mark.gpu

NODE1, NODE2 = [96, 40], [48, 24]


def _close(got, ref, rtol, atol=0.0, what=""):
    got = got.detach().float().cpu().reshape(-1)
    ref = ref.detach().float().cpu().reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    bound = rtol * ref.abs().max().item() + atol
    print(f"{what}: max|err| {err:.3e} bound {bound:.3e} max|ref| {ref.abs().max().item():.3e}")
    assert err <= bound, (what, err, bound)


def _sds(**mods):
    return {k: {n: t.detach().cpu() for n, t in m.state_dict().items()} for k, m in mods.items()}


def _setup(kind, B=2, seed=0, default_itp=False):
    """build_models(kind) with the ItpNet of other widths, fields [B, T, ...] and the oracle's PDE."""
    from mmpde_amd.interpolate import ItpNet
    from mmpde_amd.synth import build_models, burgers_grid_points, fields

    pde, model, model_b, itp, dmm, gc = build_models(kind, seed=seed)
    if not default_itp:
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed + 77)
            nx, ny = (pde.ori_grid.shape[0], None) if kind == "cy" else (48, 48)
            itp = ItpNet(nx, ny, NODE1, NODE2, [1, 4, 16, 4, 1]).eval()
    if kind == "cy":
        u = fields(pde.ori_grid, B, 30, seed=seed + 1)
        opde = refcpu.PDEConst("cy", pde.grid_size, ori_grid=pde.ori_grid)
    else:
        u = fields(burgers_grid_points(), B, 31, seed=seed + 1).reshape(B, 31, 48, 48)
        opde = refcpu.PDEConst("burgers", pde.grid_size)
    return pde, opde, model, model_b, itp, dmm, gc, u


@pytest.mark.parametrize("kind", ["cy", "burgers"])
@pytest.mark.parametrize("mode", ["1", "2"])
def test_interpolate_method_other_widths_vs_oracle(dev, kind, mode):
    from mmpde_amd import ops
    from mmpde_amd.synth import burgers_grid_points

    pde, opde, model, model_b, itp, dmm, gc, u = _setup(kind, seed=4)
    B = 2
    pts = pde.ori_grid if kind == "cy" else burgers_grid_points()
    g = torch.Generator().manual_seed(11)
    src = pts.repeat(B, 1)
    qry = (pts.repeat(B, 1) + 0.004 * torch.randn(src.shape, generator=g)).clamp(0, 1)
    vals = u[:, 5].reshape(B, *u.shape[2:])
    ref = refcpu.interpolate(_sds(i=itp)["i"], vals, src[:, :1], src[:, 1:], qry[:, :1], qry[:, 1:], mode)
    itp.to(dev)
    pack = itp.packed(mode)
    assert isinstance(pack, ops.ItpNetPack) and pack.widths == [62] + (NODE1 if mode == "1" else NODE2) + [30]
    d = [t.to(dev) for t in (vals, src[:, :1], src[:, 1:], qry[:, :1], qry[:, 1:])]
    got = gc.interpolate(itp, *d, mode)
    assert got.shape == ref.shape
    _close(got, ref, 2e-5, 1e-7, f"{kind} interpolate mode {mode}, widths {pack.widths}")


@pytest.mark.parametrize("kind", ["cy", "burgers"])
def test_interpolate_pred_and_step_other_widths_vs_oracle(dev, kind):
    from mmpde_amd.rollout import MMPDERollout

    pde, opde, model, model_b, itp, dmm, gc, u = _setup(kind)
    B, step = 2, 6
    steps = [step] * B
    sds = _sds(model=model, model_b=model_b, itp=itp, dmm=dmm)
    for m in (model, model_b, itp, dmm):
        m.to(dev)
    data, labels = gc.create_data(u, steps)

    # interpolate_pred on the drop-in path, the oracle on the engine's moved mesh
    graph = gc.create_graph(itp, data, labels, steps, dev, dmm)
    mesh = graph.pos[:, 1:3].cpu()
    rg = refcpu.create_graph(opde, sds["itp"], data, labels, steps, mesh_override=mesh)
    if kind == "burgers":   # data interpolated onto the moved mesh (ItpNet mode '1')
        _close(graph.x, rg.x, 2e-5, 1e-7, "burgers create_graph x (ItpNet mode 1)")
    out_b = model_b(graph)
    ip = gc.interpolate_pred(itp, out_b, graph, data, dev)
    rip = refcpu.interpolate_pred(opde, sds["itp"], out_b.cpu(), rg, data)
    _close(ip, rip, 2e-5, 1e-7, f"{kind} interpolate_pred")

    # one step of the rollout engine
    d = u[:, step - 1:step]
    eng = MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev)
    pred = eng.step(d[:, 0].to(dev), step)
    ref, aux = refcpu.mmpde_step(opde, sds, d, d, steps, mesh_override=eng.mesh.cpu())
    assert torch.equal(eng.nbr_u.cpu().long(), aux["graph_uni"].nbr)
    _close(pred, ref, 2.5e-5, 0.0, f"mmpde step {kind}, ItpNet {NODE1} / {NODE2}")


@pytest.mark.parametrize("kind", ["cy", "burgers"])
def test_graph_replay_other_widths_matches_eager(dev, kind):
    from mmpde_amd.rollout import MMPDERollout

    pde, opde, model, model_b, itp, dmm, gc, u = _setup(kind)
    B = 2
    for m in (model, model_b, itp, dmm):
        m.to(dev)
    eng = MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev)
    u0 = u[:, 3].to(dev).contiguous()
    ref, v = [], u0
    for s in (4, 5):
        v = eng.step(v, s)
        ref.append(v.clone())
    eng.enable_graph(u0)
    v = u0
    for i, s in enumerate((4, 5)):
        v = eng.graph_step(v, s)
        assert torch.equal(v, ref[i]), f"{kind} graph step {s}: max|diff| {(v - ref[i]).abs().max()}"


def test_default_widths_keep_the_specialised_entry(dev):
    """The shape is a property of the pack, not of the process: the default engine
    before and after an engine of other widths ran."""
    from mmpde_amd import _lib as L
    from mmpde_amd.rollout import MMPDERollout

    kind, B, step = "cy", 2, 5
    pde, _, model, model_b, itp, dmm, gc, u = _setup(kind, default_itp=True)
    _, _, _, _, itp2, _, _, _ = _setup(kind)
    for m in (model, model_b, itp, itp2, dmm):
        m.to(dev)
    u0 = u[:, step - 1].to(dev).contiguous()
    eng = MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev)
    image = itp.packed("2")
    assert isinstance(image, torch.Tensor) and image.numel() * 4 == L.lib().mmpde_itp_pack_bytes()
    before = eng.step(u0, step).clone()
    other = MMPDERollout(kind, model, model_b, itp2, dmm, gc, B, dev)
    moved = other.step(u0, step).clone()
    assert not torch.equal(moved, before)          # another interpolation network
    assert itp.packed("2") is image
    assert torch.equal(eng.step(u0, step), before)
    fresh = MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev)
    assert torch.equal(fresh.step(u0, step), before)
