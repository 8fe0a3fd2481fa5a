"""The DMM mesh mover's kernels (dmm.hip) against float64 at the shapes where
they take another path.  Inputs, references and bars: dmm_shape_cases.py; that
the bars can see a one-slot / one-weight error: test_dmm_shape_cases.py.

(a) graph branch (DMM.branch_features with a random [N, k] table) vs float64,
    bar 1e-5 of max|ref|: n_per = k + 1, around the 128-target block of
    dmm_gnn_lds_kernel, the second trip of its staging loop, 2340 (staging
    below 64 KiB, staging + static weights above), 4388 (largest LDS size),
    4389 (dmm_gnn_kernel, the global-memory layer; B = 3: a workgroup spans
    two trajectories); k = 1 .. 65 (one to three trips of the edge loop, ragged
    last quad); 0 .. 3 GNN layers; B = 1 and 65 (split-K scratch past 64 rows).
(b) array branch vs float64 refcpu.convnet, bar 1e-5 of max|ref|: s = 5 .. 48.
(c) mesh vs float64 autograd on the displacement, max|(mesh - xi) - disp_ref|
    <= 2e-5 max|disp_ref| + 2^-23 max|xi| (the second term is the rounding of
    the stored fp32 coordinate): heads (th, L, L') off the shipped ones, n_per
    around the four-point workgroup of mesh_vjp_wave_kernel<8>, B = 32 (its LDS
    limit) and 33, 65 (mesh_vjp_kernel), array mode at s = 33; with and without
    a head cache (same bits).
(d) mmpde_dmm_phi through DMM.forward(rf=True) vs float64, bar 2e-5 of
    max|ref| for phi and for second_out: 1, 5, 131 rows per trajectory.
(e) a trajectory's mesh and branch rows do not depend on the batch it runs in,
    bit for bit, across B = 32 | 33 (the two VJP kernels) and 64 | 65.
(f) every branch and mesh call of (a) - (c) runs on a workspace filled with
    0xFF bytes (NaN floats, non-zero split-K tickets) and on a zeroed one:
    same bits.

Measured on MI355X, the worst case of each family (no case past 0.09 bar, so
no bar was raised and the fp32 CPU oracle's error is printed nowhere):
    graph branch  8.9e-7 of max|ref| (n_per 513); dmm_gnn_kernel (4389) 6.7e-7
    array branch  4.2e-7 of max|ref| (s = 33, B = 3)
    mesh          0.063 bar: 5.6e-8 on max|disp| 3.9e-2 (head (1, 8, 128)),
                  7.2e-8 on 5.1e-2 (array, B = 3)
    phi           1.3e-6 of max|ref| (1 row per trajectory); second_out 1.0e-6
    (e), (f)      no differing bit
"""
import pytest
import torch

import dmm_shape_cases as C

pytestmark = pytest.mark.gpu


def _ids(cases):
    return ["-".join(str(x) for x in (c if not isinstance(c[-1], tuple) else c[:-1] + c[-1])) for c in cases]


def _ws(dmm, B, n, dev, byte):
    """A workspace of mmpde_dmm_workspace_bytes filled with `byte`."""
    from mmpde_amd import _lib as L

    _, hd = dmm.device_params()
    nb = L.lib().mmpde_dmm_workspace_bytes(B, n, hd.latent, hd.hidden)
    assert nb > 0 and nb % 4 == 0
    return torch.full((nb,), byte, dtype=torch.uint8, device=dev).view(torch.float32)


def _n_ws(c):
    return c.grid.shape[0] if c.mode == "graph" else max(c.xi.shape[0], c.s * c.s)


def _branch(c, dev, u=None):
    """branch_features on a 0xFF workspace and on a zeroed one (same bits)."""
    dmm = c.dmm.to(dev)
    u = (c.u if u is None else u).to(dev)
    nbr = c.nbr.to(dev) if c.mode == "graph" else None
    outs = [dmm.branch_features(u, nbr=nbr, workspace=_ws(dmm, u.shape[0], _n_ws(c), dev, byte))
            for byte in (0xFF, 0)]
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), "the branch depends on what its workspace held"
    return outs[0]


def _mesh(c, dev, u=None, cached=True):
    """mesh on a 0xFF workspace, on a zeroed one and with a head cache (same bits)."""
    dmm = c.dmm.to(dev)
    u = (c.u if u is None else u).to(dev)
    xi = c.xi.to(dev)
    kw = {"nbr": c.nbr.to(dev)} if c.mode == "graph" else {}
    outs = [dmm.mesh(u, xi, workspace=_ws(dmm, u.shape[0], _n_ws(c), dev, byte), **kw) for byte in (0xFF, 0)]
    if cached:
        outs.append(dmm.mesh(u, xi, head_cache=dmm.head_cache(xi), **kw))
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), "the mesh depends on what its workspace held"
    if cached:
        assert torch.equal(outs[0], outs[2]), "the mesh with a head cache differs"
    return outs[0]


def _report(tag, err, bar, scale, cpu32):
    """Print the figures; past half a bar, the fp32 CPU oracle's error beside them."""
    msg = f"{tag}: max|ref| {scale:.3e} max|err| {err:.3e} = {err / bar:.3f} bar"
    if err > 0.5 * bar:
        msg += f"; fp32 CPU oracle {cpu32():.3e}"
    print(msg)
    return msg


# --------------------------------------------------------------------------- (a) (b) branch
@pytest.mark.parametrize("n_per,k,nl,B", C.GRAPH_BRANCH_CASES, ids=_ids(C.GRAPH_BRANCH_CASES))
def test_graph_branch_vs_float64(dev, n_per, k, nl, B):
    c = C.graph_case(n_per, k, nl, B)
    ref = C.branch_ref(c)
    got = _branch(c, dev).double().cpu()
    assert got.shape == ref.shape == (B, c.head[1])
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    msg = _report(f"graph branch n_per={n_per} k={k} nl={nl} B={B}", err, C.BRANCH_BAR * scale, scale,
                  lambda: (C.branch_ref(c, torch.float32).double() - ref).abs().max().item())
    assert err <= C.BRANCH_BAR * scale, msg


@pytest.mark.parametrize("s,B", C.ARRAY_BRANCH_CASES, ids=_ids(C.ARRAY_BRANCH_CASES))
def test_array_branch_vs_float64(dev, s, B):
    c = C.array_case(s, B)
    ref = C.branch_ref(c)
    got = _branch(c, dev).double().cpu()
    assert got.shape == ref.shape == (B, 512)
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    msg = _report(f"array branch s={s} B={B}", err, C.BRANCH_BAR * scale, scale,
                  lambda: (C.branch_ref(c, torch.float32).double() - ref).abs().max().item())
    assert err <= C.BRANCH_BAR * scale, msg


# --------------------------------------------------------------------------- (c) mesh
def _mesh_vs_float64(c, dev, tag):
    ref = C.disp_ref(c)
    scale = ref.abs().max().item()
    assert scale > 1e-3, (tag, scale)
    bar = C.mesh_bar(c, ref)
    mesh = _mesh(c, dev)
    assert mesh.shape == ref.shape == (c.B * c.xi.shape[0], 2)
    disp = mesh.double().cpu() - c.xi.double().repeat(c.B, 1)
    err = (disp - ref).abs().max().item()
    msg = _report(tag + " displacement", err, bar, scale,
                  lambda: (C.disp_ref(c, torch.float32).double() - ref).abs().max().item())
    assert err <= bar, msg


@pytest.mark.parametrize("n_per,B,head", C.GRAPH_MESH_CASES, ids=_ids(C.GRAPH_MESH_CASES))
def test_graph_mesh_vs_float64(dev, n_per, B, head):
    _mesh_vs_float64(C.graph_case(n_per, 5, 1, B, head, False), dev, f"graph mesh n_per={n_per} B={B} head={head}")


@pytest.mark.parametrize("s,B", C.ARRAY_MESH_CASES, ids=_ids(C.ARRAY_MESH_CASES))
def test_array_mesh_vs_float64(dev, s, B):
    _mesh_vs_float64(C.array_case(s, B), dev, f"array mesh s={s} B={B}")


# --------------------------------------------------------------------------- (d) phi
PHI_CASES = [(1, 3, C.DEFAULT_HEAD), (5, 3, C.DEFAULT_HEAD), (5, 1, (1, 512, 128)), (131, 3, C.DEFAULT_HEAD)]


@pytest.mark.parametrize("rows,B,head", PHI_CASES, ids=_ids(PHI_CASES))
def test_phi_vs_float64(dev, rows, B, head):
    """The array branch at s = 7 feeds the head: forward needs no neighbour table then."""
    c = C.array_case(7, B, head)
    g = torch.Generator().manual_seed(100 * rows + B)
    grid = torch.rand(B * rows, 2, generator=g)
    ref, ref2 = C.phi_ref(c, grid)
    dmm = c.dmm.to(dev)
    phi, second, ones = dmm(c.u.to(dev), grid.to(dev), rf=True)
    assert torch.equal(dmm(c.u.to(dev), grid.to(dev)), phi), "rf=True phi differs"
    assert phi.shape == ref.shape == (B * rows, 1) and second.shape == ref2.shape == (B * rows, head[2])
    assert ones.shape == (second.numel(), 1) and bool((ones == 1).all())
    tag = f"phi rows={rows} B={B} head={head}"
    for i, (what, got, r) in enumerate((("phi", phi, ref), ("second_out", second, ref2))):
        scale = r.abs().max().item()
        err = (got.double().cpu() - r).abs().max().item()
        msg = _report(f"{tag} {what}", err, C.PHI_BAR * scale, scale,
                      lambda: (C.phi_ref(c, grid, torch.float32)[i].double() - r).abs().max().item())
        assert err <= C.PHI_BAR * scale, msg
    # second_out is the tanh layer that produced phi (test_gpu_dmm_api.py's check)
    L2 = dmm.out_nn.layers[1]
    lin = second.double().cpu() @ L2.weight.detach().double().cpu().t() + L2.bias.detach().double().cpu()
    err = (phi.double().cpu() - lin).abs().max().item()
    assert err <= 1e-6 * lin.abs().max().item() + 1e-6, (tag, err)


# --------------------------------------------------------------------------- (e) independence of B
@pytest.mark.parametrize("b1,b2", [(32, 33), (64, 65)])
@pytest.mark.parametrize("mode", ["graph", "array"])
def test_trajectory_does_not_depend_on_its_batch(dev, mode, b1, b2):
    """The sharded evaluation runs a trajectory in batches of any size.  32 | 33
    is mesh_vjp_wave_kernel<8> against mesh_vjp_kernel (dmm.hip: identical
    results), 64 | 65 the first row past the skinny linears' 64-row scratch."""
    c = C.graph_case(129, 35, 3, b2) if mode == "graph" else C.array_case(33, b2)
    n = c.xi.shape[0]
    big_m, big_b = _mesh(c, dev, cached=False), _branch(c, dev)
    small_m, small_b = _mesh(c, dev, u=c.u[:b1], cached=False), _branch(c, dev, u=c.u[:b1])
    assert small_m.shape == (b1 * n, 2) and small_b.shape == (b1, 512)
    db = (big_b[:b1] - small_b).abs().max().item()
    dm = (big_m[:b1 * n] - small_m).abs().max().item()
    print(f"{mode} B={b1} | {b2}: max|branch difference| {db:.3e} max|mesh difference| {dm:.3e}")
    assert torch.equal(big_b[:b1], small_b), db
    assert torch.equal(big_m[:b1 * n], small_m), dm
