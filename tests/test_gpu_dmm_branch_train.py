"""The train-mode graph branch on the HIP kernels (DMM.hip_branch_train) against
the float64 CPU restatement of dmm_branch_train_cases.py, at the kernels' edge
shapes: forward, every parameter gradient and the BatchNorm buffers within the
bars of that file (the torch route's figures are printed beside them); the two
autograd Functions alone; determinism; independence of the batch; the model's
train-mode entry points and the Monge-Ampere objective with the flag on; the
memory of one forward + backward against the torch route's."""
import copy

import numpy as np
import pytest
import torch

import dmm_branch_train_cases as C
import dmm_hess_cases as HC
import dmm_shape_cases as SC

pytestmark = pytest.mark.gpu

IDS = [C.key_id(k) for k in C.KEYS]


def _branch(dmm, u, nbr):
    return dmm._branch_train(u, nbr)


def _run(key, dev, hip):
    _, nbr, u, cot = C.inputs(key)
    dmm = C.model(key, device=dev)
    dmm.hip_branch_train = hip
    return C.run(dmm, _branch, u.to(dev), nbr.to(dev), cot.to(dev))


# ----------------------------------------------------------------------------- 1. the whole branch
@pytest.mark.parametrize("key", C.KEYS, ids=IDS)
def test_branch_forward_gradients_and_statistics_vs_float64(dev, key):
    ref = C.reference(key)
    hip, tor = C.measure(_run(key, dev, True), ref), C.measure(_run(key, dev, False), ref)
    for name, m in (("kernels", hip), ("torch", tor)):
        print(f"{C.key_id(key)} {name}: " + " ".join(f"{k} {v:.2e}" for k, v in C.worst(m).items()))
    C.check(hip, C.key_id(key))


# ----------------------------------------------------------------------------- 2. the Functions alone
def _rel_grads(got, ref):
    G = max(r.abs().max().item() for r in ref)
    return [(g.detach().double().cpu() - r).abs().max().item() / max(r.abs().max().item(), C.GRAD_FLOOR * G)
            for g, r in zip(got, ref)]


@pytest.mark.parametrize("case", [(129, 3, 3, 2), (4389, 35, 3, 3)], ids=["129-3", "4389-35"])
def test_layer_function_vs_float64_autograd(dev, case):
    from mmpde_amd import ops

    c = SC.graph_case(*case)
    n, B = case[0], case[3]
    layer = c.dmm.gnn_layers[0]
    lins = [layer.message_net_1[0], layer.message_net_2[0], layer.update_net_1[0], layer.update_net_2[0]]
    g = torch.Generator().manual_seed(5 + n)
    h = torch.randn(B * n, 4, generator=g)
    cot = torch.randn(B * n, 4, generator=g)
    u = c.u.reshape(-1)
    # float64: the torch layer's messages and update, without the residual and the BatchNorm
    h64 = h.double().requires_grad_(True)
    p64 = [t.detach().double().requires_grad_(True) for lin in lins for t in (lin.weight, lin.bias)]
    j = (c.nbr[None].long() + n * torch.arange(B)[:, None, None]).reshape(-1)
    i = torch.arange(B * n).repeat_interleave(case[1])
    pos, x = c.grid.double().repeat(B, 1), u.double()[:, None]
    m = torch.cat((h64[i], h64[j], x[i] - x[j], pos[i] - pos[j]), -1)
    m = torch.tanh(torch.tanh(m @ p64[0].t() + p64[1]) @ p64[2].t() + p64[3]).reshape(B * n, case[1], 4).mean(1)
    ref = torch.tanh(torch.tanh(torch.cat((h64, m), -1) @ p64[4].t() + p64[5]) @ p64[6].t() + p64[7])
    rg = torch.autograd.grad((ref * cot.double()).sum(), [h64] + p64)
    hd = h.to(dev).requires_grad_(True)
    pd = [t.detach().to(dev).requires_grad_(True) for lin in lins for t in (lin.weight, lin.bias)]
    nbr = c.nbr.to(dev)
    upd = ops.DmmGnnLayerTrain.apply(hd, u.to(dev), c.grid.to(dev), nbr, ops.reverse_adjacency(nbr), *pd)
    gg = torch.autograd.grad((upd * cot.to(dev)).sum(), [hd] + pd)
    fwd = (upd.detach().double().cpu() - ref.detach()).abs().max().item() / ref.abs().max().item()
    rel = _rel_grads(gg, rg)
    print(f"layer {case}: forward {fwd:.2e}, d_h {rel[0]:.2e}, worst weight gradient {max(rel[1:]):.2e}")
    assert fwd <= SC.BRANCH_BAR and max(rel) <= C.GRAD_BAR, (fwd, rel)


@pytest.mark.parametrize("rows", [2 * 129, 3 * 4389], ids=["258", "13167"])
def test_decoder_function_vs_float64_autograd(dev, rows):
    from mmpde_amd import ops

    dec = SC.graph_case(129, 3, 3, 2).dmm.decoding_mlp
    g = torch.Generator().manual_seed(rows)
    h = torch.randn(rows, 4, generator=g)
    cot = torch.randn(rows, 1, generator=g)
    ps = [dec.layers[0].weight, dec.layers[0].bias, dec.layers[1].weight, dec.layers[1].bias]
    h64 = h.double().requires_grad_(True)
    p64 = [t.detach().double().requires_grad_(True) for t in ps]
    ref = torch.tanh(h64 @ p64[0].t() + p64[1]) @ p64[2].t() + p64[3]
    rg = torch.autograd.grad((ref * cot.double()).sum(), [h64] + p64)
    hd = h.to(dev).requires_grad_(True)
    pd = [t.detach().to(dev).requires_grad_(True) for t in ps]
    out = ops.DmmDecodeTrain.apply(hd, *pd)
    gg = torch.autograd.grad((out * cot.to(dev)).sum(), [hd] + pd)
    fwd = (out.detach().double().cpu() - ref.detach()).abs().max().item() / ref.abs().max().item()
    rel = _rel_grads(gg, rg)
    print(f"decoder {rows} rows: forward {fwd:.2e}, d_h {rel[0]:.2e}, worst weight gradient {max(rel[1:]):.2e}")
    assert out.shape == (rows, 1) and fwd <= SC.BRANCH_BAR and max(rel) <= C.GRAD_BAR, (fwd, rel)


# ----------------------------------------------------------------------------- 3. the same bits
@pytest.mark.parametrize("key", [((129, 35, 3, 65), None), (C.HUB_BASE, "hub0")], ids=["129-35-3-65", "hub0"])
def test_two_runs_give_the_same_bits(dev, key):
    a, b = _run(key, dev, True), _run(key, dev, True)
    assert torch.equal(a.branch, b.branch)
    for n, g in a.grads.items():
        assert (g is None) == (b.grads[n] is None) and (g is None or torch.equal(g, b.grads[n])), n
    for n, s in a.stats.items():
        assert torch.equal(s, b.stats[n]), n


def test_rows_do_not_depend_on_the_batch(dev):
    from mmpde_amd import ops

    c = SC.graph_case(129, 35, 3, 2)
    n = 129
    layer = c.dmm.gnn_layers[0]
    ps = [t.detach().to(dev) for lin in (layer.message_net_1[0], layer.message_net_2[0], layer.update_net_1[0],
                                         layer.update_net_2[0]) for t in (lin.weight, lin.bias)]
    dl = c.dmm.decoding_mlp.layers
    pdec = [t.detach().to(dev) for t in (dl[0].weight, dl[0].bias, dl[1].weight, dl[1].bias)]
    g = torch.Generator().manual_seed(9)
    h = torch.randn(3 * n, 4, generator=g).to(dev)
    u = torch.randn(3 * n, generator=g).to(dev)
    cot = torch.randn(3 * n, 4, generator=g).to(dev)
    cd = torch.randn(3 * n, 1, generator=g).to(dev)
    nbr, grid = c.nbr.to(dev), c.grid.to(dev)
    rev = ops.reverse_adjacency(nbr)
    got = []
    for B in (1, 3):
        hb = h[:B * n].clone().requires_grad_(True)
        upd = ops.DmmGnnLayerTrain.apply(hb, u[:B * n], grid, nbr, rev, *ps)
        (dh,) = torch.autograd.grad((upd * cot[:B * n]).sum(), hb)
        hd = h[:B * n].clone().requires_grad_(True)
        out = ops.DmmDecodeTrain.apply(hd, *pdec)
        (dd,) = torch.autograd.grad((out * cd[:B * n]).sum(), hd)
        got.append([t.detach()[:n] for t in (upd, dh, out, dd)])
    for name, a, b in zip(("layer update", "layer d_h", "decoder", "decoder d_h"), *got):
        assert torch.equal(a, b), name
    # a table in which nobody reads node 5 as a source (an empty reverse list) runs and leaves its row finite
    _, hub5, _, _ = C.inputs((C.HUB_BASE, "hub5"))
    hub5 = hub5.to(dev)
    hb = h[:n].clone().requires_grad_(True)
    upd = ops.DmmGnnLayerTrain.apply(hb, u[:n], grid, hub5, ops.reverse_adjacency(hub5), *ps)
    (dh,) = torch.autograd.grad((upd * cot[:n]).sum(), hb)
    assert bool(torch.isfinite(dh).all()) and bool(dh[5].any())


# ----------------------------------------------------------------------------- 4. through the model
def _within(got, ref, bar, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = (got - ref).abs().max().item()
    bound = bar * ref.abs().max().item()
    print(f"{what}: max|err| {err:.3e} bound {bound:.3e}")
    assert got.shape == ref.shape and err <= bound, (what, err, bound)


def test_model_entry_points_flag_on_against_off(dev):
    """jet, rf_features and forward in train() mode differ between the routes by the branch alone, which both
    hold to BRANCH_BAR of float64: the outputs are held to the project's bars for them (PHI_BAR, MESH_BAR, H_BAR)."""
    key = ((129, 35, 3, 2), None)
    c = C.inputs(key)[0]
    u = c.u.to(dev)
    grid = torch.rand(2 * 40, 2, generator=torch.Generator().manual_seed(3)).to(dev)
    out = {}
    for hip in (False, True):
        dmm = C.model(key, device=dev)
        dmm.hip_branch_train = hip
        j = dmm.jet(u, grid)
        rf = dmm.rf_features(u, grid)
        phi, second, _ = dmm(u, grid, rf=True)
        out[hip] = (j, rf, phi, second, {n: b.detach().clone() for n, b in dmm.named_buffers()})
    (j0, rf0, phi0, sec0, st0), (j1, rf1, phi1, sec1, st1) = out[False], out[True]
    t = lambda j, names: torch.stack([getattr(j, n).reshape(-1) for n in names], 1)  # noqa: E731
    for names, bar in ((("phi",), SC.PHI_BAR), (("phi_x", "phi_y"), SC.MESH_BAR),
                       (("phi_xx", "phi_xy", "phi_yy"), HC.H_BAR)):
        _within(t(j1, names), t(j0, names), bar, f"jet {names}")
    for names, bar in ((("s",), SC.PHI_BAR), (("s_x", "s_y"), SC.MESH_BAR), (("s_xx", "s_xy", "s_yy"), HC.H_BAR)):
        _within(torch.stack([getattr(rf1, n) for n in names]), torch.stack([getattr(rf0, n) for n in names]), bar,
                f"rf_features {names}")
    _within(phi1, phi0, SC.PHI_BAR, "forward phi")
    _within(sec1, sec0, SC.PHI_BAR, "forward second_out")
    for n, b in st0.items():      # three model calls each
        if n.endswith("num_batches_tracked"):
            assert int(st1[n]) == int(b) == 3, n
        elif "running" in n:
            _within(st1[n], b, C.STAT_BAR, n)


@pytest.mark.parametrize("jet", [False, True], ids=["autograd", "jet"])
def test_objective_and_gradients_with_the_flag_vs_oracle(dev, jet):
    """test_gpu_dmm_train.py's cylinder fixture with hip_branch_train set: the loss and every parameter gradient
    against the float64 oracle at that file's bars, and the BatchNorm buffers after the draw against the torch
    route's."""
    from mmpde_amd import dmm_train as T
    from oracle import dmm_train_ref as R

    import test_gpu_dmm_train as G

    pde, dmm = G._models("cy")
    sd = G._sd64(dmm)
    all_u = G._data("cy", pde, 6)
    bx, bu = 8, 10
    args = G._args("cy", bx, bu)
    dmm.to(dev)
    start = {n: b.detach().clone() for n, b in dmm.named_buffers()}
    stats = {}
    for hip in (False, True):
        dmm.load_state_dict({**dmm.state_dict(), **start})
        dmm.hip_branch_train = hip
        np.random.seed(3)
        sample = T._sample(args, all_u, bx, bu, dev)
        loss, li, lb, lc, lhs, rhs = T.objective(dmm, args, sample, bx, False, dev, jet)
        dmm.zero_grad()
        loss.backward()
        stats[hip] = {n: b.detach().clone() for n, b in dmm.named_buffers()}
    s64 = tuple(t.detach().double().cpu() if torch.is_tensor(t) else [b.detach().double().cpu() for b in t]
                for t in sample)
    rl, rli, rlb, rlc = R.total_loss(G._phi("cy", pde, sd), s64, bx)
    rl.backward()
    for name, a, b in (("loss", loss, rl), ("loss_in", li, rli), ("loss_bound", lb, rlb), ("loss_convex", lc, rlc)):
        G._close(a, b, 1e-4, 1e-9, f"hip branch {name}")
    Gm = max(sd[n].grad.abs().max().item() for n, _ in dmm.named_parameters() if sd[n].grad is not None)
    for n, p in dmm.named_parameters():
        ref = sd[n].grad
        if ref is None:
            assert p.grad is None or not bool(p.grad.any()), n
            continue
        G._close(p.grad, ref, 2e-3, 1e-5 * Gm, f"hip branch d loss / d {n}")
    for n, b in stats[False].items():
        if n.endswith("num_batches_tracked"):
            assert int(stats[True][n]) == int(b), n
        elif "running" in n:
            _within(stats[True][n], b, C.STAT_BAR, n)


# ----------------------------------------------------------------------------- 5. memory, limits, the old route
def test_peak_memory_is_at_most_half_the_torch_route(dev):
    c = SC.graph_case(513, 35, 3, 16)
    u, nbr = c.u.to(dev), c.nbr.to(dev)
    cot = torch.randn(16, c.head[1], generator=torch.Generator().manual_seed(1)).to(dev)
    peak = {}
    for hip in (False, True):
        dmm = copy.deepcopy(c.dmm).to(dev).train()
        dmm.hip_branch_train = hip
        for _ in range(2):                # the first call builds the reverse adjacency and loads kernels
            dmm.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            (dmm._branch_train(u, nbr) * cot).sum().backward()
            torch.cuda.synchronize()
            peak[hip] = torch.cuda.max_memory_allocated() - base
    print(f"peak above the start: torch {peak[False]} B, kernels {peak[True]} B, ratio {peak[True] / peak[False]:.3f}")
    assert peak[True] <= 0.5 * peak[False], peak


def test_hidden_8_is_refused(dev):
    from mmpde_amd import DMM

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        dmm = DMM(mode="graph", grid=torch.rand(40, 2), branch_layer=[8, 1], trunk_layer=[2, 16, 512],
                  out_layer=[1024, 512, 1]).to(dev).train()
    dmm.hip_branch_train = True
    with pytest.raises(NotImplementedError, match="hidden_features == 4"):
        dmm._branch_train(torch.randn(2, 40, device=dev))
    dmm.hip_branch_train = False
    assert dmm._branch_train(torch.randn(2, 40, device=dev)).shape == (2, 512)


def test_flag_off_is_the_torch_route_bit_for_bit(dev):
    key = ((129, 35, 3, 2), None)
    _, nbr, u, cot = C.inputs(key)
    a = _run(key, dev, False)
    b = C.run(C.model(key, device=dev), C.restate, u.to(dev), nbr.to(dev), cot.to(dev))
    # the outputs and the buffers; torch's own gather backward adds with atomics, so its gradients are compared
    # at the bars instead (section 1 prints them)
    assert torch.equal(a.branch, b.branch)
    for n, s in b.stats.items():
        assert torch.equal(s, a.stats[n]), n
    C.check(C.measure(a, C.reference(key)), "flag off")
