"""The train-mode array branch on the HIP kernels (DMM.hip_branch_train in array
mode: ops.ConvNetTrain and the few-row fc2 / fc3) against the float64
refcpu.convnet of dmm_convnet_train_cases.py at the kernels' edge shapes: the
branch and all twelve gradients within the bars of that file (the torch route's
figures are printed beside them); the Function and the entry points alone, with
guarded output tails; determinism and an uninitialised workspace; independence
of the batch; the model's train-mode entry points and the Monge-Ampere
objective with the flag on; the resolution limit; the flag-off route bit for
bit; the memory of one forward + backward against the torch route's."""
import ctypes

import numpy as np
import pytest
import torch

import dmm_convnet_train_cases as C
import dmm_hess_cases as HC
import dmm_shape_cases as SC

pytestmark = pytest.mark.gpu

IDS = [C.case_id(c) for c in C.CASES]


def _branch(dmm, u):
    return dmm._branch_train(u)


def _run(c, dev, hip):
    _, u, cot = C.inputs(c)
    dmm = C.model(c, dev)
    dmm.hip_branch_train = hip
    return C.run_model(dmm, _branch, u.to(dev), cot.to(dev))


def _conv_params(c, dev):
    b = C.inputs(c)[0].dmm.branch
    return [t.detach().to(dev).clone() for l in b.layers for t in (l.weight, l.bias)]


# ----------------------------------------------------------------------------- 1. the whole branch
@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_branch_forward_and_gradients_vs_float64(dev, c):
    ref = C.reference(c)
    hip, tor = C.measure(_run(c, dev, True), ref), C.measure(_run(c, dev, False), ref)
    for name, m in (("kernels", hip), ("torch", tor)):
        print(f"{C.case_id(c)} {name}: " + " ".join(f"{k} {v:.2e}" for k, v in C.worst(m).items()))
    C.check(hip, C.case_id(c))


# ----------------------------------------------------------------------------- 2. the Function and the entry points
def _conv_ref(c, cot_f):
    """float64 f [B, o2^2] of the convolution stack and the gradient of sum(f * cot_f) in its eight tensors."""
    _, u, _ = C.inputs(c)
    sd = C.branch_sd(c, torch.float64)
    x = u.double().unsqueeze(1)
    cv = lambda i, t, st: torch.nn.functional.conv2d(t, sd[f"layers.{i}.weight"], sd[f"layers.{i}.bias"],  # noqa: E731
                                                     stride=st, padding=2)
    x1 = torch.tanh(cv(0, x, 2))
    x3 = torch.tanh(x1 + cv(2, torch.tanh(cv(1, x1, 1)), 1))
    f = torch.flatten(torch.tanh(cv(3, x3, 2)), 1)
    gs = torch.autograd.grad((f * cot_f.double()).sum(), [sd[n] for n in C.CONVS])
    return f.detach(), gs


def _rel_grads(got, ref):
    G = max(r.abs().max().item() for r in ref)
    return [(g.detach().double().cpu().reshape(r.shape) - r).abs().max().item() / max(r.abs().max().item(),
                                                                                      C.GRAD_FLOOR * G)
            for g, r in zip(got, ref)]


@pytest.mark.parametrize("c", [(7, 3), (48, 3)], ids=["7-3", "48-3"])
def test_function_and_entry_points_alone(dev, c):
    from mmpde_amd import _lib as L
    from mmpde_amd import ops

    s, B = c
    o2 = C.out_sizes(s)[1]
    cot_f = torch.randn(B, o2 * o2, generator=torch.Generator().manual_seed(11 + s))
    ref_f, ref_g = _conv_ref(c, cot_f)
    u = C.inputs(c)[1].to(dev)
    ps = [t.requires_grad_(True) for t in _conv_params(c, dev)]
    f = ops.ConvNetTrain.apply(u, *ps)
    gg = torch.autograd.grad((f * cot_f.to(dev)).sum(), ps)
    fwd = (f.detach().double().cpu() - ref_f).abs().max().item() / ref_f.abs().max().item()
    rel = _rel_grads(gg, ref_g)
    print(f"ConvNetTrain {c}: forward {fwd:.2e}, worst gradient {max(rel):.2e}")
    assert f.shape == (B, o2 * o2) and fwd <= SC.BRANCH_BAR and max(rel) <= C.GRAD_BAR, (fwd, rel)
    assert not u.requires_grad and all(g.shape == p.shape for g, p in zip(gg, ps))

    # the entry points through ctypes: every output 64 floats longer than the call owns, sentinel-filled
    lib = L.lib()
    st = L.stream(dev)
    wp = L.DmmConvnetWeights(*[t.data_ptr() for t in ps])
    nb = lib.mmpde_dmm_convnet_train_workspace_bytes(B)
    sent = -123.4375
    fo = torch.full((B * o2 * o2 + 64,), sent, device=dev)
    go = torch.full((L.DMM_CONVNET_TRAIN_GRADS + 64,), sent, device=dev)
    wk = torch.full((nb // 4 + 64,), sent, device=dev)
    L.check(lib.mmpde_dmm_convnet_train_forward(L.ptr(u), B, s, ctypes.byref(wp), L.ptr(fo), st), "forward")
    df = cot_f.to(dev).contiguous()
    L.check(lib.mmpde_dmm_convnet_train_backward(L.ptr(u), B, s, ctypes.byref(wp), L.ptr(df), L.ptr(go), L.ptr(wk), nb,
                                                 st), "backward")
    torch.cuda.synchronize()
    for name, t, own in (("f", fo, B * o2 * o2), ("grads", go, L.DMM_CONVNET_TRAIN_GRADS), ("workspace", wk, nb // 4)):
        assert bool((t[own:] == sent).all()), f"{name}: the tail was written"
    assert torch.equal(fo[:B * o2 * o2].view(B, -1), f.detach())
    assert torch.equal(go[:L.DMM_CONVNET_TRAIN_GRADS], torch.cat([g.reshape(-1) for g in gg]))


# ----------------------------------------------------------------------------- 3. the same bits
@pytest.mark.parametrize("c", [(33, 65), (48, 3)], ids=["33-65", "48-3"])
def test_two_runs_give_the_same_bits(dev, c):
    a, b = _run(c, dev, True), _run(c, dev, True)
    assert torch.equal(a.branch, b.branch)
    for n, g in a.grads.items():
        assert g is not None and torch.equal(g, b.grads[n]), n


def _backward_raw(c, dev, fill, fields=None):
    """mmpde_dmm_convnet_train_backward on the case's fields (or the slice `fields`) over a workspace filled with
    the byte `fill`: (grads [6833], workspace as floats)."""
    from mmpde_amd import _lib as L

    s, B = c
    u = C.inputs(c)[1].to(dev)
    o2 = C.out_sizes(s)[1]
    df = torch.randn(B, o2 * o2, generator=torch.Generator().manual_seed(5 + s)).to(dev)
    if fields is not None:
        u, df = u[fields].contiguous(), df[fields].contiguous()
    B = u.shape[0]
    ps = _conv_params(c, dev)
    lib = L.lib()
    wp = L.DmmConvnetWeights(*[t.data_ptr() for t in ps])
    nb = lib.mmpde_dmm_convnet_train_workspace_bytes(B)
    wk = torch.full((nb,), fill, dtype=torch.uint8, device=dev)
    grads = torch.empty(L.DMM_CONVNET_TRAIN_GRADS, device=dev)
    L.check(lib.mmpde_dmm_convnet_train_backward(L.ptr(u), B, s, ctypes.byref(wp), L.ptr(df), L.ptr(grads), L.ptr(wk),
                                                 nb, L.stream(dev)), "backward")
    torch.cuda.synchronize()
    return grads, wk.view(torch.float32)


@pytest.mark.parametrize("c", [(9, 2), (33, 65)], ids=["9-2", "33-65"])
def test_workspace_need_not_be_initialised(dev, c):
    a, _ = _backward_raw(c, dev, 0)
    b, _ = _backward_raw(c, dev, 0xFF)          # every float a NaN before the call
    assert bool(torch.isfinite(b).all()) and torch.equal(a, b)


# ----------------------------------------------------------------------------- 4. independence of the batch
@pytest.mark.parametrize("s", [33, 48])
def test_a_field_does_not_depend_on_its_batch(dev, s):
    from mmpde_amd import ops

    c = (s, 3)
    u = C.inputs(c)[1].to(dev)
    ps = _conv_params(c, dev)
    with torch.no_grad():
        batch = ops.ConvNetTrain.apply(u, *ps)
        alone = ops.ConvNetTrain.apply(u[1:2].contiguous(), *ps)
    assert torch.equal(batch[1:2], alone)
    # A field's gradient sums are one workgroup's work, written to the field's own workspace row, and the second
    # kernel starts from row 0 and adds the later rows in order: with one field it copies the row.  So the B = 1
    # gradients are that field's row of the B = 3 call, bit for bit.
    g1, _ = _backward_raw(c, dev, 0, fields=slice(1, 2))
    _, wk = _backward_raw(c, dev, 0)
    row = wk.numel() // 3
    assert torch.equal(g1, wk[row:row + g1.numel()])


# ----------------------------------------------------------------------------- 5. through the model
def _within(got, ref, bar, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = (got - ref).abs().max().item()
    bound = bar * ref.abs().max().item()
    print(f"{what}: max|err| {err:.3e} bound {bound:.3e}")
    assert got.shape == ref.shape and err <= bound, (what, err, bound)


def test_model_entry_points_flag_on_against_off(dev):
    """jet, rf_features and forward in train() mode differ between the routes by the branch alone, which both
    hold to BRANCH_BAR of float64: the outputs are held to the project's bars for them (PHI_BAR, MESH_BAR, H_BAR)."""
    c = (33, 3)
    u = C.inputs(c)[1].to(dev)
    grid = torch.rand(3 * 40, 2, generator=torch.Generator().manual_seed(3)).to(dev)
    out = {}
    for hip in (False, True):
        dmm = C.model(c, dev)
        dmm.hip_branch_train = hip
        j = dmm.jet(u, grid)
        rf = dmm.rf_features(u, grid)
        phi, second, _ = dmm(u, grid, rf=True)
        out[hip] = (j, rf, phi, second)
    (j0, rf0, phi0, sec0), (j1, rf1, phi1, sec1) = out[False], out[True]
    t = lambda j, names: torch.stack([getattr(j, n).reshape(-1) for n in names], 1)  # noqa: E731
    for names, bar in ((("phi",), SC.PHI_BAR), (("phi_x", "phi_y"), SC.MESH_BAR),
                       (("phi_xx", "phi_xy", "phi_yy"), HC.H_BAR)):
        _within(t(j1, names), t(j0, names), bar, f"jet {names}")
    for names, bar in ((("s",), SC.PHI_BAR), (("s_x", "s_y"), SC.MESH_BAR), (("s_xx", "s_xy", "s_yy"), HC.H_BAR)):
        _within(torch.stack([getattr(rf1, n) for n in names]), torch.stack([getattr(rf0, n) for n in names]), bar,
                f"rf_features {names}")
    _within(phi1, phi0, SC.PHI_BAR, "forward phi")
    _within(sec1, sec0, SC.PHI_BAR, "forward second_out")


@pytest.mark.parametrize("jet", [False, True], ids=["autograd", "jet"])
def test_objective_and_gradients_with_the_flag_vs_oracle(dev, jet):
    """test_gpu_dmm_train.py's Burgers fixture with hip_branch_train set: the loss terms and every parameter
    gradient against the float64 oracle at that file's bars."""
    from mmpde_amd import dmm_train as T
    from oracle import dmm_train_ref as R

    import test_gpu_dmm_train as G

    pde, dmm = G._models("burgers")
    sd = G._sd64(dmm)
    all_u = G._data("burgers", pde, 6)
    bx, bu = 8, 4
    args = G._args("burgers", bx, bu)
    dmm.to(dev)
    dmm.hip_branch_train = True
    np.random.seed(3)
    sample = T._sample(args, all_u, bx, bu, dev)
    loss, li, lb, lc, lhs, rhs = T.objective(dmm, args, sample, bx, False, dev, jet)
    dmm.zero_grad()
    loss.backward()
    s64 = tuple(t.detach().double().cpu() if torch.is_tensor(t) else [b.detach().double().cpu() for b in t]
                for t in sample)
    rl, rli, rlb, rlc = R.total_loss(G._phi("burgers", pde, sd), s64, bx)
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


# ----------------------------------------------------------------------------- 6. limits, the old route, memory
def test_above_the_limit_is_refused(dev):
    from mmpde_amd import DMM, ops

    s = ops.CONVNET_TRAIN_MAX_S + 1
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        dmm = DMM(s=s, mode="array", branch_layer=7, trunk_layer=[2, 16, 512], out_layer=[1024, 512, 1]).to(dev).train()
    u = torch.randn(2, s, s, device=dev)
    dmm.hip_branch_train = True
    with pytest.raises(NotImplementedError, match=rf"s <= {ops.CONVNET_TRAIN_MAX_S}\b"):
        dmm._branch_train(u)
    dmm.hip_branch_train = False
    assert dmm._branch_train(u).shape == (2, 512)


def test_flag_off_is_the_torch_route_bit_for_bit(dev):
    """The library's default convolution weight gradient adds with atomics (two identical torch calls differ in
    the last bits), so both calls run with its deterministic algorithms selected; the setting is restored."""
    c = (33, 3)
    _, u, cot = C.inputs(c)
    prev = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        a = _run(c, dev, False)
        b = C.run_model(C.model(c, dev), lambda dmm, x: dmm.branch(x.unsqueeze(1)), u.to(dev), cot.to(dev))
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = prev
    assert torch.equal(a.branch, b.branch)
    for n, g in b.grads.items():
        assert torch.equal(a.grads[n], g), n


def test_peak_memory_is_at_most_the_torch_route(dev):
    """One forward + backward at (48, 16).  By arithmetic the torch route keeps about 130 KB of activations per
    field for autograd, the kernel route 27 KB of gradient sums during the backward alone."""
    c = SC.array_case(48, 16)
    u = c.u.to(dev)
    cot = torch.randn(16, c.head[1], generator=torch.Generator().manual_seed(1)).to(dev)
    peak = {}
    for hip in (False, True):
        import copy

        dmm = copy.deepcopy(c.dmm).to(dev).train()
        dmm.hip_branch_train = hip
        for _ in range(2):                # the first call loads kernels and sizes the split-K scratch
            dmm.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            (dmm._branch_train(u) * cot).sum().backward()
            torch.cuda.synchronize()
            peak[hip] = torch.cuda.max_memory_allocated() - base
    print(f"peak above the start: torch {peak[False]} B, kernels {peak[True]} B, ratio {peak[True] / peak[False]:.3f}")
    assert peak[True] <= peak[False], peak
