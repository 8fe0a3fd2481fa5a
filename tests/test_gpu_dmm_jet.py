"""GPU tests of the Monge-Ampere jet of the DMM head (mmpde_dmm_jet,
mmpde_dmm_jet_grad, DMM.jet) and of DMM training through it (dmm_train's
jet=True).  float64 references: tests/dmm_jet_cases.py (the closed form and its
reverse pass, pinned on the CPU by test_dmm_jet_cases.py) and
oracle/dmm_train_ref.py; bars: the project's PHI_BAR / MESH_BAR / H_BAR for the
jet, test_gpu_dmm_train.py's gradient bar (2e-3 of max|ref| + 1e-5 of the
model's largest gradient) for the gradients, and that file's loss, Adam-step and
BatchNorm bars for the training tests.

Array-mode heads have L = 512, so the heads (1, 8, 128) and (7, 64, 1024) exist
in graph mode only.  The device's own branch goes into the references, so that
the head alone is compared.

test_gradients_vs_float64 prints (-s) each tensor's relative error (err /
max(max|ref|, 1e-5 max gradient)) beside that of the fp32 nested-autograd route
(trunk and out_nn as torch ops, the route of jet=False) on the same inputs.  On
an MI355X the worst over all cases was 2.4e-6 (T1) for the kernel and 4.4e-6
(t1_b) for fp32 autograd, against the bar's 2e-3; DESIGN.md §4 has the table.
"""
import copy

import numpy as np
import pytest
import torch

import dmm_hess_cases as HC
import dmm_jet_cases as J
import dmm_rf_cases as RF
import dmm_shape_cases as C
from oracle import dmm_train_ref as R

pytestmark = pytest.mark.gpu

HEADS = ((1, 8, 128), (7, 64, 1024), C.DEFAULT_HEAD, (64, 512, 512))
# per 65: a partial last tile of 16 rows; B 3 x per 65 = 195 rows: both trajectory boundaries fall
# where a tile of consecutive rows would span them; 3 x 700: 132 row tiles, more than the 128 groups
# of the backward's column kernel, so some group walks two tiles
CASES = ([("graph", h, B, per) for h in HEADS for B in (1, 3) for per in (1, 5, 65)] +
         [("array", h, B, per) for h in HEADS[2:] for B in (1, 3) for per in (1, 5, 65)] +
         [("array", C.DEFAULT_HEAD, 3, 700)])
_REFS = {}


def _case(mode, head, B):
    return C.graph_case(40, 5, 1, B, head, False) if mode == "graph" else C.array_case(7, B, head)


def _setup(dev, mode, head, B, per):
    """The case on the device with its float64 references, computed once per
    case and shared (read-only) by the tests below."""
    key = (mode, head, B, per)
    if key not in _REFS:
        c = _case(mode, head, B)
        dmm, u = c.dmm.to(dev), c.u.to(dev)
        grid = RF.rows_of(c, per)
        branch = dmm.branch_features(u)
        sd = RF._sd64(c)
        _REFS[key] = (c, grid, branch, sd, J.jet_closed_form(sd, branch.cpu(), grid))
    c, grid, branch, sd, ref = _REFS[key]
    return c, c.dmm.to(dev), c.u.to(dev), grid.to(dev), branch, sd, ref


def _within(got, ref, bar, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    bound = bar * ref.abs().max().item()
    print(f"{what}: max|err| {err:.3e} bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


def _groups(j):
    """(phi [rows, 1], grad [rows, 2], hess [rows, 3]) of a jet given as a dict or an ops.Jet."""
    t = (lambda n: (j[n] if isinstance(j, dict) else getattr(j, n)).reshape(-1))
    return (t("phi")[:, None], torch.stack((t("phi_x"), t("phi_y")), 1),
            torch.stack((t("phi_xx"), t("phi_xy"), t("phi_yy")), 1))


# ----------------------------------------------------------------------------- 1. the jet
@pytest.mark.parametrize("mode, head, B, per", CASES)
def test_jet_vs_float64(dev, mode, head, B, per):
    c, dmm, u, grid, branch, sd, ref = _setup(dev, mode, head, B, per)
    what = f"{mode} {head} B {B} per {per}"
    j = dmm.jet(u, grid)
    assert all(t.shape == (B * per, 1) and t.dtype == torch.float32 for t in j)
    for name, bar, got, want in zip(("phi", "(phi_x, phi_y)", "(phi_xx, phi_xy, phi_yy)"),
                                    (C.PHI_BAR, C.MESH_BAR, HC.H_BAR), _groups(j), _groups(ref)):
        _within(got, want, bar, f"{what} {name}")
    # phi is forward's phi; the jet is the rf tables contracted with w_o
    _within(j.phi, dmm(u, grid), C.PHI_BAR, f"{what} phi vs forward")
    ft = dmm.rf_features(u, grid)
    w = dmm.out_nn.layers[1].weight.detach().double().reshape(-1)
    b = dmm.out_nn.layers[1].bias.detach().double()
    con = {"phi": ft.s.double() @ w + b, "phi_x": ft.s_x.double() @ w, "phi_y": ft.s_y.double() @ w,
           "phi_xx": ft.s_xx.double() @ w, "phi_xy": ft.s_xy.double() @ w, "phi_yy": ft.s_yy.double() @ w}
    for name, bar, got, want in zip(("phi", "(phi_x, phi_y)", "(phi_xx, phi_xy, phi_yy)"),
                                    (C.PHI_BAR, C.MESH_BAR, HC.H_BAR), _groups(j), _groups(con)):
        _within(got, want, bar, f"{what} {name} vs rf_features . w_o")
    # first order only: the same bits, no second-order outputs; a given branch: the same bits
    j1 = dmm.jet(u, grid, second_order=False)
    assert j1.phi_xx is None and j1.phi_xy is None and j1.phi_yy is None
    assert torch.equal(j1.phi, j.phi) and torch.equal(j1.phi_x, j.phi_x) and torch.equal(j1.phi_y, j.phi_y)
    j2 = dmm.jet(u, grid, branch=branch)
    assert all(torch.equal(a, b) for a, b in zip(j2, j))


# ----------------------------------------------------------------------------- 2. the gradients
def _jet_grads(dmm, u, grid, branch, cots):
    """Gradients of sum_c <cots[c], jet_c> through DMM.jet's backward: dict of J.GRADS."""
    br = branch.detach().clone().requires_grad_(True)
    params = dmm._tensors()[0] + [dmm.out_nn.layers[1].bias]
    j = dmm.jet(u, grid, second_order=cots[3] is not None, branch=br)
    total = sum((c.to(grid.device).reshape(-1, 1) * t).sum() for c, t in zip(cots, j) if c is not None)
    gr = torch.autograd.grad(total, [br] + params, allow_unused=True)
    return {n: (torch.zeros_like(t) if g is None else g) for n, g, t in zip(J.GRADS, gr, [br] + params)}


def _rel_errors(got, ref):
    G = max(ref[n].abs().max().item() for n in J.GRADS)
    return {n: (got[n].detach().double().cpu() - ref[n]).abs().max().item() / max(ref[n].abs().max().item(), 1e-5 * G)
            for n in J.GRADS}, G


@pytest.mark.parametrize("first_only", [False, True])
@pytest.mark.parametrize("mode, head, B, per", CASES)
def test_gradients_vs_float64(dev, mode, head, B, per, first_only):
    c, dmm, u, grid, branch, sd, _ = _setup(dev, mode, head, B, per)
    what = f"{mode} {head} B {B} per {per} {'first order' if first_only else 'all six'}"
    cots = J.cotangents(B * per, 3, first_only)
    ref = J.jet_reverse(sd, branch.cpu(), grid.cpu(), cots)
    got = _jet_grads(dmm, u, grid, branch, cots)
    # the parent's route on the same inputs: fp32 nested autograd through trunk and out_nn on the device
    _, auto = J.jet_autograd(sd, branch, grid, cots, dtype=torch.float32, device=dev)
    ours, G = _rel_errors(got, ref)
    theirs, _ = _rel_errors(auto, ref)
    for n in J.GRADS:
        print(f"{what} d/d {n}: kernel {ours[n]:.3e} fp32 autograd {theirs[n]:.3e} (relative)")
    for n in J.GRADS:
        g, r = got[n].detach().double().cpu(), ref[n]
        assert g.shape == r.shape, (n, g.shape, r.shape)
        err = (g - r).abs().max().item()
        bound = 2e-3 * r.abs().max().item() + 1e-5 * G
        assert err <= bound, (what, n, err, bound)


# ----------------------------------------------------------------------------- 3. the same bits twice
def test_same_bits_twice(dev):
    mode, head, B, per = CASES[-1]
    c, dmm, u, grid, branch, sd, _ = _setup(dev, mode, head, B, per)
    cots = J.cotangents(B * per, 5)
    a, b = dmm.jet(u, grid, branch=branch), dmm.jet(u, grid, branch=branch)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ga, gb = _jet_grads(dmm, u, grid, branch, cots), _jet_grads(dmm, u, grid, branch, cots)
    for n in J.GRADS:
        assert torch.equal(ga[n], gb[n]), n
        assert bool(ga[n].any()), n


# ----------------------------------------------------------------------------- 4. the objective
def _train_helpers():
    import test_gpu_dmm_train as G

    return G


def _hard_phi(phi):
    """The hard boundary ansatz around the oracle's phi (dmm_utils.py:514-516)."""
    def f(u, X):
        x1, x2 = X[:, :1], X[:, 1:]
        return (x1 ** 2) * (x2 ** 2) * ((x1 - 1) ** 2) * ((x2 - 1) ** 2) * phi(u, X) + 0.5 * x1 ** 2 + 0.5 * x2 ** 2
    return f


@pytest.mark.parametrize("bound", ["soft", "hard"])
@pytest.mark.parametrize("kind", ["cy", "burgers"])
def test_objective_and_parameter_grads_with_jet_vs_oracle(dev, kind, bound):
    from mmpde_amd import dmm_train as T

    G = _train_helpers()
    pde, dmm = G._models(kind)
    sd = G._sd64(dmm)
    all_u = G._data(kind, pde, 6)
    bx, bu = 8, (10 if kind == "cy" else 4)
    args = G._args(kind, bx, bu, bound_constraint=bound)
    dmm.to(dev)
    twin = copy.deepcopy(dmm)
    np.random.seed(3)
    sample = T._sample(args, all_u, bx, bu, dev)
    loss, li, lb, lc, lhs, rhs = T.objective(dmm, args, sample, bx, False, dev, jet=True)
    dmm.zero_grad()
    loss.backward()
    s64 = tuple(t.detach().double().cpu() if torch.is_tensor(t) else [b.detach().double().cpu() for b in t]
                for t in sample)
    phi = G._phi(kind, pde, sd)
    if bound == "soft":
        rl, rli, rlb, rlc = R.total_loss(phi, s64, bx)
    else:
        rli, rlc, _ = R.interior_losses(_hard_phi(phi), s64[0], s64[1], s64[2], s64[3], s64[4], s64[5], bx)
        rl, rlb = rli + rlc, torch.zeros(())
    rl.backward()
    for name, a, b in (("loss", loss, rl), ("loss_in", li, rli), ("loss_bound", lb, rlb), ("loss_convex", lc, rlc)):
        G._close(a, b, 1e-4, 1e-9, f"{kind} {bound} jet {name}")
    Gm = max(sd[n].grad.abs().max().item() for n, _ in dmm.named_parameters() if sd[n].grad is not None)
    worst = 0.0
    for n, p in dmm.named_parameters():
        ref = sd[n].grad
        if ref is None:
            assert p.grad is None or not bool(p.grad.any()), n
            continue
        assert p.grad is not None, n
        err = (p.grad.double().cpu() - ref).abs().max().item()
        worst = max(worst, err / max(ref.abs().max().item(), 1e-5 * Gm))
        G._close(p.grad, ref, 2e-3, 1e-5 * Gm, f"{kind} {bound} jet d loss / d {n}")
    print(f"{kind} {bound} jet: worst relative gradient error {worst:.3e}")
    # BatchNorm running statistics advance as on the autograd route from the same start
    T.objective(twin, args, sample, bx, False, dev, jet=False)
    for (k, v), (_, w) in zip(dmm.state_dict().items(), twin.state_dict().items()):
        if k.endswith("running_mean") or k.endswith("running_var"):
            G._close(v, w, 1e-4, 1e-7, f"{kind} {bound} {k} jet vs autograd")
        if k.endswith("num_batches_tracked"):
            assert torch.equal(v, w), k


# ----------------------------------------------------------------------------- 5., 6. the training loop
def test_train_MA_res_adam_step_with_jet_vs_oracle(dev, tmp_path):  # noqa: N802
    from mmpde_amd import dmm_train as T

    G = _train_helpers()
    kind = "cy"
    pde, dmm = G._models(kind)
    sd = G._sd64(dmm)
    p0 = {n: p.detach().double().clone() for n, p in dmm.named_parameters()}
    all_u = G._data(kind, pde, 6)
    bx, bu = 8, 10
    args = G._args(kind, bx, bu)
    dmm.to(dev)
    np.random.seed(21)
    out = T.train_MA_res(all_u, all_u, all_u, args, dmm, False, 1, 0, dev, save_dir=str(tmp_path), jet=True)
    assert len(out) == 15 and out[0] is dmm
    assert (tmp_path / "dmm_cy_epoch1.pt").exists()
    np.random.seed(21)
    s64 = R.sample_tri(all_u, bx, bu)
    rl, rli, _, _ = R.total_loss(G._phi(kind, pde, sd), s64, bx)
    rl.backward()
    assert abs(out[1][0] - rli.item()) <= 1e-4 * abs(rli.item()), (out[1][0], rli.item())
    Gm = max(sd[n].grad.abs().max().item() for n in p0 if sd[n].grad is not None)
    for n, p in dmm.named_parameters():
        if sd[n].grad is None:     # outside the graph-mode forward: Adam skips it
            assert torch.equal(p.detach().double().cpu(), p0[n]), n
            continue
        g = sd[n].grad + args.weight_decay * p0[n]
        step = -args.lr_adam * g / (g.abs() + 1e-8)
        got = p.detach().double().cpu() - p0[n]
        big = g.abs() > 1e-3 * max(g.abs().max().item(), Gm)
        G._close(got[big], step[big], 1e-3, 0.0, f"Adam step {n} (jet)")
        assert float(got.abs().max()) <= args.lr_adam * (1 + 1e-3)
    assert len(out[4]) == 1 and np.isfinite(out[4][0])


def test_train_MA_res_lbfgs_epoch_with_jet_runs(dev):  # noqa: N802
    from mmpde_amd import dmm_train as T

    G = _train_helpers()
    pde, dmm = G._models("burgers")
    all_u = G._data("burgers", pde, 6)
    args = G._args("burgers", 8, 4)
    dmm.to(dev)
    np.random.seed(5)
    out = T.train_MA_res(all_u, all_u, all_u[:2], args, dmm, False, 0, 1, dev, save_dir=False, jet=True)
    assert len(out[1]) == 1 and np.isfinite(out[1][0]) and np.isfinite(out[2][0])
    assert len(out[8]) == 1 and all(np.isfinite(v) for v in (out[8][0], out[9][0], out[10][0]))
    assert all(torch.isfinite(p).all() for p in dmm.parameters())


# ----------------------------------------------------------------------------- 7. error cases
def test_error_cases(dev):
    c = C.array_case(7, 2)
    dmm, u = c.dmm.to(dev), c.u.to(dev)
    grid = RF.rows_of(c, 5).to(dev)
    with pytest.raises(ValueError, match="not differentiable in grid"):
        dmm.jet(u, grid.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="multiple of the batch size"):
        dmm.jet(u, grid[:9])
    # a head the kernels do not take: three trunk layers
    from mmpde_amd import DMM

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        deep = DMM(s=7, mode="array", branch_layer=7, trunk_layer=[2, 16, 16, 512], out_layer=[1024, 512, 1])
    deep.to(dev).eval()
    with pytest.raises(NotImplementedError, match="trunk DenseNet"):
        deep.jet(u, grid)
    # the autograd route is untouched by the flag's default
    import inspect

    from mmpde_amd import dmm_train as T
    for fn in (T.boundary_loss, T.ma_losses, T.objective, T.train_MA_res):
        assert inspect.signature(fn).parameters["jet"].default is False, fn.__name__
