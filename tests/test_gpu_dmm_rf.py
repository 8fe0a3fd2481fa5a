"""GPU tests of the random-feature phase of DMM training (reference
mesh/dmm_utils.py:785-1076): the feature derivatives (mmpde_dmm_rf_features), the
objective and its gradient (mmpde_rf_objective), the two dense BFGS operations
(mmpde_sym_matvec, mmpde_bfgs_update), the BFGS driver on them, and the phase in
train_MA_res.  float64 references: tests/dmm_rf_cases.py and
oracle/dmm_train_ref.py; bars: the project's PHI_BAR / MESH_BAR / H_BAR for the
tables, the bars of test_gpu_dmm_train.py's loss test for the objective, the
standard dot-product bound for the dense operations.

Array-mode heads have L = 512 (ConvNet's last Linear is 512 wide whatever
trunk_layer says), so the heads (1, 8, 128) and (7, 64, 1024) exist in graph
mode only.
"""
import copy

import numpy as np
import pytest
import torch

import dmm_hess_cases as HC
import dmm_rf_cases as RF
import dmm_shape_cases as C
from oracle import dmm_train_ref as R

pytestmark = pytest.mark.gpu

HEADS = ((1, 8, 128), (7, 64, 1024), C.DEFAULT_HEAD, (64, 512, 512))
FEATURE_CASES = ([("graph", h, B, per) for h in HEADS for B in (1, 3) for per in (1, 5, 65)] +
                 [("array", h, B, per) for h in HEADS[2:] for B in (1, 3) for per in (1, 5, 65)])


def _case(mode, head, B):
    return C.graph_case(40, 5, 1, B, head, False) if mode == "graph" else C.array_case(7, B, head)


def _within(got, ref, bar, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    bound = bar * ref.abs().max().item()
    print(f"{what}: max|err| {err:.3e} bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


# ----------------------------------------------------------------------------- features
@pytest.mark.parametrize("mode, head, B, per", FEATURE_CASES)
def test_features_vs_float64(dev, mode, head, B, per):
    c = _case(mode, head, B)
    dmm, u = c.dmm.to(dev), c.u.to(dev)
    grid = RF.rows_of(c, per).to(dev)
    ft = dmm.rf_features(u, grid)
    assert all(t.shape == (B * per, head[2]) and t.dtype == torch.float32 for t in ft)
    # s is forward(rf=True)'s second output, bit for bit
    _, second, _ = dmm(u, grid, rf=True)
    assert torch.equal(ft.s, second)
    # the head alone against float64: the device's own branch goes into the reference
    branch = dmm.branch_features(u)
    ref = RF.features_closed_form(c, grid.cpu(), branch=branch.cpu())
    for name, got in zip(RF.NAMES, ft):
        _within(got, ref[name], C.PHI_BAR if name == "s" else HC.H_BAR, f"{mode} {head} B {B} per {per} {name}")
    # first order only: the same bits, no second-order tables; a given branch: the same bits
    f1 = dmm.rf_features(u, grid, second_order=False)
    assert f1.s_xx is None and f1.s_xy is None and f1.s_yy is None
    assert torch.equal(f1.s, ft.s) and torch.equal(f1.s_x, ft.s_x) and torch.equal(f1.s_y, ft.s_y)
    f2 = dmm.rf_features(u, grid, branch=branch)
    assert all(torch.equal(a, b) for a, b in zip(f2, ft))


def _contraction(dmm, c, xi, dev, what):
    """sum_k w_o[k] of the tables against the kernels that contract inside:
    DMM.mesh - xi (first order) and mesh_hess (second order)."""
    u, xi = c.u.to(dev), xi.to(dev)
    grid = xi.repeat(c.B, 1)
    ft = dmm.rf_features(u, grid)
    w = dmm.out_nn.layers[1].weight.detach().double().reshape(-1)
    disp = torch.stack((ft.s_x.double() @ w, ft.s_y.double() @ w), dim=1)
    mesh, hess, _, _, _ = dmm.mesh_hess(u, xi)
    assert torch.equal(mesh, dmm.mesh(u, xi))
    ref = mesh.double() - grid.double()
    err = (disp - ref).abs().max().item()
    bound = C.mesh_bar(c, ref)
    print(f"{what} w_o . (s_x, s_y) vs mesh - xi: {err:.3e} bound {bound:.3e}")
    assert err <= bound, (what, err, bound)
    h = torch.stack((ft.s_xx.double() @ w, ft.s_xy.double() @ w, ft.s_yy.double() @ w), dim=1)
    _within(h, hess, HC.H_BAR, f"{what} w_o . (s_xx, s_xy, s_yy) vs mesh_hess")


@pytest.mark.parametrize("head", HEADS)
def test_graph_features_contract_to_mesh_and_hess(dev, head):
    c = HC.base_case("graph", 130, 3, head)
    _contraction(c.dmm.to(dev), c, c.xi, dev, f"graph {head}")


@pytest.mark.parametrize("per", [1, 5, 65])
def test_array_features_contract_to_mesh_and_hess(dev, per):
    c = C.array_case(7, 3)
    xi = RF.rows_of(c, per)[:per]
    _contraction(c.dmm.to(dev), c, xi, dev, f"array per {per}")


# ----------------------------------------------------------------------------- objective
def _train_helpers():
    import test_gpu_dmm_train as G

    return G


def _rf_args(G, kind, bx, bu, **kw):
    return G._args(kind, bx, bu, rf=True, rf_opt_alg="BFGS", epochs_rf=1, max_iter=5, batch_size_x_rf=bx,
                   batch_size_u_rf=bu, convex_rel=0.01, **kw)


def _objective_on(dmm, sample, convex_rel, w0=1.0, w1=1000.0, w2=1.0):
    from mmpde_amd import ops

    u, ux, uy, alpha, rhs, x, bounds, bound_us = sample
    sides = []
    for k in range(4):
        ft = dmm.rf_features(bound_us[k], bounds[k], second_order=False)
        sides.append(ft.s_x if k < 2 else ft.s_y)
    interior = dmm.rf_features(u, x)
    return ops.RfObjective(interior, sides, x, ux, uy, alpha, rhs, w0, w1, w2, convex_rel), interior, sides


@pytest.mark.parametrize("kind", ["cy", "burgers"])
def test_objective_vs_oracle_and_float64(dev, kind):
    from mmpde_amd import dmm_train as T

    G = _train_helpers()
    pde, dmm = G._models(kind)
    sd = G._sd64(dmm)
    all_u = G._data(kind, pde, 6)
    bx, bu = 8, (10 if kind == "cy" else 4)
    args = G._args(kind, bx, bu)
    dmm.to(dev)
    np.random.seed(3)
    sample = T._sample(args, all_u, bx, bu, dev)
    obj, interior, sides = _objective_on(dmm, sample, 0.0)
    w = dmm.out_nn.layers[1].weight.detach().reshape(-1).clone()
    f, g = obj(w)
    # at the model's own weight the objective is the training loss of the same sample
    s64 = tuple(t.detach().double().cpu() if torch.is_tensor(t) else [b.detach().double().cpu() for b in t]
                for t in sample)
    rl, rli, rlb, rlc = R.total_loss(G._phi(kind, pde, sd), s64, bx)
    rl.backward()
    for name, a, b in (("f", f, rl), ("loss_in", obj.parts[0], rli), ("loss_bound", obj.parts[1], rlb),
                       ("loss_convex", obj.parts[2], rlc)):
        G._close(a, b, 1e-4, 1e-9, f"{kind} {name}")
    G._close(g, sd["out_nn.layers.1.weight"].grad, 2e-3, 0.0, f"{kind} df/dw vs the oracle's weight gradient")

    # a perturbed weight and the (sum w^2)^2 term, against the float64 restatement on the same tables
    gen = torch.Generator().manual_seed(9)
    w2 = (w.cpu() * (1 + 0.5 * torch.randn(w.numel(), generator=gen))
          + 0.2 * w.abs().max().cpu() * torch.randn(w.numel(), generator=gen)).to(dev)
    from mmpde_amd import ops
    obj2 = ops.RfObjective(interior, sides, sample[5], sample[1], sample[2], sample[3], sample[4], 1.0, 1000.0,
                           1.0, 0.01)
    f2, g2 = obj2(w2)
    f2, g2, parts2, lhs2 = f2.clone(), g2.clone(), obj2.parts.clone(), obj2.lhs.clone()
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    wr = d(w2).requires_grad_(True)
    names = ("s_x", "s_y", "s_xx", "s_xy", "s_yy")
    rf, rparts, rlhs = RF.objective_ref(wr, {n: d(getattr(interior, n)) for n in names}, [d(t) for t in sides],
                                        s64[5], s64[1], s64[2], s64[3], s64[4], 1.0, 1000.0, 1.0, 0.01)
    rg, = torch.autograd.grad(rf, wr)
    G._close(f2, rf, 1e-4, 1e-9, f"{kind} perturbed f")
    for name, a, b in zip(("loss_in", "loss_bound", "loss_convex"), parts2, rparts):
        G._close(a, b, 1e-4, 1e-9, f"{kind} perturbed {name}")
    G._close(lhs2, rlhs, 1e-4, 0.0, f"{kind} perturbed LHS")
    G._close(g2, rg, 2e-3, 0.0, f"{kind} perturbed df/dw")
    # the (sum w^2)^2 term by itself: against the same call with convex_rel = 0 it adds
    # 0.01 (sum w^2)^2 to f and 0.04 (sum w^2) w to g, each up to the rounding of the sum it joins
    f0, g0 = obj(w2)
    ww = float((wr.detach() ** 2).sum())
    assert abs((f2.double().item() - f0.double().item()) - 0.01 * ww * ww) <= 2.0 ** -22 * abs(f2.item())
    gerr = ((g2.double().cpu() - g0.double().cpu()) - 0.04 * ww * wr.detach()).abs().max().item()
    assert gerr <= 2.0 ** -22 * g2.abs().max().item() + 1e-6 * 0.04 * ww * wr.detach().abs().max().item(), gerr
    # the same bits on a second call
    f3, g3 = obj2(w2)
    assert torch.equal(f3, f2) and torch.equal(g3, g2) and torch.equal(obj2.parts, parts2)
    assert torch.equal(obj2.lhs, lhs2)


def test_objective_zero_monitor_gradient_point(dev):
    """Where u_xi_x = u_xi_y = 0 the monitor's square root has no derivative:
    autograd gives NaN, the kernel contributes 0.  One field with ux = uy = 0."""
    from mmpde_amd import ops

    c = C.array_case(7, 2)
    dmm = c.dmm.to(dev)
    bx = 4
    x = RF.rows_of(c, bx, seed=1).to(dev)
    t = torch.linspace(0, 1, 2)
    z, o = torch.zeros_like(t), torch.ones_like(t)
    edges = [torch.stack(p, 1).repeat(2, 1).to(dev) for p in ((z, t), (o, t), (t, z), (t, o))]
    u = c.u.to(dev)
    sides = [getattr(dmm.rf_features(u, e, second_order=False), "s_x" if k < 2 else "s_y")
             for k, e in enumerate(edges)]
    interior = dmm.rf_features(u, x)
    n = 6
    gen = torch.Generator().manual_seed(2)
    ux = torch.randn(2, n, n, generator=gen)
    uy = torch.randn(2, n, n, generator=gen)
    ux[0], uy[0] = 0.0, 0.0
    alpha, rhs = torch.tensor([1.0, 2.0]), torch.tensor([1.5, 2.5])
    obj = ops.RfObjective(interior, sides, x, ux.to(dev), uy.to(dev), alpha.to(dev), rhs.to(dev), 1.0, 1000.0,
                          1.0, 0.0)
    w = dmm.out_nn.layers[1].weight.detach().reshape(-1)
    f, g = obj(w)
    assert torch.isfinite(f) and torch.isfinite(g).all()
    d = lambda v: v.detach().double().cpu()  # noqa: E731
    names = ("s_x", "s_y", "s_xx", "s_xy", "s_yy")
    tabs = {k: d(getattr(interior, k)) for k in names}
    wr = d(w).requires_grad_(True)
    rf, _, _ = RF.objective_ref(wr, tabs, [d(s) for s in sides], d(x), ux.double(), uy.double(), alpha.double(),
                                rhs.double(), 1.0, 1000.0, 1.0, 0.0)
    rg, = torch.autograd.grad(rf, wr)
    assert torch.isnan(rg).any()                       # the reference's route has no gradient here
    # with the zero field's points dropped from the interior sum (they contribute (1 D / RHS - 1)^2, a
    # function of p_xx, p_xy, p_yy alone, to f) the rest is differentiable: compare there
    wr2 = d(w).requires_grad_(True)
    half = {k: v[bx:] for k, v in tabs.items()}
    rf2, (li2, lb2, _), _ = RF.objective_ref(wr2, half, [d(s) for s in sides], d(x)[bx:], ux[1:].double(),
                                             uy[1:].double(), alpha[1:].double(), rhs[1:].double(), 1.0, 1000.0,
                                             1.0, 0.0)
    pxx, pxy, pyy = (tabs[k][:bx] @ wr2 for k in ("s_xx", "s_xy", "s_yy"))
    li0 = (((1 + pxx) * (1 + pyy) - pxy * pxy) / rhs[0].double() - 1) ** 2
    lc = (torch.clamp(1 + tabs["s_xx"] @ wr2, max=0) ** 2 + torch.clamp(1 + tabs["s_yy"] @ wr2, max=0) ** 2).mean()
    total = 1000.0 * lb2 + (li2 * bx + li0.sum()) / (2 * bx) + lc
    rg2, = torch.autograd.grad(total, wr2)
    err = (d(f) - total.detach()).abs().item()
    assert err <= 1e-4 * abs(total.item()) + 1e-9, (err, total.item())
    gerr = (d(g) - rg2).abs().max().item()
    assert gerr <= 2e-3 * rg2.abs().max().item(), (gerr, rg2.abs().max().item())


# ----------------------------------------------------------------------------- dense operations
def _gamma(n):
    u = 2.0 ** -24
    return n * u / (1 - n * u)


def _dense_inputs(n, dev):
    g = torch.Generator().manual_seed(40 + n)
    m = torch.randn(n, n, generator=g)
    H = (m @ m.t() / n + torch.eye(n)).float()
    H = ((H + H.t()) / 2).contiguous()
    assert torch.equal(H, H.t())
    s = torch.randn(n, generator=g)
    y = (H.double() @ s.double()).float() + 0.1 * torch.randn(n, generator=g)   # y.s > 0, well conditioned
    v = torch.randn(n, generator=g)
    return H.to(dev), s.to(dev), y.to(dev), v.to(dev)


@pytest.mark.parametrize("n", [1, 33, 512])
def test_sym_matvec_vs_float64(dev, n):
    from mmpde_amd import ops

    H, _, _, v = _dense_inputs(n, dev)
    for scale in (-1.0, 1.0):
        got = ops.sym_matvec(H, v, scale)
        ref = scale * (H.double().cpu() @ v.double().cpu())
        # a dot of n terms in any order, fused or not: gamma_n sum_j |H_ij| |v_j|; scale = +-1 is exact
        bound = _gamma(n) * (H.double().cpu().abs() @ v.double().cpu().abs())
        err = (got.double().cpu() - ref).abs()
        print(f"sym_matvec n {n} scale {scale}: worst err / bound {(err / bound).max().item():.3f}")
        assert bool((err <= bound).all()), (n, (err / bound).max().item())
    assert torch.equal(ops.sym_matvec(H, v, -1.0), ops.sym_matvec(H, v, -1.0))
    assert torch.equal(ops.sym_matvec(H, v, -1.0), -ops.sym_matvec(H, v, 1.0))


@pytest.mark.parametrize("n", [1, 33, 512])
def test_bfgs_update_secant_and_symmetry(dev, n):
    """H_new y = s.  Each entry of H_new = H - rho (s Hy^T + Hy s^T) + c s s^T, c =
    rho^2 y.Hy + rho, is a sum of four terms; Hy and y.Hy are dots of n terms
    (relative gamma_n of their absolute-value versions), rho = 1 / y.s carries
    kappa gamma_n with kappa = |y|.|s| / y.s, and the entry itself four more
    roundings.  To first order: rho s_i Hy_j errs by (kappa + 1) gamma_{n+4} of
    its absolute-value version, c by (2 kappa + 2) gamma_{n+4} of its own (rho^2
    twice kappa gamma_n, y.Hy twice gamma_n), so every term's error is below
    (2 kappa + 3) gamma_{n+4} of the term's absolute-value version T_ij, and the
    residual of row i below (2 kappa + 3) gamma_{n+4} sum_j T_ij |y_j|, checked
    against the float64 product of the float32 H_new with y."""
    from mmpde_amd import ops

    H, s, y, _ = _dense_inputs(n, dev)
    Hn = ops.bfgs_update(H.clone(), s, y)
    assert torch.equal(Hn, Hn.t())                      # symmetric bit for bit
    assert not torch.equal(Hn, H)
    H64, s64, y64 = H.double().cpu(), s.double().cpu(), y.double().cpu()
    ys = torch.dot(y64, s64).item()
    assert ys > 1e-10
    kappa = torch.dot(y64.abs(), s64.abs()).item() / ys
    rho = 1.0 / ys
    hy_abs = H64.abs() @ y64.abs()
    cabs = rho * rho * torch.dot(y64.abs(), hy_abs).item() + rho
    T = H64.abs() + rho * (torch.outer(s64.abs(), hy_abs) + torch.outer(hy_abs, s64.abs())) \
        + cabs * torch.outer(s64.abs(), s64.abs())
    bound = (2 * kappa + 3) * _gamma(n + 4) * (T @ y64.abs())
    res = (Hn.double().cpu() @ y64 - s64).abs()
    print(f"bfgs_update n {n}: kappa {kappa:.2f} worst residual / bound {(res / bound).max().item():.3f}")
    assert bool((res <= bound).all()), (n, (res / bound).max().item())
    # against the formula in float64
    eye = torch.eye(n, dtype=torch.float64)
    want = (eye - rho * torch.outer(s64, y64)) @ H64 @ (eye - rho * torch.outer(y64, s64)) + rho * torch.outer(s64, s64)
    assert bool(((Hn.double().cpu() - want).abs() <= (2 * kappa + 3) * _gamma(n + 4) * T).all())
    # y.s <= 1e-10: skipped, H keeps its bits; and the same bits on a second call
    assert torch.equal(ops.bfgs_update(H.clone(), s, -y), H)
    assert torch.equal(ops.bfgs_update(H.clone(), s, y), Hn)


def test_bfgs_on_the_device_reaches_the_minimiser(dev):
    from mmpde_amd.minimize import minimize_bfgs

    A, b, x0, xs = RF.quadratic(33)
    fun = RF.quadratic_fun(A.float().to(dev), b.float().to(dev))
    res = minimize_bfgs(fun, x0.float().to(dev), 200)
    err = (res.x.double().cpu() - xs).abs().max().item()
    print(f"device BFGS on quadratic(33): nit {res.nit} nfev {res.nfev} status {res.status} "
          f"max|x - A^-1 b| {err:.3e} (4 x recorded float32 error: {4 * RF.BFGS_F32_ERR:.3e})")
    assert err <= 4 * RF.BFGS_F32_ERR, (err, RF.BFGS_F32_ERR)
    assert res.fun <= float(fun(x0.float().to(dev))[0])


# ----------------------------------------------------------------------------- the phase
@pytest.mark.parametrize("kind", ["burgers", "cy"])
def test_random_feature_phase(dev, kind, tmp_path):
    from mmpde_amd import dmm_train as T

    G = _train_helpers()
    pde, dmm = G._models(kind)
    all_u = G._data(kind, pde, 6)
    bx, bu = 8, (10 if kind == "cy" else 4)
    args = _rf_args(G, kind, bx, bu)
    dmm.to(dev)
    twin = copy.deepcopy(dmm)
    before = {k: v.detach().clone() for k, v in dmm.state_dict().items()}
    np.random.seed(7)
    out = T.train_MA_res(all_u, all_u, all_u[:2], args, dmm, False, 0, 0, dev, save_dir=str(tmp_path),
                         evaluate_every=0)
    assert len(out) == 15 and out[0] is dmm
    # the lists grow by one, finite; the checkpoint is epoch 1's; the log tells what the fit did
    for i in (1, 2, 4, 5, 6, 7):
        assert len(out[i]) == 1 and np.isfinite(out[i][0]), i
    assert out[3] == [] and out[12] == [] and out[13] == []
    assert (tmp_path / f"dmm_{kind}_epoch1.pt").exists()
    assert any("random feature method epoch 1" in line for line in out[14])
    # what may change: the last Linear's weight, and the BatchNorm statistics as the ten train-mode
    # model calls change them (five of the fit, five of the check pass; array mode has none)
    np.random.seed(7)
    s1 = T._sample(args, all_u, bx, bu, dev)
    s2 = T._sample(args, all_u, bx, bu, dev)
    with torch.no_grad():
        for s in (s1, s2):
            for k in range(4):
                twin(s[7][k], s[6][k])
            twin(s[0], s[5])
    after, want = dmm.state_dict(), twin.state_dict()
    moved = [k for k in after if not torch.equal(after[k], before[k])]
    assert "out_nn.layers.1.weight" in moved
    for k in after:
        if k == "out_nn.layers.1.weight":
            continue
        if kind == "burgers" or not ("running_" in k or "num_batches" in k):
            assert torch.equal(after[k], before[k]), k
        else:
            assert k in moved or "num_batches" in k, k
            G._close(after[k].float(), want[k].float(), 1e-5, 1e-7, f"{kind} {k}")
    # the draws are the reference's, in its order: interior, then boundary
    np.random.seed(7)
    ref = (R.sample_tri if kind == "cy" else R.sample_arr)(all_u, bx, bu)
    assert torch.equal(s1[5].cpu().double(), ref[5])
    for k in range(4):
        assert torch.equal(s1[6][k].cpu().double(), ref[6][k])
        assert torch.equal(s1[7][k].cpu().double(), ref[7][k].float().double())


@pytest.mark.parametrize("kind", ["burgers", "cy"])
def test_random_feature_epoch_decreases_its_objective(dev, kind):
    from mmpde_amd import dmm_train as T

    G = _train_helpers()
    pde, dmm = G._models(kind)
    all_u = G._data(kind, pde, 6)
    bx, bu = 8, (10 if kind == "cy" else 4)
    args = _rf_args(G, kind, bx, bu)
    dmm.to(dev)
    w_old = dmm.out_nn.layers[1].weight.detach().reshape(-1).clone()
    np.random.seed(7)
    rec = T.random_feature_epoch(dmm, args, all_u, dev)
    w_new = dmm.out_nn.layers[1].weight.detach().reshape(-1).clone()
    print(f"{kind}: f {rec.f_before:.6e} -> {rec.f_after:.6e}, nit {rec.nit} nfev {rec.nfev} status {rec.status}")
    assert rec.f_after <= rec.f_before and 0 <= rec.nit <= 5 and rec.nfev >= rec.nit + 1
    assert not torch.equal(w_new, w_old) and rec.f_after < rec.f_before
    # on the epoch's own sample, recomputed: train-mode features do not depend on what the epoch changed
    obj, _, _ = _objective_on(dmm, rec.sample, args.convex_rel, args.loss_weight0, args.loss_weight1,
                              args.loss_weight2)
    assert float(obj(w_old)[0]) == rec.f_before
    assert float(obj(w_new)[0]) == rec.f_after


def test_rf_false_is_rf_absent(dev):
    """One Adam epoch with rf=False (and every other rf argument set) leaves the
    model, the lists and the numpy stream bit for bit as a run whose args have
    no rf at all.  The ConvNet branch's weight gradients come from the
    convolution library, whose default algorithm does not repeat its bits from
    run to run (two runs of the same args differ by 1e-9 in branch.layers.*),
    so both runs ask it for its deterministic algorithms."""
    from mmpde_amd import dmm_train as T

    G = _train_helpers()
    pde, base = G._models("burgers")
    all_u = G._data("burgers", pde, 6)
    base.to(dev)
    runs = []
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for extra in ({}, dict(rf=False, epochs_rf=3, rf_opt_alg="Newton", batch_size_x_rf=8, batch_size_u_rf=4,
                               max_iter=5, convex_rel=0.01)):
            dmm = copy.deepcopy(base)
            np.random.seed(13)
            out = T.train_MA_res(all_u, all_u, all_u[:2], G._args("burgers", 8, 4, **extra), dmm, False, 1, 0,
                                 dev, save_dir=False)
            runs.append((dmm.state_dict(), out[1:14], np.random.get_state()[1].copy()))
    finally:
        torch.backends.cudnn.deterministic = was
    (sd_a, lists_a, rng_a), (sd_b, lists_b, rng_b) = runs
    assert all(torch.equal(sd_a[k], sd_b[k]) for k in sd_a)
    assert lists_a == lists_b and np.array_equal(rng_a, rng_b)
    assert any(not torch.equal(sd_a[k], v) for k, v in base.state_dict().items())
