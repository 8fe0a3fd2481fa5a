"""The float64 references of the random-feature phase tests check themselves on
the CPU: the closed form of the features against the reference's per-feature
autograd route, the restated objective's gradient against central differences,
and the BFGS driver (mmpde_amd.minimize) with the torch backend on SPD
quadratics whose minimiser is known."""
import pytest
import torch

import dmm_rf_cases as RF
import dmm_shape_cases as C


def _driver():
    from mmpde_amd.minimize import TorchDense, minimize_bfgs

    return minimize_bfgs, TorchDense()


@pytest.mark.parametrize("kind, B, per", [("array", 1, 5), ("array", 3, 2), ("graph", 2, 3)])
def test_closed_form_features_match_the_autograd_route(kind, B, per):
    c = C.array_case(7, B, (3, 512, 16)) if kind == "array" else C.graph_case(40, 5, 1, B, (5, 8, 16), False)
    grid = RF.rows_of(c, per)
    ag = RF.features_autograd(c, grid)
    cf = RF.features_closed_form(c, grid)
    for name in RF.NAMES:
        scale = ag[name].abs().max().item()
        err = (ag[name] - cf[name]).abs().max().item()
        print(f"{kind} B {B} per {per} {name}: max|err| {err:.3e} of max {scale:.3e}")
        assert scale > 0 and err <= 1e-10 * scale, (name, err, scale)
    # the reference computes both mixed derivatives; they are one table here
    scale = ag["s_xy"].abs().max().item()
    assert (ag["s_xy"] - ag["s_yx"]).abs().max().item() <= 1e-10 * scale
    # trajectories differ (the branch enters), rows differ
    if B > 1:
        assert (cf["s"][:per] - cf["s"][per:2 * per]).abs().max().item() > 1e-6


def test_objective_gradient_matches_central_differences():
    w, kw = RF.small_problem()
    wv = w.clone().requires_grad_(True)
    f, parts, lhs = RF.objective_ref(wv, **kw)
    g, = torch.autograd.grad(f, wv)
    assert all(torch.isfinite(p) for p in parts) and torch.isfinite(lhs).all() and parts[0] > 0
    h = 1e-6
    fd = torch.zeros_like(w)
    for k in range(w.numel()):
        e = torch.zeros_like(w)
        e[k] = h
        fd[k] = (RF.objective_ref(w + e, **kw)[0] - RF.objective_ref(w - e, **kw)[0]) / (2 * h)
    err = (g - fd).abs().max().item()
    scale = g.abs().max().item()
    print(f"objective gradient vs central differences: {err:.3e} of {scale:.3e}")
    # central differences: h^2 f''' / 6 truncation + eps f / h rounding, ~1e-9 f here
    assert err <= 1e-6 * scale, (err, scale)
    # every term is live: dropping a weight changes f
    for k in ("w0", "w1", "w2", "convex_rel"):
        assert RF.objective_ref(w, **{**kw, k: 0.0})[0] < f


@pytest.mark.parametrize("n", [1, 33])
def test_bfgs_reaches_the_minimiser_of_a_quadratic(n):
    minimize_bfgs, dense = _driver()
    A, b, x0, xs = RF.quadratic(n)
    fun = RF.quadratic_fun(A, b)
    res = minimize_bfgs(fun, x0, 200, dense)
    err = (res.x - xs).abs().max().item()
    print(f"n {n}: nit {res.nit} nfev {res.nfev} status {res.status} max|x - A^-1 b| {err:.3e}")
    assert err <= RF.stall_bound(A, b, 2.0 ** -53), (err, RF.stall_bound(A, b, 2.0 ** -53))
    assert res.status in (0, 2) and res.nit <= 200 and res.nfev >= res.nit + 1
    assert abs(res.fun - float(fun(res.x)[0])) <= 1e-12 * max(1.0, abs(res.fun))
    assert torch.equal(res.grad, fun(res.x)[1])


def test_bfgs_never_increases_f():
    """max_iter = k returns the k-th iterate (the run is deterministic): f is
    non-increasing along them, and the start is returned for max_iter = 0."""
    minimize_bfgs, dense = _driver()
    A, b, x0, _ = RF.quadratic(33)
    fun = RF.quadratic_fun(A, b)
    f0 = float(fun(x0)[0])
    r0 = minimize_bfgs(fun, x0, 0, dense)
    assert torch.equal(r0.x, x0) and r0.fun == f0 and r0.nit == 0 and r0.nfev == 1 and r0.status == 1
    prev = f0
    for k in range(1, 13):
        r = minimize_bfgs(fun, x0, k, dense)
        assert r.nit == k and r.status == 1
        assert r.fun < prev, (k, r.fun, prev)
        prev = r.fun

    # a function that only gets worse away from x0 along -g: the start is kept
    def worse(x):
        return (1.0 if torch.equal(x, x0) else 2.0), torch.ones_like(x)
    r = minimize_bfgs(worse, x0, 5, dense)
    assert torch.equal(r.x, x0) and r.fun == 1.0 and r.status == 2 and r.nit == 0
    # a non-finite value stops the run at the last finite point
    r = minimize_bfgs(lambda x: (float("nan") if not torch.equal(x, x0) else 1.0, torch.ones_like(x)), x0, 5, dense)
    assert torch.equal(r.x, x0) and r.status == 3


def test_torch_backend_update_is_the_bfgs_formula():
    """TorchDense.update against (I - rho s y^T) H (I - rho y s^T) + rho s s^T written
    out, the secant equation H_new y = s, and the y.s <= 1e-10 skip."""
    _, dense = _driver()
    g = torch.Generator().manual_seed(3)
    n = 7
    m = torch.randn(n, n, generator=g, dtype=torch.float64)
    H = m @ m.t() + torch.eye(n, dtype=torch.float64)
    s = torch.randn(n, generator=g, dtype=torch.float64)
    y = s + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    rho = 1.0 / torch.dot(y, s)
    eye = torch.eye(n, dtype=torch.float64)
    want = (eye - rho * torch.outer(s, y)) @ H @ (eye - rho * torch.outer(y, s)) + rho * torch.outer(s, s)
    got = dense.update(H.clone(), s, y)
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    assert (got @ y - s).abs().max().item() <= 1e-12 * (want.abs() @ y.abs()).max().item()
    assert torch.equal(dense.update(H.clone(), s, -y), H)           # y.s < 0: skipped
    assert torch.equal(dense.matvec(H, s, -1.0), -(H @ s))


def test_bfgs_f32_error_is_the_recorded_one():
    """The same driver in float32 on the CPU: its final error against A^-1 b is
    what dmm_rf_cases.BFGS_F32_ERR records (the device test allows 4x that: only
    the summation order of a 33-term dot differs there)."""
    minimize_bfgs, dense = _driver()
    A, b, x0, xs = RF.quadratic(33)
    A32, b32 = A.float(), b.float()
    res = minimize_bfgs(RF.quadratic_fun(A32, b32), x0.float(), 200, dense)
    err = (res.x.double() - xs).abs().max().item()
    print(f"BFGS float32 on quadratic(33): nit {res.nit} nfev {res.nfev} status {res.status} "
          f"max|x - A^-1 b| {err:.3e} (recorded {RF.BFGS_F32_ERR:.3e})")
    assert res.x.dtype == torch.float32
    assert err <= 2 * RF.BFGS_F32_ERR, (err, RF.BFGS_F32_ERR)
    # and it is what float32 allows under the stopping rule, not a stalled run
    assert RF.BFGS_F32_ERR <= RF.stall_bound(A, b, 2.0 ** -24)
