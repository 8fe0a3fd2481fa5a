"""Float64 references of the random-feature phase tests (test_gpu_dmm_rf.py on
the device, test_dmm_rf_cases.py on the CPU alone).  Models and inputs are
those of dmm_shape_cases.py (graph_case / array_case, unchanged); the loss is
restated on oracle/dmm_train_ref.py's interpolate and monitor.

features_autograd follows the reference's route (mesh/dmm_utils.py:883-905): one
autograd.grad per feature and derivative, L' of each.  It costs 6 L' backward
passes, so it is used for L' <= 16 only, to pin features_closed_form, which is
the formula of include/mmpde_hip.h (mmpde_dmm_rf_features) in float64 and
serves every shape.

objective_ref is random_feature_torch2 (:351-388) with the one table so_xy in
the place of so_xy and so_yx.

quadratic(n) is an SPD quadratic of condition number <= 10 with its minimiser.
"""
import functools

import numpy as np
import torch

import dmm_shape_cases as C
from oracle import dmm_train_ref as R
from oracle import refcpu

NAMES = ("s", "s_x", "s_y", "s_xx", "s_xy", "s_yy")

# Final error max|x - A^-1 b| of minimize_bfgs(TorchDense, float32, CPU) on
# quadratic(33), max_iter 200: 13 iterations, 33 evaluations, status 2 (the
# computed f stopped decreasing; stall_bound below says where that must happen),
# as printed by
#   python -m pytest tests/test_dmm_rf_cases.py -k f32 -s
# (test_bfgs_f32_error_is_the_recorded_one asserts it stays within 2x of this).
BFGS_F32_ERR = 1.564e-4


def _sd64(c):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in c.sd.items()}


def rows_of(c, per, seed=0):
    """per random rows of the unit square for each of c.B trajectories [B per, 2]
    (float32; the first row of the first trajectory is the corner (0, 1))."""
    g = torch.Generator().manual_seed(1000 + 17 * per + c.B + seed)
    grid = torch.rand(c.B * per, 2, generator=g)
    grid[0] = torch.tensor([0.0, 1.0])
    return grid


def features_autograd(c, grid, branch=None):
    """The reference's per-feature autograd route in float64: dict of s, s_x, s_y,
    s_xx, s_xy, s_yx, s_yy [rows, L']."""
    sd = _sd64(c)
    br = C.branch_ref(c) if branch is None else branch.double()
    rep = grid.shape[0] // c.B
    br = br[:, None, :].repeat(1, rep, 1).reshape(-1, br.shape[-1])
    x1 = grid[:, :1].double().clone().requires_grad_(True)
    x2 = grid[:, 1:].double().clone().requires_grad_(True)
    trunk, _ = refcpu.densenet(sd, "trunk", torch.cat((x1, x2), dim=1), 2)
    _, second = refcpu.densenet(sd, "out_nn", torch.cat((br, trunk), dim=-1), 2)
    cols = {k: [] for k in ("s_x", "s_y", "s_xx", "s_xy", "s_yx", "s_yy")}
    for k in range(second.shape[-1]):
        so = second[:, k]
        w = torch.ones_like(so)
        sx = torch.autograd.grad(so, x1, grad_outputs=w, retain_graph=True, create_graph=True)[0]
        sy = torch.autograd.grad(so, x2, grad_outputs=w, retain_graph=True, create_graph=True)[0]
        w2 = torch.ones_like(sx)
        cols["s_x"].append(sx)
        cols["s_y"].append(sy)
        cols["s_xy"].append(torch.autograd.grad(sx, x2, grad_outputs=w2, retain_graph=True)[0])
        cols["s_xx"].append(torch.autograd.grad(sx, x1, grad_outputs=w2, retain_graph=True)[0])
        cols["s_yx"].append(torch.autograd.grad(sy, x1, grad_outputs=w2, retain_graph=True)[0])
        cols["s_yy"].append(torch.autograd.grad(sy, x2, grad_outputs=w2, retain_graph=True)[0])
    out = {k: torch.stack(v)[:, :, 0].permute(1, 0).detach() for k, v in cols.items()}
    out["s"] = second.detach()
    return out


def features_closed_form(c, grid, branch=None):
    """include/mmpde_hip.h's formulas (mmpde_dmm_rf_features) in float64: dict of
    s, s_x, s_y, s_xx, s_xy, s_yy [rows, L'].  branch: a [B, L] branch output to
    use instead of the float64 branch of c (the device tests pass the device's
    own, so that the head alone is compared)."""
    sd = _sd64(c)
    L = c.head[1]
    br = C.branch_ref(c) if branch is None else branch.double()
    rep = grid.shape[0] // c.B
    t0, b0 = sd["trunk.layers.0.weight"], sd["trunk.layers.0.bias"]
    t1, b1 = sd["trunk.layers.1.weight"], sd["trunk.layers.1.bias"]
    wo, bo = sd["out_nn.layers.0.weight"], sd["out_nn.layers.0.bias"]
    xi = grid.double()
    h = torch.tanh(xi @ t0.t() + b0)                       # [rows, th]
    P = wo[:, L:] @ t1                                     # [L', th]
    cb = br @ wo[:, :L].t() + wo[:, L:] @ b1 + bo          # [B, L']
    cb = cb[:, None, :].repeat(1, rep, 1).reshape(-1, cb.shape[-1])
    s = torch.tanh(h @ P.t() + cb)
    hp = 1 - h * h
    hpp = -2 * h * hp
    zd = [(hp * t0[:, d]) @ P.t() for d in range(2)]
    zde = {(d, e): (hpp * t0[:, d] * t0[:, e]) @ P.t() for d, e in ((0, 0), (0, 1), (1, 1))}
    g = 1 - s * s
    out = {"s": s, "s_x": g * zd[0], "s_y": g * zd[1]}
    for name, (d, e) in (("s_xx", (0, 0)), ("s_xy", (0, 1)), ("s_yy", (1, 1))):
        out[name] = g * zde[(d, e)] - 2 * s * g * zd[d] * zd[e]
    return out


def objective_ref(w, interior, sides, x, ux, uy, alpha, rhs, w0, w1, w2, convex_rel):
    """random_feature_torch2 in the dtype of its inputs: (f, (loss_in, loss_bound,
    loss_convex), LHS).  interior: dict with s_x, s_y, s_xx, s_xy, s_yy [M, L'];
    sides: the four boundary tables [Mb, L']; ux, uy [bu, n, n]; points i bx ..
    i bx + bx - 1 read field i."""
    w = w.reshape(-1, 1)
    lb = sum(torch.mean((t @ w) ** 2) for t in sides) / 4
    px, py = interior["s_x"] @ w, interior["s_y"] @ w
    pxx, pxy, pyy = interior["s_xx"] @ w, interior["s_xy"] @ w, interior["s_yy"] @ w
    pyx = pxy
    M, bu, n = x.shape[0], ux.shape[0], ux.shape[-1]
    bx = M // bu
    rep = lambda t: t[:, None].repeat(1, bx, 1, 1).reshape(-1, n, n)  # noqa: E731
    x1, x2 = x[:, :1], x[:, 1:]
    ux_ = R.interpolate(rep(ux), x1 + px, x2 + py)
    uy_ = R.interpolate(rep(uy), x1 + px, x2 + py)
    a = ux_ * (1 + pxx) + uy_ * pyx
    b = ux_ * pxy + uy_ * (1 + pyy)
    m_xi = R.monitor(alpha[:, None].repeat(1, bx).reshape(-1, 1), a, b)
    lhs = m_xi * ((1 + pxx) * (1 + pyy) - pxy * pyx)
    li = torch.mean((lhs / rhs[:, None].repeat(1, bx).reshape(-1, 1) - 1) ** 2)
    z = torch.zeros((), dtype=pxx.dtype)
    lc = torch.mean(torch.min(z, 1 + pxx) ** 2 + torch.min(z, 1 + pyy) ** 2)
    f = convex_rel * torch.sum(w ** 2) ** 2 + w1 * lb + w0 * li + w2 * lc
    return f, (li, lb, lc), lhs.reshape(-1)


@functools.lru_cache(maxsize=None)
def small_problem(bu=2, bx=8, n=8):
    """A float64 objective small enough for central differences: the features of
    array_case(7, bu, head (3, 512, 16)) at bx random interior points and bx // 4
    boundary points per side and field, random smooth fields on an n x n lattice.
    Returns (w, kwargs of objective_ref)."""
    c = C.array_case(7, bu, (3, 512, 16))
    g = torch.Generator().manual_seed(5)
    x = torch.rand(bu * bx, 2, generator=g).double()
    t = torch.linspace(0, 1, bx // 4)
    z, o = torch.zeros_like(t), torch.ones_like(t)
    edges = [torch.stack(p, 1).repeat(bu, 1).double() for p in ((z, t), (o, t), (t, z), (t, o))]
    interior = features_closed_form(c, x)
    sides = [features_closed_form(c, e)["s_x" if k < 2 else "s_y"] for k, e in enumerate(edges)]
    lin = torch.linspace(0, 1, n).double()
    u = torch.stack([torch.sin(3 * lin[None, :] + k) * torch.cos(2 * lin[:, None] - k) for k in range(bu)])
    ux, uy = R.diff_x(u) * (n - 1), R.diff_y(u) * (n - 1)
    alpha, _, rhs = R.alpha_m_rhs(ux, uy)
    # large enough that 1 + phi_xx < 0 at some points: the convexity penalty is live
    w = -10.0 * torch.randn(16, generator=g).double()
    return w, dict(interior=interior, sides=sides, x=x, ux=ux, uy=uy, alpha=alpha, rhs=rhs, w0=1.0, w1=1000.0,
                   w2=1.0, convex_rel=0.01)


@functools.lru_cache(maxsize=None)
def quadratic(n, seed=0):
    """f(x) = x.A x / 2 - b.x with A SPD of eigenvalues linspace(1, 10, n) in a
    random orthogonal basis: (A, b, x0, x_star = A^-1 b), float64."""
    g = torch.Generator().manual_seed(100 + n + seed)
    q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))
    lam = torch.tensor(np.linspace(1.0, 10.0, n))
    A = (q * lam) @ q.t()
    A = (A + A.t()) / 2
    b = torch.randn(n, generator=g, dtype=torch.float64)
    x0 = torch.randn(n, generator=g, dtype=torch.float64)
    return A, b, x0, torch.linalg.solve(A, b)


def quadratic_fun(A, b):
    def fun(x):
        ax = A @ x
        return 0.5 * torch.dot(x, ax) - torch.dot(b, x), ax - b
    return fun


def stall_bound(A, b, u):
    """How close to A^-1 b the driver can be asked to come in arithmetic of unit
    roundoff u.  With tol = 0 it stops when a step no longer decreases the
    computed f.  f(x) - f* = e.A e / 2 >= lam_min |e|^2 / 2 for e = x - x*, and
    the computed f carries an error of about u (|x.A x| / 2 + |b.x|) ~ 3 u |f*|
    near x* (f* = -b.A^-1 b / 2), so decreases stop being visible once
    lam_min |e|^2 / 2 falls under that: |e| <= sqrt(6 u |f*| / lam_min).  Twice
    that is allowed (the last visible decrease may overshoot it)."""
    fs = 0.5 * torch.dot(b, torch.linalg.solve(A, b)).abs().item()
    lam_min = torch.linalg.eigvalsh(A)[0].item()
    return 2.0 * (6.0 * u * fs / lam_min) ** 0.5
