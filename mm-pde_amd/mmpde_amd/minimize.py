"""BFGS with a strong-Wolfe line search, for the random-feature phase of DMM
training (mmpde_amd.dmm_train.random_feature_epoch; the reference calls
pytorch-minimize's ``minimize(..., method='bfgs', options=dict(line_search=
'strong-wolfe'), tol=0)``, mesh/dmm_utils.py:924-933).

Written from the algorithm (Nocedal & Wright, Numerical Optimization, alg. 6.1),
not ported: pytorch-minimize is not a dependency and was not available to
compare against.  As far as can be told without running it, its bfgs with
line_search='strong-wolfe' uses the same line-search routine,
torch.optim.lbfgs._strong_wolfe, which this driver calls; nothing more than
that is claimed about parity with it.  Newton-CG (the reference's
rf_opt_alg='Newton') is not built.

* H_0 = I, d = -H g; first trial step min(1, 1 / |g|_1), then 1;
* line search: torch.optim.lbfgs._strong_wolfe, c1 = 1e-4, c2 = 0.9, at most 25
  evaluations;
* H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T, skipped when y.s <= 1e-10;
* tol = 0 as the reference passes: the iteration stops on max_iter, on a
  non-finite value, or on a step that does not decrease f, and such a step is
  not taken -- the result is never a point with a larger objective than x0.

The two O(n^2) operations go through a small backend object: ``HipDense`` (the
default; mmpde_sym_matvec / mmpde_bfgs_update, float32, n <= 1024) or
``TorchDense`` (plain torch ops in x0's dtype on x0's device, used by the tests
to check the driver on the CPU in float64).  The O(n) vector algebra is torch
ops, control flow is on the host, and each evaluation reads one scalar back.
"""
from __future__ import annotations

import collections
import math

import torch
from torch.optim.lbfgs import _strong_wolfe

Result = collections.namedtuple("Result", ("x", "fun", "grad", "nit", "nfev", "status"))
Result.__doc__ = """minimize_bfgs's result: x, fun = f(x) (float), grad = f'(x), nit iterations taken, nfev
evaluations of fun, status: 0 the gradient vanished, 1 max_iter reached, 2 a step did not
decrease f (or d was no descent direction), 3 a non-finite value."""

YS_MIN = 1e-10


class TorchDense:
    """The dense operations as torch ops in the dtype and on the device of x0."""

    def eye(self, x0):
        return torch.eye(x0.numel(), dtype=x0.dtype, device=x0.device)

    def matvec(self, H, g, scale):
        return scale * (H @ g)

    def update(self, H, s, y):
        ys = torch.dot(y, s)
        if not float(ys) > YS_MIN:
            return H
        rho = 1.0 / ys
        hy = H @ y
        H -= rho * (torch.outer(s, hy) + torch.outer(hy, s))
        H += (rho * rho * torch.dot(y, hy) + rho) * torch.outer(s, s)
        return H


class HipDense:
    """The dense operations on mmpde_sym_matvec / mmpde_bfgs_update (float32 device
    tensors, n <= 1024; fixed-order sums, so a run repeats bit for bit)."""

    def eye(self, x0):
        from . import _lib as L
        from . import ops

        if x0.numel() > L.BFGS_MAX_N:
            raise ValueError(f"n = {x0.numel()}: the dense BFGS operations take n <= {L.BFGS_MAX_N}")
        L.require_device(x0)
        if x0.dtype != torch.float32:
            raise ValueError("HipDense works in float32")
        self._ops = ops
        self._ws = torch.empty((L.lib().mmpde_bfgs_update_workspace_bytes(x0.numel()) // 4,),
                               dtype=torch.float32, device=x0.device)
        return torch.eye(x0.numel(), dtype=torch.float32, device=x0.device)

    def matvec(self, H, g, scale):
        return self._ops.sym_matvec(H, g.contiguous(), scale)

    def update(self, H, s, y):
        return self._ops.bfgs_update(H, s.contiguous(), y.contiguous(), self._ws)


def minimize_bfgs(fun, x0: torch.Tensor, max_iter: int, dense=None) -> Result:
    """Minimise fun from x0 (a 1-D tensor; float32 on the device with the default
    backend).  fun(x) -> (f, g): f a scalar (tensor or float), g like x; both are
    copied before the next call, so fun may reuse its buffers."""
    dense = HipDense() if dense is None else dense
    x = x0.detach().clone().reshape(-1)
    nfev = [0]

    def evaluate(xx):
        f, g = fun(xx)
        nfev[0] += 1
        return float(f), g.detach().reshape(-1).clone()

    def along(xx, t, d):
        return evaluate(xx + t * d)

    f, g = evaluate(x)
    if not math.isfinite(f) or not bool(torch.isfinite(g).all()):
        return Result(x, f, g, 0, nfev[0], 3)
    H = dense.eye(x)
    nit, status = 0, 1
    while nit < max_iter:
        if not bool(g.any()):
            status = 0
            break
        d = dense.matvec(H, g, -1.0)
        gtd = float(torch.dot(g, d))
        if not gtd < 0.0:                       # no descent direction (or NaN)
            status = 2 if math.isfinite(gtd) else 3
            break
        t = min(1.0, 1.0 / float(g.abs().sum())) if nit == 0 else 1.0
        f_new, g_new, t, _ = _strong_wolfe(along, x, t, d, f, g, gtd, c1=1e-4, c2=0.9, max_ls=25)
        f_new = float(f_new)
        if not math.isfinite(f_new) or not bool(torch.isfinite(g_new).all()):
            status = 3
            break
        if not f_new < f:
            status = 2
            break
        s = t * d
        y = g_new - g
        x = x + s
        f, g = f_new, g_new
        nit += 1
        dense.update(H, s, y)
    return Result(x, f, g, nit, nfev[0], status)
