"""Cases, float64 references and the float32 host restatement of the fold guard
(mmpde_dmm_mesh_relax, ops.mesh_relax, DMM.mesh_guarded).  Used by
test_mesh_guard_cases.py on the CPU alone and by test_gpu_mesh_relax.py /
test_gpu_mesh_guard.py on the device.  Models and inputs are those of
dmm_hess_cases.py / dmm_shape_cases.py (unchanged) with the head scaled as
dmm_hess_cases.fold_sd does.

The contract: with lambda_n = (h11 + h22) / 2 - sqrt(((h11 - h22) / 2)^2 +
h12^2) the smaller eigenvalue of Hess phi at a node and lam_b its minimum over a
trajectory, alpha_b = alpha_max where 1 + alpha_max lam_b >= delta, (1 - delta) /
(-lam_b) otherwise, 0 where lam_b is NaN; x = alpha_b x1 + (1 - alpha_b) xi, every
operation rounded to float32 by itself.

Bars, from the project's Hessian bar h_bar = 2e-5 max|H_ref| (dmm_hess_cases):
by Weyl's inequality an entrywise error of h_bar moves an eigenvalue of a
symmetric 2 x 2 matrix by at most ||dH||_F <= 2 h_bar; the float32 evaluation of
the formula gets another 0.5 h_bar = 1e-5 max|H| (about 100 x its few-ulp
error): LAM_BARS = 2.5.  alpha = (1 - delta) / (-lam) then moves by at most
alpha_ref e / (|lam_ref| - e), e = 2.5 h_bar, plus 4 ulp for the float32 division
and subtraction.  A case is usable only if every trajectory's 1 + alpha_max
lam_ref is further than 100 h_bar from delta (the guarded / not guarded decision
is then defined at float32 accuracy); test_mesh_guard_cases.py asserts that.
"""
import math

import torch

import dmm_hess_cases as H

LAM_BARS = 2.5
MARGIN_BARS = 100.0

# (name, base case args, w_o factor, Wb factor, delta, alpha_max).  delta of the
# two 'mixed' graph cases sits in the middle of the widest gap of the sorted
# lam_b (float64, CPU): graph-130-B3 at 24 / 64 has lam_b -0.9064, -0.8320,
# -0.8805 (gap 0.048 between the last two), graph-130-B33 at 56 / 8 has lam_b in
# [-0.9402, -0.9023] with its widest gap, 0.0045, between -0.9121 and -0.9076.
GUARD_CASES = (
    ("array-33-B3-mixed", ("array", 33, 3), 64.0, 64.0, 0.1, 1.0),            # alpha 1, 1, 0.7456
    ("array-33-B3-d025", ("array", 33, 3), 64.0, 64.0, 0.25, 1.0),            # alpha 1, 0.9617, 0.6213
    ("array-33-B3-a09", ("array", 33, 3), 64.0, 64.0, 0.1, 0.9),              # alpha 0.9, 0.9, 0.7456
    ("graph-130-B3-all", ("graph", 130, 3), 16.0, 16.0, 0.1, 1.0),            # mesh_hess_wave_kernel<8>; all guarded
    ("graph-130-B33-all", ("graph", 130, 33), 64.0, 8.0, 0.1, 1.0),           # mesh_hess_kernel; all guarded
    ("graph-130-B3-mixed", ("graph", 130, 3), 24.0, 64.0, 0.1438, 1.0),       # guarded, not, guarded
    ("graph-130-B33-mixed", ("graph", 130, 33), 56.0, 8.0, 0.0901, 1.0),      # 3 of 33 not guarded
)
# the unscaled cases: min lam between -0.08 and -0.009, nothing guarded at any delta <= 0.5
BASE_CASES = (("graph", 130, 3), ("graph", 130, 33), ("array", 33, 3))
_REFS = {}


def f32(x):
    """x rounded to float32, as a Python float (what the C entry receives)."""
    return float(torch.tensor(x, dtype=torch.float32))


def ulp32(x):
    """The spacing of float32 at |x| (>= the smallest normal)."""
    return 2.0 ** (math.floor(math.log2(max(abs(x), 2.0 ** -126))) - 23)


def lam_of(h):
    """The smaller eigenvalue of the symmetric [.., 3] = (h11, h12, h22), in h's
    dtype, every operation rounded by itself (torch runs them one by one)."""
    d = 0.5 * (h[..., 0] - h[..., 2])
    return 0.5 * (h[..., 0] + h[..., 2]) - torch.sqrt(d * d + h[..., 1] * h[..., 1])


def lam_of_rounded32(h):
    """lam_of for float32 h with every operation correctly rounded to float32,
    whatever the host's float32 kernels do: each one is done in float64 and
    rounded (float64's 53 bits are >= 2 x 24 + 2, so the sum, difference,
    product or square root of float32 operands rounds twice to what it would
    round to once).  What the kernel must give bit for bit."""
    assert h.dtype == torch.float32

    def r(t):
        return t.float().double()

    h = h.double()
    d = r(0.5 * r(h[..., 0] - h[..., 2]))
    s = r(r(d * d) + r(h[..., 1] * h[..., 1]))
    return r(r(0.5 * r(h[..., 0] + h[..., 2])) - r(torch.sqrt(s))).float()


def alpha_of(lam_b, alpha_max, delta):
    """The contract's step per trajectory, in lam_b's dtype (alpha_max, delta:
    Python floats holding float32 values)."""
    one = torch.ones((), dtype=lam_b.dtype)
    am = torch.full_like(lam_b, alpha_max)
    dl = torch.full_like(lam_b, delta)
    keep = (one + am * lam_b) >= dl
    a = torch.where(keep, am, torch.minimum((one - dl) / (-lam_b), am))
    return torch.where(torch.isnan(lam_b), torch.zeros_like(a), a)


def lam_min(lam_n):
    """min over dim 1, NaN if any entry is."""
    m = lam_n.min(1).values
    return torch.where(torch.isnan(lam_n).any(1), torch.full_like(m, float("nan")), m)


def relax32(x1, xi, alpha_b):
    """alpha x1 + (1 - alpha) xi in float32 on the host: x1 [B N, 2], xi [N, 2],
    alpha_b [B], all float32.  Rows of alpha == 1 are x1's, of alpha == 0 xi's."""
    assert x1.dtype == xi.dtype == alpha_b.dtype == torch.float32
    B, N = alpha_b.shape[0], xi.shape[0]
    a = alpha_b[:, None, None]
    x = x1.reshape(B, N, 2)
    out = a * x + (1.0 - a) * xi[None]
    out = torch.where(a == 1.0, x, out)
    out = torch.where(a == 0.0, xi[None].expand(B, N, 2), out)
    return out.reshape(B * N, 2)


def det_alpha64(h, alpha_b):
    """(det(I + alpha H) in float64 [B, N], the float32 rounding bound of det_of's
    evaluation of it): h [B N, 3], alpha_b [B] (the float32 values)."""
    B = alpha_b.shape[0]
    s = alpha_b.double()[:, None, None] * h.double().reshape(B, -1, 3)
    s11, s12, s22 = s[..., 0], s[..., 1], s[..., 2]
    det = (1 + s11) * (1 + s22) - s12 * s12
    # three scaled entries, the product, the square and three sums, each within
    # 2^-24 of a value no larger than the sum of the magnitudes
    tol = 8 * 2.0 ** -24 * (1 + s11.abs() + s22.abs() + (s11 * s22).abs() + s12 * s12)
    return det, tol


def guard_ref(name):
    """A GUARD_CASES entry's case, scaled state dict and float64 reference: H
    [B N, 3], lam_n [B, N], lam_b, alpha_ref, guarded [B] (bool), h_bar, and the
    float32 values of delta and alpha_max."""
    if name in _REFS:
        return _REFS[name]
    _, args, f_wo, f_wb, delta, alpha_max = next(g for g in GUARD_CASES if g[0] == name)
    c = H.base_case(*args)
    sd = H.fold_sd(c, f_wo, f_wb)
    ref, _ = H.hess_ref(c, sd=sd, key=("guard", args, f_wo, f_wb))
    r = type("GuardRef", (), {})()
    r.c, r.sd, r.H = c, sd, ref
    r.delta, r.alpha_max = f32(delta), f32(alpha_max)
    r.h_bar = H.h_bar(ref)
    r.lam_n = lam_of(ref).reshape(c.B, -1)
    r.lam_b = lam_min(r.lam_n)
    r.alpha = alpha_of(r.lam_b, r.alpha_max, r.delta)
    r.guarded = (1 + r.alpha_max * r.lam_b) < r.delta
    _REFS[name] = r
    return r


def alpha_bar(alpha_ref, lam_ref, h_bar):
    """|alpha - alpha_ref| allowed on a guarded trajectory."""
    e = LAM_BARS * h_bar
    return alpha_ref * e / (abs(lam_ref) - e) + 4 * ulp32(alpha_ref)
