"""The float64 references of the Monge-Ampere jet tests check themselves on the
CPU: the closed-form jet (dmm_jet_cases.jet_closed_form, the formulas of
include/mmpde_hip.h) against float64 autograd through the oracle's model, and
the closed-form reverse pass against autograd.grad.  Both bounds are float64
roundoff with headroom, not measurements."""
import pytest
import torch

import dmm_jet_cases as J
import dmm_rf_cases as RF
import dmm_shape_cases as C
from oracle import dmm_train_ref as R


def _case():
    return C.array_case(7, 2, (3, 512, 16))


def test_closed_form_jet_matches_autograd_through_the_oracle_model():
    c = _case()
    sd = RF._sd64(c)
    grid = RF.rows_of(c, 8)
    phi = R.phi_fn(sd, "array")
    x1 = grid[:, :1].double().clone().requires_grad_(True)
    x2 = grid[:, 1:].double().clone().requires_grad_(True)
    out = phi(c.u.double(), torch.cat((x1, x2), 1))
    px, py = R._grad(out, x1), R._grad(out, x2)
    ref = dict(zip(J.NAMES, (out, px, py, R._grad(px, x1), R._grad(px, x2), R._grad(py, x2))))
    got = J.jet_closed_form(sd, C.branch_ref(c), grid)
    for name in J.NAMES:
        r = ref[name].detach().reshape(-1)
        scale = r.abs().max().item()
        err = (got[name] - r).abs().max().item()
        print(f"{name}: max|err| {err:.3e} of max {scale:.3e}")
        assert scale > 0 and err <= 1e-10 * scale, (name, err, scale)
    # the mixed derivative is symmetric: phi_xy stands for phi_yx
    pyx = R._grad(py, x1).detach().reshape(-1)
    assert (pyx - got["phi_xy"]).abs().max().item() <= 1e-10 * pyx.abs().max().item()
    # the head-only autograd route of the device tests agrees as well
    ag, _ = J.jet_autograd(sd, C.branch_ref(c), grid)
    for name in J.NAMES:
        assert (ag[name] - got[name]).abs().max().item() <= 1e-10 * got[name].abs().max().item(), name


@pytest.mark.parametrize("first_only", [False, True])
def test_closed_form_reverse_pass_matches_autograd(first_only):
    c = _case()
    sd = RF._sd64(c)
    grid = RF.rows_of(c, 8)
    branch = C.branch_ref(c)
    cots = J.cotangents(grid.shape[0], 1, first_only)
    _, ref = J.jet_autograd(sd, branch, grid, cots)
    got = J.jet_reverse(sd, branch, grid, cots)
    for name in J.GRADS:
        r = ref[name]
        assert got[name].shape == r.shape, (name, got[name].shape, r.shape)
        scale = r.abs().max().item()
        err = (got[name] - r).abs().max().item()
        print(f"d/d {name}: max|err| {err:.3e} of max {scale:.3e}")
        assert scale > 0 and err <= 1e-9 * scale, (name, err, scale)


def test_hard_ansatz_product_rule_matches_autograd():
    """dmm_train._jet_derivatives applies x1^2 x2^2 (x1 - 1)^2 (x2 - 1)^2 phi + x1^2 / 2 +
    x2^2 / 2 to the jet by the product rule; against autograd on a polynomial phi."""
    from types import SimpleNamespace

    from mmpde_amd import dmm_train as T, ops

    g = torch.Generator().manual_seed(2)
    x = torch.rand(9, 2, generator=g, dtype=torch.float64)
    x1 = x[:, :1].clone().requires_grad_(True)
    x2 = x[:, 1:].clone().requires_grad_(True)

    def phi(a, b):
        return torch.sin(2 * a + 0.3) * torch.cos(1.5 * b) + a * b * b

    out = (x1 ** 2) * (x2 ** 2) * ((x1 - 1) ** 2) * ((x2 - 1) ** 2) * phi(x1, x2) + 0.5 * x1 ** 2 + 0.5 * x2 ** 2
    px, py = R._grad(out, x1), R._grad(out, x2)
    ref = (px, py, R._grad(px, x1), R._grad(px, x2), R._grad(py, x2))
    p = phi(x1, x2)
    jx, jy = R._grad(p, x1), R._grad(p, x2)
    jet = ops.Jet(*[t.detach() for t in (p, jx, jy, R._grad(jx, x1), R._grad(jx, x2), R._grad(jy, x2))])
    model = SimpleNamespace(jet=lambda u, grid, second_order=True: jet)
    got = T._jet_derivatives(model, None, x1.detach(), x2.detach(), "hard", True)
    for name, a, b in zip(("x", "y", "xx", "xy", "yy"), got, ref):
        assert (a - b.detach()).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item()), name
    soft = T._jet_derivatives(model, None, x1.detach(), x2.detach(), "soft", True)
    assert all(a is b for a, b in zip(soft, jet[1:]))
