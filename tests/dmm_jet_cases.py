"""Float64 references of the Monge-Ampere jet tests (test_gpu_dmm_jet.py on the
device, test_dmm_jet_cases.py on the CPU alone): include/mmpde_hip.h's formulas
for mmpde_dmm_jet and the reverse pass of mmpde_dmm_jet_grad, restated in
float64 torch.

    a = T0 xi + t0_b,  h = tanh a
    P = W_o0[:, L:] T1,  c_b = W_o0[:, :L] branch_b + W_o0[:, L:] t1_b + b_o0
    v_0 = h, v_d = h' T0[:, d], v_de = h'' T0[:, d] T0[:, e]
    z = P v_0 + c_b, z_d = P v_d, z_de = P v_de, s = tanh z
    phi = w_o . s + b_o1, phi_d = w_o . (s' z_d), phi_de = w_o . (s' z_de + s'' z_d z_e)

jet_autograd is the route the training loop takes without the kernels: nested
autograd.grad(create_graph=True) through trunk and out_nn.  The state dict sd is
any dict with the DMM's head entries in float64 (dmm_rf_cases._sd64(c), or
test_gpu_dmm_train._sd64(dmm))."""
import torch

from oracle import refcpu

NAMES = ("phi", "phi_x", "phi_y", "phi_xx", "phi_xy", "phi_yy")
GRADS = ("branch", "t0_w", "t0_b", "t1_w", "t1_b", "o0_w", "o0_b", "o1_w", "o1_b")
KEYS = ("trunk.layers.0.weight", "trunk.layers.0.bias", "trunk.layers.1.weight", "trunk.layers.1.bias",
        "out_nn.layers.0.weight", "out_nn.layers.0.bias", "out_nn.layers.1.weight", "out_nn.layers.1.bias")


def head_of(sd):
    """(T0, t0_b, T1, t1_b, W_o0, b_o0, w_o [L'], b_o1 [1]) in float64, detached."""
    t = [sd[k].detach().double() for k in KEYS]
    t[6] = t[6].reshape(-1)
    return t


def _tables(sd, branch, grid):
    t0, b0, t1, b1, wo, bo, w, b2 = head_of(sd)
    L = t1.shape[0]
    xi, br = grid.double(), branch.double()
    rep = xi.shape[0] // br.shape[0]
    h = torch.tanh(xi @ t0.t() + b0)
    h1 = 1 - h * h
    h2 = -2 * h * h1
    p, q = t0[:, 0], t0[:, 1]
    v = [h, h1 * p, h1 * q, h2 * p * p, h2 * p * q, h2 * q * q]
    P = wo[:, L:] @ t1
    cb = br @ wo[:, :L].t() + wo[:, L:] @ b1 + bo
    z = [vc @ P.t() for vc in v]
    z[0] = z[0] + cb[:, None, :].repeat(1, rep, 1).reshape(-1, cb.shape[-1])
    return (t0, b0, t1, b1, wo, bo, w, b2), L, rep, xi, br, (h, h1, h2, p, q), v, P, z


def jet_closed_form(sd, branch, grid):
    """dict of NAMES -> [rows] float64; branch [B, L] (any float dtype), grid [B per, 2]."""
    (_, _, _, _, _, _, w, b2), _, _, _, _, _, _, _, z = _tables(sd, branch, grid)
    s = torch.tanh(z[0])
    s1 = 1 - s * s
    s2 = -2 * s * s1
    return {"phi": s @ w + b2, "phi_x": (s1 * z[1]) @ w, "phi_y": (s1 * z[2]) @ w,
            "phi_xx": (s1 * z[3] + s2 * z[1] * z[1]) @ w, "phi_xy": (s1 * z[4] + s2 * z[1] * z[2]) @ w,
            "phi_yy": (s1 * z[5] + s2 * z[2] * z[2]) @ w}


def jet_reverse(sd, branch, grid, cots):
    """The gradient of sum_c <cots[c], jet_c> by the closed-form reverse pass:
    dict of GRADS, each in its parameter's shape.  cots: six [rows] tensors in
    NAMES' order, None meaning zero."""
    (t0, b0, t1, b1, wo, bo, w, _), L, rep, xi, br, (h, h1, h2, p, q), v, P, z = _tables(sd, branch, grid)
    n = xi.shape[0]
    g = [(torch.zeros(n, 1, dtype=torch.float64) if c is None else c.double().reshape(-1, 1)) for c in cots]
    s = torch.tanh(z[0])
    s1 = 1 - s * s
    s2 = -2 * s * s1
    s3 = -2 * (s1 * s1 + s * s2)
    l1 = g[1] * z[1] + g[2] * z[2]
    l2 = g[3] * z[3] + g[4] * z[4] + g[5] * z[5]
    q2 = g[3] * z[1] * z[1] + g[4] * z[1] * z[2] + g[5] * z[2] * z[2]
    a0 = g[0] * s + s1 * (l1 + l2) + s2 * q2
    dz = [w * (g[0] * s1 + s2 * (l1 + l2) + s3 * q2),
          w * (g[1] * s1 + s2 * (2 * g[3] * z[1] + g[4] * z[2])),
          w * (g[2] * s1 + s2 * (g[4] * z[1] + 2 * g[5] * z[2])),
          w * g[3] * s1, w * g[4] * s1, w * g[5] * s1]
    dP = sum(d.t() @ vc for d, vc in zip(dz, v))
    dv = [d @ P for d in dz]
    dcb = dz[0].reshape(br.shape[0], rep, -1).sum(1)
    dc0 = dcb.sum(0)
    wb, wt = wo[:, :L], wo[:, L:]
    h3 = -2 * (h1 * h1 + h * h2)
    da = dv[0] * h1 + h2 * (dv[1] * p + dv[2] * q) + h3 * (dv[3] * p * p + dv[4] * p * q + dv[5] * q * q)
    dp = (dv[1] * h1 + h2 * (2 * dv[3] * p + dv[4] * q) + da * xi[:, :1]).sum(0)
    dq = (dv[2] * h1 + h2 * (dv[4] * p + 2 * dv[5] * q) + da * xi[:, 1:]).sum(0)
    return {"branch": dcb @ wb, "t0_w": torch.stack((dp, dq), 1), "t0_b": da.sum(0), "t1_w": wt.t() @ dP,
            "t1_b": wt.t() @ dc0, "o0_w": torch.cat((dcb.t() @ br, dP @ t1.t() + dc0[:, None] * b1[None, :]), 1),
            "o0_b": dc0, "o1_w": a0.sum(0)[None, :], "o1_b": g[0].sum().reshape(1)}


def jet_autograd(sd, branch, grid, cots=None, dtype=torch.float64, device="cpu"):
    """The nested-autograd route in `dtype` on `device`: (dict of NAMES -> [rows],
    dict of GRADS or None).  With cots the gradient of sum_c <cots[c], jet_c> in
    branch and the eight head tensors comes from autograd.grad."""
    leaves = [sd[k].detach().to(device, dtype).clone().requires_grad_(True) for k in KEYS]
    hsd = dict(zip(KEYS, leaves))
    br = branch.detach().to(device, dtype).clone().requires_grad_(True)
    rep = grid.shape[0] // br.shape[0]
    brr = br[:, None, :].expand(-1, rep, -1).reshape(-1, br.shape[-1])
    x1 = grid[:, :1].detach().to(device, dtype).clone().requires_grad_(True)
    x2 = grid[:, 1:].detach().to(device, dtype).clone().requires_grad_(True)
    trunk, _ = refcpu.densenet(hsd, "trunk", torch.cat((x1, x2), dim=1), 2)
    phi, _ = refcpu.densenet(hsd, "out_nn", torch.cat((brr, trunk), dim=-1), 2)

    def d(out, x):
        return torch.autograd.grad(out, x, grad_outputs=torch.ones_like(out), retain_graph=True, create_graph=True)[0]

    px, py = d(phi, x1), d(phi, x2)
    jet = [phi, px, py, d(px, x1), d(px, x2), d(py, x2)]
    out = {n: t.detach().reshape(-1) for n, t in zip(NAMES, jet)}
    if cots is None:
        return out, None
    total = sum((c.to(device, dtype).reshape(-1, 1) * t).sum() for c, t in zip(cots, jet) if c is not None)
    gr = torch.autograd.grad(total, [br] + leaves, allow_unused=True)
    gr = [torch.zeros_like(t) if g is None else g for g, t in zip(gr, [br] + leaves)]
    return out, dict(zip(GRADS, gr))


def cotangents(rows, seed, first_only=False):
    """Six random [rows] float32 cotangents (the last three None with first_only)."""
    g = torch.Generator().manual_seed(4000 + seed + 7 * rows)
    c = [torch.randn(rows, generator=g) for _ in range(6)]
    return c[:3] + [None] * 3 if first_only else c
