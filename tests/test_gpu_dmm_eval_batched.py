"""dmm_train.evaluate / evaluate_tri with batch=K (K fields per model call on
DMM.mesh_fields, ops.mesh_monitor and ops.mesh_quality) against the per-field
route (batch=None) and against the float64 oracle/dmm_train_ref.evaluate_one /
evaluate_tri_one, in train() and eval() mode; models and fields as
test_gpu_dmm_train.py builds them.

Burgers, s = 48: 5 fields, batch 1, 2 (chunks 2 + 2 + 1), 5, 8 (more than the
fields).  Cylinder, 2521 points: 3 fields, batch 1, 2, 3.  Every route of a case
starts from the same model state and the same numpy seed, runs once and is
shared by the tests below.

Bars: 2e-4 relative on mean, std and range against the per-field route and
against float64 (the bar test_evaluate_vs_oracle / test_evaluate_tri_vs_oracle
hold the per-field route to); 1e-6 relative between batch sizes and on the
running statistics against the per-field route with hip_branch_train (the same
kernels, K rows of work in one launch or in K: fp32 rounding of a handful of
operations at most; whether they are bitwise equal is printed); 2e-6 absolute
on DMM.mesh_fields' rows against each field's mesh computed alone (the bar the
rollout tests hold the analytic mesh to against autograd)."""
import copy

import numpy as np
import pytest
import torch

import test_gpu_dmm_train as D
from oracle import dmm_train_ref as R
from oracle import refcpu

pytestmark = pytest.mark.gpu

FIELDS = {"burgers": 5, "cy": 3}
BATCHES = {"burgers": (1, 2, 5, 8), "cy": (1, 2, 3)}
SEED = 11
NAMES = ("mean", "std", "range")
CASES = [(k, m, b) for k in ("burgers", "cy") for m in ("train", "eval") for b in BATCHES[k]]
MODES = [(k, m) for k in ("burgers", "cy") for m in ("train", "eval")]

_SETUP, _RUNS, _ORACLE = {}, {}, {}


def _setup(kind, dev):
    if kind not in _SETUP:
        pde, dmm = D._models(kind)
        sds = (D._sd64(dmm), D._sd64(dmm))            # the train-mode oracle advances its running statistics
        all_u = D._data(kind, pde, FIELDS[kind])
        dmm.to(dev)
        _SETUP[kind] = (pde, dmm, sds, all_u, copy.deepcopy(dmm.state_dict()))
    return _SETUP[kind]


def _bns(dmm):
    return [m for m in dmm.modules() if isinstance(m, torch.nn.BatchNorm1d)]


def _call(kind, dmm, all_u, dev, batch):
    from mmpde_amd import dmm_train as T
    if kind == "burgers":
        return T.evaluate(dmm, all_u, dev, batch=batch)
    return T.evaluate_tri(dmm, all_u[:, :, 2], all_u[0, :, :2], dev, batch=batch)


def _run(kind, mode, batch, dev, hip_branch=False):
    """One evaluate[_tri] call from the initial model state and numpy seed:
    (mean, std, range), the numpy state after it, the BatchNorm buffers after it."""
    key = (kind, mode, batch, hip_branch)
    if key not in _RUNS:
        _, dmm, _, all_u, state0 = _setup(kind, dev)
        dmm.load_state_dict(state0)
        dmm.train(mode == "train")
        dmm.hip_branch_train = hip_branch
        np.random.seed(SEED)
        try:
            got = _call(kind, dmm, all_u, dev, batch)
        finally:
            dmm.hip_branch_train = False
        rng = np.random.get_state()
        bn = [(int(m.num_batches_tracked), m.running_mean.cpu().clone(), m.running_var.cpu().clone())
              for m in _bns(dmm)]
        _RUNS[key] = (got, rng, bn)
    return _RUNS[key]


def _oracle(kind, mode, dev):
    key = (kind, "train" if kind == "burgers" else mode)   # the array model has no BatchNorm: one function
    if key not in _ORACLE:
        pde, _, sds, all_u, _ = _setup(kind, dev)
        F = FIELDS[kind]
        if kind == "burgers":
            phi = D._phi(kind, pde, sds[0])
            per = [R.evaluate_one(phi, all_u[[t]].double(), 48) for t in range(F)]
        else:
            from scipy.spatial import Delaunay
            grid = all_u[0, :, :2]
            tris = torch.from_numpy(Delaunay(grid.numpy()).simplices.astype(np.int64))
            if mode == "train":
                phi = D._phi(kind, pde, sds[0])
            else:   # eval(): DMM.mesh takes the grid it is given for the branch as well
                def phi(u, X):
                    return refcpu.dmm_forward(sds[1], "graph", u, X, ori_grid=grid.double(), train=False)
            per = [R.evaluate_tri_one(phi, all_u[[t], :, 2].double(), grid.double(), tris) for t in range(F)]
        _ORACLE[key] = [float(np.mean([p[i] for p in per])) for i in range(3)]
    return _ORACLE[key]


def _rel(got, ref, bar, what):
    for name, a, b in zip(NAMES, got, ref):
        err = abs(a - b) / abs(b)
        print(f"{what} {name}: {a!r} against {b!r}, relative {err:.3e} (bar {bar:.0e})")
    for name, a, b in zip(NAMES, got, ref):
        assert abs(a - b) <= bar * abs(b), (what, name, a, b)


@pytest.mark.parametrize("kind,mode,batch", CASES, ids=[f"{k}-{m}-batch{b}" for k, m, b in CASES])
def test_batched_against_per_field_and_oracle(dev, kind, mode, batch):
    got, rng, bn = _run(kind, mode, batch, dev)
    assert isinstance(got, tuple) and len(got) == 3 and all(type(v) is float and np.isfinite(v) for v in got)
    want, rng0, bn0 = _run(kind, mode, None, dev)
    _rel(got, want, 2e-4, f"{kind} {mode} batch={batch} against the per-field route")              # (a)
    _rel(got, _oracle(kind, mode, dev), 2e-4, f"{kind} {mode} batch={batch} against float64")      # (b)
    assert rng[0] == rng0[0] and np.array_equal(rng[1], rng0[1]) and rng[2:] == rng0[2:], \
        "the numpy generator is left in another state than by the per-field route"                 # (c)
    if kind == "cy":                                                                               # (d)
        F = FIELDS[kind]
        assert len(bn) == 5
        steps = F if mode == "train" else 0
        base = int(_SETUP[kind][4]["embedding_mlp.1.num_batches_tracked"])
        assert [b[0] for b in bn] == [b[0] for b in bn0] == [base + steps] * 5
        _, _, bn_hip = _run(kind, mode, None, dev, hip_branch=True)
        for i, (a, h) in enumerate(zip(bn, bn_hip)):
            for name, x, y in (("running_mean", a[1], h[1]), ("running_var", a[2], h[2])):
                err, scale = (x - y).abs().max().item(), y.abs().max().item()
                print(f"cy {mode} batch={batch} BatchNorm {i} {name}: max|diff| {err:.3e} of max {scale:.3e}, "
                      f"bitwise {torch.equal(x.view(torch.int32), y.view(torch.int32))}")
                assert err <= 1e-6 * scale, (i, name, err, scale)


@pytest.mark.parametrize("kind,mode", MODES, ids=[f"{k}-{m}" for k, m in MODES])
def test_batch_sizes_agree(dev, kind, mode):                                                       # (e)
    first = _run(kind, mode, BATCHES[kind][0], dev)[0]
    for batch in BATCHES[kind][1:]:
        got = _run(kind, mode, batch, dev)[0]
        print(f"{kind} {mode}: batch={batch} bitwise equal to batch={BATCHES[kind][0]}: {got == first}")
        _rel(got, first, 1e-6, f"{kind} {mode} batch={batch} against batch={BATCHES[kind][0]}")


@pytest.mark.parametrize("kind,mode", MODES, ids=[f"{k}-{m}" for k, m in MODES])
def test_mesh_fields_rows_are_each_field_alone(dev, kind, mode):                                   # (f)
    from mmpde_amd import dmm_train as T
    _, dmm, _, all_u, state0 = _setup(kind, dev)
    dmm.load_state_dict(state0)
    dmm.train(mode == "train")
    if kind == "burgers":
        u, xi = all_u.to(dev), T.unit_lattice(48, dev)
    else:
        u, xi = all_u[:, :, 2].contiguous().to(dev), all_u[0, :, :2].contiguous().to(dev)
    N = xi.shape[0]
    mesh = dmm.mesh_fields(u, xi)
    assert mesh.shape == (u.shape[0] * N, 2) and mesh.dtype == torch.float32 and not mesh.requires_grad
    for f in range(u.shape[0]):
        rows = mesh[f * N:(f + 1) * N]
        alone = dmm.mesh_fields(u[[f]], xi)
        moved = T._moved(dmm, u[[f]], xi)            # train(): autograd through the torch forward; eval(): DMM.mesh
        for what, other in (("mesh_fields of the field alone", alone), ("the per-field route's mesh", moved)):
            err = (rows - other).abs().max().item()
            print(f"{kind} {mode} field {f} against {what}: max|diff| {err:.3e}, bitwise {torch.equal(rows, other)}")
            assert err <= 2e-6, (what, f, err)


def test_mesh_fields_refuses_another_hidden_width(dev):
    from mmpde_amd.dmm_model import DMM
    pde, _, _, all_u, _ = _setup("cy", dev)
    wide = DMM(mode="graph", grid=pde.ori_grid, branch_layer=[8, 3], trunk_layer=[2, 16, 512],
               out_layer=[1024, 512, 1]).to(dev).train()
    u, xi = all_u[:2, :, 2].contiguous().to(dev), all_u[0, :, :2].contiguous().to(dev)
    with pytest.raises(NotImplementedError, match="hidden_features == 4"):
        wide.mesh_fields(u, xi)


KEYS = {"model_state_dict", "loss_in", "loss_bound", "loss_convex", "args", "train_std", "train_minmax", "test_std",
        "test_minmax", "test_equ_loss", "logs"}


@pytest.mark.parametrize("kind", ["burgers", "cy"])
def test_train_MA_res_eval_batch(dev, tmp_path, kind):  # noqa: N802                                (g)
    from mmpde_amd import dmm_train as T
    pde, dmm = D._models(kind)
    all_u = D._data(kind, pde, 6)
    args = D._args(kind, 8, 10 if kind == "cy" else 4)      # the cylinder sampler draws fields in tens
    dmm.to(dev)
    np.random.seed(21)
    out = T.train_MA_res(all_u, all_u, all_u[:2], args, dmm, False, 1, 0, dev, save_dir=str(tmp_path),
                         evaluate_every=1, eval_batch=4)
    assert len(out) == 15 and out[0] is dmm
    for i in (8, 9, 10, 11):                          # train_std, train_minmax, test_std, test_minmax
        assert len(out[i]) == 1 and np.isfinite(out[i][0]) and out[i][0] > 0, (i, out[i])
    ckpt = torch.load(tmp_path / f"dmm_{kind}_epoch1.pt", weights_only=False)
    assert set(ckpt) == KEYS
    assert ckpt["train_std"] == out[8] and ckpt["test_std"] == out[10]
    with pytest.raises(ValueError):
        T.train_MA_res(all_u, all_u, all_u[:2], args, dmm, False, 1, 0, dev, save_dir=False, eval_batch=0)
