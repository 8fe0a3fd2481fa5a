"""Mesh quality on HIP (csrc/mesh_quality.hip, ops.mesh_monitor / ops.mesh_quality,
MMPDERollout.mesh_quality) against float64 on the CPU.

Every reference is float64 computed from the same fp32 inputs, through the
oracle's restatement of the reference (oracle.dmm_train_ref: diff_x, diff_y,
alpha_m_rhs, tri_lattice_derivatives, interpolate) and the short restatement
of area, centre and statistics below.  Bars, both the project's own:
per-element quantities (m, mg) 2e-5 max|ref| + 1e-6 (test_gpu_dmm_train.py's
smoother bars), the three statistics and rhs / alpha 2e-4 relative per
trajectory (its evaluate bars), counts exact.  area_ratio_min has the bound
that fp32 gives the two signed areas of a cell: each cross product p1 - p2 of
fp32 edge differences carries at most 4 u (|p1| + |p2|), u = 2^-24 (two rounded
factors and the product's own rounding per term, the difference's rounding on
top), the quotient 2 u more, so |d ratio| <= |ratio| (4 u (k_moved + k_fixed) +
2 u) with k = (|p1| + |p2|) / |p1 - p2| of that cell; the minimum over cells
lies between the minima of ratio -/+ that bound.

Meshes: xi itself, the smooth move xi + 0.01 (sin 2 pi y, cos 2 pi x) and the
same move at amplitude 0.05 (which inverts one of the 91 triangles of the 50
random points: slivers invert under a map whose Jacobian is positive
everywhere) in every batch of three; the lattice quadrilaterals do not invert
at 0.05 (|grad| = 0.31 < 1), so the quad batches carry a fourth trajectory at
amplitude 0.25 (det(dx/dxi) down to 1 - 2.47), which does fold them (6 of 25,
8 of 64, 501 of 2209 cells; none of the 3 x 3 lattice's four, whose nodes sit on
the zeros of sin 2 pi y).  The shapes fixed at B = 2 run two batches: (xi, 0.25)
and (0.01, 0.05) for s = 48, (xi, 0.05) and (0.01, 0.05) for the 2521 points,
whose slivers invert at both amplitudes (5 and 17 of 5022 triangles in
float64).  Exact counts need every cell of the float64 reference to hold
|signed area| >= 1e-4 of its fixed-grid area: asserted on the reference alone
before anything is compared (it holds for every case below; no cell is
excluded).  A trajectory's reference is computed once and shared.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import dmm_train_ref as R

pytestmark = pytest.mark.gpu

ELEM_RTOL, ELEM_ATOL = 2e-5, 1e-6
STAT_RTOL = 2e-4
MARGIN = 1e-4
U24 = 2.0 ** -24
AMPS = {"xi": 0.0, "smooth": 0.01, "fold": 0.05, "fold_big": 0.25}


def _eq(a, b):
    """torch.equal on the bits (NaN statistics compare equal to themselves)."""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _elem(got, ref, what):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    bound = ELEM_RTOL * ref.abs().max().item() + ELEM_ATOL
    print(f"{what}: max|err| {err:.3e} bound {bound:.3e} max|ref| {ref.abs().max().item():.3e}")
    assert err <= bound, (what, err, bound)


def _stat(got, ref, what):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    rel = ((got - ref).abs() / ref.abs()).max().item()
    print(f"{what}: max rel err {rel:.3e} bound {STAT_RTOL:.1e} ref {ref.tolist()}")
    assert rel <= STAT_RTOL, (what, rel)


# ----------------------------------------------------------------------------- inputs
def _lattice32(s):
    from mmpde_amd.dmm_train import unit_lattice

    return unit_lattice(s, "cpu").clone()


def _field(points, batches, seed):
    from mmpde_amd.synth import fields

    return fields(points, batches, 1, seed=seed)[:, 0].contiguous()          # [B, N] fp32


def _moved32(xi32, kinds):
    """[B, N, 2] fp32: xi + a (sin 2 pi y, cos 2 pi x), formed in float64 and rounded once."""
    xi = xi32.double()
    out = []
    for k in kinds:
        a = AMPS[k]
        if a == 0.0:
            out.append(xi32.clone())
        else:
            d = torch.stack((torch.sin(2 * math.pi * xi[:, 1]), torch.cos(2 * math.pi * xi[:, 0])), 1)
            out.append((xi + a * d).float())
    return torch.stack(out)


# ----------------------------------------------------------------------------- float64 restatement
def _geom64(pts, cells):
    """pts [N, 2] float64, cells [C, 3 | 4] -> (area, centre [C, 2], signed area,
    k = (|p1| + |p2|) / |p1 - p2| of the signed area's cross product)."""
    v = pts[cells.long()]
    if cells.shape[1] == 4:
        bl, br, tl, tr = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
        d1 = ((bl - tr) ** 2).sum(1) ** 0.5                  # dmm_utils.py:1269-1272
        d2 = ((br - tl) ** 2).sum(1) ** 0.5
        area = d1 * d2 / 2
        cen = (bl + br + tl + tr) / 4
        a, b = tr - bl, tl - br
    else:
        # the reference's determinant form of the triangle area
        area = 0.5 * (v[:, 0, 0] * (v[:, 1, 1] - v[:, 2, 1]) + v[:, 1, 0] * (v[:, 2, 1] - v[:, 0, 1])
                      + v[:, 2, 0] * (v[:, 0, 1] - v[:, 1, 1])).abs()
        cen = v.mean(1)
        a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    p1, p2 = a[:, 0] * b[:, 1], a[:, 1] * b[:, 0]
    sgn = 0.5 * (p1 - p2)
    return area, cen, sgn, (p1.abs() + p2.abs()) / (p1 - p2).abs()


def _m_at(m64, cen):
    """R.interpolate (one field per query) in chunks of queries."""
    out = []
    for c in cen.split(512):
        out.append(R.interpolate(m64[None].expand(c.shape[0], -1, -1), c[:, :1], c[:, 1:]).reshape(-1))
    return torch.cat(out)


def _traj64(mesh32, xi32, cells, m32):
    """The float64 reference of one trajectory: mesh32 [N, 2], m32 [n, n]."""
    _, _, sgn_f, k_f = _geom64(xi32.double(), cells)
    assert bool((sgn_f.abs() > 0).all())
    area, cen, sgn, k = _geom64(mesh32.double(), cells)
    ratio = sgn / sgn_f
    # the condition for exact counts, on the reference alone, every cell
    assert bool((ratio.abs() >= MARGIN).all()), ratio.abs().min().item()
    mg = _m_at(m32.double(), cen) * area
    bound = ratio.abs() * (4 * U24 * (k + k_f) + 2 * U24)
    return dict(mg=mg, mean=mg.mean(), std=mg.std(), range=mg.max() - mg.min(),
                inverted=int((~(sgn * torch.sign(sgn_f) > 0)).sum()), ratio=ratio.min(),
                ratio_lo=(ratio - bound).min(), ratio_hi=(ratio + bound).min())


def _batch64(per):
    """Per-trajectory references -> the reference of the batch."""
    return {k: [p[k] for p in per] if k == "inverted" else torch.stack([p[k] for p in per]) for k in per[0]}


@functools.lru_cache(maxsize=None)
def _array_monitor_case(s, B=3):
    u = _field(_lattice32(s), B, seed=11 + s).reshape(B, s, s)
    u64 = u.double()
    alpha, m, rhs = R.alpha_m_rhs(R.diff_x(u64) * (s - 1), R.diff_y(u64) * (s - 1))
    return u, m, alpha, rhs


def _point_grid(N):
    from mmpde_amd.synth import cy_synth_mesh

    if N == 50:
        return torch.rand(50, 2, generator=torch.Generator().manual_seed(0))
    assert N == 2521
    return cy_synth_mesh()


@functools.lru_cache(maxsize=None)
def _point_monitor_case(N, B):
    grid = _point_grid(N)
    u = _field(grid, B, seed=7)
    ux, uy = R.tri_lattice_derivatives(u.double(), grid.double()[None].repeat(B, 1, 1))
    alpha, m, rhs = R.alpha_m_rhs(ux, uy)
    return grid, u, m, alpha, rhs


QUAD4 = ("xi", "smooth", "fold", "fold_big")
TRI3 = ("xi", "smooth", "fold")
CELL_CASES = [("quad", 3, QUAD4), ("quad", 6, QUAD4), ("quad", 9, QUAD4),
              ("quad", 48, ("xi", "fold_big")), ("quad", 48, ("smooth", "fold")),
              ("tri", 50, TRI3), ("tri", 2521, ("xi", "fold")), ("tri", 2521, ("smooth", "fold"))]


@functools.lru_cache(maxsize=None)
def _cell_grid(shape, size):
    """(xi32, cells, the m fields [F, n, n] fp32): m is the float64 monitor of a
    synthetic u, rounded to fp32 once, so the cell cases isolate the cell kernels
    (the monitor kernels have their own tests)."""
    from mmpde_amd import ops

    if shape == "quad":
        xi = _lattice32(size)
        return xi, ops.mesh_cells_lattice(size), _array_monitor_case(size, 3)[1].float().contiguous()
    xi = _point_grid(size)
    m = _point_monitor_case(size, 3 if size == 50 else 1)[2]
    return xi, ops.mesh_cells_delaunay(xi), m.float().contiguous()


@functools.lru_cache(maxsize=None)
def _cell_traj(shape, size, kind, field):
    """One trajectory's mesh and float64 reference, computed once and shared."""
    xi, cells, m = _cell_grid(shape, size)
    mesh = _moved32(xi, (kind,))[0]
    return mesh, _traj64(mesh, xi, cells, m[field])


def _cell_case(shape, size, kinds):
    """(xi32, cells, mesh32 [B, N, 2], m32 [B, n, n], float64 reference);
    trajectory b reads the m field b mod F."""
    xi, cells, m = _cell_grid(shape, size)
    fields = [b % m.shape[0] for b in range(len(kinds))]
    per = [_cell_traj(shape, size, k, f) for k, f in zip(kinds, fields)]
    return xi, cells, torch.stack([p[0] for p in per]), m[fields].contiguous(), _batch64([p[1] for p in per])


def _run(dev, xi, cells, mesh, m32, **kw):
    from mmpde_amd import ops

    B = mesh.shape[0]
    q = ops.mesh_quality(mesh.reshape(-1, 2).to(dev), xi.to(dev), cells, m32.to(dev), B, mg=True, **kw)
    torch.cuda.synchronize()
    return q


# ----------------------------------------------------------------------------- monitor
@pytest.mark.parametrize("s", [3, 6, 9, 48])
def test_monitor_array_vs_float64(dev, s):
    from mmpde_amd import ops

    u, m_ref, alpha_ref, rhs_ref = _array_monitor_case(s)
    m, alpha, rhs = ops.mesh_monitor(u.to(dev))
    assert m.shape == (3, s, s) and alpha.shape == (3,) and rhs.shape == (3,)
    _elem(m, m_ref, f"monitor array s={s} m")
    _stat(alpha, alpha_ref, f"monitor array s={s} alpha")
    _stat(rhs, rhs_ref, f"monitor array s={s} rhs")
    # two runs, and each trajectory alone, give the same bits
    m2, alpha2, rhs2 = ops.mesh_monitor(u.to(dev))
    assert _eq(m, m2) and _eq(alpha, alpha2) and _eq(rhs, rhs2)
    for b in range(3):
        m1, a1, r1 = ops.mesh_monitor(u[b:b + 1].to(dev))
        assert _eq(m1[0], m[b]) and _eq(a1, alpha[b:b + 1]) and _eq(r1, rhs[b:b + 1]), b


@pytest.mark.parametrize("N,B", [(50, 3), (2521, 1)])
def test_monitor_points_vs_float64(dev, N, B):
    from mmpde_amd import ops

    grid, u, m_ref, alpha_ref, rhs_ref = _point_monitor_case(N, B)
    n = math.isqrt(N)
    m, alpha, rhs = ops.mesh_monitor(u.to(dev), grid.to(dev))
    assert m.shape == (B, n, n)
    _elem(m, m_ref, f"monitor points N={N} m")
    _stat(alpha, alpha_ref, f"monitor points N={N} alpha")
    _stat(rhs, rhs_ref, f"monitor points N={N} rhs")
    m2, alpha2, rhs2 = ops.mesh_monitor(u.to(dev), grid.to(dev))
    assert _eq(m, m2) and _eq(alpha, alpha2) and _eq(rhs, rhs2)
    for b in range(B if B > 1 else 0):
        m1, a1, r1 = ops.mesh_monitor(u[b:b + 1].to(dev), grid.to(dev))
        assert _eq(m1[0], m[b]) and _eq(a1, alpha[b:b + 1]) and _eq(r1, rhs[b:b + 1]), b


def test_monitor_constant_field_is_nan_as_in_the_reference(dev):
    from mmpde_amd import ops

    u = torch.full((2, 6, 6), 0.5)
    u[1] = _array_monitor_case(6)[0][0]
    m, alpha, rhs = ops.mesh_monitor(u.to(dev))
    assert alpha[0].item() == 0.0 and bool(torch.isnan(m[0]).all()) and math.isnan(rhs[0].item())
    assert bool(torch.isfinite(m[1]).all())      # and it stays in its own trajectory


# ----------------------------------------------------------------------------- cells
@pytest.mark.parametrize("shape,size,kinds", CELL_CASES)
def test_cell_quality_vs_float64(dev, shape, size, kinds):
    xi, cells, mesh, m32, ref = _cell_case(shape, size, kinds)
    B, C = len(kinds), cells.shape[0]
    q = _run(dev, xi, cells, mesh, m32)
    assert q.mg.shape == (B, C) and q.inverted.dtype == torch.int32
    print(f"{shape} {size} {kinds}: C {C} inverted ref {ref['inverted']} got {q.inverted.tolist()} "
          f"ratio ref {ref['ratio'].tolist()} got {q.area_ratio_min.tolist()}")
    _elem(q.mg, ref["mg"], f"{shape} {size} mg")
    _stat(q.mean, ref["mean"], f"{shape} {size} mean")
    _stat(q.std, ref["std"], f"{shape} {size} std")
    _stat(q.range, ref["range"], f"{shape} {size} range")
    assert q.inverted.tolist() == ref["inverted"]
    got = q.area_ratio_min.double().cpu()
    assert bool((got >= ref["ratio_lo"]).all()) and bool((got <= ref["ratio_hi"]).all()), \
        (got.tolist(), ref["ratio_lo"].tolist(), ref["ratio_hi"].tolist())
    for b, k in enumerate(kinds):
        if k == "xi":        # the fixed grid itself: nothing inverted, every ratio exactly 1
            assert q.inverted[b].item() == 0 and q.area_ratio_min[b].item() == 1.0
        # every batch holds a trajectory that folds (the 3 x 3 lattice apart: its
        # nodes sit on the zeros of sin 2 pi y, the move only shifts its columns)
        if (k == "fold_big" and size != 3) or (k == "fold" and shape == "tri"):
            assert q.inverted[b].item() > 0 and q.area_ratio_min[b].item() < 0
    # two runs of the same call, and each trajectory alone against the batch
    q2 = _run(dev, xi, cells, mesh, m32)
    for name in q._fields:
        assert _eq(getattr(q, name), getattr(q2, name)), name
    for b in range(B):
        q1 = _run(dev, xi, cells, mesh[b:b + 1], m32[b:b + 1])
        for name in q._fields:
            assert _eq(getattr(q1, name)[0], getattr(q, name)[b]), (b, name)


def test_float64_figures_on_the_50_points():
    """What the float64 restatement gives on the 50 random points: 91
    triangles; amplitude 0.01: none inverted, smallest ratio 0.218; amplitude
    0.05: one inverted, smallest ratio -2.87 (no device needed)."""
    xi, cells, mesh, m32, ref = _cell_case("tri", 50, TRI3)
    assert cells.shape == (91, 3)
    assert ref["inverted"] == [0, 0, 1]
    assert ref["ratio"][0].item() == 1.0
    assert abs(ref["ratio"][1].item() - 0.218) < 5e-4 and abs(ref["ratio"][2].item() + 2.87) < 5e-3


def test_nan_node_stays_in_its_trajectory(dev):
    xi, cells, mesh, m32, ref = _cell_case("tri", 50, TRI3)
    node = 17
    touching = int((cells == node).any(1).sum())
    assert touching > 0
    bad = mesh.clone()
    bad[1, node, 0] = float("nan")
    q = _run(dev, xi, cells, bad, m32)
    # the smooth trajectory inverts nothing by itself: its count is the touching cells
    assert ref["inverted"][1] == 0 and q.inverted[1].item() == touching
    for name in ("mean", "std", "range", "area_ratio_min"):
        assert math.isnan(getattr(q, name)[1].item()), name
    assert int(torch.isnan(q.mg[1]).sum()) == touching
    # the others: bitwise a run without that trajectory
    keep = [0, 2]
    q0 = _run(dev, xi, cells, mesh[keep], m32[keep])
    for name in q._fields:
        assert _eq(getattr(q, name)[keep], getattr(q0, name)), name
    assert q.inverted[keep].tolist() == [ref["inverted"][b] for b in keep]


def test_counter_buffers_and_the_cell_table_object(dev):
    from mmpde_amd import ops

    xi, cells, mesh, m32, ref = _cell_case("quad", 6, QUAD4)
    B = 4
    table = ops.MeshCells(cells, xi.shape[0], dev)
    total = torch.full((B,), 5, dtype=torch.int32, device=dev)
    q = _run(dev, xi, table, mesh, m32, inverted_total=total)
    q = _run(dev, xi, table, mesh, m32, inverted_total=total)
    assert total.tolist() == [5 + 2 * c for c in ref["inverted"]]
    assert q.inverted.tolist() == ref["inverted"]
    # without the per-cell output (the workspace path): the same statistics
    qn = ops.mesh_quality(mesh.reshape(-1, 2).to(dev), xi.to(dev), table, m32.to(dev), B)
    assert qn.mg is None
    for name in ("mean", "std", "range", "inverted", "area_ratio_min"):
        assert _eq(getattr(qn, name), getattr(q, name)), name
    with pytest.raises(ValueError):
        ops.mesh_quality(mesh.reshape(-1, 2).to(dev), xi[:-1].to(dev), table, m32.to(dev), B)
    with pytest.raises(ValueError):
        ops.mesh_quality(mesh.reshape(-1, 2).to(dev), xi.to(dev), cells + 1, m32.to(dev), B)   # an index == N


# ----------------------------------------------------------------------------- the offline tool
def test_statistics_match_dmm_train_evaluate(dev):
    """test_gpu_dmm_train.py::test_evaluate_vs_oracle's shapes and seeds, the DMM
    in eval mode: the field-mean of the new statistics is dmm_train.evaluate's."""
    import test_gpu_dmm_train as D
    from mmpde_amd import dmm_train as T
    from mmpde_amd import ops

    pde, dmm = D._models("burgers")
    dmm.eval()
    all_u = D._data("burgers", pde, 2)
    dmm.to(dev)
    np.random.seed(0)
    want = T.evaluate(dmm, all_u, dev)
    xi = T.unit_lattice(48, dev)
    u = all_u.to(dev)
    mesh = torch.cat([dmm.mesh(u[[t]], xi) for t in range(2)])
    m, _, _ = ops.mesh_monitor(u)
    q = ops.mesh_quality(mesh, xi, ops.mesh_cells_lattice(48), m, 2)
    for name, got, ref in zip(("mean", "std", "range"), (q.mean, q.std, q.range), want):
        _stat(got.double().mean().reshape(1), torch.tensor([ref], dtype=torch.float64), f"evaluate {name}")
    assert q.inverted.tolist() == [0, 0]


def test_statistics_match_dmm_train_evaluate_tri(dev):
    """test_gpu_dmm_train.py::test_evaluate_tri_vs_oracle's shapes and seeds,
    the DMM in eval mode."""
    import test_gpu_dmm_train as D
    from mmpde_amd import dmm_train as T
    from mmpde_amd import ops

    pde, dmm = D._models("cy")
    dmm.eval()
    all_u = D._data("cy", pde, 3)
    u1 = all_u[[1], :, 2]
    grid = all_u[0, :, :2].contiguous()
    dmm.to(dev)
    np.random.seed(0)
    want = T.evaluate_tri(dmm, u1, grid, dev)
    mesh = dmm.mesh(u1.to(dev), grid.to(dev))
    m, _, _ = ops.mesh_monitor(u1.to(dev), grid.to(dev))
    q = ops.mesh_quality(mesh, grid.to(dev), ops.mesh_cells_delaunay(grid), m, 1)
    for name, got, ref in zip(("mean", "std", "range"), (q.mean, q.std, q.range), want):
        _stat(got.double().reshape(1), torch.tensor([ref], dtype=torch.float64), f"evaluate_tri {name}")


# ----------------------------------------------------------------------------- rollout
REPORT_KEYS = ["mean", "std", "range", "rhs", "alpha", "inverted", "area_ratio_min", "inverted_total"]


def _engines(kind, dev, guard):
    import test_gpu_rollout_mesh_check as M
    from mmpde_amd.rollout import MMPDERollout

    pde, model, model_b, itp, dmm, gc, B, u0, sd = M._case(kind, dev)
    off = MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev)
    on = MMPDERollout(kind, model, model_b, itp, dmm, gc, B, dev)
    assert on.mesh_quality is False and on.mesh_quality_report() is None
    on.mesh_quality = True
    off.mesh_guard = on.mesh_guard = guard
    return off, on, u0.to(dev)


def _standalone(eng, u):
    from mmpde_amd import ops

    if eng.kind == "burgers":
        m, alpha, rhs = ops.mesh_monitor(u.reshape(eng.B, eng.s, eng.s))
        cells = ops.mesh_cells_lattice(eng.s)
    else:
        m, alpha, rhs = ops.mesh_monitor(u.reshape(eng.B, eng.N), eng.grid)
        cells = ops.mesh_cells_delaunay(eng.grid)
    q = ops.mesh_quality(eng.mesh, eng.xi, cells, m, eng.B)
    torch.cuda.synchronize()
    return dict(mean=q.mean, std=q.std, range=q.range, rhs=rhs, alpha=alpha, inverted=q.inverted,
                area_ratio_min=q.area_ratio_min)


def _check_report(eng, u, total, what):
    rep = eng.mesh_quality_report()
    assert list(rep) == REPORT_KEYS, what
    alone = _standalone(eng, u)
    for k, t in alone.items():
        assert _eq(getattr(eng.mesh_q, k), t), (what, k)
        assert rep[k] == t.tolist(), (what, k)
    total += alone["inverted"].cpu().long()
    assert rep["inverted_total"] == total.tolist(), what
    assert all(math.isfinite(x) and x > 0 for x in rep["mean"] + rep["std"] + rep["range"] + rep["alpha"]), rep
    return rep


@pytest.mark.parametrize("guard", [None, 0.1])
@pytest.mark.parametrize("kind", ["cy", "burgers"])
def test_rollout_eager_quality_changes_nothing_and_reports(dev, kind, guard):
    off, on, u = _engines(kind, dev, guard)
    total = torch.zeros(on.B, dtype=torch.int64)
    for s in (1, 2, 3):
        want = off.step(u, s).clone()
        got = on.step(u, s).clone()
        torch.cuda.synchronize()
        assert _eq(got, want), (kind, guard, s, "mesh_quality changed the prediction")
        assert _eq(on.mesh, off.mesh), (kind, guard, s)
        assert on.mesh_report() == off.mesh_report(), (kind, guard, s)
        assert (on.mesh_report() is None) == (guard is None)
        rep = _check_report(on, u, total, (kind, guard, s))
        u = got
    print(f"{kind} guard {guard}: {rep}")
    # a default engine holds no quality state
    assert off.mesh_quality is False and off.mesh_q is None and off.mesh_quality_report() is None


@pytest.mark.parametrize("guard", [None, 0.1])
@pytest.mark.parametrize("kind", ["cy", "burgers"])
def test_rollout_graph_step_quality_changes_nothing_and_reports(dev, kind, guard):
    off, on, u = _engines(kind, dev, guard)
    for eng in (off, on):
        # weight images and caches; the kNN table policy's read-back of the first
        # step is consumed by the second (it cannot be queried inside a capture)
        eng.step(u, 1)
        torch.cuda.synchronize()
        eng.step(u, 1)
        eng.enable_graph(u)
    total = torch.tensor(on.mesh_quality_report()["inverted_total"], dtype=torch.int64)
    for s in (1, 2, 3):
        want = off.graph_step(u, s).clone()
        got = on.graph_step(u, s).clone()
        torch.cuda.synchronize()
        assert _eq(got, want), (kind, guard, s, "mesh_quality changed the replayed prediction")
        assert _eq(on.mesh, off.mesh), (kind, guard, s)
        assert on.mesh_report() == off.mesh_report(), (kind, guard, s)
        _check_report(on, u, total, (kind, guard, s))
        u = got


def test_rollout_quality_needs_the_unit_square(dev):
    off, on, u = _engines("burgers", dev, None)
    pde = off.gc.pde
    lx = pde.Lx
    try:
        pde.Lx = 2.0
        with pytest.raises(ValueError):
            off.mesh_quality = True
        assert off.mesh_quality is False
        off.mesh_quality = False          # switching it off never raises
    finally:
        pde.Lx = lx
    off.mesh_quality = True
    assert off.mesh_quality is True
