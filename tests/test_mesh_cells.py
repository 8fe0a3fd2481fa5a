"""The cell tables of the mesh-quality stage, on the host: the lattice
quadrilaterals against the reference's slicing (dmm_utils.py:1264-1267)
restated in torch, the Delaunay triangles against scipy's (the same simplex
set, positively oriented on the fixed grid, indices in range), and the lattice
coordinates the cell kernel computes, float(i) / float(n - 1), against
dmm_train.unit_lattice bit for bit."""
import numpy as np
import pytest
import torch


@pytest.mark.parametrize("s", [2, 3, 9])
def test_lattice_cells_are_the_reference_slicing(s):
    from mmpde_amd import ops

    cells = ops.mesh_cells_lattice(s)
    assert cells.dtype == torch.int32 and cells.shape == ((s - 1) ** 2, 4)
    # the reference slices x.reshape(s, s); do the same to the flat node index
    x = torch.arange(s * s).reshape(s, s)
    bl, br, tl, tr = x[:(s - 1), :(s - 1)], x[1:s, :(s - 1)], x[:(s - 1), 1:s], x[1:s, 1:s]
    want = torch.stack([t.reshape(-1) for t in (bl, br, tl, tr)], dim=1)
    assert torch.equal(cells.long(), want)
    # on the 'xy' lattice: bl -> br steps in y, bl -> tl in x; the four are one cell
    from mmpde_amd.dmm_train import unit_lattice
    g = unit_lattice(s, "cpu").double()
    v = g[cells.long()]                                   # [C, 4, 2]
    h = 1.0 / (s - 1)
    for k, step in ((1, [0.0, h]), (2, [h, 0.0]), (3, [h, h])):
        want_step = torch.tensor(step, dtype=torch.float64).expand(len(v), 2)
        assert torch.allclose(v[:, k] - v[:, 0], want_step, atol=1e-6), k


def _grids():
    from mmpde_amd.synth import cy_synth_mesh

    return {"rand50": (torch.rand(50, 2, generator=torch.Generator().manual_seed(0)), 91),
            "cy": (cy_synth_mesh(), 5022)}


@pytest.mark.parametrize("name", ["rand50", "cy"])
def test_delaunay_cells(name):
    from scipy.spatial import Delaunay

    from mmpde_amd import ops

    grid, n_tri = _grids()[name]
    cells = ops.mesh_cells_delaunay(grid)
    assert cells.dtype == torch.int32 and cells.dim() == 2 and cells.shape[1] == 3
    ref = Delaunay(grid.numpy().astype(np.float64)).simplices
    assert cells.shape[0] == ref.shape[0] == n_tri
    # the same simplex set
    got = {tuple(sorted(t)) for t in cells.tolist()}
    assert got == {tuple(sorted(int(i) for i in t)) for t in ref} and len(got) == n_tri
    # indices in range, three distinct vertices
    assert int(cells.min()) >= 0 and int(cells.max()) < grid.shape[0]
    assert all(len(set(t)) == 3 for t in cells.tolist())
    # positively oriented on the fixed grid, in the cell kernel's own formula and in fp32
    for dt in (torch.float64, torch.float32):
        v = grid.to(dt)[cells.long()]
        e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        assert bool((e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1] > 0).all()), dt
    # the device table pads a triangle with its last vertex
    t = ops.MeshCells(cells, grid.shape[0], "cpu")
    assert t.arity == 3 and torch.equal(t.table[:, :3], cells) and torch.equal(t.table[:, 3], cells[:, 2])


def test_kernel_lattice_coordinates_are_unit_lattice_bits():
    """csrc/mesh_quality.hip computes the lattice coordinate of index i as the
    fp32 quotient float(i) / float(n - 1); unit_lattice rounds numpy's float64
    linspace to fp32.  The same bits for every n the entry accepts."""
    from mmpde_amd.dmm_train import unit_lattice

    for n in range(2, 257):
        i = np.arange(n, dtype=np.float32)
        q = i / np.float32(n - 1)
        assert q.dtype == np.float32
        g = unit_lattice(n, "cpu").reshape(n, n, 2).numpy()
        assert np.array_equal(g[0, :, 0].view(np.int32), q.view(np.int32)), n    # x_j along a row
        assert np.array_equal(g[:, 0, 1].view(np.int32), q.view(np.int32)), n    # y_i down a column
        assert np.all(g[:, :, 0] == g[:1, :, 0]) and np.all(g[:, :, 1] == g[:, :1, 1])
