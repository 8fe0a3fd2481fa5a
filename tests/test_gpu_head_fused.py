"""The Conv1d output head fused into the last layer's node kernel
(mmpde_gnn_forward_ex) against the separate head launch (mmpde_gnn_head) on
the last layer's node features the forward hands out through
mmpde_gnn_exec.h_last: bit for bit, at one row, around the kernel's 32-row
tile, over many tiles, time_window 1 and 3, both GEMM arithmetics and a ragged
neighbour table.  Storing h_last must not change the forward's output."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

K = 5


@functools.lru_cache(maxsize=None)
def _solver(tw):
    from mmpde_amd.gnn_2d import MP_PDE_Solver_2D
    from mmpde_amd.pdes import cy
    from mmpde_amd.synth import _randomise_bn, cy_synth_mesh

    torch.manual_seed(40 + tw)
    grid = cy_synth_mesh()
    pde = cy(ori_grid=grid)
    pde.grid_size = [30, grid.shape[0]]
    model = MP_PDE_Solver_2D(pde=pde, time_window=tw, eq_variables={})
    _randomise_bn(model, torch.Generator().manual_seed(41 + tw))
    return model.eval()


def _graph(n, tw, ragged, dev):
    from mmpde_amd.graph import Data

    g = torch.Generator().manual_seed(1000 * n + 10 * tw + ragged)
    data = Data(x=torch.randn(n, tw, generator=g).to(dev))
    data.pos = torch.cat((torch.full((n, 1), 1.3), torch.rand(n, 2, generator=g)), 1).to(dev)
    data.nbr = torch.randint(0, n, (n, K), generator=g, dtype=torch.int32).to(dev)
    if ragged:
        deg = torch.randint(0, K + 1, (n,), generator=g, dtype=torch.int32)
        deg[0], deg[n - 1] = 0, K
        data.deg = deg.to(dev)
    return data


def _forward(model, data, h_last):
    """One eval forward through mmpde_gnn_forward_ex, exec.h_last = h_last (None: NULL)."""
    from mmpde_amd import _lib as L

    trace = L.GnnExec(None, None, 0, None)
    trace.h_last = L.ptr(h_last) if h_last is not None else None
    return model(data, trace=trace)


def _separate_head(model, h):
    from mmpde_amd import _lib as L

    _, _, _, head = model.device_params()
    out = torch.empty((h.shape[0], model.time_window), dtype=torch.float32, device=h.device)
    L.check(L.lib().mmpde_gnn_head(L.ptr(h), h.shape[0], ctypes.addressof(head), L.ptr(out),
                                   L.stream(h.device)), "mmpde_gnn_head")
    return out


CASES = [(n, tw, mode, False) for n in (1, 31, 32, 33, 2521) for tw in (1, 3) for mode in ("f32", "f16x3")]
CASES += [(33, 3, "f16x3", True), (2521, 1, "f32", True)]


@pytest.mark.parametrize("n,tw,mode,ragged", CASES)
def test_fused_head_equals_separate_head(dev, n, tw, mode, ragged):
    model = _solver(tw).to(dev)
    model.edge_gemm = mode
    data = _graph(n, tw, ragged, dev)
    # NaN-filled: every row the kernel does not store fails the finite check
    h_last = torch.full((n, 128), float("nan"), dtype=torch.float32, device=dev)
    out = _forward(model, data, h_last)
    assert out.shape == (n, tw)
    assert torch.isfinite(h_last).all()
    assert torch.isfinite(out).all()
    assert torch.equal(out, _separate_head(model, h_last))
    # the store is an output only: the same forward without it gives the same bits
    assert torch.equal(out, _forward(model, data, None))
