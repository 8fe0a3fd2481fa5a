"""Host side of the cell-binned radius graph (csrc/knn_bins.hip
mmpde_radius_graph_binned): the bindings know the entry point, and every
refused argument is refused before any launch.  No GPU."""
import ctypes

import pytest
import torch


def test_bindings_hold_the_entry():
    from mmpde_amd import _lib, ops

    h = ctypes.CDLL(_lib.LIB_PATH)
    assert "mmpde_radius_graph_binned" in _lib.EXPORTS and hasattr(h, "mmpde_radius_graph_binned")
    assert "mmpde_radius_graph" in _lib.EXPORTS
    assert isinstance(ops.RADIUS_BINNED_MIN_POINTS, int) and ops.RADIUS_BINNED_MIN_POINTS >= 1
    assert ops.RADIUS_METHODS == ("scan", "binned")


def test_refused_arguments_never_launch():
    """Host memory stands in for the device pointers: a call that got as far as
    a launch would fail differently (no device here); each of these returns
    MMPDE_ERR_INVALID_ARG from the argument checks."""
    from mmpde_amd import _lib

    f = _lib.lib().mmpde_radius_graph_binned
    buf = (ctypes.c_uint64 * 16)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    ok = dict(pos=p, bins=p, batches=1, n_per=100, r=0.1, mnn=32, nbr=p, deg=p)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["pos"], a["bins"], a["batches"], a["n_per"], a["r"], a["mnn"], a["nbr"], a["deg"], None, None)

    for name in ("pos", "bins", "nbr", "deg"):
        assert call(**{name: None}) == -1, name
    assert call(bins=p + 4) == -1                      # not 8-byte aligned
    for n_per in (0, -1, 65537, 1 << 40):
        assert call(n_per=n_per) == -1, n_per
    for mnn in (0, -3, 64, 1000):                      # w = mnn + 1 <= 64: one index per lane
        assert call(mnn=mnn) == -1, mnn
    for r in (0.0, -0.5, float("nan")):
        assert call(r=r) == -1, r
    for b in (0, -1, 65536):
        assert call(batches=b) == -1, b


def test_wrapper_refuses_an_unknown_method():
    from mmpde_amd import ops

    with pytest.raises(ValueError, match="cells"):
        ops.radius_graph_nbr(torch.zeros(10, 2), 1, 0.1, method="cells")


def test_graph_creator_and_engine_settings():
    from mmpde_amd.synth import build_models

    _, _, _, _, _, gc = build_models("burgers", moving_mesh=False)
    assert gc.radius_method == "scan" and gc.knn_method == "full"
