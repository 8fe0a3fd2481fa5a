"""Host side of the cell-binned kNN (csrc/knn_bins.hip mmpde_knn_bin*): the sizing
helpers are pure host arithmetic and the bindings know the new entry points.
No GPU."""
import ctypes


def test_bins_bytes_is_host_arithmetic():
    from mmpde_amd import _lib

    lib = _lib.lib()
    sizes = (1, 2, 35, 36, 37, 100, 700, 2304, 2521, 4096, 4097, 9216, 16384, 16385, 36864, 65535, 65536)
    prev_row = None
    for b in (1, 2, 3, 32, 65535):
        row = [lib.mmpde_knn_bins_bytes(b, n) for n in sizes]
        assert all(v > 0 for v in row)
        assert all(a <= c for a, c in zip(row, row[1:])), (b, row)        # non-decreasing in n_per
        if prev_row is not None:
            assert all(a <= c for a, c in zip(prev_row, row)), b          # and in batches
        prev_row = row
        # room for the sorted points (8 B), their indices (4 B) and the cell tables
        for n, v in zip(sizes, row):
            g = lib.mmpde_knn_bins_grid(n)
            assert v >= b * (12 * n + 4 * (2 * g * g + 1))
            assert v % 8 == 0
    for b, n in ((0, 100), (-1, 100), (1, 0), (1, -5), (0, 0)):
        assert lib.mmpde_knn_bins_bytes(b, n) <= 0


def test_bins_grid_follows_the_point_count():
    from mmpde_amd import _lib

    lib = _lib.lib()
    assert lib.mmpde_knn_bins_grid(1) == 1 and lib.mmpde_knn_bins_grid(36) == 3
    assert lib.mmpde_knn_bins_grid(49 * 49) == 24        # 48 intervals: points on cell boundaries
    assert lib.mmpde_knn_bins_grid(65536) == 128
    prev = 0
    for n in range(1, 70000, 37):
        g = lib.mmpde_knn_bins_grid(n)
        if n <= 65536:
            assert g >= max(prev, 1) and 4 * g * g <= max(n, 4)
            prev = g
        else:
            assert g == 0
    assert lib.mmpde_knn_bins_grid(0) == 0 and lib.mmpde_knn_bins_grid(-3) == 0


def test_bindings_hold_the_binned_entries():
    from mmpde_amd import _lib, ops

    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mmpde_knn_bins_grid", "mmpde_knn_bins_bytes", "mmpde_knn_bin", "mmpde_knn_graph_binned",
                 "mmpde_knn_query_binned"):
        assert name in _lib.EXPORTS and hasattr(h, name), name
    lib = _lib.lib()
    # null pointers are refused before any launch
    assert lib.mmpde_knn_bin(None, 1, 100, None, 0, None) == -1
    assert lib.mmpde_knn_graph_binned(None, None, 1, 100, 35, None, None, None, None) == -1
    assert lib.mmpde_knn_query_binned(None, None, None, 1, 100, 100, 30, None, None, None, None) == -1
    assert ops.KNN_BINNED_MIN_POINTS > 4096
    assert ops.knn_bins_grid(2401) == 24
