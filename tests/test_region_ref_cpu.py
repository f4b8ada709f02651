"""tests/_region_ref.py, the numpy statement of the ``ace_diag_region_segments`` contract that tests/test_gpu_region_kernels.py holds
the kernel to, against tests/_timeseg_ref.py (which tests/test_timeseg_ref_cpu.py holds to the reference): on touching segments it is
``time_segments`` applied to the cut-out field, bit for bit, and with the whole plane as the region it is the statement on the full
field.  Then what only the bounds table can say: gaps, overlaps, empty and out-of-range segments, and the sign of a lone -0.0."""
import numpy as np
import pytest

import _region_ref as RR
import _timeseg_ref as R

B, T, H, W = 2, 11, 6, 20


def fields(seed=0, n=2):
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, T, H, W)).astype(np.float32)
    y = (1e5 + 900 * g.standard_normal((B, T, H, W))).astype(np.float32)
    x[0, 3, 2, 7], y[1, 5, 3, 9], y[1, 6, 3, 9] = np.nan, np.inf, -np.inf
    return [x, y][:n]


def edge_table(seed, nseg):
    g = np.random.default_rng(seed)
    e = np.sort(g.integers(0, T + 1, (B, nseg + 1)), axis=1)
    e[0, 0], e[0, -1] = -3, T + 4                       # clamped ends
    return e


@pytest.mark.parametrize("region", [(1, 3, 4, 8), (0, 1, 0, 1), (5, 1, 19, 1), (2, 4, 5, 7), (0, H, 0, W)])
def test_touching_segments_equal_time_segments_on_the_cut_out_field(region):
    lat0, nlat_r, lon0, nlon_r = region
    planes = fields()
    edges = edge_table(1, 4)
    edges[1, 2] = edges[1, 1]                           # an empty segment
    shape = (3, B, 4, nlat_r, nlon_r)
    sums, means = np.full(shape, -1.0), np.full(shape, -1.0, np.float32)
    RR.region_segments(planes, [2, 0], 3, RR.bounds_of_edges(edges), region, sums=sums, means=means)
    cut = [np.ascontiguousarray(x[..., lat0:lat0 + nlat_r, lon0:lon0 + nlon_r]).reshape(B, T, -1) for x in planes]
    flat = (3, B, 4, nlat_r * nlon_r)
    rs, rm = np.full(flat, -1.0), np.full(flat, -1.0, np.float32)
    R.time_segments(cut, [2, 0], 3, edges, sums=rs, means=rm)
    assert np.array_equal(sums.reshape(flat).view(np.int64), rs.view(np.int64))
    assert np.array_equal(means.reshape(flat).view(np.int32), rm.view(np.int32))
    assert np.all(sums[1] == -1.0) and np.all(means[1] == -1.0)          # row 1: no plane names it


def test_the_whole_plane_is_the_statement_on_the_full_field():
    planes = fields(2)
    edges = edge_table(3, 3)
    shape = (2, B, 3, H, W)
    sums, means = np.zeros(shape), np.zeros(shape, np.float32)
    RR.region_segments(planes, [0, 1], 2, RR.bounds_of_edges(edges), (0, H, 0, W), sums=sums, means=means)
    rs, rm = np.zeros((2, B, 3, H * W)), np.zeros((2, B, 3, H * W), np.float32)
    R.time_segments([x.reshape(B, T, -1) for x in planes], [0, 1], 2, edges, sums=rs, means=rm)
    assert np.array_equal(sums.reshape(rs.shape), rs, equal_nan=True) and np.array_equal(means.reshape(rm.shape), rm, equal_nan=True)


def test_gaps_overlaps_empty_and_clamped_segments():
    (x,) = fields(4, n=1)
    x = np.nan_to_num(x, nan=1.0)
    region = (1, 2, 3, 5)
    bounds = np.array([[[0, 1], [4, 4], [3, 9], [5, 7], [-4, 2], [9, 40], [8, 2]]] * B)
    bounds[1, 0] = [10, 11]
    sums, means = np.zeros((1, B, 7, 2, 5)), np.zeros((1, B, 7, 2, 5), np.float32)
    RR.region_segments([x], [0], 1, bounds, region, sums=sums, means=means)
    box = x[:, :, 1:3, 3:8].astype(np.float64)
    assert np.array_equal(means[0, 0, 0], x[0, 0, 1:3, 3:8]) and np.array_equal(means[0, 1, 0], x[1, 10, 1:3, 3:8])       # one step
    for s in (1, 6):                                                                                                  # hi <= lo
        assert np.all(sums[0, :, s] == 0) and np.all(np.isnan(means[0, :, s]))
    for s, (lo, hi) in ((2, (3, 9)), (3, (5, 7)), (4, (0, 2)), (5, (9, T))):
        want = np.zeros((B, 2, 5))
        for t in range(lo, hi):
            want = want + box[:, t]
        assert np.array_equal(sums[0, :, s], want), s
        assert np.array_equal(means[0, :, s], (want / (hi - lo)).astype(np.float32)), s


def test_nothing_outside_the_region_or_the_segments_is_read():
    (x,) = fields(5, n=1)
    x = np.nan_to_num(x, nan=1.0)
    region, bounds = (2, 3, 5, 7), np.array([[[1, 3], [6, 7]]] * B)
    keep = np.zeros(x.shape, bool)
    keep[:, 1:3, 2:5, 5:12] = keep[:, 6:7, 2:5, 5:12] = True
    poisoned = np.where(keep, x, np.nan).astype(np.float32)
    sums = np.zeros((1, B, 2, 3, 7))
    RR.region_segments([poisoned], [0], 1, bounds, region, sums=sums)
    assert not np.isnan(sums).any()


def test_a_lone_negative_zero_comes_back_positive():
    x = np.full((1, 2, 2, 2), -0.0, np.float32)
    sums, means = np.ones((1, 1, 1, 2, 2)), np.ones((1, 1, 1, 2, 2), np.float32)
    RR.region_segments([x], [0], 1, [[[1, 2]]], (0, 2, 0, 2), sums=sums, means=means)
    assert not np.signbit(sums).any() and not np.signbit(means).any() and np.all(sums == 0) and np.all(means == 0)
