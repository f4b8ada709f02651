"""tests/_timeseg_ref.py, the numpy statement of the ``ace_diag_time_segments`` contract that tests/test_gpu_timeseg_kernels.py holds
the kernel to, against tests/golden/gen_data_writer.pt, which the reference's own ``_coarsen_tensor_dict`` and ``add_data`` produced on
the records of tests/_data_writer_cases.py.

Bars, with u = 2^-24 and m = max |x| over the steps that enter one output pixel (the reference means in fp32, the statement in fp64
with one rounding; the generator asserted the reference's own share, see its docstring):
  block means     |statement - reference| <= (f + 2) u m
  monthly means   |statement - reference| <= (N + 3 k + 1) u m for a month of N steps delivered in k windows, and
                  |statement - exact| <= u |mean|
The fields are built so that fp64 sums of them are exact: the statement's sums must EQUAL the exact ones."""
import os

import numpy as np
import pytest
import torch

import _data_writer_cases as C
import _timeseg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_data_writer.pt")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def planes_of(data):
    return [data[n].numpy().reshape(C.B, -1, C.H * C.W) for n in C.NAMES]


def within(got, ref, bar, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaN pattern")
    err = np.nan_to_num(np.abs(got - ref))
    assert np.all(err <= bar), (what, float(np.max(err / np.maximum(bar, 1e-300))))


def test_records_are_the_generators(golden):
    assert C.checksum(C.coarsen()["data"]) == golden["coarsen"]["checksum"]
    for key in C.MONTHLY:
        assert C.checksum(C.monthly(key)["data"]) == golden["monthly"][key]["checksum"]


@pytest.mark.parametrize("f", C.FACTORS)
def test_block_means_against_the_reference(golden, f):
    data = C.coarsen()["data"]
    nseg = 10 // f
    means = np.full((3, C.B, nseg, C.H * C.W), -7.0, np.float32)
    sums = np.full((3, C.B, nseg, C.H * C.W), -7.0)
    R.time_segments(planes_of(data), [0, 1, 2], 3, R.block_edges(C.B, 10, f), sums=sums, means=means)
    for i, n in enumerate(C.NAMES):
        m = np.abs(np.nan_to_num(data[n].double().numpy())).reshape(C.B, nseg, f, -1).max(axis=2)
        within(means[i], golden["coarsen"]["ref"][f][n].reshape(C.B, nseg, -1), (f + 2) * U * m, (f, n, "reference"))
        exact = golden["coarsen"]["exact"][f][n].numpy().reshape(C.B, nseg, -1)
        within(means[i], exact, U * np.abs(np.nan_to_num(exact)), (f, n, "exact"))
        # exact sums whatever the order: numpy's own sum serves
        assert np.array_equal(sums[i], data[n].double().numpy().reshape(C.B, nseg, f, -1).sum(axis=2), equal_nan=True)


@pytest.mark.parametrize("key", list(C.MONTHLY))
@pytest.mark.parametrize("cut", C.CUTS)
def test_monthly_means_against_the_reference(golden, key, cut):
    c, g = C.monthly(key), golden["monthly"][key]
    year, month = c["time"].year_month()
    months = 12 * (year - year[:, :1]) + (month - month[:, :1])
    n_months = g["counts"].shape[1]
    totals = np.zeros((3, C.B, n_months, C.H * C.W))
    counts = np.zeros((C.B, n_months), np.int64)
    for a, b in C.windows(c["n"], cut):
        lo, edges = R.month_edges(months[:, a:b])
        nseg = edges.shape[1] - 1
        sums = np.zeros((3, C.B, nseg, C.H * C.W))
        R.time_segments([p[:, a:b] for p in planes_of(c["data"])], [0, 1, 2], 3, edges, sums=sums)
        totals[:, :, lo:lo + nseg] += sums
        counts[:, lo:lo + nseg] += np.diff(edges, axis=1)
    assert np.array_equal(counts, g["counts"].numpy()) and np.array_equal(counts, g["ref"][cut]["counts"].numpy())
    for i, n in enumerate(C.NAMES):
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(counts[:, :, None] > 0, totals[i] / counts[:, :, None], 0.0).astype(np.float32)
        exact = g["exact"][n].numpy().reshape(C.B, n_months, -1)
        x = c["data"][n].double().numpy().reshape(C.B, c["n"], -1)
        for b in range(C.B):
            for k in range(n_months):                       # exact sums whatever the order: numpy's own sum serves
                assert np.array_equal(totals[i, b, k], x[b, months[b] == k].sum(axis=0), equal_nan=True), (n, b, k)
        within(mean, exact, U * np.abs(np.nan_to_num(exact)), (n, "exact"))
        bar = (counts + 3 * g["windows"][cut].numpy() + 1)[:, :, None] * U * g["absmax"][n].numpy().reshape(C.B, n_months, -1)
        within(mean, g["ref"][cut][n].numpy().reshape(C.B, n_months, -1), bar, (n, "reference"))


def test_edges_are_clamped_and_a_falling_edge_is_an_empty_segment():
    x = np.arange(2 * 6 * 3, dtype=np.float32).reshape(2, 6, 3)
    edges = np.array([[-4, 2, 1, 9], [6, 6, 0, 3]])
    sums, means = np.full((2, 2, 3, 3), -7.0), np.full((2, 2, 3, 3), -7.0, np.float32)
    R.time_segments([x, x], [1, 5], 2, edges, sums=sums, means=means)
    assert np.all(sums[0] == -7.0) and np.all(means[0] == -7.0)                  # row 5 is out of range: plane 1 writes nothing
    assert np.array_equal(sums[1, 0, 0], x[0, 0] + x[0, 1]) and np.array_equal(means[1, 0, 0], (x[0, 0] + x[0, 1]) / 2)
    assert np.all(sums[1, 0, 1] == 0) and np.all(np.isnan(means[1, 0, 1]))       # 2 -> 1: empty
    assert np.array_equal(sums[1, 0, 2], x[0, 1:6].sum(axis=0))                  # 1 -> 9, clamped to 6
    assert np.all(sums[1, 1, :2] == 0) and np.all(np.isnan(means[1, 1, :2]))
    assert np.array_equal(sums[1, 1, 2], x[1, 0:3].sum(axis=0))
