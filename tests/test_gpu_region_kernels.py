"""csrc/region.hip through the C ABI (ace_diag_region_segments) against tests/_region_ref.py, the numpy statement of the header
contract that tests/test_region_ref_cpu.py holds to tests/_timeseg_ref.py.

Bar: equality.  The kernel adds in fp64 in step order without reassociation and divides in IEEE fp64, as the statement does, so
``np.array_equal(..., equal_nan=True)`` on sums and means alike.  Both outputs lie between guards, which must come back intact, and
are pre-filled with a sentinel, so a slot that should have been written and was not shows, as does one that should have been left
alone and was not; the input planes must come back unchanged.  Every source value outside the region, or at a step no segment
covers, is NaN on the device, so a stray read shows in the result.

Shapes: the smallest that reach each branch - B = 2, 3 planes of 6 x 20 unless said otherwise; the vector path needs nlon_r, lon0,
nlon, the base and both strides all multiples of 4 floats, so each of those is broken in turn; 33 x 37 in 40 x 72 is more than one
1024-pixel chunk with a ragged tail."""
import numpy as np
import pytest
import torch

import _region_ref as RR
from test_gpu_diag_kernels import INVALID, Guarded, dev, lib  # noqa: F401
from test_gpu_timeseg_kernels import Guarded32, lay
from test_gpu_timeseg_kernels import call as timeseg_call

pytestmark = pytest.mark.gpu

SENT = -12345.0                                      # pre-fill of the outputs
B, T, H, W = 2, 19, 6, 20
# lengths 0, 1, 8, 11 and 19 with gaps, an overlap, and bounds below 0 and above T
BOUNDS = np.array([[[4, 4], [0, 1], [2, 10], [8, 19], [-3, 40], [17, 12]],
                   [[18, 19], [9, 9], [11, 19], [-2000000000, 11], [0, 2000000000], [3, 4]]])
SPARSE = np.array([[[1, 2], [5, 9], [7, 8]], [[12, 30], [0, 0], [3, 5]]])          # steps 0, 2 .. 4, 9 .. 18 / 2, 5 .. 11 never read


def place_any(data, layout, g):
    """``lay`` of tests/test_gpu_timeseg_kernels.py, and "sampleoffset": an aligned base and step stride with a sample stride that
    is no multiple of 4 floats"""
    if layout != "sampleoffset":
        return lay(data, layout, g)
    Bn, Tn, hw = data.shape
    sb = Tn * hw + 2
    s = torch.randn(Bn * sb, generator=g) * 1e30
    s.view(Bn, sb)[:, :Tn * hw] = data.reshape(Bn, -1)
    return s, 0, sb, hw


def poison(x, bounds, region):
    """``x`` (B, T, H, W) with NaN wherever the contract says nothing is read"""
    lat0, nlat_r, lon0, nlon_r = region
    keep = torch.zeros(x.shape, dtype=torch.bool)
    e = np.clip(np.asarray(bounds, np.int64), 0, x.shape[1])
    for b in range(x.shape[0]):
        for lo, hi in e[b]:
            keep[b, lo:hi, lat0:lat0 + nlat_r, lon0:lon0 + nlon_r] = True
    return torch.where(keep, x, torch.full((), float("nan")))


def call(dev, planes, rows, nrows, bounds, region, layout="contiguous", want=("sums", "means"), expect=0, seed=0, null=(),
         alloc=None, override=None):
    """one ace_diag_region_segments on (B, T, H, W) CPU fields, poisoned as above; ``null``: planes passed as NULL; ``override``:
    integer arguments replaced in the call; ``alloc``: the region the outputs are sized for when ``region`` is not a valid one.
    Returns (sums, means) as numpy and the statement's."""
    L = lib()
    g = torch.Generator().manual_seed(seed)
    Bn, Tn, Hn, Wn = planes[0].shape
    bounds = np.ascontiguousarray(np.asarray(bounds), dtype=np.int32)
    lat0, nlat_r, lon0, nlon_r = region
    size = alloc or region
    planes = [poison(x, bounds, size) for x in planes]
    placed = [place_any(x.reshape(Bn, Tn, Hn * Wn), layout, g) for x in planes]
    store = [p[0].to(dev) for p in placed]
    tab = [0 if j in null else s.data_ptr() + 4 * p[1] for j, (p, s) in enumerate(zip(placed, store))]
    for p in placed:
        tab += [p[2], p[3]]
    tab = torch.tensor(tab, dtype=torch.int64, device=dev)
    rows_d = torch.tensor(rows, dtype=torch.int32, device=dev)
    bounds_d = torch.from_numpy(bounds).to(dev)
    nseg = bounds.shape[1]
    shape = (nrows, Bn, max(nseg, 1), size[1], size[3])
    sums = Guarded(torch.full(shape, SENT, dtype=torch.float64), dev)
    means = Guarded32(torch.full(shape, SENT, dtype=torch.float32), dev)
    a = dict(nrows=nrows, nseg=nseg, nplanes=len(planes), batch=Bn, steps=Tn, nlat=Hn, nlon=Wn, lat0=lat0, nlat_r=nlat_r, lon0=lon0,
             nlon_r=nlon_r)
    a.update(override or {})
    base = tab.data_ptr()
    rc = L.ace_diag_region_segments(base, base + 8 * len(planes), rows_d.data_ptr(), bounds_d.data_ptr(),
                                    sums.ptr if "sums" in want else None, means.ptr if "means" in want else None, *a.values(), None)
    assert rc == expect, L.ace_diag_last_error().decode()
    torch.cuda.synchronize()
    got = (sums.read().numpy(), means.read().numpy())
    for p, s in zip(placed, store):
        assert torch.equal(s.cpu().view(torch.int32), p[0].view(torch.int32)), "an input plane changed"
    ref = (np.full(shape, SENT), np.full(shape, SENT, np.float32))
    if rc == 0 and a["nplanes"] and a["nseg"]:
        RR.region_segments([None if j in null else x.numpy() for j, x in enumerate(planes)], rows, nrows, bounds, region,
                           sums=ref[0] if "sums" in want else None, means=ref[1] if "means" in want else None)
    return got, ref


def same(got, ref, what=""):
    assert np.array_equal(got[0], ref[0], equal_nan=True), (what, "sums")
    assert np.array_equal(got[1], ref[1], equal_nan=True), (what, "means")


def fields(g, shape=(B, T, H, W)):
    """a unit Gaussian, a surface-pressure-like field and a small-valued one"""
    return [torch.randn(*shape, generator=g), (1e5 + 900 * torch.randn(*shape, generator=g)).float(),
            1e-4 * torch.randn(*shape, generator=g)]


REGIONS = {"aligned": (1, 3, 4, 8), "lon0_5": (1, 3, 5, 8), "nlon_r_7": (2, 4, 4, 7), "corner": (5, 1, 19, 1), "origin": (0, 1, 0, 1),
           "one_row": (3, 1, 0, 20), "one_column": (0, 6, 7, 1)}


@pytest.mark.parametrize("region", list(REGIONS))
@pytest.mark.parametrize("layout", ["contiguous", "odd", "timeoffset", "sampleoffset"])
def test_regions_and_layouts(dev, region, layout):
    g = torch.Generator().manual_seed(len(region))
    got, ref = call(dev, fields(g), [2, 0, 1], 3, BOUNDS, REGIONS[region], layout=layout)
    same(got, ref, (region, layout))
    assert not np.any(got[0] == SENT) and not np.any(got[1] == SENT)
    assert np.all(got[0][:, 0, 0] == 0) and np.all(np.isnan(got[1][:, 0, 0]))          # [4, 4): empty, sums 0 and means NaN
    assert np.all(got[0][:, 0, 5] == 0) and np.all(np.isnan(got[1][:, 0, 5]))          # [17, 12): empty too


def test_a_plane_width_that_is_no_multiple_of_four(dev):
    g = torch.Generator().manual_seed(1)
    same(*call(dev, fields(g, (B, T, 6, 22)), [0, 1, 2], 3, SPARSE, (1, 4, 4, 8)))


@pytest.mark.parametrize("layout", ["contiguous", "odd"])
def test_steps_between_segments_are_not_read(dev, layout):
    g = torch.Generator().manual_seed(2)
    got, ref = call(dev, fields(g), [0, 1, 2], 3, SPARSE, REGIONS["aligned"], layout=layout)
    same(got, ref)
    assert not np.isnan(got[0][:, :, [0, 2]]).any() and not np.isnan(got[0][:, 0, 1]).any()


@pytest.mark.parametrize("layout", ["contiguous", "odd"])
@pytest.mark.parametrize("shape, region", [((6, 20), (0, 6, 0, 20)), ((7, 9), (0, 7, 0, 9))])
def test_the_whole_plane_equals_time_segments(dev, layout, shape, region):
    g = torch.Generator().manual_seed(3)
    planes = fields(g, (B, T) + shape)
    edges = np.array([[0, 3, 3, 11, 19], [-2, 1, 9, 17, 25]])
    got, ref = call(dev, planes, [1, 2, 0], 3, RR.bounds_of_edges(edges), region, layout=layout)
    same(got, ref)
    (ts, tm), _ = timeseg_call(dev, [x.reshape(B, T, -1) for x in planes], [1, 2, 0], 3, edges, layout=layout)
    assert np.array_equal(got[0].reshape(ts.shape).view(np.int64), ts.view(np.int64))
    assert np.array_equal(got[1].reshape(tm.shape).view(np.int32), tm.view(np.int32))


@pytest.mark.parametrize("layout", ["contiguous", "odd"])
@pytest.mark.parametrize("region", [(3, 33, 20, 37), (4, 33, 8, 40)])
def test_more_than_one_chunk_with_a_ragged_tail(dev, layout, region):
    g = torch.Generator().manual_seed(4)
    got, ref = call(dev, fields(g, (2, 9, 40, 72))[:2], [1, 0], 2, [[[0, 9], [2, 3]], [[1, 4], [5, 9]]], region, layout=layout)
    same(got, ref, region)
    assert not np.any(got[0] == SENT)


def test_nan_and_infinities_inside_the_region_propagate(dev):
    g = torch.Generator().manual_seed(5)
    x, y, _ = fields(g)
    x[:, :, 2, 5:7] = float("nan")                      # a masked patch, every step
    x[0, 3, 1, 4] = float("nan")
    y[0, 2, 3, 8], y[0, 6, 3, 9], y[1, 12, 2, 10], y[1, 13, 2, 10] = float("inf"), float("-inf"), float("inf"), float("-inf")
    got, ref = call(dev, [x, y], [0, 1], 2, BOUNDS, REGIONS["aligned"])
    same(got, ref)
    assert np.all(np.isnan(got[0][0, 0, 1:5, 1, 1:3])) and np.isnan(got[0][0, 0, 2, 0, 0]) and not np.isnan(got[0][0, 0, 1, 0, 0])
    assert got[0][1, 0, 2, 2, 4] == np.inf and got[1][1, 0, 2, 2, 5] == -np.inf and np.isnan(got[0][1, 1, 2, 1, 6])


def test_a_lone_negative_zero_comes_back_positive(dev):
    x = torch.full((1, 2, 6, 20), -0.0)
    got, ref = call(dev, [x], [0], 1, [[[1, 2]]], REGIONS["aligned"])
    same(got, ref)
    assert np.all(got[0] == 0) and not np.signbit(got[0]).any() and not np.signbit(got[1]).any()


@pytest.mark.parametrize("want", [("sums",), ("means",)])
@pytest.mark.parametrize("region", ["aligned", "nlon_r_7"])
def test_either_output_alone(dev, want, region):
    g = torch.Generator().manual_seed(6)
    got, ref = call(dev, fields(g), [0, 1, 2], 3, BOUNDS, REGIONS[region], want=want)
    same(got, ref)
    assert np.all(got[1 if want == ("sums",) else 0] == SENT)


def test_an_out_of_range_row_and_a_null_plane_write_nothing(dev):
    g = torch.Generator().manual_seed(7)
    x = fields(g) + fields(g)[:1]
    got, ref = call(dev, x, [3, -1, 0, 4], 4, BOUNDS, REGIONS["lon0_5"], null=(2,))
    same(got, ref)
    for r in (0, 1, 2):                                 # row 0: its plane is NULL; rows 1 and 2: no plane names them
        assert np.all(got[0][r] == SENT) and np.all(got[1][r] == SENT)
    assert not np.any(got[0][3] == SENT)


def test_refused_calls_write_nothing(dev):
    g = torch.Generator().manual_seed(8)
    x = fields(g)
    ok = REGIONS["aligned"]
    refused = [dict(region=(-1, 3, 4, 8)), dict(region=(1, 0, 4, 8)), dict(region=(4, 3, 4, 8)), dict(region=(1, 3, -4, 8)),
               dict(region=(1, 3, 4, 0)), dict(region=(1, 3, 16, 8)), dict(region=(2147483647, 3, 4, 8)),
               dict(region=(1, 3, 4, 2147483647)), dict(want=()), dict(nplanes=-1), dict(nplanes=65536), dict(nseg=-1),
               dict(batch=0), dict(batch=65536), dict(steps=0), dict(nrows=0), dict(nlat=0), dict(nlon=0)]
    for kw in refused:
        kw = dict(kw)
        region, want = kw.pop("region", ok), kw.pop("want", ("sums", "means"))
        got, _ = call(dev, x, [0, 1, 2], 3, BOUNDS, region, expect=INVALID, alloc=ok, want=want, override=kw)
        assert np.all(got[0] == SENT) and np.all(got[1] == SENT), kw
        assert "ace_diag_region_segments" in lib().ace_diag_last_error().decode()
    for kw in (dict(nplanes=0), dict(nseg=0)):          # no-ops
        got, _ = call(dev, x, [0, 1, 2], 3, BOUNDS, ok, override=kw)
        assert np.all(got[0] == SENT) and np.all(got[1] == SENT)


def test_two_identical_calls_are_bitwise_equal(dev):
    runs = []
    for _ in range(2):
        g = torch.Generator().manual_seed(9)
        runs.append(call(dev, fields(g, (2, 9, 40, 72))[:2], [1, 0], 2, [[[0, 9], [2, 3]], [[1, 4], [5, 9]]], (3, 33, 20, 37),
                         layout="odd")[0])
    assert np.array_equal(runs[0][0].view(np.int64), runs[1][0].view(np.int64))
    assert np.array_equal(runs[0][1].view(np.int32), runs[1][1].view(np.int32))
