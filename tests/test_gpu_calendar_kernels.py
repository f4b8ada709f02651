"""csrc/calendar.hip through the C ABI (ace_diag_calendar_window) against tests/_calendar_ref.py, the numpy statement of the header
contract that tests/test_calendar_ref_cpu.py holds to the reference.

Bars.  binned sums: |got - ref| <= 1e-12 x sum|x| over the steps of the bin per (side, row, bin, pixel), the bar of the other diag
kernels (the kernel follows the stated order and multiplies nothing, so the difference is in fact 0), NaN and infinity in the same
places; two runs on finite planes bitwise equal.  series: |got - ref| <= 1e-12 x sum|w x| / sum w per entry (the kernel adds the
pixels of a plane wave by wave, numpy pairwise), NaN in the same places; an entry the call does not assign keeps its value (the
series start at 7, not 0).  Every output buffer (bins, series, scratch) lies between guards, which must come back intact; the
input planes must come back unchanged; the scratch is pre-filled with NaN, so a partial that is read without having been written
shows.  Shapes: hw = 162 is under one wave of 256 pixels, 17 x 31 = 527 two full waves and a tail (hw % 4 != 0), 1024 + 260 a
second workgroup; the "odd" layout puts every plane one float past a 16-byte boundary with padded strides."""
import numpy as np
import pytest
import torch

import _calendar_ref as R
from test_gpu_diag_kernels import INVALID, Guarded, dev, lib  # noqa: F401
from test_gpu_regress_kernels import place

pytestmark = pytest.mark.gpu

MAX_BINS = 8
UNSET = 7.0


class State:
    """the persistent device buffers between guards, and their numpy twins"""

    def __init__(self, dev, nrows, nbins, nsrows, B, n_time, hw):
        self.dev, self.nrows, self.nbins, self.nsrows, self.hw = dev, nrows, nbins, nsrows, hw
        self.bins = Guarded(torch.zeros(2, nrows, max(nbins, 1), hw, dtype=torch.float64), dev)
        self.series = Guarded(torch.full((2, max(nsrows, 1), B, n_time), UNSET, dtype=torch.float64), dev)
        self.ref_bins = np.zeros((2, nrows, max(nbins, 1), hw))
        self.ref_series = np.full((2, max(nsrows, 1), B, n_time), UNSET)
        self.bin_scale = np.zeros_like(self.ref_bins)
        self.series_scale = np.zeros_like(self.ref_series)

    def read(self):
        return self.bins.read(), self.series.read()

    def check(self):
        bins, series = self.read()
        for name, got, ref, scale in (("bins", bins.numpy(), self.ref_bins, self.bin_scale),
                                      ("series", series.numpy(), self.ref_series, self.series_scale)):
            with np.errstate(invalid="ignore"):
                err = np.abs(got - ref)
                ok = (err <= 1e-12 * scale) | (np.isnan(got) & np.isnan(ref)) | (np.isinf(ref) & (got == ref))
            worst = float(np.nanmax(np.where(np.isfinite(err), err, 0) / np.maximum(scale, 1e-300)))
            print(f"CALACC {name}: max err / scale {worst:.3e}")
            assert ok.all(), (name, worst, np.argwhere(~ok)[:5])
        return bins, series


def window(st, gens, tgts, rows, bin=None, nbins=None, regions=None, srow=None, mode=None, weights=None, wrows=None, t0=0, t_begin=0,
           layout="contiguous", seed=0, expect=0, with_bins=True, with_series=True):
    """one ace_diag_calendar_window on (B, T, hw) CPU fields; the numpy twin gets the same window"""
    L, dev = lib(), st.dev
    g = torch.Generator().manual_seed(seed)
    n = len(gens)
    B, T, hw = gens[0].shape
    nbins = st.nbins if nbins is None else nbins
    placed = [[place(x, layout, g) if x is not None else None for x in side] for side in (gens, tgts)]
    store = [[p[0].to(dev) if p is not None else None for p in side] for side in placed]
    tab = []
    for side, stores in zip(placed, store):
        tab += [s.data_ptr() + 4 * p[1] if p is not None else 0 for p, s in zip(side, stores)]
        for p in side:
            tab += [p[2], p[3]] if p is not None else [0, 0]
    tab = torch.tensor(tab, dtype=torch.int64, device=dev)
    i32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(dev)                # noqa: E731
    off = lambda v: torch.cat([torch.zeros(1), torch.from_numpy(np.ascontiguousarray(v, np.float32)).reshape(-1)]).to(dev)[1:]  # noqa: E731
    rows_d = i32(rows)
    bin_d = i32(bin) if bin is not None else None
    nreg = 0 if regions is None else regions.shape[0]
    ser = with_series and weights is not None
    reg_d = off(regions) if nreg else None                                       # off a 16-byte boundary
    srow_d = i32(srow) if nreg else None
    mode_d = i32(mode) if nreg else None
    w_d = off(weights) if ser else None
    wrows_d = i32(wrows) if ser else None
    ndoubles = int(L.ace_diag_calendar_partial_doubles(n, nreg, B, T, hw))
    assert ndoubles == 2 * n * nreg * B * T * 4 * ((hw + 1023) // 1024) * 2
    scratch = Guarded(torch.full((max(ndoubles, 1),), float("nan"), dtype=torch.float64), dev)
    base = tab.data_ptr()
    n_time = st.ref_series.shape[-1]
    ptr = lambda t: t.data_ptr() if t is not None else None                       # noqa: E731
    rc = L.ace_diag_calendar_window(base, base + 8 * n, base + 24 * n, base + 32 * n, rows_d.data_ptr(), ptr(bin_d),
                                    st.bins.ptr if with_bins else None, ptr(reg_d), ptr(srow_d), ptr(mode_d), ptr(wrows_d), ptr(w_d),
                                    weights.shape[0] if ser else 0, scratch.ptr if ser else None, st.series.ptr if ser else None,
                                    st.nrows, nbins, nreg, st.nsrows, n_time, t0, t_begin, n, B, T, hw, None)
    assert rc == expect, L.ace_diag_last_error().decode()
    torch.cuda.synchronize()
    scratch.read()
    for side, stores in zip(placed, store):
        for p, s in zip(side, stores):
            if p is not None:
                assert torch.equal(s.cpu().view(torch.int32), p[0].view(torch.int32)), "an input plane changed"
    if rc == 0:
        planes = [[x.numpy() if x is not None else None for x in side] for side in (gens, tgts)]
        R.calendar_window(planes[0], planes[1], rows, st.nrows, bin=None if bin is None else np.asarray(bin), nbins=nbins,
                          bins=st.ref_bins if with_bins else None, regions=regions, srow=srow, mode=mode, weights=weights, wrows=wrows,
                          series=st.ref_series if ser else None, t0=t0, t_begin=t_begin, scale=st.series_scale)
        if with_bins and bin is not None:
            for s in (0, 1):
                for j, x in enumerate(planes[s]):
                    if x is None or not 0 <= rows[j] < st.nrows:
                        continue
                    a = np.abs(np.nan_to_num(x.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0))
                    for m in range(nbins):
                        sel = np.asarray(bin) == m
                        sel[:, :t_begin] = False
                        st.bin_scale[s, rows[j], m] += a[sel].sum(axis=0)


def fields(B, T, hw, g, n=3):
    """a unit Gaussian, a surface-temperature-like field near 300 and a zero-inflated one"""
    r = lambda: torch.randn(B, T, hw, generator=g)                                # noqa: E731
    wet = torch.rand(B, T, hw, generator=g) < 0.3
    return [r().float(), (290 + 9 * r()).float(), torch.where(wet, 3e-4 * r().abs() ** 3, torch.zeros(())).float()][:n]


def area(hw, zero=()):
    w = np.cos(np.linspace(-1.5, 1.5, hw)).astype(np.float32)
    for a, b in zero:
        w[a:b] = 0.0
    return w[None]


def boxes(hw, g, nreg):
    """region 0 all ones, the others a band of cos-like weights on a quarter of the pixels"""
    reg = np.zeros((nreg, hw), np.float32)
    reg[0] = 1.0
    for r in range(1, nreg):
        lo = (r * hw) // (nreg + 1)
        reg[r, lo:lo + hw // 4] = 0.2 + torch.rand(len(reg[r, lo:lo + hw // 4]), generator=g).numpy()
    return reg


SEASON = np.array([[0, 0, 1, -1, 3], [3, 0, 0, 1, 9]])                            # bin 2 is empty; -1 and 9 name no bin


@pytest.mark.parametrize("layout", ["contiguous", "odd"])
@pytest.mark.parametrize("t_begin", [0, 1])
@pytest.mark.parametrize("hw", [162, 17 * 31, 1024 + 260])
def test_shapes_and_layouts(dev, hw, t_begin, layout):
    g = torch.Generator().manual_seed(hw + t_begin)
    B, T, n_time = 2, 5, 13
    st = State(dev, 4, 4, 9, B, n_time, hw)
    reg = boxes(hw, g, 3)
    srow = [[0, 1, 2], [3, -1, 4], [5, 6, 99]]
    w = np.concatenate([area(hw, zero=[(3, 9)]), area(hw)[:, ::-1]])
    for k in range(2):                                                          # a second call adds to the bins and assigns further on
        window(st, fields(B, T, hw, g), fields(B, T, hw, g), [2, 0, 3], bin=SEASON, regions=reg, srow=srow, mode=[0, 0, 1], weights=w,
               wrows=[0, 1, 0], t0=1 + k * T, t_begin=t_begin, layout=layout, seed=k)
    bins, series = st.check()
    assert not bins[:, 1].any() and not bins[:, :, 2].any() and bins[0, 2, 0].any() and bins[1, 3, 3].any()
    assert bool((series[:, 7:] == UNSET).all()) and bool((series[:, :, :, 0] == UNSET).all()) and bool((series[:, :, :, 11:] == UNSET).all())
    assert bool((series[:, 0, :, 1 + t_begin:1 + T] != UNSET).all()) and bool((series[:, :, :, 1:1 + t_begin] == UNSET).all())
    assert 280 < float(series[0, 3, 0, 2]) < 300                                 # plane 1 over the whole plane: about 290


def test_t_begin_past_the_window_changes_nothing(dev):
    g = torch.Generator().manual_seed(2)
    B, T, hw = 2, 5, 162
    st = State(dev, 3, 4, 3, B, T, hw)
    window(st, fields(B, T, hw, g), fields(B, T, hw, g), [0, 1, 2], bin=SEASON, regions=boxes(hw, g, 1), srow=[[0], [1], [2]], mode=[0],
           weights=area(hw), wrows=[0, 0, 0], t_begin=T)
    bins, series = st.check()
    assert torch.equal(bins.view(torch.int64), torch.zeros_like(bins).view(torch.int64)) and bool((series == UNSET).all())


def test_a_nan_step_stays_in_its_bin(dev):
    g = torch.Generator().manual_seed(3)
    B, T, hw = 2, 5, 17 * 31
    x, y = fields(B, T, hw, g, 2)
    x[0, 2, 40:60] = float("nan")                                                # a step of bin 1
    x[1, 4] = float("nan")                                                      # a step of no bin
    y[1, 0, 7] = float("inf")                                                   # a step of bin 3
    st = State(dev, 2, 4, 0, B, T, hw)
    window(st, [x, y], [y, x], [0, 1], bin=SEASON)
    bins, _ = st.check()
    assert bool(bins[0, 0, 1, 40:60].isnan().all()) and int(bins[0, 0].isnan().sum()) == 20          # the other bins stay finite
    assert bool(bins[0, 1, 3, 7].isinf()) and bool(torch.isfinite(bins[0, 1, :3]).all())
    assert not bins[:, :, 2].any()                                              # the empty bin


def test_the_cap_on_bins(dev):
    g = torch.Generator().manual_seed(4)
    B, T, hw = 2, 5, 17 * 31
    gens, tgts = fields(B, T, hw, g, 1), fields(B, T, hw, g, 1)
    every = np.array([[0, 1, 2, 3, 4], [5, 6, 7, 0, 1]])
    st = State(dev, 1, MAX_BINS, 0, B, T, hw)
    window(st, gens, tgts, [0], bin=every)
    bins, _ = st.check()
    assert all(bins[0, 0, m].any() for m in range(MAX_BINS))
    st = State(dev, 1, 0, 1, B, T, hw)                                          # nbins = 0: the series alone, no bin table at all
    window(st, gens, tgts, [0], bin=None, nbins=0, regions=boxes(hw, g, 1), srow=[[0]], mode=[0], weights=area(hw), wrows=[0])
    bins, series = st.check()
    assert not bins.any() and bool((series != UNSET).all())
    st = State(dev, 1, MAX_BINS + 1, 0, B, T, hw)
    window(st, gens, tgts, [0], bin=every, expect=INVALID)
    msg = lib().ace_diag_last_error().decode()
    assert msg.startswith("ace_diag_calendar_window") and "nbins" in msg
    assert not st.check()[0].any()


def test_zero_weights_and_nan_pixels_under_both_modes(dev):
    g = torch.Generator().manual_seed(5)
    B, T, hw = 2, 5, 17 * 31
    x = fields(B, T, hw, g, 2)[1]
    x[0, 1, 100:110] = float("nan")                                             # inside regions 0, 1 (mode 0) and 2 (mode 1)
    x[1, 3, 3:9] = float("nan")                                                 # at pixels of weight 0: enters nothing
    reg = np.zeros((4, hw), np.float32)
    reg[0] = 1.0
    reg[1, 90:200] = 0.5
    reg[2, 90:200] = 0.5
    reg[3, 3:9] = 1.0                                                           # region x weight row all zero: 0 / 0
    w = area(hw, zero=[(3, 9)])
    st = State(dev, 1, 0, 4, B, T, hw)
    window(st, [x], [x], [0], regions=reg, srow=[[0, 1, 2, 3]], mode=[0, 0, 1, 0], weights=w, wrows=[0], with_bins=False)
    _, series = st.check()
    assert bool(series[:, 0, 0, 1].isnan().all()) and bool(series[:, 1, 0, 1].isnan().all())          # mode 0: the NaN propagates
    assert bool(torch.isfinite(series[:, 2]).all()) and 280 < float(series[0, 2, 0, 1]) < 300          # mode 1: it is left out
    assert int(series[:, :2].isnan().sum()) == 4 and bool(series[:, 3].isnan().all())
    keep = np.ones(hw, bool)
    keep[100:110] = False
    want = float((reg[2][keep].astype(np.float64) * x[0, 1].numpy()[keep].astype(np.float64)).sum() / reg[2][keep].astype(np.float64).sum())
    assert abs(float(series[0, 2, 0, 1]) - want) <= 1e-12 * abs(want)
    allnan = State(dev, 1, 0, 1, B, T, hw)                                      # mode 1 with no pixel left: NaN
    window(allnan, [torch.full((B, T, hw), float("nan"))], [None], [0], regions=reg[2:3], srow=[[0]], mode=[1], weights=w, wrows=[0],
           with_bins=False)
    _, series = allnan.check()
    assert bool(series[0].isnan().all()) and bool((series[1] == UNSET).all())


def test_null_target_bad_rows_and_idle_series_rows(dev):
    g = torch.Generator().manual_seed(6)
    B, T, hw = 2, 5, 17 * 31
    gens, tgts = fields(B, T, hw, g), fields(B, T, hw, g)
    st = State(dev, 2, 4, 4, B, T, hw)
    reg = boxes(hw, g, 2)
    for rows in ([1, 0, 7], [1, 0, -1]):                                        # plane 2: a row out of range, bins and series alike
        window(st, gens, [tgts[0], None, tgts[2]], rows, bin=SEASON, regions=reg, srow=[[0, -1], [1, 2], [3, 3]], mode=[0, 1],
               weights=area(hw), wrows=[0, 5, 0])
    bins, series = st.check()
    assert not bins[1, 0].any() and bins[0, 0].any() and bins[1, 1].any()       # plane 1: the generated side only
    assert bool((series[:, 1:] == UNSET).all())                                 # plane 1: a weight row out of range; plane 2: no row
    assert bool((series[:, 0] != UNSET).all())
    none = State(dev, 2, 4, 4, B, T, hw)                                        # nreg = 0 with the series given: the bins alone
    window(none, gens, tgts, [0, 1, -1], bin=SEASON, regions=None, weights=area(hw), wrows=[0, 0, 0])
    bins, series = none.check()
    assert bins.any() and bool((series == UNSET).all())


def test_two_runs_are_bitwise_equal(dev):
    outs = []
    for _ in range(2):
        g = torch.Generator().manual_seed(8)
        B, T, hw = 2, 5, 1024 + 260
        st = State(dev, 3, 4, 6, B, 2 * T, hw)
        reg = boxes(hw, g, 2)
        for k in range(2):
            window(st, fields(B, T, hw, g), fields(B, T, hw, g), [0, 1, 2], bin=SEASON, regions=reg, srow=[[0, 1], [2, 3], [4, 5]],
                   mode=[0, 1], weights=area(hw), wrows=[0, 0, 0], t0=k * T, layout="odd", t_begin=k)
        outs.append(st.read())
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("change,word", [
    (dict(nplanes=-1), "nplanes"), (dict(nplanes=65536), "nplanes"), (dict(nbins=-1), "nbins"), (dict(nbins=9), "nbins"),
    (dict(nreg=-1), "nreg"), (dict(nreg=9), "nreg"), (dict(batch=0), "batch"), (dict(steps=0), "steps"), (dict(hw=0), "hw"),
    (dict(nrows=0), "nrows"), (dict(t_begin=-1), "t_begin"), (dict(t0=3), "n_time"), (dict(t0=-1), "n_time"), (dict(nsrows=0), "nsrows"),
    (dict(null=0), "null"), (dict(null=4), "null"), (dict(null=5), "null"), (dict(null=7), "null"), (dict(null=8), "null"),
    (dict(null=9), "null"), (dict(null=10), "null"), (dict(null=11), "null"), (dict(null=13), "null")])
def test_refusals(dev, change, word):
    L = lib()
    st = State(dev, 1, 2, 1, 1, 4, 4)
    x = torch.zeros(64, dtype=torch.float64, device=dev)
    a = dict(nrows=1, nbins=2, nreg=1, nsrows=1, n_time=4, t0=2, t_begin=0, nplanes=1, batch=1, steps=2, hw=4)
    a.update({k: v for k, v in change.items() if k in a})
    p = [x.data_ptr()] * 6 + [st.bins.ptr] + [x.data_ptr()] * 5 + [1, x.data_ptr(), st.series.ptr]
    if "null" in change:
        p[change["null"]] = None
    rc = L.ace_diag_calendar_window(*p, a["nrows"], a["nbins"], a["nreg"], a["nsrows"], a["n_time"], a["t0"], a["t_begin"], a["nplanes"],
                                    a["batch"], a["steps"], a["hw"], None)
    msg = L.ace_diag_last_error().decode()
    assert rc == INVALID and word in msg and msg.startswith("ace_diag_calendar_window"), (rc, msg)
    torch.cuda.synchronize()
    bins, series = st.check()
    assert not bins.any() and bool((series == UNSET).all())


def test_no_planes_is_a_no_op(dev):
    L = lib()
    assert L.ace_diag_calendar_window(*([None] * 12), 0, None, None, 1, 4, 0, 0, 0, 0, 0, 0, 1, 40, 64800, None) == 0
    assert L.ace_diag_calendar_partial_doubles(0, 5, 1, 1, 64800) == 0 and L.ace_diag_calendar_partial_doubles(3, 0, 1, 1, 64800) == 0
    assert L.ace_diag_calendar_partial_doubles(50, 5, 1, 40, 64800) == 2 * 50 * 5 * 40 * 4 * 64 * 2
    assert L.ace_diag_calendar_partial_doubles(1, 1, 0, 1, 5) == -1 and L.ace_diag_calendar_partial_doubles(1, 9, 1, 1, 5) == -1
    assert L.ace_diag_calendar_partial_doubles(65536, 1, 1, 1, 5) == -1
