"""tests/_calendar_ref.py, the numpy statement of the header contract of ``ace_diag_calendar_window``, held to the reference's formulas
on tests/golden/gen_calendar.pt ("f64": the reference's own functions on the fp64 cast of the same fp32 fields, see
tests/golden/make_golden_calendar.py).  Both sides are fp64 sums of the same numbers in different orders: 1e-12 of the magnitude the
sums are formed from (values near 300 K).  The GPU tests hold the kernel to this statement."""
import os

import numpy as np
import pytest
import torch

import _calendar_cases as C
import _calendar_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_calendar.pt")
REGIONS = ("globe", "nino34", "T1", "T2", "T3")
MODES = [0, 0, 1, 1, 1]


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)["main"]


def through_the_contract(c, golden, windows=None):
    """bins (2, names, 4, hw) and series (2, names x regions, B, n_time) of the record, window by window"""
    names, hw = c["names"], C.H * C.W
    regions = np.stack([np.ones(hw, np.float32)] + [golden["f64"]["regions"][r].reshape(-1).numpy() for r in REGIONS[1:]])
    weights = c["info"].area_weights.to(torch.float32).reshape(1, -1).numpy()
    bins = np.zeros((2, len(names), 4, hw))
    series = np.full((2, len(names) * len(REGIONS), C.B, c["n_time"]), -1.0)
    srow = [[j * len(REGIONS) + r for r in range(len(REGIONS))] for j in range(len(names))]
    t0 = 0
    for (gen, tgt), time in (windows or c["windows"]):
        _, month = time.year_month()
        T = month.shape[1]
        flat = lambda d: [d[n].reshape(C.B, T, hw).numpy() for n in names]                       # noqa: E731
        R.calendar_window(flat(gen), flat(tgt), list(range(len(names))), len(names), bin=(month % 12) // 3, nbins=4, bins=bins,
                          regions=regions, srow=srow, mode=MODES, weights=weights, wrows=[0] * len(names), series=series, t0=t0)
        t0 += T
    return bins, series


def test_the_series_are_the_references_regional_means(golden):
    c = C.main()
    _, series = through_the_contract(c, golden)
    raw = golden["f64"]["raw"]
    for s, side in enumerate(("gen", "target")):
        for j, n in enumerate(c["names"]):
            got = series[s, j * len(REGIONS)]
            want = raw[side]["globe"][n].numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).all() == (n == "sst")       # no mask: NaN propagates
            assert np.nanmax(np.abs(got - want), initial=0) <= 1e-12 * 300
        j = c["names"].index("sst")
        for r, region in enumerate(REGIONS[1:], start=1):
            got, want = series[s, j * len(REGIONS) + r], raw[side][region].numpy()
            assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-12 * 300, (side, region)


def test_mode_one_takes_the_regional_weights_alone_and_leaves_nan_pixels_out(golden):
    """the T1 box holds a land cell: _nan_aware_regional_mean (ipo_index.py:43-58) drops it, and its weights are mask x cos(lat)
    without the area weights (ipo_index.py:121-124), where the Nino 3.4 mean multiplies the two (gridded_ops.py:336)"""
    c = C.main()
    x = c["gen"]["sst"][:, :3].reshape(C.B, 3, -1).numpy()
    w = golden["f64"]["regions"]["T1"].reshape(-1).numpy()
    assert np.isnan(x[0, 0][w != 0]).sum() == 1
    series = np.zeros((2, 2, C.B, 3))
    R.calendar_window([x], [None], [0], 1, regions=np.stack([w, w]), srow=[[0, 1]], mode=[1, 0],
                      weights=c["info"].area_weights.float().reshape(1, -1).numpy(), wrows=[0], series=series)
    keep = (w != 0) & ~np.isnan(x[0, 0])
    want = (w[keep].astype(np.float64) * x[0, 0][keep]).sum() / w[keep].astype(np.float64).sum()
    assert abs(series[0, 0, 0, 0] - want) <= 1e-12 * 300 and np.isnan(series[0, 1]).all() and not series[1].any()


def test_the_binned_sums_are_the_references_seasonal_sums(golden):
    c = C.main()
    bins, _ = through_the_contract(c, golden)
    counts = golden["f64"]["seasonal"]["counts"].numpy()
    for j, n in enumerate(c["names"]):
        gen, tgt = (bins[s, j].reshape(4, C.H, C.W) / counts[:, None, None] for s in (0, 1))
        want = golden["f64"]["seasonal"]["bias"][n].numpy()
        assert np.array_equal(np.isnan(gen - tgt), np.isnan(want))
        assert np.nanmax(np.abs((gen - tgt) - want)) <= 1e-12 * 300
        pattern = tgt.mean(axis=0)
        assert np.nanmax(np.abs(np.stack([tgt - pattern, gen - pattern]) - golden["f64"]["seasonal"]["anomaly"][n].numpy())) <= 1e-12 * 300


def test_a_nan_step_stays_in_its_season_and_windows_add_up(golden):
    c = C.main(cuts=(100,))
    x = {n: v.clone() for n, v in c["windows"][0][0][0].items()}
    _, month = c["windows"][0][1].year_month()
    assert (month[0, 20] % 12) // 3 == 1                                                 # a step in April
    x["t"][0, 20, 2, 3] = float("nan")
    windows = [((x, c["windows"][0][0][1]), c["windows"][0][1]), c["windows"][1]]
    bins, _ = through_the_contract(c, golden, windows)
    t = bins[0, c["names"].index("t")].reshape(4, C.H, C.W)
    assert np.isnan(t[1, 2, 3]) and np.isnan(t).sum() == 1                               # groupby(season).sum(skipna=False)
    whole, _ = through_the_contract(C.main(cuts=()), golden)
    three, _ = through_the_contract(C.main(), golden)
    assert np.nanmax(np.abs(whole - three)) <= 1e-12 * 300 * 151
