"""tests/_diag_ref.py (the fp64 statement of ace_diag_window / ace_diag_spectrum that the GPU kernel tests are judged by) against the
aggregator's torch path run in fp64 on the CPU: the reference's formulas in torch ops, which tests/test_aggregator_cpu.py pins in
fp32.  The initial condition, two windows, a masked name (NaN where the weight is 0) and a name that is not in the initial
condition, on a 12 x 24 grid and a 13 x 27 one (odd nlat, hw % 4 == 3)."""
import pytest
import torch

from ace_amd.aggregator import InferenceAggregatorConfig
from oracle.sht import RealSHT as OracleSHT

import _diag_ref as R
from test_aggregator_cpu import make_case

WINDOWS = (3, 2)


def sht64(nlat, nlon):
    return OracleSHT(nlat, nlon, grid="legendre-gauss", dtype=torch.float64)


@pytest.mark.parametrize("h,w", [(12, 24), (13, 27)])
def test_diag_ref_matches_the_torch_path_in_fp64(h, w):
    info, ic, wins = make_case(seed=3, h=h, w=w, windows=WINDOWS)
    n_time, B, hw = 1 + sum(WINDOWS), 2, h * w
    agg = InferenceAggregatorConfig().build(info, n_time, sht_factory=sht64)
    agg.fused = False
    agg._area = agg._area.double()          # the same fp32 values, so that the path sums the weights in fp64 as well
    agg.record_initial_condition({k: v.double() for k, v in ic.items()})
    for win in wins:
        agg.record_batch({k: v.double() for k, v in win.items()})
    ds = agg.get_dataset()
    assert all(v.dtype == torch.float64 for d in ds.values() for v in d.values())

    names = ["a", "ps", "sst", "diag"]                                   # "diag" first appears in the first window
    row = {n: i for i, n in enumerate(names)}
    weights = torch.stack([agg.weights_for("a", "cpu").reshape(-1), agg.weights_for("sst", "cpu").reshape(-1)])
    assert torch.equal(weights, weights.float().double())
    weights = weights.float()
    assert weights.dtype == torch.float32 and bool((weights[1] == 0).any())
    series = torch.zeros(2, len(names), n_time, dtype=torch.float64)
    bar = torch.zeros_like(series)
    tsum = torch.zeros(len(names), hw, dtype=torch.float64)
    spec = torch.zeros(len(names), h, dtype=torch.float64)
    sht = sht64(h, w)
    t0 = 0
    for k, rec in enumerate([ic] + wins):
        T = next(iter(rec.values())).shape[1]
        rows = [row[n] for n in rec]
        wrows = [1 if n == "sst" else 0 for n in rec]
        fields = [x.reshape(B, T, hw) for x in rec.values()]
        scale = R.window_ref(fields, weights, wrows, rows, B, T, t0, 0, k > 0, series, tsum)
        R.add_scale(bar, scale, rows, t0)
        if k > 0:
            spec_names = [n for n in rec if n != "sst"]
            coeffs = torch.stack([sht(rec[n].double()).reshape(B * T, h, -1) for n in spec_names])
            R.spectrum_ref(coeffs, [row[n] for n in spec_names], spec)
        t0 += T

    got = torch.stack([torch.stack([ds["mean"][f"{m}-{n}"] for n in names]) for m in ("weighted_mean_gen", "weighted_std_gen")])
    assert float(series[0, row["diag"], 0]) == 0.0 and float(got[0, row["diag"], 0]) == 0.0
    # one record per time index: the series are the accumulators themselves
    e_mean, e_std = R.series_errors(got, series, bar)
    assert e_mean <= 1.0 and e_std <= 1.0, (e_mean, e_std)
    steps = sum(WINDOWS)
    for n in names:
        g, want = ds["time_mean"][f"gen_map-{n}"].reshape(-1), tsum[row[n]] / steps / B
        ok = ~torch.isnan(want)
        assert torch.equal(torch.isnan(g), ~ok), n
        assert bool(ok.any()) and (n != "sst" or not bool(ok.all()))
        scale = sum(win[n].double().abs().sum((0, 1)) for win in wins).reshape(-1) / steps / B
        assert bool(((g - want).abs()[ok] <= 1e-14 * scale[ok]).all()), n
    assert set(ds["power_spectrum"]) == {"a", "ps", "diag"}
    for n, g in ds["power_spectrum"].items():
        want = spec[row[n]] / (steps * B)
        assert float(((g - want).abs() / want).max()) <= 1e-12, n


def test_moments_ref_edges():
    w = torch.tensor([0.0, 2.0, 0.0, 1.0])
    x = torch.tensor([float("nan"), 3.0, float("inf"), 6.0])
    m, s, a = R.moments_ref(x, w)
    assert (m, a) == (4.0, 4.0) and s == pytest.approx(2.0 ** 0.5, rel=1e-15)
    assert all(v != v for v in R.moments_ref(x, torch.zeros(4)))            # no valid pixel: 0 / 0
    assert R.moments_ref(torch.full((1000,), 101325.0), torch.rand(1000, generator=torch.Generator().manual_seed(0)))[1] <= 1e-11


def test_window_ref_bookkeeping():
    """rows out of range contribute nothing, the series and the sums accumulate, t_begin past the window adds zero"""
    g = torch.Generator().manual_seed(0)
    f = [torch.randn(2, 3, 5, generator=g) for _ in range(3)]
    w = torch.ones(1, 5)
    series, tsum = torch.zeros(2, 4, 6, dtype=torch.float64), torch.zeros(4, 5, dtype=torch.float64)
    R.window_ref(f, w, [0, 0, -1], [2, -1, 1], 2, 3, 1, 1, True, series, tsum)
    assert bool((series[:, [0, 1, 3]] == 0).all()) and bool((tsum[[0, 1, 3]] == 0).all())
    assert bool((series[:, 2, 1:4] != 0).all()) and bool((series[:, 2, [0, 4, 5]] == 0).all())
    assert torch.equal(tsum[2], (f[0][0, 1].double() + f[0][0, 2].double()) + f[0][1, 1].double() + f[0][1, 2].double())
    once = (series.clone(), tsum.clone())
    R.window_ref(f, w, [0, 0, -1], [2, -1, 1], 2, 3, 1, 1, True, series, tsum)
    assert torch.equal(series, 2 * once[0]) and torch.equal(tsum, 2 * once[1])
    R.window_ref(f, w, [0, 0, -1], [2, -1, 1], 2, 3, 1, 5, True, series, tsum)
    assert torch.equal(tsum, 2 * once[1])
    assert R.bits_equal(torch.tensor([float("nan"), 1.0]).double(), torch.tensor([float("nan"), 1.0]).double())
    assert not R.bits_equal(torch.tensor([0.0]).double(), torch.tensor([-0.0]).double())
