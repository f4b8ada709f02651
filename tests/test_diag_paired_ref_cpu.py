"""tests/_diag_paired_ref.py (the fp64 statement of ace_diag_paired_window that the GPU kernel tests are judged by) against the
evaluator aggregator's torch path run in fp64 on the CPU: the reference's formulas in torch ops, which
tests/test_evaluator_aggregator_cpu.py pins in fp32.  The initial condition, two windows, a masked name, a prediction-only name
and a zonal coarsening factor of 2, on a 12 x 24 grid and a 13 x 27 one."""
import pytest
import torch

from ace_amd.evaluator import InferenceEvaluatorAggregatorConfig, MetricConfig, PowerSpectrumMetricConfig, ZonalMeanMetricConfig

import _diag_paired_ref as P
from test_aggregator_cpu import make_case
from test_diag_ref_cpu import sht64

WINDOWS = (3, 2)


def perturbed(win, seed):
    g = torch.Generator().manual_seed(seed)
    return {n: x + 0.1 * x.abs().nan_to_num(0.0).mean() * torch.randn(x.shape, generator=g) for n, x in win.items() if n != "diag"}


@pytest.mark.parametrize("h,w", [(12, 24), (13, 27)])
def test_paired_ref_matches_the_torch_path_in_fp64(h, w):
    info, ic, wins = make_case(seed=5, h=h, w=w, windows=WINDOWS)
    tgts = [perturbed(win, 50 + i) for i, win in enumerate(wins)]
    n_time, B = 1 + sum(WINDOWS), 2
    cfg = InferenceEvaluatorAggregatorConfig(mean_norm=MetricConfig(enabled=False), time_mean_norm=MetricConfig(enabled=False),
                                             power_spectrum=PowerSpectrumMetricConfig(enabled=False),
                                             zonal_mean=ZonalMeanMetricConfig(zonal_mean_max_size=3))
    agg = cfg.build(info, 1, sum(WINDOWS), normalize=None, sht_factory=sht64)
    assert (agg._factor, agg._n_slots) == (2, 3)
    agg.fused = False
    agg._area = agg._area.double()
    dbl = lambda d: {k: v.double() for k, v in d.items()}                  # noqa: E731
    agg.record_initial_condition(dbl(ic))
    for win, tgt in zip(wins, tgts):
        agg.record_batch(dbl(win), dbl(tgt))
    ds = agg.get_dataset()

    names = ["a", "ps", "sst", "diag"]
    row = {n: i for i, n in enumerate(names)}
    weights = torch.stack([agg.weights_for("a", "cpu"), agg.weights_for("sst", "cpu")]).float()
    series = torch.zeros(6, len(names), n_time, dtype=torch.float64)
    bar = torch.zeros_like(series)
    tsum = torch.zeros(2, len(names), h * w, dtype=torch.float64)
    zonal = torch.zeros(2, len(names), 3, h, dtype=torch.float64)
    zbar = torch.zeros_like(zonal)
    t0 = 0
    for k, (rec, tgt) in enumerate([(ic, ic)] + list(zip(wins, tgts))):
        T = next(iter(rec.values())).shape[1]
        rows = [row[n] for n in rec]
        scale = P.paired_window_ref(list(rec.values()), [tgt.get(n) for n in rec], weights, [1 if n == "sst" else 0 for n in rec],
                                    rows, B, T, t0, 0, k > 0, max(t0 - 1, 0), 2, series, tsum, zonal, zbar)
        P.add_paired_scale(bar, scale, rows, t0)
        t0 += T
    metrics = ("weighted_mean_gen", "weighted_std_gen", "weighted_mean_target", "weighted_bias", "weighted_rmse",
               "weighted_grad_mag_percent_diff")
    got = torch.zeros_like(series)
    for i, m in enumerate(metrics):
        for n in names:
            if f"{m}-{n}" in ds["mean"]:
                got[i, row[n]] = ds["mean"][f"{m}-{n}"]
    assert "weighted_rmse-diag" not in ds["mean"] and "weighted_mean_gen-diag" in ds["mean"]
    errs = P.paired_series_errors(got, series, bar)
    assert max(errs) <= 1.0, errs
    assert float(got[4, row["a"], 0]) == 0.0                               # the initial condition is its own target
    steps = sum(WINDOWS)
    for n in ("a", "ps", "sst"):
        g = ds["time_mean"][f"gen_map-{n}"].reshape(-1)
        want = tsum[0, row[n]] / steps / B
        ok = ~torch.isnan(want)
        assert torch.equal(torch.isnan(g), ~ok)
        assert bool(((g - want).abs()[ok] <= 1e-13 * want.abs()[ok].clamp_min(1e-30)).all()), n
        bias = ds["time_mean"][f"bias_map-{n}"].reshape(-1)
        want_b = (tsum[0, row[n]] - tsum[1, row[n]]) / steps / B
        assert bool(((bias - want_b).abs()[ok] <= 1e-13 * want.abs()[ok]).all()), n
        z, zw = ds["zonal_mean"][f"gen-{n}"], zonal[0, row[n]].clone()
        zw[steps // 2:] = float("nan")                                      # 5 steps, factor 2: the third slot is never completed
        assert torch.equal(torch.isnan(z), torch.isnan(zw)), n
        okz = ~torch.isnan(zw)
        assert bool(((z - zw).abs()[okz] <= 1e-12 * zbar[0, row[n]][okz]).all()), n
        e = ds["zonal_mean"][f"error-{n}"]
        ew = zw - zonal[1, row[n]]
        assert bool(((e - ew).abs()[okz] <= 1e-12 * zbar[0, row[n]][okz]).all()), n
    assert "gen-diag" not in ds["zonal_mean"]


def test_sample_ref_edges():
    w = torch.tensor([[0.0, 2.0, 1.0], [1.0, 1.0, 1.0]])
    x = torch.tensor([[float("nan"), 3.0, 5.0], [1.0, 2.0, 4.0]])
    # the NaN pixel has no weight, but the gradients of its two neighbours are NaN: they leave the gradient mean
    gy, gx = torch.gradient(x.double(), dim=(-2, -1))
    g = torch.sqrt(gy ** 2 + gx ** 2)
    assert bool(torch.isnan(g[0, 0])) and bool(torch.isnan(g[0, 1])) and bool(torch.isnan(g[1, 0]))
    want = float((g[0, 2] + g[1, 1] + g[1, 2]) / 3)
    assert P.grad_mag_mean_ref(x, w) == pytest.approx(want, rel=1e-15)
    vals, _ = P.sample_ref(x, x, w)
    assert vals[3] == 0.0 and vals[4] == 0.0 and vals[5] == 0.0
    vals, _ = P.sample_ref(x, None, w)
    assert all(v != v for v in vals[2:])
