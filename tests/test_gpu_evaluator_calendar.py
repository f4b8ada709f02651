"""The evaluator's seasonal, annual, enso_index and ipo_index metrics on the fused path (csrc/calendar.hip: one
ace_diag_calendar_window per window) on the records of tests/_calendar_cases.py, against

  * a twin whose device buffers are filled by tests/_calendar_ref.py, the numpy statement of the header contract, window by window
    through the class's own bookkeeping, and then read by the same fp64 host post-processing: 1e-9 relative to the largest value of
    each output (both sides see the same fp32 inputs; only the order of the pixel sums differs, 1e-12 of sums of values near 300 K,
    which the anomaly step - a cancellation down to a few tenths - and the spectra amplify by some hundreds);
  * the aggregator's own torch path on the same device, as tests/test_gpu_evaluator_regress.py holds its fused path to its torch
    path: within 3 x the torch path's own fp32 error against the fp64 twin, that floor computed on the CPU
    (tests/test_evaluator_calendar_cpu.py holds the torch path to the reference).  This bar is applied to the series, maps and
    spectra; the scalars formed from them are held to the contract twin alone, at the 1e-9 above.

Two and three windows, a ``variables`` filter on annual and seasonal, all four metrics in one call (the 82-year record), one native
``ace_diag_calendar_window`` call per window (C-ABI calls, not kernel launches), the initial condition left out, and bitwise repeatability."""
import math

import numpy as np
import pytest
import torch

import _calendar_cases as C
import _calendar_ref as R
from ace_amd.evaluator import AnnualMetricConfig, EnsoIndexMetricConfig, IpoIndexMetricConfig, SeasonalMetricConfig
from test_evaluator_calendar_cpu import config
from test_gpu_diag_kernels import dev  # noqa: F401

pytestmark = pytest.mark.gpu


def four(**kw):
    m = dict(seasonal=SeasonalMetricConfig(enabled=True), annual=AnnualMetricConfig(), enso_index=EnsoIndexMetricConfig(),
             ipo_index=IpoIndexMetricConfig())
    m.update(kw)
    return m


def on(dev, d):
    return {n: v.to(dev) for n, v in d.items()}


def record(c, device, fused, metrics, n_ic=0):
    agg = config(**metrics).build(c["info"], n_ic, c["n_time"] - n_ic, normalize=lambda d: d)
    agg.fused = fused
    for (gen, tgt), time in c["windows"]:
        agg.record_batch(on(device, gen), on(device, tgt), time=time)
    return agg


def twin(c, metrics):
    """the contract in numpy behind the class's bookkeeping and host post-processing: what the fused path must give"""
    agg = config(**metrics).build(c["info"], 0, c["n_time"], normalize=lambda d: d)
    cal, cpu, t0 = agg._calendar, torch.device("cpu"), 0
    for (gen, tgt), time in c["windows"]:
        B, T, season, wanted = cal._prepare(gen, tgt, t0, time)
        planes, rows, srow = cal._layout(gen, wanted, B, C.H * C.W, cpu)
        flat = lambda d: [d[n].reshape(B, T, -1).numpy() if n in d else None for n in planes]          # noqa: E731
        weights = np.stack([agg.weights_for(n, cpu).reshape(-1).numpy() for n in planes])
        nreg = len(cal._region_names)
        R.calendar_window(flat(gen), flat(tgt), rows, len(cal._rows), bin=season, nbins=4,
                          bins=cal._bins.numpy() if cal.seasonal is not None else None,
                          regions=cal._regions.reshape(nreg, -1).numpy() if nreg else None, srow=srow, mode=cal._modes,
                          weights=weights, wrows=list(range(len(planes))), series=cal._series.numpy() if nreg else None, t0=t0)
        t0 += T
    return agg


def flatten(agg):
    out = dict(agg.get_summary_logs())
    for label, d in agg.get_dataset().items():
        out.update({f"dataset:{label}/{k}": v for k, v in d.items()})
    return out


def err_of(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().nan_to_num().max())


def compare(name, got, want, rel=None, floors=None, low=None):
    """``rel``: every output of ``want`` in ``got``, NaN in the same places and |got - want| <= rel x max|want|.  Otherwise the
    regress test's bar on every series, map and spectrum: |got - want| <= 3 x the floor |low - floors| of the same output; the
    scalars formed from them are held to the contract twin alone (the floor of a single number can vanish by chance)"""
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    worst, checked = 0.0, 0
    for k, w in want.items():
        if rel is None and not torch.is_tensor(w):
            continue
        g, w = torch.as_tensor(got[k]).double().cpu(), torch.as_tensor(w).double().cpu()
        assert g.shape == w.shape and torch.equal(g.isnan(), w.isnan()), (name, k)
        err, top = float((g - w).abs().nan_to_num().max()), float(w.abs().nan_to_num().max())
        bar = rel * top if rel is not None else 3 * err_of(low[k], floors[k])
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else math.inf)
        if ratio > 0.3:
            print(f"CALEVAL {name}: {k} err {err:.3e} bar {bar:.3e}")
        worst, checked = max(worst, ratio), checked + 1
        assert err <= bar, (name, k, err, bar)
    print(f"CALEVAL {name}: {checked} outputs, worst err / bar {worst:.3e}")


@pytest.fixture(scope="module")
def main_truth():
    c = C.main()
    metrics = four(ipo_index=IpoIndexMetricConfig(enabled=False))
    return c, metrics, flatten(twin(c, metrics)), flatten(record(c, torch.device("cpu"), False, metrics))


def test_three_windows_against_the_contract_and_the_torch_path(dev, main_truth):
    c, metrics, truth, cpu_torch = main_truth
    fused, torch_ = record(c, dev, True, metrics), record(c, dev, False, metrics)
    assert fused._path == "fused" and torch_._path == "torch"
    assert fused.calendar_launches() == 3 and torch_.calendar_launches() == 0 and fused.launches() == 3      # + the paired windows
    got = flatten(fused)
    assert got["dataset:annual/t"].dtype == torch.float64 and got["dataset:annual/year"].tolist() == [2001, 2002, 2003]
    assert "seasonal/bias/sst" in got and "enso_index/sst_nino34_index_std_norm" in got and 0 < got["annual/rmse/t"] < 1
    compare("fused vs contract, 3 windows", got, truth, rel=1e-9)
    compare("fused vs torch, 3 windows", got, flatten(torch_), floors=truth, low=cpu_torch)


def test_two_windows_give_the_same(dev, main_truth):
    c, metrics, truth, _ = main_truth
    two = C.main(cuts=(101,))
    fused = record(two, dev, True, metrics)
    assert fused.calendar_launches() == 2
    compare("fused vs contract, 2 windows", flatten(fused), flatten(twin(two, metrics)), rel=1e-9)
    compare("2 windows vs 3 windows", flatten(fused), truth, rel=1e-9)


def test_variable_filters_and_one_metric_alone(dev):
    c = C.main()
    metrics = dict(annual=AnnualMetricConfig(variables=["t"]), seasonal=SeasonalMetricConfig(enabled=True, variables=["sst"]))
    fused = record(c, dev, True, metrics)
    got = flatten(fused)
    assert "annual/rmse/t" in got and "annual/rmse/sst" not in got and "seasonal/bias/sst" in got and "seasonal/bias/t" not in got
    compare("filters vs contract", got, flatten(twin(c, metrics)), rel=1e-9)
    for alone in (dict(seasonal=SeasonalMetricConfig(enabled=True)), dict(enso_index=EnsoIndexMetricConfig())):      # bins alone, series alone
        compare(f"{list(alone)[0]} alone", flatten(record(c, dev, True, alone)), flatten(twin(c, alone)), rel=1e-9)


def test_all_four_metrics_in_one_call_on_the_long_record(dev):
    c = C.long()
    metrics = four()
    fused, torch_ = record(c, dev, True, metrics), record(c, dev, False, metrics)
    assert fused.calendar_launches() == 2 and [m.name for m in fused._calendar.on()] == ["seasonal", "annual", "enso_index", "ipo_index"]
    got, truth = flatten(fused), flatten(twin(c, metrics))
    assert got["dataset:ipo_index/sst"].shape == (2, C.B, 984) and got["ipo_index/sst_ipo_tpi_filtered"].shape == (2, C.B, 984 - 312)
    assert got["dataset:annual/year"].tolist() == list(range(1901, 1983)) and 0 < got["ipo_index/sst_ipo_tpi_std_norm"] < 2
    compare("all four vs contract", got, truth, rel=1e-9)
    compare("all four vs torch", got, flatten(torch_), floors=truth, low=flatten(record(c, torch.device("cpu"), False, metrics)))


def test_the_initial_condition_stays_out_and_two_runs_are_bitwise_equal(dev):
    c = C.main()
    metrics = four(ipo_index=IpoIndexMetricConfig(enabled=False))
    runs = []
    for _ in range(2):
        agg = config(**metrics).build(c["info"], 1, c["n_time"] - 1, normalize=lambda d: d)
        agg.record_initial_condition(on(dev, {n: v[:, :1] for n, v in c["gen"].items()}), on(dev, {n: v[:, :1] for n, v in c["target"].items()}))
        agg.record_batch(on(dev, {n: v[:, 1:] for n, v in c["gen"].items()}), on(dev, {n: v[:, 1:] for n, v in c["target"].items()}),
                         time=c["time"][:, 1:])
        assert agg._path == "fused" and agg.calendar_launches() == 1
        runs.append((agg._calendar._bins.cpu(), agg._calendar._series.cpu()))
    series = runs[0][1]
    row = agg._calendar._srows[("globe", "t")]
    assert bool(series[:, :, :, 0].isnan().all()) and not bool(series[:, row, :, 1:].isnan().any())     # time level 0: never assigned
    assert sum(agg._calendar._season_counts) == C.B * (c["n_time"] - 1)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
