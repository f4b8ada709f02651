"""The evaluator's seasonal, annual, enso_index and ipo_index metrics on the torch path (ace_amd/evaluator.py ``_Calendar``) against
tests/golden/gen_calendar.pt, which the reference's own functions produced on the records of tests/_calendar_cases.py
(tests/golden/make_golden_calendar.py), and the build rules of the four configurations.

Bars.  The golden holds every quantity twice: "f32", the reference's functions in the reference's dtypes, and "f64", the same
functions on fp64 inputs.  The torch path is held to the fp64 numbers within 4 x the gap between the two, per quantity (the anomaly
step cancels values near 300 K, so the fp32 error is far above one rounding of the result and depends on the order of the sums).
One quantity has gap 0: the annual CRPS of "t", whose fp32 and fp64 yearly means happen to round to the same fp32 numbers before
``get_crps``.  A bar of 0 would ask for bitwise equality of a number formed from fp32 sums; it is held instead to 4 x the measured
gap of the annual RMSE of the same name (1.6e-5: the same yearly series, the same kind of distance between them).
Measured gaps on this fixture (max |f32 - f64| per quantity; magnitude in brackets):
  main (noleap, 5-day step, 249 steps)
    annual series t          5.8e-5 [296]     annual rmse t       1.6e-5 [0.051]    annual crps t          0 [0.059]
    nino34 index             1.9e-5 [0.89]    index std           2.4e-7 [0.40]     index std_norm         1.1e-6 [0.76]
    power spectrum           9.2e-4 [202]     power 1-16 yr       4.6e-5 [18.3]     power 1-16 yr norm     9.5e-7 [0.57]
    power 2-5 yr             NaN on both (43 months resolve one bin of that band)
    seasonal anomaly         7.4e-5 [2.4]     seasonal bias       1.1e-4 [0.50]     seasonal r2 t          7.7e-7 [0.93]
    seasonal rmse t          1.6e-6 [0.19]    per-season rmse t   4.0e-6 [0.20]
  long (360_day, 30-day step, 984 steps)
    tripole index            8.5e-5 [1.1]     filtered index      1.8e-5 [0.24]     filtered std           4.5e-8 [0.076]
    filtered std_norm        6.6e-7 [0.70]    power spectrum      1.6e-1 [2.9e4]
"sst" has NaN over a land patch and no mask: its area means, and so its annual and seasonal scalars, are NaN on both sides, which
is checked; the patch reaches into the T1 box, which the NaN-excluding mean of the tripole index leaves out."""
import datetime
import math
import os

import pytest
import torch

import _calendar_cases as C
from ace_amd.dataset_info import DatasetInfo
from ace_amd.evaluator import AnnualMetricConfig, EnsoIndexMetricConfig, InferenceEvaluatorAggregatorConfig, IpoIndexMetricConfig, \
    MetricConfig, PowerSpectrumMetricConfig, SeasonalMetricConfig, ZonalMeanMetricConfig

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_calendar.pt")
DAY = datetime.timedelta(days=1)


def config(**metrics):
    """every metric off but the given ones"""
    off = lambda: MetricConfig(enabled=False)                                  # noqa: E731
    base = dict(mean_denorm=off(), mean_norm=off(), step_means=[], ensembles=[], power_spectrum=PowerSpectrumMetricConfig(enabled=False),
                zonal_mean=ZonalMeanMetricConfig(enabled=False), time_mean_denorm=off(), time_mean_norm=off(), annual=off(),
                enso_index=off(), enso_coefficient=off(), ipo_index=off())
    base.update(metrics)
    return InferenceEvaluatorAggregatorConfig(**base)


def build(cfg, info, n_forward, n_ic=0):
    agg = cfg.build(info, n_ic, n_forward, normalize=lambda d: d)
    agg.fused = False
    return agg


def run(c, **metrics):
    agg = build(config(**metrics), c["info"], c["n_time"])
    for (gen, tgt), time in c["windows"]:
        assert agg.record_batch(gen, tgt, time=time) == []
    return agg


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


@pytest.fixture(scope="module")
def main_run():
    c = C.main()
    agg = run(c, seasonal=SeasonalMetricConfig(enabled=True), annual=AnnualMetricConfig(), enso_index=EnsoIndexMetricConfig())
    return c, agg, agg.get_dataset(), agg.get_summary_logs()


def close(name, got, f32, f64, gap=None):
    """|got - f64| <= 4 x |f32 - f64| (``gap``: another quantity's measured gap, for the one whose own is 0), NaN in the same
    places"""
    got, f32, f64 = (torch.as_tensor(v).double() for v in (got, f32, f64))
    assert got.shape == f64.shape, (name, got.shape, f64.shape)
    assert torch.equal(got.isnan(), f64.isnan()), name
    own = float((f32 - f64).abs().nan_to_num().max())
    err = float((got - f64).abs().nan_to_num().max())
    bar = 4 * (own if gap is None else gap)
    print(f"CALCPU {name}: err {err:.3e} gap {own:.3e} bar {bar:.3e}")
    assert err <= bar, (name, err, own, bar)


def same(a, b):
    return a.dtype == b.dtype and torch.allclose(a, b, rtol=0, atol=0, equal_nan=True)


def test_the_golden_was_made_on_these_records(golden):
    assert C.checksum(C.main()) == golden["main"]["checksum"] and C.checksum(C.long()) == golden["long"]["checksum"]


def test_annual_matches_the_reference(main_run, golden):
    c, agg, ds, logs = main_run
    g32, g64 = golden["main"]["f32"]["annual"], golden["main"]["f64"]["annual"]
    assert torch.equal(ds["annual"]["year"], g64["years"]) and ds["annual"]["year"].tolist() == [2001, 2002, 2003]
    for n in c["names"]:
        assert ds["annual"][n].dtype == torch.float32 and ds["annual"][n].shape == (2, C.B, 3)
        for i, side in enumerate(("target", "gen")):
            close(f"annual series {n} {side}", ds["annual"][n][i], g32["series"][n][side], g64["series"][n][side])
        assert same(logs[f"annual/{n}"], ds["annual"][n])
        close(f"annual rmse {n}", logs[f"annual/rmse/{n}"], g32["rmse"][n], g64["rmse"][n])
        rmse_gap = abs(g32["rmse"][n] - g64["rmse"][n]) if not math.isnan(g64["rmse"][n]) else 0.0
        close(f"annual crps {n}", logs[f"annual/crps/{n}"], g32["crps"][n], g64["crps"][n], gap=rmse_gap)
    t = ds["annual"]["t"]
    assert bool(t[:, 1, 0].isnan().all()) and not bool(t[:, 0].isnan().any())        # sample 1 starts 40 days in: 65 steps of 2001
    assert math.isnan(logs["annual/rmse/sst"]) and logs["annual/rmse/t"] > 0
    assert not any(k.startswith("annual/r2") for k in logs)                             # needs reference data: not emitted


def test_annual_report_flags_and_the_variable_filter():
    c = C.main(cuts=(100,))
    logs = run(c, annual=AnnualMetricConfig(variables=["t"], report_crps=False)).get_summary_logs()
    assert "annual/rmse/t" in logs and "annual/crps/t" not in logs and not any(k.endswith("/sst") for k in logs)
    logs = run(c, annual=AnnualMetricConfig(report_rmse=False, name="yearly")).get_summary_logs()
    assert "yearly/crps/t" in logs and "yearly/rmse/t" not in logs and "yearly/sst" in logs


def test_enso_index_matches_the_reference(main_run, golden):
    c, agg, ds, logs = main_run
    g32, g64 = golden["main"]["f32"]["enso"], golden["main"]["f64"]["enso"]
    d = ds["enso_index"]
    assert sorted(d) == ["month", "sst", "year"] and torch.equal(d["year"], g64["years"]) and torch.equal(d["month"], g64["months"])
    for i, side in enumerate(("target", "gen")):
        close(f"nino34 index {side}", d["sst"][i], g32["index"][side], g64["index"][side])
    assert bool(d["sst"][:, :, :4].isnan().all()) and not bool(d["sst"][:, :, 4:].isnan().any())       # the 5-month running mean
    p = "enso_index/sst_nino34_index"
    assert same(logs[p], d["sst"])
    for k in ("std", "std_norm", "power_1_16yr", "power_1_16yr_norm"):
        close(f"nino34 {k}", logs[f"{p}_{k}"], g32[k], g64[k])
    assert math.isnan(logs[f"{p}_power_2_5yr"]) and math.isnan(g64["power_2_5yr"]) and f"{p}_power_2_5yr_norm" not in logs
    assert torch.equal(logs[f"{p}_power_spectrum"][0], g64["freq"])
    close("nino34 power", logs[f"{p}_power_spectrum"][1], g32["power"], g64["power"])
    close("nino34 power of the target", logs[f"{p}_power_spectrum_target"][1], g32["power_target"], g64["power_target"])


def test_seasonal_matches_the_reference(main_run, golden):
    c, agg, ds, logs = main_run
    g32, g64 = golden["main"]["f32"]["seasonal"], golden["main"]["f64"]["seasonal"]
    assert "seasonal" not in ds                                                          # seasonal.py:177-182: no dataset
    assert agg._calendar._season_counts == g64["counts"].tolist() and min(agg._calendar._season_counts) > 0
    for n in c["names"]:
        assert logs[f"seasonal/anomaly/{n}"].shape == (2, 4, C.H, C.W) and logs[f"seasonal/bias/{n}"].shape == (4, C.H, C.W)
        assert logs[f"seasonal/anomaly/{n}"].dtype == torch.float64                      # fp32 sums over fp64 counts
        close(f"seasonal anomaly {n}", logs[f"seasonal/anomaly/{n}"], g32["anomaly"][n], g64["anomaly"][n])
        close(f"seasonal bias {n}", logs[f"seasonal/bias/{n}"], g32["bias"][n], g64["bias"][n])
        close(f"seasonal r2 {n}", logs[f"seasonal/r2/{n}"], g32["r2"][n], g64["r2"][n])
        close(f"seasonal rmse {n}", logs[f"seasonal/time-mean-rmse/{n}"], g32["rmse"][n], g64["rmse"][n])
        per = torch.tensor([logs[f"seasonal/time-mean-rmse/{n}-{s}"] for s in ("DJF", "MAM", "JJA", "SON")])
        close(f"seasonal rmse per season {n}", per, g32["rmse_season"][n], g64["rmse_season"][n])
    land = logs["seasonal/bias/sst"][:, C.LAND[0], C.LAND[1]]
    assert bool(land.isnan().all()) and int(logs["seasonal/bias/sst"].isnan().sum()) == land.numel()
    assert math.isnan(logs["seasonal/time-mean-rmse/sst"]) and 0.9 < logs["seasonal/r2/t"] < 1


def test_seasonal_needs_all_four_seasons_and_honours_its_filter():
    c = C.main()
    agg = build(config(seasonal=SeasonalMetricConfig(enabled=True, variables=["t"])), c["info"], c["n_time"])
    (gen, tgt), time = c["windows"][0]
    agg.record_batch({n: v[:, :30] for n, v in gen.items()}, {n: v[:, :30] for n, v in tgt.items()}, time=time[:, :30])      # 150 days
    assert not any(k.startswith("seasonal/") for k in agg.get_summary_logs())
    agg.record_batch({n: v[:, 30:] for n, v in gen.items()}, {n: v[:, 30:] for n, v in tgt.items()}, time=time[:, 30:])
    logs = agg.get_summary_logs()
    assert "seasonal/bias/t" in logs and "seasonal/bias/sst" not in logs


def test_the_split_into_windows_does_not_matter(main_run):
    c, _, ds, logs = main_run
    other = run(C.main(cuts=(40,)), seasonal=SeasonalMetricConfig(enabled=True), annual=AnnualMetricConfig(),
                enso_index=EnsoIndexMetricConfig())
    ods, ologs = other.get_dataset(), other.get_summary_logs()
    assert torch.allclose(ods["annual"]["t"], ds["annual"]["t"], rtol=1e-6, atol=0, equal_nan=True)
    assert torch.allclose(ods["enso_index"]["sst"], ds["enso_index"]["sst"], rtol=0, atol=1e-4, equal_nan=True)
    assert torch.allclose(ologs["seasonal/bias/t"], logs["seasonal/bias/t"], rtol=0, atol=5e-4)


def test_the_initial_condition_stays_out():
    """main.py:660-661: the initial condition goes to the time series only; the calendar metrics see record_batch's steps"""
    c = C.main()
    agg = build(config(annual=AnnualMetricConfig(), seasonal=SeasonalMetricConfig(enabled=True)), c["info"], c["n_time"] - 1, n_ic=1)
    agg.record_initial_condition({n: v[:, :1] for n, v in c["gen"].items()}, {n: v[:, :1] for n, v in c["target"].items()})
    agg.record_batch({n: v[:, 1:] for n, v in c["gen"].items()}, {n: v[:, 1:] for n, v in c["target"].items()}, time=c["time"][:, 1:])
    assert sum(agg._calendar._season_counts) == C.B * (c["n_time"] - 1) and agg._calendar._seen[0] is False
    assert agg.get_dataset()["annual"]["year"].tolist() == [2001, 2002, 2003]            # 72 of sample 0's 73 steps of 2001: kept


def test_ipo_index_matches_the_reference(golden):
    c = C.long()
    agg = run(c, ipo_index=IpoIndexMetricConfig(), enso_index=EnsoIndexMetricConfig())
    ds, logs = agg.get_dataset(), agg.get_summary_logs()
    g32, g64 = golden["long"]["f32"], golden["long"]["f64"]
    assert ds["ipo_index"]["sst"].shape == (2, C.B, 984) and ds["ipo_index"]["month"][:13].tolist() == list(range(1, 13)) + [1]
    for i, side in enumerate(("target", "gen")):
        close(f"tripole index {side}", ds["ipo_index"]["sst"][i], g32["ipo"]["tpi"][side], g64["ipo"]["tpi"][side])
        close(f"filtered tripole index {side}", logs["ipo_index/sst_ipo_tpi_filtered"][i], g32["ipo"]["filtered"][side],
              g64["ipo"]["filtered"][side])
        close(f"nino34 index {side} (long)", ds["enso_index"]["sst"][i], g32["enso"]["index"][side], g64["enso"]["index"][side])
    assert logs["ipo_index/sst_ipo_tpi_filtered"].shape == (2, C.B, 984 - 2 * 156)
    close("filtered std", logs["ipo_index/sst_ipo_tpi_std"], g32["ipo"]["std"], g64["ipo"]["std"])
    close("filtered std_norm", logs["ipo_index/sst_ipo_tpi_std_norm"], g32["ipo"]["std_norm"], g64["ipo"]["std_norm"])
    assert torch.equal(logs["ipo_index/sst_ipo_tpi_power_spectrum"][0], g64["ipo"]["freq"])
    close("tripole power", logs["ipo_index/sst_ipo_tpi_power_spectrum"][1], g32["ipo"]["power"], g64["ipo"]["power"])
    close("tripole power of the target", logs["ipo_index/sst_ipo_tpi_power_spectrum_target"][1], g32["ipo"]["power_target"],
          g64["ipo"]["power_target"])
    for k in ("power_2_5yr", "power_2_5yr_norm", "power_1_16yr", "power_1_16yr_norm"):                 # 82 years resolve both bands
        close(f"nino34 {k} (long)", logs[f"enso_index/sst_nino34_index_{k}"], g32["enso"][k], g64["enso"][k])


def test_a_short_tripole_record_emits_the_index_only():
    """ipo_index.py:300-312: under 80 years of months no filtered scalars and no spectrum; the monthly index is still a dataset"""
    from ace_amd.evaluator import _Calendar
    c = C.main()
    agg = build(config(), c["info"], c["n_time"])
    agg._families.append(_Calendar(agg, {"ipo_index": IpoIndexMetricConfig()}, c["info"]))    # the build rule would leave it out
    for (gen, tgt), time in c["windows"]:
        agg.record_batch(gen, tgt, time=time)
    g = torch.load(GOLDEN, weights_only=False)["main"]
    for i, side in enumerate(("target", "gen")):
        close(f"short tripole index {side}", agg.get_dataset()["ipo_index"]["sst"][i], g["f32"]["ipo"]["tpi"][side], g["f64"]["ipo"]["tpi"][side])
    assert not any(k.startswith("ipo_index/") for k in agg.get_summary_logs())


# ---- the build rules ------------------------------------------------------------------------------------------------------------
def info(timestep, lat=True, lon=True):
    if lat and lon:
        return C.info(timestep)
    return DatasetInfo((C.H, C.W), timestep=timestep, area_weights=C.info(timestep).area_weights)


def test_defaults_are_the_typed_configurations():
    cfg = InferenceEvaluatorAggregatorConfig()
    assert isinstance(cfg.annual, AnnualMetricConfig) and isinstance(cfg.enso_index, EnsoIndexMetricConfig)
    assert isinstance(cfg.ipo_index, IpoIndexMetricConfig) and isinstance(cfg.seasonal, SeasonalMetricConfig)
    a, e, i, s = cfg.annual, cfg.enso_index, cfg.ipo_index, cfg.seasonal
    assert (a.variables, a.name, a.reference_data, a.enabled, a.strict, a.report_crps, a.report_rmse) == \
        (None, "annual", None, True, False, True, True)
    assert (e.name, e.enabled, e.strict) == ("enso_index", True, False) and (i.name, i.enabled, i.strict) == ("ipo_index", True, False)
    assert (s.variables, s.name, s.enabled, s.strict) == (None, "seasonal", False, True)


def test_a_default_build_on_a_long_record_builds_annual_and_enso_index(caplog):
    with caplog.at_level("WARNING"):
        agg = InferenceEvaluatorAggregatorConfig(power_spectrum=PowerSpectrumMetricConfig(enabled=False)).build(
            C.info(5 * DAY), 1, 248, normalize=lambda d: d)
    assert agg.skipped == ["step_means", "ensembles", "enso_coefficient", "ipo_index"]
    assert agg.uses_time and not agg.needs_time                                          # non-strict: taken when given
    assert [m.name for m in agg._calendar.on()] == ["annual", "enso_index"]
    long = InferenceEvaluatorAggregatorConfig(power_spectrum=PowerSpectrumMetricConfig(enabled=False)).build(
        C.info(30 * DAY), 1, 983, normalize=lambda d: d)
    assert long.skipped == ["step_means", "ensembles", "enso_coefficient"] and len(long._calendar.on()) == 3


@pytest.mark.parametrize("field,typed,days_short,days_long", [
    ("annual", AnnualMetricConfig, 730, 735), ("enso_index", EnsoIndexMetricConfig, 730, 735),
    ("ipo_index", IpoIndexMetricConfig, 80 * 365, 80 * 365 + 5)])
def test_the_duration_thresholds(field, typed, days_short, days_long, caplog):
    short, enough = days_short // 5, days_long // 5                                      # time levels at a 5-day step
    with caplog.at_level("WARNING"):
        agg = build(config(**{field: typed()}), C.info(5 * DAY), short - 1, n_ic=1)
    assert agg.skipped == [field] and agg._calendar is None and not agg.uses_time and field in caplog.text
    with pytest.raises(NotImplementedError, match=f"{field} metric is not supported.*years of data"):
        build(config(**{field: typed(strict=True)}), C.info(5 * DAY), short - 1, n_ic=1)
    agg = build(config(**{field: typed(strict=True)}), C.info(5 * DAY), enough - 1, n_ic=1)
    assert agg.skipped == [] and agg.needs_time and [m.name for m in agg._calendar.on()] == [field]


def test_bare_metric_configs_behave_as_before(caplog):
    """a bare MetricConfig in one of the four fields: skipped with the warning, raised when strict, seasonal "not built" """
    i = C.info(5 * DAY)
    with caplog.at_level("WARNING"):
        agg = build(config(annual=MetricConfig(), enso_index=MetricConfig(), ipo_index=MetricConfig()), i, 7999, n_ic=1)
    assert agg.skipped == ["annual", "enso_index", "ipo_index"] and agg._calendar is None and not agg.uses_time
    assert "omitting: annual, enso_index, ipo_index" in caplog.text
    for field in ("annual", "enso_index", "ipo_index"):
        with pytest.raises(NotImplementedError, match=f"the {field} metric is not built"):
            build(config(**{field: MetricConfig(strict=True)}), i, 7999, n_ic=1)
    with pytest.raises(NotImplementedError, match="the seasonal metric is not built"):
        build(config(seasonal=MetricConfig(enabled=True)), i, 10)
    assert build(config(seasonal=MetricConfig(enabled=False)), i, 10)._calendar is None
    agg = build(config(seasonal=SeasonalMetricConfig(enabled=True)), i, 10)              # the typed one builds, whatever the length
    assert agg.needs_time and agg.skipped == []


def test_reference_data_is_refused():
    with pytest.raises(NotImplementedError, match="netCDF"):
        build(config(annual=AnnualMetricConfig(reference_data="monthly.nc")), C.info(5 * DAY), 248)
    build(config(annual=AnnualMetricConfig(enabled=False, reference_data="monthly.nc")), C.info(5 * DAY), 248)


def test_a_grid_without_lat_lon_keeps_annual_and_skips_the_indices(caplog):
    plain = info(30 * DAY, lon=False)
    assert plain.horizontal_coordinates is None
    with caplog.at_level("WARNING"):
        agg = build(config(annual=AnnualMetricConfig(), enso_index=EnsoIndexMetricConfig(), ipo_index=IpoIndexMetricConfig()), plain, 984)
    assert agg.skipped == ["enso_index", "ipo_index"] and [m.name for m in agg._calendar.on()] == ["annual"]
    with pytest.raises(NotImplementedError, match="enso_index metric is not supported.*lat-lon"):
        build(config(enso_index=EnsoIndexMetricConfig(strict=True)), plain, 984)


def test_ipo_index_without_scipy_is_skipped(monkeypatch):
    import builtins
    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.split(".")[0] == "scipy":
            raise ImportError("no scipy here")
        return real(name, *a, **k)

    monkeypatch.setattr(builtins, "__import__", no_scipy)
    agg = build(config(ipo_index=IpoIndexMetricConfig()), C.info(30 * DAY), 984)
    assert agg.skipped == ["ipo_index"] and agg._calendar is None
    with pytest.raises(NotImplementedError, match="scipy"):
        build(config(ipo_index=IpoIndexMetricConfig(strict=True)), C.info(30 * DAY), 984)


def test_recording_without_a_time_axis(caplog):
    c = C.main()
    (gen, tgt), time = c["windows"][0]
    agg = build(config(annual=AnnualMetricConfig(), enso_index=EnsoIndexMetricConfig()), c["info"], c["n_time"])
    with caplog.at_level("WARNING"):
        agg.record_batch(gen, tgt)                                                       # non-strict: dropped, as at build time
    assert agg.skipped == ["annual", "enso_index"] and not agg.uses_time and "annual, enso_index" in caplog.text
    assert "annual" not in agg.get_dataset()
    strict = build(config(seasonal=SeasonalMetricConfig(enabled=True)), c["info"], c["n_time"])
    with pytest.raises(ValueError, match="seasonal.*time axis"):
        strict.record_batch(gen, tgt)
    late = build(config(annual=AnnualMetricConfig()), c["info"], c["n_time"])
    late.record_batch(gen, tgt, time=time)
    with pytest.raises(ValueError, match="time axis"):
        late.record_batch(gen, tgt)
    with pytest.raises(ValueError, match="samples, steps"):
        build(config(annual=AnnualMetricConfig()), c["info"], c["n_time"]).record_batch(gen, tgt, time=time[:, :5])


def test_run_evaluator_hands_the_time_axis_over_when_the_windows_have_one():
    """a non-strict calendar metric makes ``uses_time`` true, not ``needs_time``: windows with a time axis feed it, windows without
    one drop it with the warning instead of raising"""
    from ace_amd.inference import ForcingWindows, InferenceData, run_evaluator
    c = C.main()
    n = c["n_time"] - 1

    def predict(state, win):                                                  # the prediction: 1.01 x the window's own target
        out = {k: 1.01 * win[k][:, 1:] for k in c["names"]}
        return out, {k: v[:, -1] for k, v in out.items()}

    def data(time):
        return InferenceData({k: v[:, 0] for k, v in c["target"].items()},
                             ForcingWindows(c["target"], total_forward_steps=n, forward_steps_in_memory=62, device="cpu", time=time))
    agg = build(config(annual=AnnualMetricConfig()), c["info"], n, n_ic=1)
    assert agg.uses_time and not agg.needs_time
    run_evaluator(predict, data(c["time"]), agg)
    series = agg.get_dataset()["annual"]["t"]
    assert agg.skipped == [] and torch.allclose(series[1, 0], 1.01 * series[0, 0], rtol=1e-6)
    agg = build(config(annual=AnnualMetricConfig()), c["info"], n, n_ic=1)
    run_evaluator(predict, data(None), agg)
    assert agg.skipped == ["annual"] and "annual" not in agg.get_dataset()
    strict = build(config(seasonal=SeasonalMetricConfig(enabled=True)), c["info"], n, n_ic=1)
    with pytest.raises(ValueError, match="time"):
        run_evaluator(predict, data(None), strict)
