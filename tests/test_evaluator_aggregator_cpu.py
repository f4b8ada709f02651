"""ace_amd.evaluator on its torch path (CPU, fp32) against an fp64 restatement of the reference's InferenceEvaluatorAggregator
(fme/ace/aggregator/inference: main.py:526-732, reduced.py:221-348, time_mean.py:246-444, spectrum.py:112-276,
zonal_mean.py:50-355; fme/core/metrics.py:63-224), on the small masked case of test_aggregator_cpu.py: an 8 x 16 grid, "sst" NaN on
land, a surface-pressure-like "ps", a prediction-only "diag", uneven windows and an initial condition.

Tolerances are those of the project's aggregator tests: 1e-6 relative for means and linear quantities, 1e-5 for std-like ones
(std, rmse, the gradient score, spectra 1e-4 as in test_aggregator_cpu.py).  Two scales are explicit: a difference (bias, percent
diff, error maps) is judged against the scale of its minuend, and a normalised quantity on this fp32 path against
(scale + |mu|) / sigma, because normalising in fp32 cancels there."""
import math

import pytest
import torch

from ace_amd.evaluator import (InferenceEvaluatorAggregatorConfig, MetricConfig, PowerSpectrumMetricConfig, ZonalMeanMetricConfig,
                               zonal_coarsening)
from ace_amd.inference import InferenceData, run_evaluator
from ace_amd.normalizer import StandardNormalizer
from oracle.sht import RealSHT as OracleSHT

from test_aggregator_cpu import B, H, W, WINDOWS, _HpxCoords, _Info, make_case, oracle_sht_factory, weights64

STATS = {"a": (0.1, 1.3), "ps": (1e5, 2e2), "sst": (288.0, 6.0)}         # "diag" has no statistics: normalize drops it
PAIRED = ("a", "ps", "sst")
N_TIME = 1 + sum(WINDOWS)


def normalizer():
    return StandardNormalizer({k: v[0] for k, v in STATS.items()}, {k: v[1] for k, v in STATS.items()}, device="cpu")


def targets(wins, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [{n: x + (0.05 * STATS[n][1]) * torch.randn(x.shape, generator=g) for n, x in win.items() if n in PAIRED} for win in wins]


def case(seed=0, windows=WINDOWS):
    info, ic, wins = make_case(seed=seed, windows=windows)
    return info, ic, wins, targets(wins)


# ---- the fp64 restatement ---------------------------------------------------------------------------------------------------
def wmean(x, w):
    return (x.where(w != 0, 0.0) * w).sum((-2, -1)) / w.sum()


def wnanmean(g, w):
    return (g * w).nansum((-2, -1)) / torch.where(torch.isnan(g), 0.0, w.expand(g.shape)).sum((-2, -1))


def gradmag(x):
    gy, gx = torch.gradient(x, dim=(-2, -1))
    return torch.sqrt(gy ** 2 + gx ** 2)


def norm64(d):
    return {n: (x.double() - STATS[n][0]) / STATS[n][1] for n, x in d.items() if n in STATS}


def expected_series(info, recs, kind):
    """reduced.py:221-316: metric -> name -> (N_TIME,), and the |x|-scale of each name (for differences)"""
    out, scale = {}, {}
    for t0, gen, tgt in recs:
        gen, tgt = ({k: v.double() for k, v in gen.items()}, {k: v.double() for k, v in tgt.items()}) if kind == "denorm" else \
            (norm64(gen), norm64(tgt))
        T = next(iter(gen.values())).shape[1]

        def add(metric, n, v):
            out.setdefault(metric, {}).setdefault(n, torch.zeros(N_TIME, dtype=torch.float64))[t0:t0 + T] += v.mean(0)
        for n, x in gen.items():
            w = weights64(info, n)
            m = wmean(x, w)
            add("weighted_mean_gen", n, m)
            add("weighted_std_gen", n, wmean((x - m[..., None, None]) ** 2, w).sqrt())
            scale[n] = max(scale.get(n, 0.0), float(wmean(x.abs(), w).max()))
        for n, y in tgt.items():
            x, w = gen[n], weights64(info, n)
            add("weighted_mean_target", n, wmean(y, w))
            add("weighted_bias", n, wmean(x - y, w))
            add("weighted_rmse", n, wmean((x - y) ** 2, w).sqrt())
            if kind == "denorm":
                gt, gg = wnanmean(gradmag(y), w), wnanmean(gradmag(x), w)
                add("weighted_grad_mag_percent_diff", n, 100 * (gg - gt) / gt)
    return out, scale                       # one record per time index: the counts are all 1


def expected_time_means(recs):
    """time_mean.py:103-162 for both sides, denormalised fp64: name -> (gen, target or None)"""
    sums, steps = [{}, {}], 0
    for t0, gen, tgt in recs:
        part = slice(1, None) if t0 == 0 else slice(0, None)
        for side, d in enumerate((gen, tgt)):
            for n, x in d.items():
                sums[side][n] = sums[side].get(n, 0) + x[:, part].double().sum((0, 1))
        T = next(iter(gen.values())).shape[1]
        steps = T - 1 if t0 == 0 else steps + T
    return {n: (v / steps / B, sums[1][n] / steps / B if n in sums[1] else None) for n, v in sums[0].items()}


def expected_spectra(info, recs):
    sht = OracleSHT(H, W, grid="legendre-gauss", dtype=torch.float64)
    tot, cnt = [{}, {}], [{}, {}]
    for _, gen, tgt in recs:
        for side, d in enumerate((gen, tgt)):
            for n, x in d.items():
                if n == "sst":
                    continue
                c = sht(x.double())
                tot[side][n] = tot[side].get(n, 0) + (c.real ** 2 + c.imag ** 2).sum(-1).sum((0, 1))
                cnt[side][n] = cnt[side].get(n, 0) + x.shape[0] * x.shape[1]
    return [{n: v / cnt[s][n] for n, v in tot[s].items()} for s in (0, 1)]


def expected_zonal(recs, n_timesteps, max_size):
    """zonal_mean.py:89-127, 153-306: the reference's buffer-carry algorithm, fp64"""
    max_size = min(max_size, n_timesteps)
    factor = int(math.ceil(n_timesteps / max_size)) if n_timesteps > max_size else 1
    n_slots = n_timesteps // factor if n_timesteps > max_size else n_timesteps
    acc, buf, count = [None, None], [None, None], torch.zeros(n_slots)
    offset, last_step = None, 0
    for t0, gen, tgt in recs:
        if acc[0] is None:
            acc = [{n: torch.zeros(B, n_slots, H, dtype=torch.float64) for n in d} for d in (gen, tgt)]
        if offset is None:
            offset = t0
        i0, T = t0 - offset, next(iter(tgt.values())).shape[1]
        if T < factor:
            continue
        start = last_step if buf[0] else i0 // factor
        sl = slice(start, (i0 + T) // factor)
        last_step = (i0 + T) // factor
        rest = (i0 + T) - last_step * factor
        n_coarse = (sl.stop - sl.start) * factor
        for side, d in enumerate((gen, tgt)):
            new = {}
            for n, x in d.items():
                if n not in acc[side]:
                    continue
                zm = x.double().nanmean(-1)
                if buf[side] is not None and n in buf[side]:
                    zm = torch.cat([buf[side][n], zm], dim=1)
                acc[side][n][:, sl] += zm[:, :n_coarse].unfold(1, factor, factor).mean(-1)
                if rest > 0:
                    new[n] = zm[:, n_coarse:n_coarse + rest]
            buf[side] = new
        count[sl] += 1
    out = {}
    for n in sorted(acc[0]):
        if n in acc[1]:
            g, t = ((acc[s][n] / count[None, :, None]).mean(0) for s in (0, 1))
            out[n] = (g, t)
    return factor, n_slots, out


def records(ic, wins, tgts, with_ic=True):
    recs, t = ([(0, ic, ic)] if with_ic else []), (1 if with_ic else 0)
    for win, tgt in zip(wins, tgts):
        recs.append((t, win, tgt))
        t += next(iter(win.values())).shape[1]
    return recs


def run(info, ic, wins, tgts, config=None, normalize="default", **kw):
    config = config or InferenceEvaluatorAggregatorConfig()
    agg = config.build(info, 1, N_TIME - 1, normalize=normalizer() if normalize == "default" else normalize,
                       sht_factory=oracle_sht_factory, **kw)
    agg.fused = False
    assert agg.record_initial_condition(ic) == []
    for win, tgt in zip(wins, tgts):
        assert agg.route(win, tgt) == "torch"
        assert agg.record_batch(win, tgt) == []
    return agg


def close(got, want, tol, scale):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert got.shape == want.shape
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    return float((got[ok] - want[ok]).abs().max()) <= tol * scale if bool(ok.any()) else True


STD_LIKE = ("weighted_std_gen", "weighted_rmse", "weighted_grad_mag_percent_diff")


# ---- tests --------------------------------------------------------------------------------------------------------------
def test_every_dataset_key_matches_the_fp64_reference():
    info, ic, wins, tgts = case()
    agg = run(info, ic, wins, tgts)
    ds = agg.get_dataset()
    assert set(ds) == {"mean", "mean_norm", "time_mean", "time_mean_norm", "power_spectrum", "zonal_mean"}
    recs = records(ic, wins, tgts)
    checked = set()
    for kind, label in (("denorm", "mean"), ("norm", "mean_norm")):
        want, scale = expected_series(info, recs, kind)
        assert set(ds[label]) == {f"{m}-{n}" for m, d in want.items() for n in d}
        for m, d in want.items():
            for n, v in d.items():
                tol = 1e-5 if m in STD_LIKE else 1e-6
                s = float(v.abs().max())
                if m in ("weighted_bias", "weighted_grad_mag_percent_diff"):        # differences: the scale of the minuend
                    s = scale[n] if m == "weighted_bias" else 100.0 * (1 + s / 100.0)
                if kind == "norm":                                                  # fp32 normalisation cancels |mu|
                    _, raw = expected_series(info, recs, "denorm")
                    s = max(s, (raw[n] + abs(STATS[n][0])) / STATS[n][1])
                assert close(ds[label][f"{m}-{n}"], v, tol, s), (label, m, n)
                checked.add((label, f"{m}-{n}"))
    assert "weighted_grad_mag_percent_diff-a" in ds["mean"] and "weighted_grad_mag_percent_diff-a" not in ds["mean_norm"]
    assert "weighted_mean_gen-diag" in ds["mean"] and "weighted_mean_gen-diag" not in ds["mean_norm"]
    assert "weighted_rmse-diag" not in ds["mean"]
    tm = expected_time_means(recs[1:])
    for label, norm in (("time_mean", False), ("time_mean_norm", True)):
        names = [n for n in PAIRED]
        assert set(ds[label]) == {f"{k}-{n}" for n in names for k in ("bias_map", "gen_map")}
        for n in names:
            g, t = tm[n]
            mu, sigma = STATS[n] if norm else (0.0, 1.0)
            scale = (float(g.nan_to_num(0.0).abs().max()) + abs(mu)) / sigma
            assert close(ds[label][f"gen_map-{n}"], (g - mu) / sigma, 1e-6, scale), (label, n)
            assert close(ds[label][f"bias_map-{n}"], (g - t) / sigma, 1e-6, scale), (label, n)
            checked.update({(label, f"gen_map-{n}"), (label, f"bias_map-{n}")})
        assert bool(torch.isnan(ds[label]["gen_map-sst"]).any()) and not bool(torch.isnan(ds[label]["gen_map-a"]).any())
    spec = expected_spectra(info, recs[1:])
    assert set(ds["power_spectrum"]) == {"a", "ps", "diag"} and agg.omitted == ["sst"]
    for n, got in ds["power_spectrum"].items():
        assert got.shape == (2, H)
        assert close(got[0], spec[0][n], 1e-4, float(spec[0][n].abs().max())), n
        if n in spec[1]:
            assert close(got[1], spec[1][n], 1e-4, float(spec[1][n].abs().max())), n
        else:
            assert bool(torch.isnan(got[1]).all())
        checked.add(("power_spectrum", n))
    factor, n_slots, zon = expected_zonal(recs[1:], N_TIME, 4096)
    assert (factor, n_slots) == (1, N_TIME) == zonal_coarsening(N_TIME, 4096)
    assert set(ds["zonal_mean"]) == {f"{k}-{n}" for n in PAIRED for k in ("gen", "error")}
    for n, (g, t) in zon.items():
        scale = float(g.nan_to_num(0.0).abs().max())
        assert close(ds["zonal_mean"][f"gen-{n}"], g, 1e-6, scale) and close(ds["zonal_mean"][f"error-{n}"], g - t, 1e-6, scale), n
        checked.update({("zonal_mean", f"gen-{n}"), ("zonal_mean", f"error-{n}")})
    assert bool(torch.isnan(ds["zonal_mean"]["gen-a"][-1]).all())                 # the slot nothing reached (the IC is not recorded)
    assert not bool(torch.isnan(ds["zonal_mean"]["gen-sst"][:-1]).any())          # a row that is partly land: the nan-mean of the rest
    assert checked == {(sub, k) for sub, d in ds.items() for k in d}


def test_summary_scalars_loss_and_spectrum_scores():
    info, ic, wins, tgts = case()
    agg = run(info, ic, wins, tgts)
    summary = agg.get_summary()
    logs = summary.logs
    recs = records(ic, wins, tgts)
    tm = expected_time_means(recs[1:])
    rmse_norm, tol_norm = {}, {}
    for n in PAIRED:
        g, t = tm[n]
        w = weights64(info, n)
        rmse = float(wmean((g - t) ** 2, w).sqrt())
        gscale = float(g.nan_to_num(0.0).abs().max())
        # the RMSE of the error map g - t: the fp32 maps carry 1e-6 of their own scale each, and so does their difference
        assert logs[f"time_mean/rmse/{n}"] == pytest.approx(rmse, abs=1e-5 * rmse + 1e-6 * gscale)
        assert logs[f"time_mean/bias/{n}"] == pytest.approx(float(wmean(g - t, w)), abs=1e-6 * gscale)
        rmse_norm[n] = rmse / STATS[n][1]
        tol_norm[n] = 1e-5 * rmse_norm[n] + 1e-6 * (gscale + abs(STATS[n][0])) / STATS[n][1]
        assert logs[f"time_mean_norm/rmse/{n}"] == pytest.approx(rmse_norm[n], abs=tol_norm[n])
        assert f"time_mean_norm/bias/{n}" not in logs and f"time_mean_norm/bias_map/{n}" not in logs
        assert logs[f"time_mean/bias_map/{n}"].shape == (H, W)
    assert "time_mean/gen_map/diag" in logs and "time_mean/rmse/diag" not in logs
    want = sum(rmse_norm.values()) / 3
    assert summary.loss == logs["time_mean_norm/rmse/channel_mean"]
    assert summary.loss == pytest.approx(want, abs=sum(tol_norm.values()) / 3)
    spec = expected_spectra(info, recs[1:])
    for n in ("a", "ps"):
        ratio = spec[0][n] / spec[1][n] - 1
        pos, neg = float(ratio[ratio > 0].sum() / H), float(ratio[ratio < 0].sum() / H)
        tol = 1e-4 * float((spec[0][n] / spec[1][n]).max())
        assert logs[f"power_spectrum/smallest_scale_norm_bias/{n}"] == pytest.approx(float(ratio[-1]), abs=tol)
        assert logs[f"power_spectrum/positive_norm_bias/{n}"] == pytest.approx(pos, abs=tol)
        assert logs[f"power_spectrum/negative_norm_bias/{n}"] == pytest.approx(neg, abs=tol)
        assert logs[f"power_spectrum/mean_abs_norm_bias/{n}"] == pytest.approx(abs(pos) + abs(neg), abs=2 * tol)
    assert "power_spectrum/mean_abs_norm_bias/diag" not in logs and logs["power_spectrum/diag"].shape == (2, H)
    assert logs["zonal_mean/gen/a"].shape == (2, N_TIME, H) and logs["zonal_mean/error/a"].shape == (N_TIME, H)


def test_channel_mean_names():
    info, ic, wins, tgts = case()
    one = run(info, ic, wins, tgts, channel_mean_names=["ps"]).get_summary()
    assert one.loss == one.logs["time_mean_norm/rmse/ps"]
    with pytest.raises(KeyError, match="channel_mean_names"):
        run(info, ic, wins, tgts, channel_mean_names=["ps", "nope"]).get_summary()
    nan_t = [{n: torch.full_like(y, float("nan")) for n, y in tgt.items()} for tgt in tgts]
    with pytest.raises(ValueError, match="All target variables are NaN"):
        run(info, ic, wins, nan_t).get_summary()
    partly = [{n: (torch.full_like(y, float("nan")) if n == "a" else y) for n, y in tgt.items()} for tgt in tgts]
    s = run(info, ic, wins, partly).get_summary()
    assert s.loss == pytest.approx((s.logs["time_mean_norm/rmse/ps"] + s.logs["time_mean_norm/rmse/sst"]) / 2, rel=1e-6)


def test_skipped_and_refused_metrics(caplog):
    info, _, _, _ = case()
    with caplog.at_level("WARNING"):
        agg = InferenceEvaluatorAggregatorConfig().build(info, 1, 6, normalize=normalizer())
    assert agg.skipped == ["step_means", "ensembles", "annual", "enso_index", "enso_coefficient", "ipo_index"]
    assert len([r for r in caplog.records if "omitting" in r.getMessage()]) == 1
    for field in ("video", "histogram", "seasonal", "trend", "near_zero_fraction"):
        with pytest.raises(NotImplementedError, match=field):
            InferenceEvaluatorAggregatorConfig(**{field: MetricConfig(enabled=True)}).build(info, 1, 6, normalize=normalizer())
    with pytest.raises(NotImplementedError, match="annual"):
        InferenceEvaluatorAggregatorConfig(annual=MetricConfig(strict=True)).build(info, 1, 6, normalize=normalizer())
    with pytest.raises(NotImplementedError, match="netCDF"):
        InferenceEvaluatorAggregatorConfig(time_mean_reference_data="m.nc").build(info, 1, 6, normalize=normalizer())
    with pytest.raises(NotImplementedError, match="netCDF"):
        InferenceEvaluatorAggregatorConfig(monthly_reference_data="m.nc").build(info, 1, 6, normalize=normalizer())
    with pytest.raises(NotImplementedError, match="HEALPix"):
        InferenceEvaluatorAggregatorConfig().build(_Info(torch.ones(H, W), _HpxCoords()), 1, 6, normalize=normalizer())
    with pytest.raises(ValueError, match="Output directory"):
        InferenceEvaluatorAggregatorConfig().build(info, 1, 6, normalize=normalizer(), save_diagnostics=True)
    quiet = InferenceEvaluatorAggregatorConfig(step_means=[], ensembles=[], annual=MetricConfig(enabled=False),
                                               enso_index=MetricConfig(enabled=False), enso_coefficient=MetricConfig(enabled=False),
                                               ipo_index=MetricConfig(enabled=False)).build(info, 1, 6, normalize=normalizer())
    assert quiet.skipped == []


def test_recording_refusals():
    info, ic, wins, tgts = case()
    agg = InferenceEvaluatorAggregatorConfig().build(info, 1, 6, normalize=normalizer(), sht_factory=oracle_sht_factory)
    agg.fused = False
    with pytest.raises(ValueError, match="No target"):
        agg.record_batch(wins[0], {})
    with pytest.raises(ValueError, match="No prediction"):
        agg.record_batch({}, tgts[0])
    with pytest.raises(ValueError, match="has no prediction"):
        agg.record_batch({"a": wins[0]["a"]}, {"ps": tgts[0]["ps"]})
    with pytest.raises(ValueError, match="initial condition steps"):
        agg.record_initial_condition({k: torch.cat([v, v], dim=1) for k, v in ic.items()})
    agg.record_initial_condition(ic)
    with pytest.raises(RuntimeError, match="only be called once"):
        agg.record_initial_condition(ic)


@pytest.mark.parametrize("windows,max_size", [((3, 2, 3), 5), ((3, 4, 3, 2), 7), ((5, 3, 4), 5)])
def test_coarsened_zonal_mean_matches_the_buffer_algorithm(windows, max_size):
    """windows whose lengths are not multiples of the factor: the slot form equals the reference's buffer-carry form"""
    info, ic, wins = make_case(seed=2, windows=windows)
    tgts = targets(wins)
    n_time = 1 + sum(windows)
    cfg = InferenceEvaluatorAggregatorConfig(zonal_mean=ZonalMeanMetricConfig(zonal_mean_max_size=max_size),
                                             power_spectrum=PowerSpectrumMetricConfig(enabled=False))
    agg = cfg.build(info, 1, n_time - 1, normalize=normalizer())
    agg.fused = False
    agg.record_initial_condition(ic)
    for win, tgt in zip(wins, tgts):
        agg.record_batch(win, tgt)
    recs, t = [], 1
    for win, tgt in zip(wins, tgts):
        recs.append((t, win, tgt))
        t += next(iter(win.values())).shape[1]
    factor, n_slots, zon = expected_zonal(recs, n_time, max_size)
    assert factor > 1 and (agg._factor, agg._n_slots) == (factor, n_slots)
    assert any(w % factor for w in windows) and min(windows) >= factor
    ds = agg.get_dataset()["zonal_mean"]
    for n, (g, t) in zon.items():
        assert ds[f"gen-{n}"].shape == (n_slots, H)
        scale = float(g.nan_to_num(0.0).abs().max())
        assert close(ds[f"gen-{n}"], g, 1e-6, scale) and close(ds[f"error-{n}"], g - t, 1e-6, scale), n


def test_too_short_window_for_the_zonal_factor_is_refused():
    info, ic, wins = make_case(seed=2, windows=(3, 1))
    tgts = targets(wins)
    cfg = InferenceEvaluatorAggregatorConfig(zonal_mean=ZonalMeanMetricConfig(zonal_mean_max_size=2))
    agg = cfg.build(info, 1, 4, normalize=normalizer(), sht_factory=oracle_sht_factory)
    agg.fused = False
    assert agg._factor == 3
    agg.record_initial_condition(ic)
    agg.record_batch(wins[0], tgts[0])
    with pytest.raises(ValueError, match="coarsening factor"):
        agg.record_batch(wins[1], tgts[1])


def test_log_layout_and_diagnostics_files(tmp_path):
    info, ic, wins, tgts = case()
    agg = run(info, ic, wins, tgts, output_dir=str(tmp_path), save_diagnostics=True)
    logs = agg.get_inference_logs()
    assert len(logs) == N_TIME and logs[3]["mean/forecast_step"] == 3 and logs[3]["mean_norm/forecast_step"] == 3
    assert isinstance(logs[1]["mean/weighted_rmse/a"], float) and "mean_norm/weighted_rmse/ps" in logs[0]
    assert "mean_norm/weighted_grad_mag_percent_diff/a" not in logs[0] and "mean/weighted_grad_mag_percent_diff/a" in logs[0]
    assert logs[0]["mean/weighted_rmse/a"] == 0.0                       # the unpaired initial condition is its own target
    assert set(agg.get_summary_logs()) <= set(logs[-1]) and "time_mean_norm/rmse/channel_mean" not in logs[0]
    agg.flush_diagnostics()
    ds = agg.get_dataset()
    for sub in ds:
        saved = torch.load(tmp_path / f"{sub}_diagnostics.pt", weights_only=True)
        assert set(saved) == set(ds[sub])


def test_a_bare_callable_serves_the_torch_path_and_counts():
    info, ic, wins, tgts = case()
    calls = []
    norm = normalizer()

    def bare(d):
        calls.append(len(d))
        return norm.normalize(d)
    agg = run(info, ic, wins, tgts, normalize=bare)
    assert agg._stats is None and len(calls) == 2 * (1 + len(wins))
    ref = run(info, ic, wins, tgts).get_dataset()
    for sub, d in agg.get_dataset().items():
        for k, v in d.items():
            assert torch.equal(v.nan_to_num(0.0), ref[sub][k].nan_to_num(0.0)), (sub, k)


def test_run_evaluator_call_order_and_target_slicing():
    """a toy predict: the target is win[name][:, 1:] of every output name the window holds; the writer sees the prediction only"""
    g = torch.Generator().manual_seed(3)
    T = 2
    record = {"x": torch.randn(B, 2 * T + 1, H, W, generator=g), "force": torch.randn(B, 2 * T + 1, H, W, generator=g)}
    wins = [{k: v[:, i * T:i * T + T + 1] for k, v in record.items()} for i in range(2)]
    events = []

    class Agg:
        def record_initial_condition(self, initial_condition):
            events.append(("ic", sorted(initial_condition)))
            return ["ic-logs"]

        def record_batch(self, prediction, target):
            events.append(("batch", prediction, target))
            return ["batch-logs"]

    class Writer:
        def write(self, data, filename):
            events.append(("write", filename))

        def append_batch(self, batch):
            events.append(("append", sorted(batch)))

    def predict(state, win):
        out = {"x": win["force"][:, 1:] + state["x"][:, -1:], "diag": win["force"][:, 1:] * 2}
        return out, {"x": out["x"][:, -1:]}
    ic = {"x": record["x"][:, :1]}
    seen = []
    state = run_evaluator(predict, InferenceData(ic, wins), Agg(), writer=Writer(), record_logs=seen.append)
    kinds = [e[0] if e[0] != "write" else e[1] for e in events]
    assert kinds == ["ic", "initial_condition.nc", "append", "batch", "append", "batch", "restart.nc"]
    assert seen == [["ic-logs"], ["batch-logs"], ["batch-logs"]]
    batches = [e for e in events if e[0] == "batch"]
    for i, (_, pred, tgt) in enumerate(batches):
        assert sorted(pred) == ["diag", "x"] and sorted(tgt) == ["x"]
        assert torch.equal(tgt["x"], wins[i]["x"][:, 1:])
    assert torch.equal(state["x"], batches[-1][1]["x"][:, -1:])
    assert [e[1] for e in events if e[0] == "append"] == [["diag", "x"]] * 2


def test_initial_condition_name_without_a_window_target_is_not_paired_in_the_maps():
    """"ps" is in the initial condition (its own target there) but no window carries a target for it: it has a series at step 0
    only, and no bias map, time-mean RMSE, zonal error or share of the loss"""
    info, ic, wins, tgts = case()
    tgts = [{n: y for n, y in tgt.items() if n != "ps"} for tgt in tgts]
    agg = run(info, ic, wins, tgts)
    ds = agg.get_dataset()
    assert "gen_map-ps" not in ds["time_mean"] and "bias_map-ps" not in ds["time_mean_norm"]
    assert "gen-ps" not in ds["zonal_mean"] and "error-ps" not in ds["zonal_mean"] and "gen-a" in ds["zonal_mean"]
    rmse = ds["mean"]["weighted_rmse-ps"]
    assert float(rmse[0]) == 0.0 and bool((rmse[1:] == 0).all())          # reduced.py:201-218: a record without the name adds 0
    s = agg.get_summary()
    assert "time_mean/rmse/ps" not in s.logs and "time_mean_norm/rmse/ps" not in s.logs and "time_mean/gen_map/ps" in s.logs
    assert s.loss == pytest.approx((s.logs["time_mean_norm/rmse/a"] + s.logs["time_mean_norm/rmse/sst"]) / 2, rel=1e-6)
    assert bool(torch.isnan(ds["power_spectrum"]["ps"][1]).all())
