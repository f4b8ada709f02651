"""ace_amd.aggregator on its torch path (CPU) against an fp64 restatement of the reference's no-target InferenceAggregator
(fme/ace/aggregator/inference: reduced.py, time_mean.py, spectrum.py; fme/core/metrics.py weighted_mean / spherical_power_spectrum)."""

import pytest
import torch

from ace_amd.aggregator import InferenceAggregatorConfig
from ace_amd.dataset_info import DatasetInfo
from ace_amd.masking import SpatialMaskProvider
from oracle.sht import RealSHT as OracleSHT

H, W, B = 8, 16, 2
WINDOWS = (3, 2, 1)            # uneven window lengths


def lat_lon(h=H, w=W):
    lat = torch.tensor([-90 + (i + 0.5) * 180 / h for i in range(h)], dtype=torch.float64)
    lon = torch.tensor([j * 360 / w for j in range(w)], dtype=torch.float64)
    return lat, lon


def land_mask(h=H, w=W):
    m = torch.ones(h, w)
    m[: h // 3, : w // 4] = 0.0
    return m


def make_case(seed=0, h=H, w=W, batch=B, windows=WINDOWS):
    """(dataset_info, initial condition, windows): "a", "ps" (surface-pressure-like), "sst" (NaN on land), "diag" (not in the
    initial condition: a diagnostic-only output)."""
    g = torch.Generator().manual_seed(seed)
    lat, lon = lat_lon(h, w)
    mask = land_mask(h, w)
    info = DatasetInfo((h, w), lat=lat, lon=lon, mask_provider=SpatialMaskProvider({"mask_sst": mask}))

    def field(t):
        d = {"a": torch.randn(batch, t, h, w, generator=g),
             "ps": 1e5 + 1e2 * torch.randn(batch, t, h, w, generator=g),
             "sst": 290 + 5 * torch.randn(batch, t, h, w, generator=g)}
        d["sst"] = d["sst"].where(mask.expand_as(d["sst"]) != 0, torch.tensor(float("nan")))
        d["diag"] = torch.rand(batch, t, h, w, generator=g)
        return d

    ic = {k: v for k, v in field(1).items() if k != "diag"}
    return info, ic, [field(t) for t in windows]


# ---- the fp64 restatement -----------------------------------------------------------------------------------------------
def weights64(info, name):
    w = info.area_weights.double()
    m = info.mask_provider.get_mask_tensor_for(name) if info.mask_provider else None
    return w if m is None else w * m.double()


def wmean64(x, w):
    x = x.double().where(w != 0, 0.0)
    return (x * w).sum((-2, -1)) / w.sum()


def wstd64(x, w):
    m = wmean64(x, w)[..., None, None]
    return wmean64(((x.double() - m) ** 2).where(w != 0, 0.0), w).sqrt()


def expected(info, ic, windows, n_time, with_ic=True):
    """reduced.py / time_mean.py / spectrum.py in fp64 over the whole record"""
    recs = ([(0, ic)] if with_ic else [])
    t = 1 if with_ic else 0
    for win in windows:
        recs.append((t, win))
        t += next(iter(win.values())).shape[1]
    names = sorted({n for _, r in recs for n in r})
    total = {m: {n: torch.zeros(n_time, dtype=torch.float64) for n in names} for m in ("weighted_mean_gen", "weighted_std_gen")}
    count = torch.zeros(n_time, dtype=torch.float64)
    for t0, r in recs:
        T = next(iter(r.values())).shape[1]
        for n, x in r.items():
            w = weights64(info, n)
            total["weighted_mean_gen"][n][t0:t0 + T] += wmean64(x, w).mean(0)
            total["weighted_std_gen"][n][t0:t0 + T] += wstd64(x, w).mean(0)
        count[t0:t0 + T] += 1
    series = {m: {n: v / count for n, v in d.items()} for m, d in total.items()}
    # time_mean.py:127-146: the first batch at i_time_start == 0 drops its initial step and resets the step count
    maps, steps = {}, 0
    for t0, r in recs[1 if with_ic else 0:]:
        first = t0 == 0
        for n, x in r.items():
            s = x[:, 1:] if first else x
            maps[n] = maps.get(n, 0) + s.double().sum((0, 1))
        T = next(iter(r.values())).shape[1]
        steps = T - 1 if first else steps + T
    maps = {n: v / steps / B for n, v in maps.items()}
    sht = OracleSHT(info.img_shape[0], info.img_shape[1], grid="legendre-gauss", dtype=torch.float64)
    spec, cnt = {}, {}
    for _, r in recs[1 if with_ic else 0:]:
        for n, x in r.items():
            if n == "sst":
                continue
            c = sht(x.double())
            spec[n] = spec.get(n, 0) + (c.real ** 2 + c.imag ** 2).sum(-1).sum((0, 1))
            cnt[n] = cnt.get(n, 0) + x.shape[0] * x.shape[1]
    spec = {n: v / cnt[n] for n, v in spec.items()}
    return series, maps, spec


def oracle_sht_factory(nlat, nlon):
    return OracleSHT(nlat, nlon, grid="legendre-gauss")


def run(info, ic, windows, n_time, with_ic=True, **kw):
    agg = InferenceAggregatorConfig().build(info, n_time, sht_factory=oracle_sht_factory, **kw)
    agg.fused = False
    if with_ic:
        assert agg.record_initial_condition(ic) == []
    for win in windows:
        assert agg.route(win) == "torch"
        assert agg.record_batch(win) == []
    return agg


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ---- tests --------------------------------------------------------------------------------------------------------------
def test_series_maps_and_spectra_match_the_fp64_reference():
    info, ic, wins = make_case()
    n_time = 1 + sum(WINDOWS)
    agg = run(info, ic, wins, n_time)
    series, maps, spec = expected(info, ic, wins, n_time)
    ds = agg.get_dataset()
    assert set(ds) == {"mean", "time_mean", "power_spectrum"}
    for metric, d in series.items():
        for n, want in d.items():
            got = ds["mean"][f"{metric}-{n}"]
            assert got.shape == (n_time,)
            assert rel(got, want) <= 1e-5, (metric, n)
    for n, want in maps.items():
        got = ds["time_mean"][f"gen_map-{n}"]
        assert got.shape == (H, W)
        ok = ~torch.isnan(want)
        assert torch.equal(torch.isnan(got), ~ok)                   # the reference's time mean keeps NaN on land
        assert rel(got[ok], want[ok]) <= 1e-5, n
    assert set(ds["power_spectrum"]) == set(spec)
    for n, want in spec.items():
        assert ds["power_spectrum"][n].shape == (H,)
        assert rel(ds["power_spectrum"][n], want) <= 1e-4, n


def test_diagnostic_only_name_reads_zero_at_the_initial_step():
    info, ic, wins = make_case()
    agg = run(info, ic, wins, 1 + sum(WINDOWS))
    d = agg.get_dataset()["mean"]
    assert float(d["weighted_mean_gen-diag"][0]) == 0.0 and float(d["weighted_std_gen-diag"][0]) == 0.0
    assert float(d["weighted_mean_gen-diag"][1]) > 0.0
    assert float(d["weighted_mean_gen-a"][0]) != 0.0


def test_unrecorded_steps_are_nan_and_overflow_is_refused():
    info, ic, wins = make_case()
    agg = run(info, ic, wins[:1], 1 + sum(WINDOWS))
    d = agg.get_dataset()["mean"]["weighted_mean_gen-a"]
    assert not torch.isnan(d[:4]).any() and torch.isnan(d[4:]).all()       # total / _n_batches: 0 / 0 past the record
    short = run(info, ic, [], 3)
    with pytest.raises(ValueError):
        short.record_batch(wins[0])


def test_time_mean_drops_the_first_step_without_an_initial_condition():
    info, ic, wins = make_case(seed=1)
    n_time = sum(WINDOWS)
    agg = run(info, ic, wins, n_time, with_ic=False)
    series, maps, _ = expected(info, ic, wins, n_time, with_ic=False)
    got = agg.get_dataset()
    a = got["time_mean"]["gen_map-a"]
    assert rel(a, maps["a"]) <= 1e-5
    # the exclusion matters: the mean over every step differs
    every = sum(w["a"].double().sum((0, 1)) for w in wins) / sum(WINDOWS) / B
    assert rel(a, every) > 1e-3
    for n, want in series["weighted_mean_gen"].items():
        assert rel(got["mean"][f"weighted_mean_gen-{n}"], want) <= 1e-5


def test_masked_names_are_finite_and_omitted_from_the_spectrum():
    info, ic, wins = make_case()
    agg = run(info, ic, wins, 1 + sum(WINDOWS))
    d = agg.get_dataset()
    assert torch.isfinite(d["mean"]["weighted_mean_gen-sst"]).all()
    assert torch.isfinite(d["mean"]["weighted_std_gen-sst"]).all()
    assert agg.omitted == ["sst"]
    assert "sst" not in d["power_spectrum"] and "a" in d["power_spectrum"]


def test_log_keys_follow_the_reference_layout(tmp_path):
    info, ic, wins = make_case()
    n_time = 1 + sum(WINDOWS)
    agg = run(info, ic, wins, n_time, output_dir=str(tmp_path), save_diagnostics=True)
    summary = agg.get_summary_logs()
    names = ["a", "diag", "ps", "sst"]
    assert set(summary) == {f"time_mean/gen_map/{n}" for n in names} | {f"power_spectrum/{n}" for n in names if n != "sst"}
    logs = agg.get_inference_logs()
    assert len(logs) == n_time
    assert logs[2]["mean/forecast_step"] == 2
    want = {"mean/forecast_step"} | {f"mean/{m}/{n}" for m in ("weighted_mean_gen", "weighted_std_gen") for n in names}
    assert set(logs[0]) == want
    assert set(logs[-1]) == want | set(summary)
    assert all(isinstance(v, float) for k, v in logs[1].items() if k != "mean/forecast_step")
    agg.flush_diagnostics()
    for sub in ("mean", "time_mean", "power_spectrum"):
        saved = torch.load(tmp_path / f"{sub}_diagnostics.pt", weights_only=True)
        assert set(saved) == set(agg.get_dataset()[sub])


def test_without_time_series():
    info, ic, wins = make_case()
    agg = InferenceAggregatorConfig(log_global_mean_time_series=False).build(info, 1 + sum(WINDOWS), sht_factory=oracle_sht_factory)
    agg.fused = False
    agg.record_initial_condition(ic)
    for win in wins:
        agg.record_batch(win)
    assert set(agg.get_dataset()) == {"time_mean", "power_spectrum"}
    assert set(agg.get_inference_logs()[-1]) == set(agg.get_summary_logs())


class _HpxCoords:
    face = list(range(12))


class _Info:
    def __init__(self, area_weights=None, horizontal_coordinates=None):
        self.area_weights = area_weights
        self.horizontal_coordinates = horizontal_coordinates
        self.mask_provider = None
        self.img_shape = (H, W)


def test_build_time_refusals():
    info, _, _ = make_case()
    with pytest.raises(NotImplementedError, match="netCDF"):
        InferenceAggregatorConfig(time_mean_reference_data="means.nc").build(info, 4)
    with pytest.raises(NotImplementedError, match="step_diagnostics"):
        InferenceAggregatorConfig(step_diagnostics={"per_step": True}).build(info, 4)
    with pytest.raises(NotImplementedError, match="HEALPix"):
        InferenceAggregatorConfig().build(_Info(torch.ones(H, W), _HpxCoords()), 4)
    with pytest.raises(ValueError, match="area weights"):
        InferenceAggregatorConfig().build(_Info(), 4)
    with pytest.raises(ValueError, match="Output directory"):
        InferenceAggregatorConfig().build(info, 4, save_diagnostics=True)
    with pytest.raises(ValueError, match="empty"):
        InferenceAggregatorConfig().build(info, 4).record_batch({})
    agg = InferenceAggregatorConfig().build(info, 4)
    with pytest.raises(ValueError, match="No batches"):
        agg.get_dataset()
