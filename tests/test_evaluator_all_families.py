"""Every metric family of the evaluator on in one aggregator: what it reports under each label is, exactly, what an aggregator with
that family alone reports for the same record - on the CPU the torch path (``torch.equal`` / ``==``), on the GPU the fused path
against itself, bitwise (the kernels are fixed-order and atomics-free), with the launch counts the ``launches()`` docstring states.

The record, in the manner of tests/_calendar_cases.py (exact hashed noise, so every machine builds the same fp32 bits),
tests/_regress_cases.py (an initial condition, two windows of T = 3 and a time axis whose samples start 40 days apart) and
tests/_ensemble_cases.py (sample b = i * E + e): B = 4 = two initial conditions x two members; ``sst`` under a mask with zeros and
NaN there, ``t``, ``pr`` (zero-inflated, planes not contiguous) and a prediction-only ``diag``.  The timestep is 300 days: seven
steps are 2100 days, more than the 1800 the ENSO coefficient and the 730 that annual and enso_index ask for, the steps fall in
all four seasons and some calendar years hold two of them (more than annual's 350 days' worth), so ``build`` skips nothing.
``ipo_index`` is left to its own tests (tests/test_evaluator_calendar_cpu.py, tests/test_gpu_evaluator_calendar.py): it needs more
than 80 x 365 days, 11.4 years a step over seven steps, at which no calendar year holds two steps and no month is recorded twice.

Grids: (9, 57) has an odd H * W, so the paired, hist, regress, calendar and ensemble kernels take their scalar path; (16, 72)
takes their 16-byte path."""
import datetime
import functools

import pytest
import torch

import _calendar_cases as CC
import _regress_cases as RC
from ace_amd.dataset_info import DatasetInfo
from ace_amd.evaluator import (AnnualMetricConfig, EnsembleMetricConfig, EnsoCoefficientMetricConfig, EnsoIndexMetricConfig,
                               HistogramMetricConfig, InferenceEvaluatorAggregatorConfig, MetricConfig, NearZeroFractionMetricConfig,
                               PowerSpectrumMetricConfig, SeasonalMetricConfig, StepMeanMetricConfig, TrendMetricConfig,
                               ZonalMeanMetricConfig)
from ace_amd.masking import SpatialMaskProvider
from ace_amd.normalizer import StandardNormalizer
from ace_amd.timeaxis import TimeAxis
from test_aggregator_cpu import oracle_sht_factory
from test_gpu_diag_kernels import dev  # noqa: F401

SHAPES = [(9, 57), (16, 72)]
N_IC, E, T = 2, 2, RC.T
B, N_TIME = N_IC * E, 1 + 2 * RC.T
STEP = datetime.timedelta(days=300)
LAND = (slice(1, 3), slice(2, 5))
STATS = {"sst": (288.0, 6.0), "t": (0.5, 2.0), "pr": (1e-4, 3e-4)}       # "diag" has none: normalize drops it


@functools.lru_cache(maxsize=None)
def record(H, W):
    """the record of one grid on the CPU, built once and never written to"""
    lat = torch.tensor([-75.0 + 150.0 / (H - 1) * i for i in range(H)], dtype=torch.float32)      # 0 (H = 9) or -5, 5 (H = 16): in Nino 3.4
    lon = torch.tensor([j * 360.0 / W for j in range(W)], dtype=torch.float32)
    mask = torch.ones(H, W)
    mask[LAND] = 0.0
    info = DatasetInfo((H, W), timestep=STEP, lat=lat, lon=lon, mask_provider=SpatialMaskProvider({"mask_sst": mask}))
    time = TimeAxis.regular((2011, 3, 1), STEP, N_TIME, n_samples=B)
    time = TimeAxis(time.calendar, time.us + (torch.arange(B)[:, None] * 40 * 86_400_000_000).numpy())
    index = torch.from_numpy(CC._noise((B, N_TIME), 5))
    noise = lambda salt, w=W: torch.from_numpy(CC._noise((B, N_TIME, H, w), salt)).float()          # noqa: E731
    shared = lambda salt: noise(salt).view(N_IC, E, N_TIME, H, W)[:, :1].expand(-1, E, -1, -1, -1).reshape(B, N_TIME, H, W)  # noqa: E731
    ramp = torch.arange(N_TIME, dtype=torch.float32)[None, :, None, None]
    gen, tgt = {}, {}
    for side, d in enumerate((gen, tgt)):                                    # the members of an initial condition share its target
        field = noise if side == 0 else shared
        d["sst"] = 288.0 + 6.0 * field(11 + side) + 0.3 * side
        d["sst"][:, :, LAND[0], LAND[1]] = float("nan")
        d["t"] = (0.2 + 0.1 * side) * ramp + index.float()[:, :, None, None] * lat[:, None] / 90.0 + field(21 + side)
        d["pr"] = torch.where(field(31 + side) < -0.2, 3e-4 * field(41 + side).abs() ** 3, torch.zeros(()))
    gen["diag"] = noise(51)
    cut = lambda d, a, b: {n: v[:, a:b] for n, v in d.items()}              # noqa: E731
    windows = [((cut(gen, a, a + T), cut(tgt, a, a + T)), time[:, a:a + T]) for a in (1, 1 + T)]
    return {"info": info, "index": index, "ic": (cut(gen, 0, 1), cut(tgt, 0, 1)), "windows": windows}


def families(c):
    """family -> the configuration fields that turn it on"""
    return {
        "paired": dict(mean_denorm=MetricConfig(), mean_norm=MetricConfig(), time_mean_denorm=MetricConfig(),
                       time_mean_norm=MetricConfig(), zonal_mean=ZonalMeanMetricConfig()),
        "spectrum": dict(power_spectrum=PowerSpectrumMetricConfig()),
        "histogram": dict(histogram=HistogramMetricConfig(enabled=True)),
        "regress": dict(trend=TrendMetricConfig(enabled=True), enso_coefficient=EnsoCoefficientMetricConfig(index=c["index"]),
                        near_zero_fraction=NearZeroFractionMetricConfig(enabled=True, variables=["pr", "t"], include_maps=True)),
        "calendar": dict(seasonal=SeasonalMetricConfig(enabled=True), annual=AnnualMetricConfig(), enso_index=EnsoIndexMetricConfig()),
        "step_means": dict(step_means=[StepMeanMetricConfig(step=2), StepMeanMetricConfig(step=5, target="norm")]),
        "ensembles": dict(ensembles=[EnsembleMetricConfig(step=2, log_mean_maps=True), EnsembleMetricConfig(step=5, target="norm")]),
    }


def gappy(x):
    """the same values with rows W + 1 apart: planes that are not contiguous"""
    wide = x.new_zeros(*x.shape[:-1], x.shape[-1] + 1)
    wide[..., :-1] = x
    return wide[..., :-1]


def run(c, device, fused, fields):
    off = lambda: MetricConfig(enabled=False)                                # noqa: E731
    base = dict(mean_denorm=off(), mean_norm=off(), step_means=[], ensembles=[], power_spectrum=off(), zonal_mean=off(),
                time_mean_denorm=off(), time_mean_norm=off(), annual=off(), enso_index=off(), enso_coefficient=off(), ipo_index=off())
    norm = StandardNormalizer({k: v[0] for k, v in STATS.items()}, {k: v[1] for k, v in STATS.items()}, device=device)
    agg = InferenceEvaluatorAggregatorConfig(**{**base, **fields}).build(
        c["info"], 1, 2 * T, normalize=norm, n_ensemble_per_ic=E, sht_factory=None if fused else oracle_sht_factory)
    agg.fused = fused
    on = lambda d: {n: gappy(v.to(device)) if n == "pr" else v.to(device) for n, v in d.items()}      # noqa: E731
    agg.record_initial_condition(*(on(d) for d in c["ic"]))
    for (gen, tgt), time in c["windows"]:
        agg.record_batch(on(gen), on(tgt), time=time)
    assert agg.skipped == [] and agg._path == ("fused" if fused else "torch")
    return agg


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and \
            torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())
    return type(a) is type(b) and (a == b or (a != a and b != b))


def combined_equals_each_family(c, device, fused):
    on = families(c)
    both = run(c, device, fused, {k: v for fields in on.values() for k, v in fields.items()})
    dataset, logs = both.get_dataset(), both.get_summary().logs
    seen_blocks, seen_logs = [], []
    for family, fields in on.items():
        alone = run(c, device, fused, fields)
        for label, block in alone.get_dataset().items():
            assert same(dataset[label], block), (family, label)
            seen_blocks.append(label)
        want = alone.get_summary().logs
        assert want and [k for k in logs if k in want] == list(want), family
        for k, v in want.items():
            assert same(logs[k], v), (family, k)
        seen_logs += list(want)
        assert alone.omitted == ["sst"]
    assert sorted(seen_blocks) == sorted(dataset) and sorted(seen_logs) == sorted(logs)
    assert both.omitted == ["sst"] and both.get_summary().loss == logs["time_mean_norm/rmse/channel_mean"]
    return both


@pytest.mark.parametrize("shape", SHAPES)
def test_every_family_on_reports_what_each_reports_alone(shape):
    c = record(*shape)
    assert N_TIME * STEP > datetime.timedelta(days=1800)
    both = combined_equals_each_family(c, torch.device("cpu"), False)
    assert both.launches() == 0 and both.calendar_launches() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_every_family_on_reports_what_each_reports_alone_fused(dev, shape):  # noqa: F811
    both = combined_equals_each_family(record(*shape), dev, True)
    # launches(): a paired window for the initial condition and each window; per window of record_batch one histogram call, one
    # regress call (no window starts at time index 0: the initial condition holds it) and, for prediction and target, one chunk of
    # the unmasked names = one SHT + one spectrum call; one ensemble call per entry, in the window that holds its step
    assert both.launches() == 3 + 2 + 2 + 2 * 2 * 2 + 2
    assert both.calendar_launches() == 2
