"""The host logic of the masked-spectrum fill on the torch path (CPU), for both aggregators, on the small masked case of
test_aggregator_cpu.py ("sst" NaN on land): with the option off nothing changes - ``omitted == ["sst"]``, the same spectra - and
with it on "sst" is filled, listed in ``filled`` and its spectrum is that of ``sht(smooth_flood_fill(...))``; a name without a valid
pixel stays omitted; both configuration fields reach the aggregators through ``build``."""
import dataclasses

import torch

from ace_amd.aggregator import InferenceAggregatorConfig
from ace_amd.dataset_info import DatasetInfo
from ace_amd.evaluator import InferenceEvaluatorAggregatorConfig, PowerSpectrumMetricConfig
from ace_amd.fill import smooth_flood_fill
from ace_amd.masking import SpatialMaskProvider

from test_aggregator_cpu import B, H, W, WINDOWS, land_mask, lat_lon, make_case, oracle_sht_factory
from test_aggregator_cpu import run as run_plain
from test_evaluator_aggregator_cpu import N_TIME, case
from test_evaluator_aggregator_cpu import run as run_paired


def mean_spectrum(fields, mask=None):
    """the mean over samples, steps and windows of sum over m of |SHT|^2, in fp32 torch as the torch path computes it"""
    sht, total, count = oracle_sht_factory(H, W), 0, 0
    for x in fields:
        if mask is not None:
            x = smooth_flood_fill(x, mask)
        total = total + torch.sum(abs(sht(x)) ** 2, dim=-1).sum(dim=(0, 1)).double()
        count += x.shape[0] * x.shape[1]
    return total / count


def close(got, want, tol=1e-5):
    return float((got.double() - want).abs().max()) <= tol * float(want.abs().max())


def test_off_by_default_and_nothing_changes():
    assert InferenceAggregatorConfig().fill_masked_spectrum is False and PowerSpectrumMetricConfig().fill_masked is False
    info, ic, wins = make_case()
    base = run_plain(info, ic, wins, N_TIME)
    assert base.omitted == ["sst"] and base.filled == [] and not base.fill_masked_spectrum
    assert set(base.get_dataset()["power_spectrum"]) == {"a", "ps", "diag"}
    on = InferenceAggregatorConfig(fill_masked_spectrum=True).build(info, N_TIME, sht_factory=oracle_sht_factory)
    on.fused = False
    on.record_initial_condition(ic)
    for win in wins:
        on.record_batch(win)
    for n, v in base.get_dataset()["power_spectrum"].items():                # the unmasked names are not touched by the option
        assert torch.equal(on.get_dataset()["power_spectrum"][n], v), n


def test_the_plain_aggregator_fills_sst():
    info, ic, wins = make_case()
    agg = InferenceAggregatorConfig(fill_masked_spectrum=True).build(info, N_TIME, sht_factory=oracle_sht_factory)
    agg.fused = False
    agg.record_initial_condition(ic)
    for win in wins:
        agg.record_batch(win)
    assert agg.omitted == [] and agg.filled == ["sst"]
    spec = agg.get_dataset()["power_spectrum"]
    assert set(spec) == {"a", "ps", "diag", "sst"} and bool(torch.isfinite(spec["sst"]).all())
    assert close(spec["sst"], mean_spectrum([w["sst"] for w in wins], land_mask()))
    assert "power_spectrum/sst" in agg.get_summary_logs()


def test_the_evaluator_fills_sst_on_both_sides():
    info, ic, wins, tgts = case()
    off = run_paired(info, ic, wins, tgts)
    assert off.omitted == ["sst"] and off.filled == []
    cfg = InferenceEvaluatorAggregatorConfig(power_spectrum=PowerSpectrumMetricConfig(fill_masked=True))
    agg = run_paired(info, ic, wins, tgts, config=cfg)
    assert agg.fill_masked_spectrum and agg.omitted == [] and agg.filled == ["sst"]
    spec, base = agg.get_dataset()["power_spectrum"], off.get_dataset()["power_spectrum"]
    assert set(spec) == {"a", "ps", "diag", "sst"} and set(base) == {"a", "ps", "diag"}
    for n, v in base.items():
        assert torch.equal(spec[n].nan_to_num(-1.0), v.nan_to_num(-1.0)), n      # "diag" has no target: a NaN row
    assert spec["sst"].shape == (2, H) and bool(torch.isfinite(spec["sst"]).all())
    assert close(spec["sst"][0], mean_spectrum([w["sst"] for w in wins], land_mask()))
    assert close(spec["sst"][1], mean_spectrum([t["sst"] for t in tgts], land_mask()))
    logs = agg.get_summary_logs()
    assert "power_spectrum/mean_abs_norm_bias/sst" in logs and "power_spectrum/mean_abs_norm_bias/sst" not in off.get_summary_logs()


def test_a_name_without_a_valid_pixel_stays_omitted():
    lat, lon = lat_lon()
    masks = SpatialMaskProvider({"mask_sst": land_mask(), "mask_ice": torch.zeros(H, W)})
    info = DatasetInfo((H, W), lat=lat, lon=lon, mask_provider=masks)
    g = torch.Generator().manual_seed(1)
    win = {"a": torch.randn(B, 2, H, W, generator=g), "sst": 290 + torch.randn(B, 2, H, W, generator=g),
           "ice": torch.full((B, 2, H, W), float("nan"))}
    win["sst"] = win["sst"].where(land_mask() != 0, torch.tensor(float("nan")))
    agg = InferenceAggregatorConfig(fill_masked_spectrum=True, log_global_mean_time_series=False).build(
        info, 2, sht_factory=oracle_sht_factory)
    agg.fused = False
    agg.record_batch(win)
    assert agg.omitted == ["ice"] and agg.filled == ["sst"]
    assert set(agg.get_dataset()["power_spectrum"]) == {"a", "sst"}


def test_the_fields_go_through_build():
    info, _, _ = make_case()
    assert "fill_masked_spectrum" in {f.name for f in dataclasses.fields(InferenceAggregatorConfig)}
    assert "fill_masked" in {f.name for f in dataclasses.fields(PowerSpectrumMetricConfig)}
    for flag in (False, True):
        plain = InferenceAggregatorConfig(fill_masked_spectrum=flag).build(info, 4)
        assert plain.fill_masked_spectrum is flag
        cfg = InferenceEvaluatorAggregatorConfig(power_spectrum=PowerSpectrumMetricConfig(fill_masked=flag))
        paired = cfg.build(info, 1, 3, normalize=lambda d: d)
        assert paired.fill_masked_spectrum is flag
        again = InferenceEvaluatorAggregatorConfig(**{f.name: getattr(cfg, f.name) for f in dataclasses.fields(cfg)})
        assert again.power_spectrum.fill_masked is flag and dataclasses.asdict(again) == dataclasses.asdict(cfg)
