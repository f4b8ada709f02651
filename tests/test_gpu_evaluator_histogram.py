"""The evaluator's histogram metric on its fused path (csrc/hist.hip: one ace_diag_hist_window per window) against its own torch
path on the same device at 180 x 360 - counts, edges and percentiles exactly: both state the same integers and the same fp64
formulas, and tests/test_evaluator_histogram_cpu.py holds the torch path to the reference - the launch count against a
histogram-less twin, and a run under ``run_evaluator`` on the small SFNO fixture of test_gpu_evaluator_aggregator.py."""
import tempfile

import pytest
import torch

from ace_amd.evaluator import HistogramMetricConfig, InferenceEvaluatorAggregatorConfig
from ace_amd.normalizer import StandardNormalizer
from _util import load_golden
from test_gpu_aggregator import NLAT, NLON, dev, one_degree_info  # noqa: F401

pytestmark = pytest.mark.gpu


def build(dev, names, n_time, histogram=None, fused=True):
    norm = StandardNormalizer({n: 0.5 for n in names}, {n: 2.0 for n in names}, device=dev)
    cfg = InferenceEvaluatorAggregatorConfig() if histogram is None else InferenceEvaluatorAggregatorConfig(histogram=histogram)
    agg = cfg.build(one_degree_info(), 1, n_time - 1, normalize=norm)
    agg.fused = fused
    return agg


def windows(dev, n, B=2, T=2):
    """a zero-inflated "precip" (about 92 % exact zeros) and an "sst" that is NaN on land in the target only; ranges that grow"""
    g = torch.Generator().manual_seed(21)
    land = one_degree_info().mask_provider.get_mask_tensor_for("sst") == 0
    out = []
    for w in range(n):
        pair = []
        for side in range(2):
            wet = torch.rand(B, T, NLAT, NLON, generator=g) < 0.08
            precip = torch.where(wet, (1 + w) * 3e-4 * torch.randn(B, T, NLAT, NLON, generator=g).abs() ** 3, torch.zeros(()))
            sst = 290 + (5 + 4 * w) * torch.randn(B, T, NLAT, NLON, generator=g) - 3 * w
            if side == 1:
                sst = sst.where(~land, torch.tensor(float("nan")))
            pair.append({"precip": precip.float().to(dev), "sst": sst.float().to(dev)})
        out.append(pair)
    return out


def test_fused_equals_the_torch_path_exactly(dev):
    wins = windows(dev, 3)
    aggs = {}
    for fused in (True, False):
        agg = aggs[fused] = build(dev, ["precip", "sst"], 7, HistogramMetricConfig(enabled=True), fused)
        for gen, tgt in wins:
            assert agg.route(gen, tgt) == ("fused" if fused else "torch")
            agg.record_batch(gen, tgt)
    got, want = aggs[True].get_dataset()["histogram"], aggs[False].get_dataset()["histogram"]
    assert sorted(got) == sorted(want) == ["precip", "precip_bin_edges", "sst", "sst_bin_edges"]
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    land = int((one_degree_info().mask_provider.get_mask_tensor_for("sst") == 0).sum())
    assert got["sst"].sum(-1).tolist() == [3 * 4 * (NLAT * NLON - land)] * 2 and got["precip"].sum(-1).tolist() == [3 * 4 * NLAT * NLON] * 2
    assert int(got["precip"].max()) > 0.9 * 3 * 4 * NLAT * NLON                                  # the zero bin
    flogs, tlogs = aggs[True].get_summary_logs(), aggs[False].get_summary_logs()
    keys = [f"histogram/{s}/99.9999th-percentile/{n}" for s in ("target", "prediction") for n in ("precip", "sst")]
    for k in keys:
        assert flogs[k] == tlogs[k] and flogs[k] > 0, k
    assert not [k for k in flogs if "dropped_windows" in k]


@pytest.mark.parametrize("n_names", [1, 5])
def test_one_launch_per_window_whatever_the_names(dev, n_names):
    g = torch.Generator().manual_seed(n_names)
    names = [f"v{i}" for i in range(n_names)]
    wins = [[{n: torch.randn(1, 2, NLAT, NLON, generator=g).to(dev) for n in names} for _ in range(2)] for _ in range(2)]
    with_hist, twin = build(dev, names, 5, HistogramMetricConfig(enabled=True)), build(dev, names, 5)
    for i, (gen, tgt) in enumerate(wins):
        with_hist.record_batch(gen, tgt)
        twin.record_batch(gen, tgt)
        assert with_hist.launches() - twin.launches() == i + 1
    assert "histogram" not in twin.get_dataset() and sorted(with_hist.get_dataset()["histogram"])[0] == "v0"


def test_run_evaluator_returns_the_percentile_keys(dev):
    import ace_amd
    from ace_amd.inference import EnginePredict, ForcingWindows, InferenceData, TensorFileWriter, run_evaluator, run_inference
    g = load_golden("gen_checkpoint.pt")["ace2_like"]
    loaded = ace_amd.load_stepper(g["state"], device=dev)
    ic = {k: v.to(dev) for k, v in g["ic"].items()}
    forcing, total, T = g["forcing"], len(g["steps"]), 2
    with tempfile.TemporaryDirectory() as tmp:
        run_inference(EnginePredict(loaded.stepper, batch=2, graph="step"),
                      InferenceData(ic, ForcingWindows(forcing, total_forward_steps=total, forward_steps_in_memory=T, device=dev)),
                      writer=TensorFileWriter(tmp), compute_derived_variables=False)
        pred = torch.load(tmp + "/autoregressive_predictions.pt", weights_only=True)
    names = [n for n in pred if n not in forcing]
    first = {n: (ic[n].cpu() if n in ic else torch.full_like(pred[n][:, :1], float("nan"))) for n in names}
    record = {**forcing, **{n: torch.cat([first[n], 1.01 * pred[n]], dim=1) for n in names}}
    agg = InferenceEvaluatorAggregatorConfig(histogram=HistogramMetricConfig(enabled=True, percentile_variables=names[:2])).build(
        loaded.dataset_info, 1, total, normalize=loaded.stepper.normalizer)
    run_evaluator(EnginePredict(loaded.stepper, batch=2, graph="step"),
                  InferenceData(ic, ForcingWindows(record, total_forward_steps=total, forward_steps_in_memory=T, device=dev)), agg)
    assert agg._path == "fused"
    logs = agg.get_inference_logs()[-1]
    pct = sorted(k for k in logs if "th-percentile" in k)
    assert pct == sorted(f"histogram/{s}/99.9999th-percentile/{n}" for s in ("target", "prediction") for n in names[:2])
    assert all(isinstance(logs[k], float) and logs[k] == logs[k] for k in pct)
    ds = agg.get_dataset()["histogram"]
    for n in names:
        assert f"histogram/{n}" in logs and ds[n].shape == (2, 200) and int(ds[n].sum()) > 0, n
