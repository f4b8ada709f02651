"""The histogram metric of ace_amd.evaluator on its torch path (CPU) against the reference's own ComparedDynamicHistograms on
tests/golden/gen_histogram.pt: counts, edges and percentile keys and values; the variable filters, the refusals, a dropped window,
and the metric's absence by default.  Counts and edges are integers and exact fp64 formulas of the same inputs: compared bitwise."""
import os

import pytest
import torch

from ace_amd.dataset_info import DatasetInfo
from ace_amd.evaluator import HistogramMetricConfig, InferenceEvaluatorAggregatorConfig, MetricConfig, PowerSpectrumMetricConfig, \
    ZonalMeanMetricConfig

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_histogram.pt")
H, W = 9, 18


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def info():
    lat = torch.tensor([-90 + (i + 0.5) * 180 / H for i in range(H)], dtype=torch.float64)
    lon = torch.tensor([j * 360 / W for j in range(W)], dtype=torch.float64)
    return DatasetInfo((H, W), lat=lat, lon=lon)


def histogram_only(histogram, n_steps=12):
    """an evaluator aggregator with every other metric off"""
    off = lambda: MetricConfig(enabled=False)                                  # noqa: E731
    cfg = InferenceEvaluatorAggregatorConfig(
        mean_denorm=off(), mean_norm=off(), step_means=[], ensembles=[], power_spectrum=PowerSpectrumMetricConfig(enabled=False),
        zonal_mean=ZonalMeanMetricConfig(enabled=False), time_mean_denorm=off(), time_mean_norm=off(), annual=off(),
        enso_index=off(), enso_coefficient=off(), ipo_index=off(), histogram=histogram)
    agg = cfg.build(info(), 0, n_steps, normalize=lambda d: d)
    agg.fused = False
    return agg


def run(golden, histogram):
    agg = histogram_only(histogram)
    for t, p in zip(golden["target"], golden["prediction"]):
        assert agg.record_batch(prediction=p, target=t) == []
    return agg


def test_golden_counts_edges_and_percentiles(golden):
    agg = run(golden, HistogramMetricConfig(enabled=True))
    ds = agg.get_dataset()["histogram"]
    assert sorted(ds) == sorted(golden["names"] + [f"{n}_bin_edges" for n in golden["names"]])
    for n in golden["names"]:
        assert ds[n].dtype == torch.int64 and ds[n].shape == (2, 200)
        assert ds[f"{n}_bin_edges"].dtype == torch.float64 and ds[f"{n}_bin_edges"].shape == (2, 201)
        for i, source in enumerate(("target", "prediction")):
            assert torch.equal(ds[n][i], golden["counts"][source][n]), (source, n)
            assert torch.equal(ds[f"{n}_bin_edges"][i], golden["edges"][source][n]), (source, n)
    logs = agg.get_summary_logs()
    scalars = {k: v for k, v in logs.items() if isinstance(v, float)}
    assert sorted(scalars) == sorted(f"histogram/{k}" for k in golden["logs"])
    for k, v in golden["logs"].items():
        assert scalars[f"histogram/{k}"] == pytest.approx(v, rel=1e-12), k
    for n in golden["names"]:
        fig = logs[f"histogram/{n}"]
        for source in ("target", "prediction"):
            d, e = fig[f"{source}_density"], fig[f"{source}_bin_edges"]
            assert e.numel() == d.numel() + 1 and d[0] > 0 and d[-1] > 0
            assert float((d * e.diff()).sum()) == pytest.approx(1.0, rel=1e-12)
    assert not [k for k in logs if "dropped_windows" in k]
    assert agg.get_inference_logs()[-1]["histogram/target/99.9999th-percentile/q"] == scalars["histogram/target/99.9999th-percentile/q"]


def test_variable_filters_and_label(golden):
    agg = run(golden, HistogramMetricConfig(enabled=True, variables=["q", "ps"], percentile_variables=["q"], name="hist"))
    ds = agg.get_dataset()["hist"]
    assert sorted(ds) == ["ps", "ps_bin_edges", "q", "q_bin_edges"]
    assert torch.equal(ds["ps"][1], golden["counts"]["prediction"]["ps"])
    logs = agg.get_summary_logs()
    assert sorted(k for k, v in logs.items() if isinstance(v, float)) == ["hist/prediction/99.9999th-percentile/q",
                                                                           "hist/target/99.9999th-percentile/q"]
    assert "hist/ps" in logs and "hist/q" in logs and "hist/a" not in logs
    with pytest.raises(ValueError, match=r"percentile_variables contains names not in variables: \['a'\]"):
        HistogramMetricConfig(variables=["q"], percentile_variables=["a", "q"])


def test_typed_config_only_and_defaults(golden):
    with pytest.raises(NotImplementedError, match="HistogramMetricConfig"):
        histogram_only(MetricConfig(enabled=True))
    cfg = HistogramMetricConfig()
    assert (cfg.enabled, cfg.strict, cfg.name, cfg.variables, cfg.percentile_variables) == (False, True, "histogram", None, None)
    assert isinstance(InferenceEvaluatorAggregatorConfig().histogram, HistogramMetricConfig)
    agg = run(golden, HistogramMetricConfig())
    assert "histogram" not in agg.get_dataset() and not [k for k in agg.get_summary_logs() if "histogram" in k]


def test_changed_name_set_is_refused(golden):
    agg = histogram_only(HistogramMetricConfig(enabled=True))
    t, p = golden["target"][0], golden["prediction"][0]
    agg.record_batch(prediction=p, target=t)
    with pytest.raises(ValueError, match="differ from initial call to record_batch"):
        agg.record_batch(prediction=p, target={n: v for n, v in t.items() if n != "a"})
    none = histogram_only(HistogramMetricConfig(enabled=True, variables=["nope"]))
    with pytest.raises(ValueError, match="No overlapping keys"):
        none.record_batch(prediction=p, target=t)


def test_a_window_with_a_nan_at_an_unmasked_pixel_is_dropped_and_counted(golden):
    names = ["a", "ps"]
    wins = [({n: t[n] for n in names}, {n: p[n].clone() for n in names}) for t, p in zip(golden["target"], golden["prediction"])]
    wins[1][1]["a"][1, 2, 4, 5] = float("nan")                              # the second window of the prediction of "a"
    land = golden["target"][0]["ps"][0, 0].isnan()
    i, j = (~land).nonzero()[0].tolist()                                    # a sea pixel; on land the value would be masked out
    wins[2][1]["ps"][0, 0, i, j] = float("inf")
    agg = histogram_only(HistogramMetricConfig(enabled=True))
    clean = histogram_only(HistogramMetricConfig(enabled=True))
    for i, (t, p) in enumerate(wins):
        agg.record_batch(prediction=p, target=t)
        if i != 1:
            clean.record_batch(prediction={"a": p["a"]}, target={"a": t["a"]})
    ds, want = agg.get_dataset()["histogram"], clean.get_dataset()["histogram"]
    # the prediction side of "a" is what it would be had the window never come; its target side recorded all four
    assert torch.equal(ds["a"][1], want["a"][1]) and torch.equal(ds["a_bin_edges"][1], want["a_bin_edges"][1])
    assert torch.equal(ds["a"][0], golden["counts"]["target"]["a"])
    assert int(ds["a"][1].sum()) == 3 * 2 * 3 * H * W and int(ds["a"][0].sum()) == 4 * 2 * 3 * H * W
    assert int(ds["ps"][1].sum()) == 3 * 2 * 3 * int((~land).sum())
    logs = agg.get_summary_logs()
    assert logs["histogram/dropped_windows/a"] == 1 and logs["histogram/dropped_windows/ps"] == 1


def test_the_abi_refuses_on_the_host_before_any_launch():
    """the argument checks of ace_diag_hist_window run before the first HIP call, so they hold without a GPU"""
    from ace_amd import _lib
    L = _lib.lib()
    nulls = [None] * 10
    for args, word in (((1, 7, 1, 1, 1, 4), "n_bins"), ((1, 8, -1, 1, 1, 4), "nplanes"), ((1, 8, 1, 0, 1, 4), "batch"),
                       ((1, 8, 1, 4096, 1024, 4), "batch * steps"), ((1, 8, 1, 1, 1, 0), "hw"), ((0, 8, 1, 1, 1, 4), "nrows"),
                       ((1, 8, 1, 1, 1, 4), "null argument")):
        assert L.ace_diag_hist_window(*nulls, *args, None) == _lib.ACE_ERR_INVALID
        msg = L.ace_diag_last_error().decode()
        assert msg.startswith("ace_diag_hist_window: ") and word in msg, msg
    assert L.ace_diag_hist_window(*nulls, 1, 200, 0, 1, 1, 64800, None) == _lib.ACE_OK           # no planes: a no-op
    assert L.ace_diag_hist_scratch_bytes(40, 1, 40, 64800) == 2 * 40 * (16 * 64 + 16)
    assert L.ace_diag_hist_scratch_bytes(1, 4096, 1024, 5) == -1 and L.ace_diag_hist_scratch_bytes(0, 1, 1, 5) == 0
