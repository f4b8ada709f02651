"""The video metric of ace_amd.evaluator on its torch path (CPU), through ``InferenceEvaluatorAggregatorConfig.build`` and
``record_batch``, against tests/golden/gen_video.pt (the reference's ``VideoAggregator``), and the rules of its configuration.

The torch path states the reference's formulas in the reference's dtypes, so it is held to the golden at the bars
tests/test_video_ref_cpu.py derives (N B u m for the means, (B + 1) u m_d^2 for the squared error per visit; extrema equal as
values); gen_var, a cancelling difference, is held to the formula on the module's own accumulators.  The golden visits every window
twice; ``record_batch`` counts the steps itself, so the second pass rewinds the aggregator's step counter."""
import os

import numpy as np
import pytest
import torch

import ace_amd
from ace_amd.evaluator import (HistogramMetricConfig, InferenceEvaluatorAggregatorConfig, MetricConfig, PowerSpectrumMetricConfig,
                               StepMeanMetricConfig, VideoMetricConfig, ZonalMeanMetricConfig)
from test_video_ref_cpu import U, scales, within

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_video.pt")
H, W, N_TIME, B = 5, 9, 7, 3


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def info(h=H, w=W):
    lat = torch.tensor([-90 + (i + 0.5) * 180 / h for i in range(h)], dtype=torch.float64)
    return ace_amd.DatasetInfo((h, w), lat=lat, lon=torch.arange(w, dtype=torch.float64) * (360.0 / w))


def config(video, **kw):
    """the video as the only metric"""
    off = lambda: MetricConfig(enabled=False)                                  # noqa: E731
    base = dict(mean_denorm=off(), mean_norm=off(), step_means=[], ensembles=[], power_spectrum=PowerSpectrumMetricConfig(enabled=False),
                zonal_mean=ZonalMeanMetricConfig(enabled=False), time_mean_denorm=off(), time_mean_norm=off(), annual=off(),
                enso_index=off(), enso_coefficient=off(), ipo_index=off())
    base.update(kw)
    return InferenceEvaluatorAggregatorConfig(video=video, **base)


def build(video, n_forward=N_TIME - 1, fused=False, grid=(H, W), **kw):
    agg = config(video).build(info(*grid), 1, n_forward, normalize=lambda d: d, **kw)
    agg.fused = fused
    return agg


def replay(agg, visits, device="cpu", names=None):
    """the golden's visits through record_batch: the second pass over the same slots rewinds the step counter"""
    for t0, gen, tgt in visits:
        agg._n_seen = t0
        keep = lambda d: {k: v.to(device) for k, v in d.items() if names is None or k in names}      # noqa: E731
        assert agg.record_batch(keep(gen), keep(tgt)) == []
    return agg


def check_against_golden(ds, golden, names=("a", "m")):
    """a ``video`` dataset block against the golden at the derived bars"""
    data = golden["data"]
    for name in names:
        mg, mt, md = scales(golden, name)
        within(ds[name][0], data[name][0], B * U * mg, f"{name} prediction")
        within(ds[name][1], data[name][1], B * U * mt, f"{name} target")
        within(ds[f"bias_{name}"], data[f"bias/{name}"][0], B * U * (mg + mt), f"{name} bias")
        within(ds[f"rmse_{name}"] ** 2, data[f"rmse/{name}"][0] ** 2, (B + 1) * U * md ** 2, f"{name} rmse^2")
        for key in ("min_err", "max_err"):
            assert np.array_equal(ds[f"{key}_{name}"].numpy(), data[f"{key}/{name}"][0].numpy(), equal_nan=True), (key, name)
        assert torch.isnan(ds[name][:, 0]).all() and torch.isnan(ds[f"gen_var_{name}"][0]).all()
        assert (ds[f"min_err_{name}"][0] == np.inf).all() and (ds[f"max_err_{name}"][0] == -np.inf).all()


def check_gen_var(agg, ds, names=("a", "m")):
    """gen_var against the formula on the module's own accumulators"""
    v = agg._video
    for name in names:
        acc = {c: v._channel(c, name) for c in ("gen", "target", "gen_sq", "target_sq")}      # on the device they live on
        n = torch.from_numpy(v._n).double().to(acc["gen"].device)[:, None, None]
        want = (acc["gen_sq"] / n - (acc["gen"] / n) ** 2) / (acc["target_sq"] / n - (acc["target"] / n) ** 2)
        assert np.array_equal(ds[f"gen_var_{name}"].numpy(), want.cpu().numpy(), equal_nan=True), name


def test_torch_path_against_the_golden(golden):
    agg = replay(build(VideoMetricConfig(enabled=True, enable_extended_videos=True)), golden["visits"])
    assert agg.launches() == 0
    ds = agg.get_dataset()
    assert list(ds) == ["video"]
    ds = ds["video"]
    check_against_golden(ds, golden)
    check_gen_var(agg, ds)
    # the order of the reference's keys and the shapes
    assert list(ds) == [k.replace("/", "_") for k in golden["keys"]]
    for k, v in ds.items():
        assert v.dtype == torch.float64 and v.device.type == "cpu"
        assert tuple(v.shape) == ((2, N_TIME, H, W) if k in ("a", "m") else (N_TIME, H, W)), k
    logs = agg.get_summary_logs()
    assert list(logs) == [f"video/{k}" for k in golden["keys"]]
    for k in golden["keys"]:
        assert np.array_equal(logs[f"video/{k}"].numpy(), ds[k.replace("/", "_")].numpy(), equal_nan=True)


def test_basic_videos_only_and_the_variable_filter(golden):
    ds = replay(build(VideoMetricConfig(enabled=True)), golden["visits"]).get_dataset()["video"]
    assert list(ds) == ["a", "m"]
    full = replay(build(VideoMetricConfig(enabled=True, enable_extended_videos=True)), golden["visits"]).get_dataset()["video"]
    assert all(np.array_equal(ds[k].numpy(), full[k].numpy(), equal_nan=True) for k in ds)
    only = replay(build(VideoMetricConfig(enabled=True, enable_extended_videos=True, variables=["a"], name="films")),
                  golden["visits"]).get_dataset()
    assert list(only) == ["films"] and list(only["films"]) == ["a", "bias_a", "rmse_a", "min_err_a", "max_err_a", "gen_var_a"]
    assert all(np.array_equal(only["films"][k].numpy(), full[k].numpy(), equal_nan=True) for k in only["films"])


def test_a_prediction_without_target_has_a_nan_target_half_and_no_paired_keys(golden):
    agg = build(VideoMetricConfig(enabled=True, enable_extended_videos=True))
    for t0, gen, tgt in golden["visits"]:
        agg._n_seen = t0
        agg.record_batch(gen, {"a": tgt["a"]})
    ds = agg.get_dataset()["video"]
    full = replay(build(VideoMetricConfig(enabled=True, enable_extended_videos=True)), golden["visits"]).get_dataset()["video"]
    assert list(ds) == ["a", "bias_a", "m", "rmse_a", "min_err_a", "max_err_a", "gen_var_a"]
    assert torch.isnan(ds["m"][1]).all() and np.array_equal(ds["m"][0].numpy(), full["m"][0].numpy(), equal_nan=True)
    with pytest.raises(ValueError, match="without a target"):
        agg._n_seen = 1
        agg.record_batch(golden["visits"][0][1], golden["visits"][0][2])


def test_configuration_rules():
    typed = VideoMetricConfig()
    assert (typed.variables, typed.name, typed.enable_extended_videos, typed.enabled, typed.strict) == (None, "video", False, False, True)
    assert build(typed)._video is None and build(VideoMetricConfig(enabled=True))._video is not None
    default = InferenceEvaluatorAggregatorConfig()
    assert type(default.video) is MetricConfig and not default.video.enabled
    agg = default.build(info(8, 16), 1, 6, normalize=lambda d: d)
    assert agg._video is None
    assert agg.skipped == ["step_means", "ensembles", "annual", "enso_index", "enso_coefficient", "ipo_index"]
    assert list(agg._labels.values()) == ["mean", "mean_norm", "time_mean", "time_mean_norm", "power_spectrum", "zonal_mean"]
    with pytest.raises(NotImplementedError, match="video"):
        config(MetricConfig(enabled=True)).build(info(), 1, 6, normalize=lambda d: d)
    with pytest.raises(ValueError, match="two metrics are named 'video'"):
        config(VideoMetricConfig(enabled=True), step_means=[StepMeanMetricConfig(step=2, name="video")]).build(
            info(), 1, 6, normalize=lambda d: d)
    config(VideoMetricConfig(enabled=True, name="films"), step_means=[StepMeanMetricConfig(step=2, name="video")],
           histogram=HistogramMetricConfig()).build(info(), 1, 6, normalize=lambda d: d)


@pytest.mark.parametrize("extended,per", [(False, 16), (True, 48)])
def test_memory_rule(golden, extended, per):
    need = 2 * N_TIME * H * W * per
    cfg = VideoMetricConfig(enabled=True, enable_extended_videos=extended)
    replay(build(cfg, video_max_bytes=need), golden["visits"][:1])
    agg = build(cfg, video_max_bytes=need - 1)
    with pytest.raises(ValueError, match=rf"{need} bytes = 2 names x {N_TIME} steps x {H} x {W} x {per} bytes.*variables"):
        replay(agg, golden["visits"][:1])
    assert agg._video._pairs == {} and agg._video._mean is None and agg._video._t == {}
    one = VideoMetricConfig(enabled=True, enable_extended_videos=extended, variables=["m"])
    replay(build(one, video_max_bytes=need // 2), golden["visits"][:1])


def test_the_initial_condition_and_late_windows(golden):
    agg = build(VideoMetricConfig(enabled=True, enable_extended_videos=True))
    _, gen, tgt = golden["visits"][0]
    agg.record_initial_condition({k: v[:, :1] for k, v in gen.items()}, {k: v[:, :1] for k, v in tgt.items()})
    assert agg._video._pairs == {} and not agg._video._n.any() and agg.get_dataset().get("video") is None
    replay(agg, golden["visits"])
    assert agg._video._n.tolist() == [0, 2, 2, 2, 2, 2, 2]
    with pytest.raises(ValueError, match="past"):
        agg.record_batch(gen, tgt)                                           # steps 7..8 of 7
    assert agg._video._n.tolist() == [0, 2, 2, 2, 2, 2, 2]
