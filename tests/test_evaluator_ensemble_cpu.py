"""The evaluator's step means and ensemble metrics on the torch path (ace_amd/evaluator.py ``_StepMeans``, ``_Ensembles``) against
tests/golden/gen_ensemble.pt, which the reference's own classes produced on the records of tests/_ensemble_cases.py
(tests/golden/make_golden_ensemble.py), the build rules of the two configurations, and ``inference.repeat_members``.

Bars.  The golden holds every quantity twice: "f32", the reference's classes in the reference's dtypes, and "f64", the same classes
on fp64 inputs.  The torch path is held to the fp64 numbers within 4 x the gap between the two, per output (the largest gap over
a map); where the two agree exactly - the -1 of the spread-skill convention, the 0 of a prescribed field, NaN - so must the torch
path.  NaN has to sit in the same places.  A ``channel_mean`` is the average of per-name scalars, so its error is at most the
largest per-name error; it is held to 4 x the largest gap among the per-name scalars of its metric (and its own), not to the gap of
the two channel means alone, which is one sample of a rounding and can be small by luck (1.4e-9 for the norm step mean at step 5,
whose two names are off by 1.5e-8 and 2.4e-9)."""
import logging
import math
import os

import pytest
import torch

import _ensemble_cases as C
from ace_amd.evaluator import EnsembleMetricConfig, HistogramMetricConfig, InferenceEvaluatorAggregatorConfig, MetricConfig, \
    NearZeroFractionMetricConfig, SeasonalMetricConfig, StepMeanMetricConfig, TrendMetricConfig
from ace_amd.inference import repeat_members
from test_evaluator_calendar_cpu import config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_ensemble.pt")
# (key, n_ic_steps, step, target, channel_mean_names, variables): as tests/golden/make_golden_ensemble.py lists them
STEP_MEANS = [("sm_2", 1, 2, "denorm", None, None), ("sm_2_only_a", 1, 2, "denorm", None, ["a"]),
              ("sm_5_norm", 1, 5, "norm", None, None), ("sm_5_norm_names", 1, 5, "norm", ["a"], ["b"]),
              ("sm_2_ic2", 2, 2, "denorm", None, None)]
ENSEMBLES = [("en_2", 1, 2, "denorm", None, None), ("en_5_norm", 1, 5, "norm", None, None),
             ("en_5_norm_names", 1, 5, "norm", ["a"], None), ("en_2_ic2", 2, 2, "denorm", None, None)]


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def step_mean(entry):
    _, _, step, target, names, variables = entry
    return StepMeanMetricConfig(step=step, target=target, channel_mean_names=names, variables=variables, name="x")


def ensemble(entry):
    _, _, step, target, names, _ = entry
    return EnsembleMetricConfig(step=step, target=target, channel_mean_names=names, log_mean_maps=True, name="x")


def run(c, fused=False, device="cpu", n_members=C.E, channel_mean_names=None, **metrics):
    agg = config(**metrics).build(c["info"], c["n_ic_steps"], C.N_FORWARD, C.stats(device), n_ensemble_per_ic=n_members,
                                  channel_mean_names=channel_mean_names)
    agg.fused = fused
    on = lambda d: {n: v.to(device) for n, v in d.items()}                      # noqa: E731
    agg.record_initial_condition(on(c["ic"][0]), on(c["ic"][1]))
    for gen, tgt, _ in c["windows"]:
        assert agg.record_batch(on(gen), on(tgt)) == []
    return agg


def held(got, golden, key):
    """every output of the golden entry in ``got``, and no other; NaN in the same places; within 4 x the fp32 - fp64 gap"""
    f32, f64 = golden["f32"][key], golden["f64"][key]
    assert sorted(got) == sorted(f64)
    for k, want in f64.items():
        g, w, lo = (torch.as_tensor(v, dtype=torch.float64) for v in (got[k], want, f32[k]))
        assert torch.equal(g.isnan(), w.isnan()), k
        gap = float((lo - w).abs().nan_to_num().max())
        if k.endswith("/channel_mean"):
            metric = k.rsplit("/", 1)[0]
            gap = max([gap] + [abs(f32[m] - f64[m]) for m in f64 if m.rsplit("/", 1)[0] == metric and not math.isnan(f64[m])])
        err = float((g - w).abs().nan_to_num().max())
        print(f"ENSCPU {key} {k}: err {err:.3e} gap {gap:.3e}")
        assert err <= 4 * gap, (k, err, gap)


def test_the_golden_was_made_from_these_records(golden):
    for n in (1, 2):
        assert golden["checksum"][n] == C.checksum(C.case(n))


@pytest.mark.parametrize("entry", STEP_MEANS, ids=[e[0] for e in STEP_MEANS])
def test_step_means_against_the_reference(golden, entry):
    """denorm and norm, a ``variables`` filter, ``channel_mean_names``, the all-NaN name ``c`` left out of the channel mean, a step
    in the second window, and ``n_ic_steps = 2``, where the step mean sits at ``step + 1``"""
    agg = run(C.case(entry[1]), step_means=[step_mean(entry)])
    logs = agg.get_summary_logs()
    held(logs, golden, entry[0])
    assert {k.replace("/", "-") for k in logs} == {f"x-{k}" for k in agg.get_dataset()["x"]}


def test_the_channel_mean_leaves_the_all_nan_target_out(golden):
    agg = run(C.case(), step_means=[step_mean(STEP_MEANS[2])])
    logs = agg.get_summary_logs()
    assert math.isnan(logs["x/weighted_rmse/c"])
    assert logs["x/weighted_rmse/channel_mean"] == pytest.approx((logs["x/weighted_rmse/a"] + logs["x/weighted_rmse/b"]) / 2, rel=1e-6)
    # the aggregator's names serve an entry that has none of its own; a name that is not there raises
    agg = run(C.case(), channel_mean_names=["a"], step_means=[step_mean(STEP_MEANS[2])])
    assert agg.get_summary_logs()["x/weighted_rmse/channel_mean"] == pytest.approx(logs["x/weighted_rmse/a"], rel=1e-6)
    agg = run(C.case(), channel_mean_names=["nope"], step_means=[step_mean(STEP_MEANS[2])])
    with pytest.raises(KeyError, match="nope"):
        agg.get_summary_logs()


@pytest.mark.parametrize("entry", ENSEMBLES, ids=[e[0] for e in ENSEMBLES])
def test_ensembles_against_the_reference(golden, entry):
    """denorm and norm with the maps, a step in the second window, and ``n_ic_steps = 2``, where the ensemble entry still sits at
    ``step`` (the step mean of the same ``step`` sits one index later)"""
    agg = run(C.case(entry[1]), ensembles=[ensemble(entry)])
    logs = agg.get_summary_logs()
    held(logs, golden, entry[0])
    assert {k.replace("/", "-") for k in logs} == {f"x-{k}" for k in agg.get_dataset()["x"]}
    if entry[0] == "en_2":
        ssr = logs["x/ssr_bias/mean_map/a"]
        assert bool((ssr[C.PRESCRIBED] == 0).all())                            # prescribed cells: 0, not the -1 floor
        assert bool((ssr[C.CALM] == -1).all())                                  # zero clamped skill: -1 by convention
        assert bool((logs["x/ssr_bias/mean_map/c"] == -1).all())                # NaN skill is not > 0
        assert not any("channel_mean" in k for k in logs)
    if entry[0] == "en_5_norm":
        want = (logs["x/crps/a"] + logs["x/crps/b"]) / 2                        # c's target is all NaN
        assert logs["x/crps/channel_mean"] == pytest.approx(want, rel=1e-6)


def test_without_log_mean_maps_only_the_scalars_are_reported():
    agg = run(C.case(), ensembles=[EnsembleMetricConfig(step=2, variables=["a", "b"])])
    assert sorted(agg.get_summary_logs()) == sorted(f"ensemble_step_2/{m}/{n}" for m in ("crps", "ensemble_mean_rmse", "ssr_bias")
                                                    for n in ("a", "b"))


def test_default_names():
    assert StepMeanMetricConfig(step=3).name == "mean_step_3" and StepMeanMetricConfig(step=3, target="norm").name == "mean_step_3_norm"
    assert EnsembleMetricConfig().name == "ensemble_step_20" and EnsembleMetricConfig(step=4, target="norm").name == "ensemble_step_4_norm"
    with pytest.raises(ValueError):
        StepMeanMetricConfig(target="raw")


def test_one_member_per_initial_condition_reports_no_ensemble_keys():
    agg = run(C.case(), n_members=1, ensembles=[EnsembleMetricConfig(step=2)], step_means=[StepMeanMetricConfig(step=2)])
    assert agg.n_ensemble_per_ic == 1
    logs = agg.get_summary_logs()
    assert logs and all(k.startswith("mean_step_2/") for k in logs)
    assert "ensemble_step_2" not in agg.get_dataset()


def test_bare_entries_are_still_skipped_and_typed_ones_built(caplog):
    c = C.case()
    default = InferenceEvaluatorAggregatorConfig().build(c["info"], 1, C.N_FORWARD, C.stats())
    assert default.skipped[:2] == ["step_means", "ensembles"]
    with caplog.at_level(logging.WARNING):
        agg = run(c, step_means=[MetricConfig(), StepMeanMetricConfig(step=2)], ensembles=[EnsembleMetricConfig(step=2), MetricConfig()])
    assert agg.skipped == ["step_means", "ensembles"]
    assert "omitting: step_means, ensembles" in caplog.text
    logs = agg.get_summary_logs()
    assert "mean_step_2/weighted_rmse/a" in logs and "ensemble_step_2/crps/a" in logs
    with pytest.raises(NotImplementedError, match="step_means"):
        config(step_means=[MetricConfig(strict=True)]).build(c["info"], 1, C.N_FORWARD, C.stats())


def test_a_step_past_the_rollout_is_skipped_or_raises():
    c = C.case()
    agg = config(step_means=[StepMeanMetricConfig(step=7)], ensembles=[EnsembleMetricConfig(step=20)]).build(
        c["info"], 1, C.N_FORWARD, C.stats(), n_ensemble_per_ic=C.E)
    assert agg.skipped == ["mean_step_7", "ensemble_step_20"]
    with pytest.raises(NotImplementedError, match="step_mean step 7 exceeds n_forward_steps=6"):
        config(step_means=[StepMeanMetricConfig(step=7, strict=True)]).build(c["info"], 1, C.N_FORWARD, C.stats())
    with pytest.raises(NotImplementedError, match="ensemble step 7 exceeds n_forward_steps=6"):
        config(ensembles=[EnsembleMetricConfig(step=7, strict=True)]).build(c["info"], 1, C.N_FORWARD, C.stats())
    config(step_means=[StepMeanMetricConfig(step=6, strict=True)]).build(c["info"], 1, C.N_FORWARD, C.stats())


def test_duplicate_names_raise():
    c = C.case()
    with pytest.raises(ValueError, match="mean_step_2"):
        config(step_means=[StepMeanMetricConfig(step=2), StepMeanMetricConfig(step=2)]).build(c["info"], 1, C.N_FORWARD, C.stats())
    with pytest.raises(ValueError, match="'x'"):
        config(step_means=[StepMeanMetricConfig(step=2, name="x")], ensembles=[EnsembleMetricConfig(step=3, name="x")]).build(
            c["info"], 1, C.N_FORWARD, C.stats())
    # the labels of the other built metrics head blocks of the same logs and dataset
    for taken in (dict(mean_denorm=MetricConfig()), dict(trend=TrendMetricConfig(enabled=True)),
                  dict(near_zero_fraction=NearZeroFractionMetricConfig(enabled=True, variables=["a"], name="nzf")),
                  dict(histogram=HistogramMetricConfig(enabled=True)), dict(seasonal=SeasonalMetricConfig(enabled=True))):
        label = {"mean_denorm": "mean", "near_zero_fraction": "nzf"}.get(list(taken)[0], list(taken)[0])
        with pytest.raises(ValueError, match=f"'{label}'"):
            config(ensembles=[EnsembleMetricConfig(step=2, name=label)], **taken).build(c["info"], 1, C.N_FORWARD, C.stats())
        config(ensembles=[EnsembleMetricConfig(step=2, name=label + "_too")], **taken).build(c["info"], 1, C.N_FORWARD, C.stats())


def test_a_batch_that_is_no_multiple_of_the_members_raises():
    c = C.case()
    agg = config(ensembles=[EnsembleMetricConfig(step=2)]).build(c["info"], 1, C.N_FORWARD, C.stats(), n_ensemble_per_ic=4)
    agg.fused = False
    gen, tgt, _ = c["windows"][0]
    with pytest.raises(ValueError, match="n_ensemble_per_ic"):
        agg.record_batch(gen, tgt)
    with pytest.raises(ValueError):
        config().build(c["info"], 1, C.N_FORWARD, C.stats(), n_ensemble_per_ic=0)


def test_step_means_work_with_the_mean_series_off(golden):
    """the series rows are recorded for the step mean alone; the ``mean`` and ``mean_norm`` labels stay out of every output"""
    agg = run(C.case(), step_means=[step_mean(STEP_MEANS[0])])
    rows = agg.get_inference_logs()
    assert len(rows) == 1 and all(k.startswith("x/") for k in rows[0])
    assert sorted(agg.get_dataset()) == ["x"]
    with_series = run(C.case(), mean_denorm=MetricConfig(), mean_norm=MetricConfig(), step_means=[step_mean(STEP_MEANS[0])])
    assert {k: v for k, v in with_series.get_summary_logs().items() if k.startswith("x/")} == \
        pytest.approx(agg.get_summary_logs(), nan_ok=True)
    assert "mean" in with_series.get_dataset() and "mean_norm" in with_series.get_dataset()


def test_flush_diagnostics_writes_a_file_per_new_label(tmp_path):
    c = C.case()
    agg = config(step_means=[StepMeanMetricConfig(step=2), StepMeanMetricConfig(step=5, target="norm")],
                 ensembles=[EnsembleMetricConfig(step=2, log_mean_maps=True)]).build(
        c["info"], 1, C.N_FORWARD, C.stats(), output_dir=str(tmp_path), save_diagnostics=True, n_ensemble_per_ic=C.E)
    agg.fused = False
    agg.record_initial_condition(*c["ic"])
    for gen, tgt, _ in c["windows"]:
        agg.record_batch(gen, tgt)
    agg.flush_diagnostics()
    assert sorted(os.listdir(tmp_path)) == ["ensemble_step_2_diagnostics.pt", "mean_step_2_diagnostics.pt",
                                            "mean_step_5_norm_diagnostics.pt"]
    saved = torch.load(os.path.join(tmp_path, "ensemble_step_2_diagnostics.pt"))
    assert saved["crps-mean_map-a"].shape == (C.H, C.W) and float(saved["crps-a"]) == agg.get_summary_logs()["ensemble_step_2/crps/a"]
    assert "weighted_rmse-channel_mean" in torch.load(os.path.join(tmp_path, "mean_step_5_norm_diagnostics.pt"))


def test_repeat_members():
    d = {"a": torch.arange(24.0).reshape(2, 3, 4), "b": torch.arange(2.0)}
    out = repeat_members(d, 3)
    assert out["a"].shape == (6, 3, 4) and out["b"].tolist() == [0, 0, 0, 1, 1, 1]
    for i in range(2):
        for e in range(3):
            assert torch.equal(out["a"][i * 3 + e], d["a"][i])                  # sample b = i * n + e
    same = repeat_members(d, 1)
    assert same is not d and all(same[k] is d[k] for k in d)
    with pytest.raises(ValueError):
        repeat_members(d, 0)
