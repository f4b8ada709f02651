"""The host logic of the step diagnostics on the emulated C ABI (tests/_fake_stepdiag.py): ``CorrectionDeltaRecorder``'s pointer and
stride tables, ``RolloutEngine(step_diagnostics=True)`` and ``EnginePredict`` through ``run_evaluator``, and the fused path of
``CorrectionDeltaAggregator`` (row and weight tables, the table blob, accumulation over windows) against its torch path and against
the real reference's outputs (tests/golden/gen_step_diagnostics.pt)."""
import pytest
import torch

import ace_amd
from _fake_stepdiag import fake_stepdiag
from _util import conditioning_floor, load_golden
from ace_amd.aggregator import InferenceAggregatorConfig
from ace_amd.step_diagnostics import CorrectionDeltaAggregator, CorrectionDeltaRecorder, StepDiagnostics, StepDiagnosticsMetricConfig
from test_aggregator_cpu import oracle_sht_factory
from test_step_diagnostics_cpu import _reference_case


@pytest.fixture(scope="module")
def gold():
    return load_golden("gen_step_diagnostics.pt")


def _buffers(B, T, H, W, names, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {n: torch.randn(B, T, H, W, generator=g) for n in names}


def test_recorder_tables_snapshot_and_delta():
    B, T, H, W = 3, 4, 5, 7                                               # hw = 35: not a multiple of 4
    names = ["a", "b", "c"]
    out = _buffers(B, T, H, W, names)
    # "b" lives inside a larger allocation with a wider sample stride
    wide = torch.zeros(B, T + 2, H, W)
    wide[:, 1:T + 1] = out["b"]
    out["b"] = wide[:, 1:T + 1]

    def locate(n, s):
        p = out[n][:, s]
        return p.data_ptr(), p.stride(0)

    with fake_stepdiag():
        rec = CorrectionDeltaRecorder(names, B, (H, W), T, locate, "cpu")
        raw = {n: v.clone() for n, v in out.items()}
        for s in range(T):
            rec.snapshot(s, None)
            assert all(torch.equal(rec.buffer[k, :, s], raw[n][:, s]) for k, n in enumerate(names))
            assert float(rec.buffer[:, :, s + 1:].abs().sum()) == 0.0      # later time slots untouched
        for n in names:
            out[n].mul_(1.5).add_(0.25)                                   # the corrector edits the outputs in place
        rec.finish_window(None)
    delta = rec.delta()
    assert list(delta) == names
    for n in names:
        assert delta[n].shape == (B, T, H, W) and torch.equal(delta[n], out[n] - raw[n])
    assert float(wide[:, 0].abs().sum()) == 0.0 and float(wide[:, -1].abs().sum()) == 0.0          # nothing written beside the planes
    assert rec.step_diagnostics().sample_dim_size() == B


def test_recorder_refuses_planes_that_are_not_evenly_strided():
    B, T, H, W = 2, 3, 4, 4
    out = _buffers(B, T, H, W, ["a"])
    other = torch.zeros(B, T, H, W)

    def jumps(n, s):                                                      # step 2 lives in another allocation
        p = (other if s == 2 else out[n])[:, s]
        return p.data_ptr(), p.stride(0)

    def restrided(n, s):                                                  # step 1 has another sample stride
        p = out[n][:, s]
        return p.data_ptr(), p.stride(0) + (4 if s == 1 else 0)

    for locate in (jumps, restrided):
        with pytest.raises(ValueError, match="evenly strided"):
            CorrectionDeltaRecorder(["a"], B, (H, W), T, locate, "cpu")
    with pytest.raises(KeyError):
        CorrectionDeltaRecorder(["a"], B, (H, W), T, lambda n, s: None, "cpu")
    empty = CorrectionDeltaRecorder([], B, (H, W), T, jumps, "cpu")
    empty.snapshot(0, None)
    empty.finish_window(None)
    assert empty.delta() == {} and empty.step_diagnostics() is None


def test_engine_and_loop_on_the_emulated_abi(gold):
    """the golden rollout's stepper: the engine's deltas against the reference's (the bar of tests/test_step_diagnostics_cpu.py), the
    graph modes against each other bit for bit, and two windows through EnginePredict + run_evaluator"""
    from ace_amd.evaluator import InferenceEvaluatorAggregatorConfig
    from ace_amd.inference import EnginePredict, ForcingWindows, InferenceData, run_evaluator
    from ace_amd.rollout import RolloutEngine
    from ace_amd.step_diagnostics import WindowData
    case = gold["rollout"]
    loaded = ace_amd.load_stepper(case["state"], device="cpu")
    stepper = loaded.stepper
    floor = conditioning_floor(case)
    runs = {}
    with fake_stepdiag():
        for graph in (None, "step"):
            out, _ = RolloutEngine(stepper, batch=2, n_forward_steps=3, graph=graph, step_diagnostics=True).predict(case["ic"], case["forcing"])
            assert isinstance(out, WindowData)
            runs[graph] = ({k: v.clone() for k, v in out.items()}, {k: v.clone() for k, v in out.step_diagnostics.delta.items()})
        plain, _ = RolloutEngine(stepper, batch=2, n_forward_steps=3, graph="step").predict(case["ic"], case["forcing"])
        assert type(plain) is dict
        for k, v in plain.items():
            assert torch.equal(v, runs["step"][0][k]), k                  # the flag changes no output bit
        # the loop: windows of 2 + 1 steps, scalars, maps and series
        logs = {}
        for cfg, flag in ((StepDiagnosticsMetricConfig(correction_maps=True), True), (None, True), (None, False)):
            agg = InferenceEvaluatorAggregatorConfig(step_diagnostics=cfg).build(loaded.dataset_info, 1, 3, normalize=stepper.normalizer,
                                                                                 sht_factory=oracle_sht_factory)
            loader = ForcingWindows(case["forcing"], total_forward_steps=3, forward_steps_in_memory=2, device="cpu")
            run_evaluator(EnginePredict(stepper, batch=2, graph="step", step_diagnostics=flag), InferenceData(case["ic"], loader), agg)
            logs[(cfg is not None, flag)] = (agg.get_inference_logs(), agg.get_dataset(), agg)
    delta = runs[None][1]
    assert set(delta) == set(case["delta"])
    for k in delta:
        assert torch.equal(delta[k], runs["step"][1][k]), k
        for s in range(3):
            scale = float(case["steps"][s][k].abs().max())
            err = float((delta[k][:, s] - case["delta"][k][:, s]).abs().max()) / scale
            assert err <= 2.0 * max(1e-6, 3.0 * floor[s][k]), (k, s, err)
    rows, ds, agg = logs[(True, True)]
    names = sorted(delta)
    assert {f"mean_norm/{m}/{n}" for n in names for m in ("weighted_correction_magnitude", "weighted_correction_std")} <= set(rows[1])
    assert {f"time_mean_norm/correction_magnitude/{n}" for n in names} | {f"time_mean_norm/correction_map/{n}" for n in names} \
        <= set(rows[-1])
    assert {"time_mean_norm_correction", "mean_norm_correction"} <= set(ds)
    # recorded at i_time_start = the steps seen so far: index 0 is the initial condition's, 1 .. 3 the three steps, each once
    series = torch.tensor([r["mean_norm/weighted_correction_magnitude/PRESsfc"] for r in rows])
    assert torch.isnan(series[0]) and torch.isfinite(series[1:]).all() and agg._correction._n_batches == [0, 1, 1, 1]
    # the same deltas recorded by hand give the same series: the second window's clone was not the first's buffer
    by_hand = CorrectionDeltaAggregator(agg, stepper.normalizer, 4, record_maps=True)
    by_hand.record_batch(StepDiagnostics(delta={k: v[:, :2] for k, v in delta.items()}), 1)
    by_hand.record_batch(StepDiagnostics(delta={k: v[:, 2:] for k, v in delta.items()}), 3)
    want = by_hand.series_data()["weighted_correction_magnitude"]["PRESsfc"]
    torch.testing.assert_close(series[1:].float(), want[1:], rtol=1e-5, atol=0.0)
    # left None: the logs of the tree without the option, key for key, whether or not the predict function attaches the record
    for key in ((False, True), (False, False)):
        other_rows, other_ds, _ = logs[key]
        assert [set(r) for r in other_rows] == [{k for k in r if "correction" not in k} for r in rows]
        assert set(other_ds) == set(ds) - {"time_mean_norm_correction", "mean_norm_correction"}


@pytest.mark.parametrize("series", [True, False])
def test_fused_path_on_the_emulated_abi_against_the_torch_path_and_the_reference(gold, series):
    info, delta, norm, want = _reference_case(gold)
    host = InferenceAggregatorConfig().build(info, want["n_timesteps"], sht_factory=oracle_sht_factory)
    T = next(iter(delta.values())).shape[1]
    aggs = {}
    with fake_stepdiag():
        for fused in (True, False):
            agg = CorrectionDeltaAggregator(host, norm, want["n_timesteps"], record_scalars=True, record_maps=True, time_series=series)
            if fused:
                agg.route = lambda d: "fused"                              # the device check is the only thing the host lacks
            for sl, t0 in zip((slice(0, 2), slice(2, T)), want["i_time_start"]):
                # non-contiguous views: the planes are read in place through the table
                agg.record_batch(StepDiagnostics(delta={k: v[:, sl] for k, v in delta.items()}), t0)
            aggs[fused] = agg
    fused, torch_path = aggs[True], aggs[False]
    assert fused._path == "fused" and fused.launches() == 2 and torch_path._path == "torch"
    flog, tlog = fused.summary_logs(), torch_path.summary_logs()
    assert set(flog) == set(tlog)
    ref = want["fp32"]
    for n in delta:
        assert flog[f"time_mean_norm/correction_magnitude/{n}"] == pytest.approx(float(ref["correction_magnitude"][n]), rel=1e-6)
        torch.testing.assert_close(flog[f"time_mean_norm/correction_map/{n}"], ref["signed"][n], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(flog[f"time_mean_norm/correction_map/{n}"], tlog[f"time_mean_norm/correction_map/{n}"],
                                   rtol=1e-5, atol=1e-6)
    if not series:
        assert fused.series_rows() == [] and fused._scratch_series is not None and fused._series is not None
        assert float(fused._series.abs().sum()) == 0.0                    # the unlogged series went to the scratch
        return
    fs, ts = fused.series_data(), torch_path.series_data()
    for metric in fs:
        for n in delta:
            torch.testing.assert_close(fs[metric][n], ref["series"][metric][n], rtol=2e-5, atol=1e-6, equal_nan=True)
            torch.testing.assert_close(fs[metric][n], ts[metric][n], rtol=2e-5, atol=1e-6, equal_nan=True)
