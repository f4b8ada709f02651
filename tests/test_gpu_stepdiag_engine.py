"""The corrector deltas on the device: ``CorrectionDeltaRecorder`` around ``FusedPhysics`` on the buffers of tests/_physics_ref.py,
and ``RolloutEngine(step_diagnostics=True)`` / ``EnginePredict`` / ``run_evaluator`` / ``CorrectionDeltaAggregator`` on the reference's own small stepper
(tests/golden/gen_step_diagnostics.pt: the 16-wide 2-layer SFNO of the stepper goldens with the ace2_like corrector, a prescribed-SST
ocean and a prescribed prognostic name)."""
import copy

import pytest
import torch

from _util import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


# ---- the recorder around the fused physics -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 4, 8, 1), (3, 9, 57, 4)], ids=["B1-4x8x1", "B3-9x57x4"])      # smallest; three workgroups
@pytest.mark.parametrize("name", ["ace2_like", "force_positive"])
def test_recorder_delta_is_out_minus_network_output(dev, shape, name):
    import _physics_ref as P
    from ace_amd import _lib
    from ace_amd.corrector import AtmosphereCorrectorConfig
    from ace_amd.step_diagnostics import CorrectionDeltaRecorder
    c, config = P.case(*shape), P.config_for(name, shape[3])
    phys, out, keep = P.physics_buffers(dev, c, config)
    corrector = AtmosphereCorrectorConfig.from_state(config).get_corrector(P.dataset_info(c))
    names = corrector.modified_names(sorted(c["gen0"]))
    B, H, W = c["gen0"]["PRESsfc"].shape
    T = 2

    def locate(n, s):
        p = out[n][:, s]
        return p.data_ptr(), p.stride(0)

    rec = CorrectionDeltaRecorder(names, B, (H, W), T, locate, dev)
    st = _lib.current_stream()
    phys.reset(st)
    for s in range(T):
        for n, v in c[f"gen{s}"].items():
            out[n][:, s].copy_(v.to(dev))
        rec.snapshot(s, st)
        phys.apply(s, st)
    rec.finish_window(st)
    torch.cuda.synchronize()
    delta = rec.delta()
    assert list(delta) == names and len(names) > 0
    changed = set()
    for s in range(T):
        for n, gen in c[f"gen{s}"].items():
            after = out[n][:, s].cpu()
            if n in delta:
                assert torch.equal(delta[n][:, s].cpu(), after - gen), (n, s)       # fl32(out_after - gen_s), bit for bit
                changed.add(n) if not torch.equal(after, gen) else None
            else:
                assert torch.equal(after, gen), (n, s)                               # outside modified_names: bitwise untouched
    assert changed                                                                   # the corrector did write


# ---- the engine ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    return load_golden("gen_step_diagnostics.pt")["rollout"]


def _stepper(case, dev, corrector=True):
    import ace_amd
    state = case["state"]
    if not corrector:
        state = copy.deepcopy(state)
        state["config"]["step"]["config"]["corrector"] = {"type": "atmosphere_corrector", "config": {}}
    return ace_amd.load_stepper(state, device=dev)


def _window(case, dev):
    return {k: v.to(dev) for k, v in case["ic"].items()}, {k: v.to(dev) for k, v in case["forcing"].items()}


@pytest.fixture(scope="module")
def engine_runs(case, dev):
    """the window of the golden rollout through the engine in its three graph modes with the flag, and without it"""
    from ace_amd.rollout import RolloutEngine
    stepper = _stepper(case, dev).stepper
    ic, forcing = _window(case, dev)
    runs = {}
    for graph in (None, "step", "window"):
        eng = RolloutEngine(stepper, batch=2, n_forward_steps=3, graph=graph, step_diagnostics=True)
        out, _ = eng.predict(ic, forcing)
        torch.cuda.synchronize()
        runs[graph] = ({k: v.clone() for k, v in out.items()}, {k: v.clone() for k, v in out.step_diagnostics.delta.items()})
    eng = RolloutEngine(stepper, batch=2, n_forward_steps=3, graph="step")
    out, _ = eng.predict(ic, forcing)
    torch.cuda.synchronize()
    assert type(out) is dict                                                         # as before the option existed
    runs["plain"] = ({k: v.clone() for k, v in out.items()}, None)
    return stepper, runs


def test_engine_modes_agree_bitwise_and_outputs_are_unchanged(case, engine_runs):
    stepper, runs = engine_runs
    out0, delta0 = runs[None]
    assert set(delta0) == set(case["delta"]) and case["prescribed"] not in delta0
    for graph in ("step", "window"):
        out, delta = runs[graph]
        for k in out0:
            assert torch.equal(out[k], out0[k]), (graph, k)
        for k in delta0:
            assert torch.equal(delta[k], delta0[k]), (graph, k)
    for k, v in runs["plain"][0].items():
        assert torch.equal(v, out0[k]), k                                            # the flag changes no output bit
    assert any(float(d.abs().max()) > 0 for d in delta0.values())


def test_out_minus_delta_is_the_uncorrected_network_output(case, engine_runs, dev):
    """Step 0 of an engine on the same stepper with the corrector removed is the network output the recorder snapshots: the delta
    is bit for bit fl32(out - that output).  (Stated this way round because fl32(out - delta) need not give the output back: where
    the corrector takes a value to near zero, out - raw is rounded and the subtraction does not invert - measured on PRATEsfc.)"""
    from ace_amd.rollout import RolloutEngine
    _, runs = engine_runs
    out0, delta0 = runs[None]
    bare = _stepper(case, dev, corrector=False).stepper
    assert bare._step_obj._corrector is None
    ic, forcing = _window(case, dev)
    raw, _ = RolloutEngine(bare, batch=2, n_forward_steps=3, graph="step").predict(ic, forcing)
    torch.cuda.synchronize()
    for k, d in delta0.items():
        # step 0 sees the same inputs with or without the corrector; delta = fl32(out - raw) exactly, so out - raw is the delta
        assert torch.equal(out0[k][:, 0] - raw[k][:, 0], d[:, 0]), k


def test_engine_deltas_agree_with_the_eager_stepper(case, engine_runs, dev):
    stepper, runs = engine_runs
    ic, forcing = _window(case, dev)
    out, _ = stepper.predict(ic, forcing, step_diagnostics=True)
    torch.cuda.synchronize()
    eager = out.step_diagnostics.delta
    assert set(eager) == set(runs[None][1])
    for k, d in runs[None][1].items():
        # test_fused_physics_vs_reference_corrector holds the fields to 2e-6 of their maximum; a delta is a difference of two
        for s in range(d.shape[1]):
            scale = float(out[k][:, s].abs().max())
            err = float((d[:, s] - eager[k][:, s]).abs().max()) / scale
            print(f"{k} step {s}: |engine - eager| / max|field| = {err:.3e}")
            assert err <= 4e-6, (k, s, err)


STD_LIKE = ("weighted_correction_std",)


def test_fused_aggregator_on_the_engine_deltas_against_the_torch_path(case, dev):
    """two windows (2 + 1 steps) of ``RolloutEngine(step_diagnostics=True)`` recorded by ``CorrectionDeltaAggregator`` on its fused and
    on its torch path, at the bar the evaluator's fused-against-torch checks hold (tests/test_gpu_evaluator_aggregator.py: 1e-6 of the
    scale, 1e-5 for the std-like series, a series held relative to the magnitude of its field when that is the larger)."""
    from ace_amd.aggregator import InferenceAggregatorConfig
    from ace_amd.rollout import RolloutEngine
    from ace_amd.step_diagnostics import StepDiagnostics, StepDiagnosticsMetricConfig
    loaded = _stepper(case, dev)
    stepper, info = loaded.stepper, loaded.dataset_info
    ic, forcing = _window(case, dev)
    windows = []
    state = ic
    for sl, T in ((slice(0, 3), 2), (slice(2, 4), 1)):
        eng = RolloutEngine(stepper, batch=2, n_forward_steps=T, graph="step", step_diagnostics=True)
        out, state = eng.predict(state, {k: v[:, sl] for k, v in forcing.items()})
        windows.append(StepDiagnostics(delta={k: v.clone() for k, v in out.step_diagnostics.delta.items()}))
    torch.cuda.synchronize()
    host = InferenceAggregatorConfig().build(info, 4)
    got = {}
    for fused in (True, False):
        agg = StepDiagnosticsMetricConfig(correction_maps=True).build(host, 4, True, stepper.normalizer)
        agg.fused = fused
        agg.record_batch(windows[0], 1)
        agg.record_batch(windows[1], 3)
        torch.cuda.synchronize()
        assert agg._path == ("fused" if fused else "torch") and agg.launches() == (2 if fused else 0)
        got[fused] = ({**agg.summary_logs(), **{k: torch.tensor([r[k] for r in agg.series_rows()]) for k in agg.series_rows()[0]}},
                      agg.datasets())
    names = sorted(case["delta"])
    flog, tlog = got[True][0], got[False][0]
    assert set(flog) == set(tlog) == {f"time_mean_norm/correction_magnitude/{n}" for n in names} | \
        {f"time_mean_norm/correction_map/{n}" for n in names} | \
        {f"mean_norm/{m}/{n}" for n in names for m in ("weighted_correction_magnitude", "weighted_correction_std")}
    for k in flog:
        f, t = torch.as_tensor(flog[k], dtype=torch.float64).cpu(), torch.as_tensor(tlog[k], dtype=torch.float64).cpu()
        fin = torch.isfinite(t)
        assert torch.equal(torch.isfinite(f), fin), k
        scale = max(float(t[fin].abs().max()), 1e-30)
        if "weighted_correction_std" in k:
            # the fp32 torch path forms the std of a nearly uniform correction (the dry-air shift) by cancellation
            mag = tlog[k.replace("weighted_correction_std", "weighted_correction_magnitude")]
            scale = max(scale, float(mag[torch.isfinite(mag)].abs().max()))
        err = float((f[fin] - t[fin]).abs().max()) / scale
        print(f"{k}: fused against torch {err:.3e}")
        assert err <= (1e-5 if any(m in k for m in STD_LIKE) else 1e-6), (k, err)
    series = flog["mean_norm/weighted_correction_std/PRESsfc"]
    assert torch.isnan(series[0]) and torch.isfinite(series[1:]).all()          # index 0 was never recorded
    assert set(got[True][1]) == {"time_mean_norm_correction", "mean_norm_correction"}


def test_run_evaluator_logs_the_correction_metrics(case, dev):
    """two windows (2 + 1 steps) through EnginePredict + run_evaluator: the fused path's correction logs against the torch path's, at
    the bar the evaluator's other fused-against-torch checks hold (tests/test_gpu_evaluator_aggregator.py: 1e-6 of the scale,
    1e-5 for the std-like series); with the configuration left None the logs are those without the option, key for key."""
    from ace_amd.evaluator import InferenceEvaluatorAggregatorConfig
    from ace_amd.inference import EnginePredict, ForcingWindows, InferenceData, run_evaluator
    from ace_amd.step_diagnostics import StepDiagnosticsMetricConfig, WindowData
    loaded = _stepper(case, dev)
    stepper, info = loaded.stepper, loaded.dataset_info
    ic = {k: v.to(dev) for k, v in case["ic"].items()}
    got = {}
    for key, cfg, fused, flag in (("fused", StepDiagnosticsMetricConfig(correction_maps=True), True, True),
                                  ("torch", StepDiagnosticsMetricConfig(correction_maps=True), False, True),
                                  ("none", None, True, False), ("none_flag", None, True, True)):
        loader = ForcingWindows(case["forcing"], total_forward_steps=3, forward_steps_in_memory=2, device=dev)
        agg = InferenceEvaluatorAggregatorConfig(step_diagnostics=cfg).build(info, 1, 3, normalize=stepper.normalizer)
        agg.fused = fused
        run_evaluator(EnginePredict(stepper, batch=2, graph="step", step_diagnostics=flag), InferenceData(ic, loader), agg)
        torch.cuda.synchronize()
        got[key] = (agg, agg.get_inference_logs(), agg.get_dataset())
    assert got["fused"][0]._correction._path == "fused" and got["torch"][0]._correction._path == "torch"
    assert got["fused"][0]._correction.launches() == 2
    names = sorted(case["delta"])
    flogs, tlogs = got["fused"][1], got["torch"][1]
    assert [set(r) for r in flogs] == [set(r) for r in tlogs]
    keys = [k for k in flogs[-1] if "correction" in k]
    assert {f"time_mean_norm/correction_magnitude/{n}" for n in names} | {f"time_mean_norm/correction_map/{n}" for n in names} | \
        {f"mean_norm/{m}/{n}" for n in names for m in ("weighted_correction_magnitude", "weighted_correction_std")} == set(keys)
    for k in keys:
        rows = flogs if k.startswith("mean_norm/") else flogs[-1:]
        trows = tlogs if k.startswith("mean_norm/") else tlogs[-1:]
        f = torch.stack([torch.as_tensor(r[k], dtype=torch.float64) for r in rows])
        t = torch.stack([torch.as_tensor(r[k], dtype=torch.float64) for r in trows])
        fin = torch.isfinite(t)
        assert torch.equal(torch.isfinite(f), fin), k
        scale = max(float(t[fin].abs().max()), 1e-30)
        if "weighted_correction_std" in k:
            # as there, a series is held relative to the magnitude of its field, wmean(|n|), when that is the larger: the fp32
            # torch path forms the std of a nearly uniform correction (the dry-air shift) by cancellation
            mag = torch.tensor([r[k.replace("weighted_correction_std", "weighted_correction_magnitude")] for r in trows])
            scale = max(scale, float(mag[torch.isfinite(mag)].abs().max()))
        err = float((f[fin] - t[fin]).abs().max()) / scale
        print(f"{k}: fused against torch {err:.3e}")
        assert err <= (1e-5 if any(m in k for m in STD_LIKE) else 1e-6), (k, err)
    assert torch.isnan(torch.tensor(flogs[0]["mean_norm/weighted_correction_std/PRESsfc"]))       # the initial condition's index
    assert {"time_mean_norm_correction", "mean_norm_correction"} <= set(got["fused"][2])
    # left None: the logs and datasets of the tree without the option, with or without the predict function's flag
    for key in ("none", "none_flag"):
        assert not any("correction" in k for r in got[key][1] for k in r) and not any("correction" in k for k in got[key][2])
        assert [set(r) for r in got[key][1]] == [set(r) - set(keys) for r in flogs]
    assert set(got["none"][2]) == set(got["fused"][2]) - {"time_mean_norm_correction", "mean_norm_correction"}
