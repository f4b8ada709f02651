"""Corrector step diagnostics on the CPU (ace_amd/step_diagnostics.py) against the REAL reference (tests/golden/gen_step_diagnostics.pt,
tests/golden/make_golden_step_diagnostics.py): the corrector's tracked changes and ``modified_names``, the deltas of the eager step
and of ``Stepper.predict(step_diagnostics=True)``, the configuration of both aggregators and the torch path of
``CorrectionDeltaAggregator``."""
import dataclasses

import pytest
import torch

import ace_amd
from _util import load_golden
from ace_amd.aggregator import InferenceAggregatorConfig
from ace_amd.corrector import AtmosphereCorrectorConfig
from ace_amd.evaluator import InferenceEvaluatorAggregatorConfig
from ace_amd.normalizer import StandardNormalizer
from ace_amd.registry import Module
from ace_amd.step_diagnostics import CorrectionDeltaAggregator, StepDiagnostics, StepDiagnosticsMetricConfig, WindowData
from test_aggregator_cpu import make_case, oracle_sht_factory
from test_corrector_cpu import CONFIGS, _info


@pytest.fixture(scope="module")
def gold():
    return load_golden("gen_step_diagnostics.pt")


@pytest.fixture(scope="module")
def gold_corrector():
    return load_golden("gen_corrector.pt")


# ---- the corrector's modified names and deltas -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_modified_names_and_deltas_match_the_reference(gold, gold_corrector, name):
    g, want = gold_corrector, gold["corrector"][name]
    corrector = AtmosphereCorrectorConfig.from_state(CONFIGS[name]).get_corrector(_info(g))
    assert set(corrector.modified_names(list(g["gen0"]))) == set(want["step0"])         # from the configuration alone
    out0, st0 = corrector(g["input0"], g["gen0"], g["forcing"], None)
    assert set(corrector.last_modified_names) == set(want["step0"])
    assert sorted(corrector.last_modified_names) == sorted(corrector.modified_names(list(g["gen0"])))
    out1, _ = corrector({**out0, **g["forcing"]}, g["gen1"], g["forcing"], st0)
    assert set(corrector.last_modified_names) == set(want["step1"])
    for out, gen, exp in ((out0, g["gen0"], want["step0"]), (out1, g["gen1"], want["step1"])):
        for k, v in exp.items():
            # both are fp32 subtractions of outputs that are themselves only close (test_corrector_cpu.py holds the fields to
            # rtol 1e-6): relative to the field, so absolute here
            scale = float(out[k].abs().max())
            torch.testing.assert_close(out[k] - gen[k], v, rtol=1.3e-6, atol=2e-6 * scale, msg=lambda m: f"{name} {k}: {m}")


# ---- the eager step and Stepper.predict ---------------------------------------------------------------------------------------------
def _oracle_stepper(case):
    """the golden rollout's stepper on the CPU: the loaded configuration and hooks around the oracle network (oracle/sfno.py)"""
    from oracle.sfno import SFNOConfig, SFNOOracle
    loaded = ace_amd.load_stepper(case["state"], device="cpu")
    cfg = loaded.config
    fields = {f.name for f in dataclasses.fields(SFNOConfig)}
    ocfg = SFNOConfig(in_chans=len(cfg.in_names), out_chans=len(cfg.out_names), img_shape=loaded.dataset_info.img_shape,
                      **{k: v for k, v in cfg.builder.config.items() if k in fields})
    weights = {k: v for k, v in case["state"]["step"]["module"].items() if isinstance(v, torch.Tensor)}
    net = SFNOOracle(ocfg, weights, dtype=torch.float32)

    class Net(torch.nn.Module):
        def forward(self, x):
            return net(x)

    loaded.stepper._step_obj.module = Module(Net(), None)
    return loaded


def test_predict_reproduces_the_reference_rollout_delta(gold):
    case = gold["rollout"]
    loaded = _oracle_stepper(case)
    stepper = loaded.stepper
    assert stepper.get_prescribed_prognostic_names() == [case["prescribed"]]
    plain, _ = stepper.predict(case["ic"], case["forcing"])
    assert type(plain) is dict                                              # nothing changes for a caller who does not ask
    out, state = stepper.predict(case["ic"], case["forcing"], step_diagnostics=True)
    assert isinstance(out, WindowData) and isinstance(out.step_diagnostics, StepDiagnostics)
    for k in plain:
        assert torch.equal(plain[k], out[k])
    delta = out.step_diagnostics.delta
    assert set(delta) == set(case["delta"]) and case["prescribed"] not in delta
    assert out.step_diagnostics.sample_dim_size() == 2 and out.step_diagnostics.to_cpu().delta.keys() == delta.keys()
    # tests/test_checkpoint_cpu.py holds the rollout's fields to 1e-6 of the field's maximum (3 x the conditioning floor for the
    # ill-conditioned ones); a delta is a difference of two such fields: twice that, relative to the field's maximum
    from _util import conditioning_floor
    floor = conditioning_floor({**case, "steps": case["steps"]})
    for k, want in case["delta"].items():
        for s in range(want.shape[1]):
            scale = float(case["steps"][s][k].abs().max())
            err = float((delta[k][:, s] - want[:, s]).abs().max()) / scale
            assert err <= 2.0 * max(1e-6, 3.0 * floor[s][k]), (k, s, err)
    derived = ace_amd.stepper.derive_over_window(stepper.derive_func, out, case["ic"], case["forcing"], 1, 3)
    assert derived.step_diagnostics is out.step_diagnostics                 # handed on


def _tiny_step(corrector, ocean=None, prescribed=()):
    """a 3-variable step around a fixed network: q' = -|q| - 1 (negative everywhere), sst' = sst - 10, d = f"""
    from ace_amd.step import NormalizationConfig, SingleModuleStep
    IN, OUT = ["f", "sst", "q", "frac"], ["sst", "q", "d"]

    class Net(torch.nn.Module):
        def forward(self, x):
            return torch.stack([x[:, 1] - 10.0, -x[:, 2].abs() - 1.0, x[:, 0]], dim=1)

    names = sorted(set(IN) | set(OUT))
    norm = NormalizationConfig(means={n: 0.0 for n in names}, stds={n: 1.0 for n in names})
    cfg = ace_amd.SingleModuleStepConfig(
        builder=ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet",
                                       config={"embed_dim": 8, "num_layers": 1, "encoder_layers": 1, "operator_type": "dhconv"}),
        in_names=IN, out_names=OUT, normalization=norm, ocean=ocean, corrector=corrector,
        prescribed_prognostic_names=list(prescribed))
    step = SingleModuleStep(cfg, ace_amd.DatasetInfo((4, 8)), cfg.normalization.build(names, device="cpu"), device="cpu")
    step.module = Module(Net(), None)
    g = torch.Generator().manual_seed(1)
    ic = {n: torch.randn(2, 1, 4, 8, generator=g) for n in ("sst", "q")}
    forcing = {n: torch.randn(2, 3, 4, 8, generator=g) for n in ("f", "frac", "sst", "q")}
    return ace_amd.Stepper(step), ic, forcing


OCEAN = {"surface_temperature_name": "sst", "ocean_fraction_name": "frac", "interpolate": False, "slab": None}


def test_step_delta_rules():
    stepper, ic, forcing = _tiny_step({"force_positive_names": ["q"]}, ocean=OCEAN)
    out, _ = stepper.predict(ic, forcing, step_diagnostics=True)
    delta = out.step_diagnostics.delta
    assert list(delta) == ["q"] and delta["q"].shape == (2, 2, 4, 8)
    assert float(delta["q"].min()) >= 1.0                                   # corrected 0 - network output <= -1
    assert torch.equal(out["q"], torch.zeros_like(out["q"]))
    # the ocean's surface temperature among the modified names
    stepper, ic, forcing = _tiny_step({"force_positive_names": ["q", "sst"]}, ocean=OCEAN)
    stepper.predict(ic, forcing)                                            # fine without the flag
    with pytest.raises(ValueError, match="overlap"):
        stepper.predict(ic, forcing, step_diagnostics=True)
    # a prescribed prognostic name is dropped from the delta; with nothing left the record is None
    stepper, ic, forcing = _tiny_step({"force_positive_names": ["q"]}, prescribed=["q"])
    assert stepper.predict(ic, forcing, step_diagnostics=True)[0].step_diagnostics is None
    stepper, ic, forcing = _tiny_step({"force_positive_names": ["q", "d"]}, prescribed=["q"])
    assert list(stepper.predict(ic, forcing, step_diagnostics=True)[0].step_diagnostics.delta) == ["d"]
    # no corrector: None
    stepper, ic, forcing = _tiny_step(None)
    out, _ = stepper.predict(ic, forcing, step_diagnostics=True)
    assert isinstance(out, WindowData) and out.step_diagnostics is None


@pytest.mark.parametrize("kind", ["OceanCorrector", "IceCorrector"])
def test_other_correctors_are_refused_by_name(kind):
    stepper, ic, forcing = _tiny_step(None)
    stepper._step_obj._corrector = type(kind, (), {"__call__": lambda self, i, o, n, s: (dict(o), s)})()
    stepper.predict(ic, forcing)
    with pytest.raises(NotImplementedError, match=kind):
        stepper.predict(ic, forcing, step_diagnostics=True)


def test_engines_other_than_the_atmosphere_one_refuse_the_flag():
    from ace_amd.coupled_rollout import CoupledRolloutEngine
    from ace_amd.ocean_rollout import OceanRolloutEngine
    with pytest.raises(NotImplementedError, match="step_diagnostics"):
        OceanRolloutEngine(None, 1, 1, step_diagnostics=True)
    with pytest.raises(NotImplementedError, match="step_diagnostics"):
        CoupledRolloutEngine(None, 1, 1, step_diagnostics=True)


# ---- the configuration of both aggregators -------------------------------------------------------------------------------------------
def _normalizer(names, dev="cpu"):
    return StandardNormalizer({n: torch.tensor(0.5 * i) for i, n in enumerate(names)},
                              {n: torch.tensor(1.0 + 0.5 * i) for i, n in enumerate(names)}, device=dev)


def _builders(info):
    norm = _normalizer(["a", "ps", "sst", "diag"])
    return [("inference", lambda cfg, normalize=norm: InferenceAggregatorConfig(step_diagnostics=cfg).build(
                info, 7, sht_factory=oracle_sht_factory, normalize=normalize)),
            ("evaluator", lambda cfg, normalize=norm: InferenceEvaluatorAggregatorConfig(step_diagnostics=cfg).build(
                info, 1, 6, normalize=normalize, sht_factory=oracle_sht_factory))]


def test_configuration_of_both_aggregators():
    info, ic, wins = make_case()
    for which, build in _builders(info):
        for off in (None, {}):
            agg = build(off)
            assert agg._correction is None and agg.records_step_diagnostics is False, which
        for on in (StepDiagnosticsMetricConfig(), {"correction_scalars": True}, {"correction_maps": True, "correction_scalars": False},
                   StepDiagnosticsMetricConfig(correction_maps=True)):
            agg = build(on)
            assert isinstance(agg._correction, CorrectionDeltaAggregator) and agg.records_step_diagnostics, which
        assert build({"correction_scalars": False, "correction_maps": False})._correction is None
        with pytest.raises(NotImplementedError, match="step_diagnostics"):
            build({"per_step": True})
        with pytest.raises(NotImplementedError, match="step_diagnostics"):
            build({"correction_scalars": True, "writer": True})
    build = _builders(info)[0][1]
    assert build(StepDiagnosticsMetricConfig(), normalize=None)._correction is None      # the default without a normaliser: none
    with pytest.raises(ValueError, match="normalizer"):
        build(StepDiagnosticsMetricConfig(correction_maps=True), normalize=None)
    assert StepDiagnosticsMetricConfig() == StepDiagnosticsMetricConfig(correction_scalars=True, correction_maps=False)


def test_existing_logs_are_unchanged_and_silent_until_data_arrives():
    info, ic, wins = make_case()
    logs = {}
    for cfg in (None, StepDiagnosticsMetricConfig(correction_maps=True)):
        agg = InferenceAggregatorConfig(step_diagnostics=cfg).build(info, 7, sht_factory=oracle_sht_factory,
                                                                    normalize=_normalizer(["a", "ps", "sst", "diag"]))
        agg.record_initial_condition(ic)
        for w in wins:
            agg.record_batch(w) if cfg is None else agg.record_batch(w, step_diagnostics=None)
        logs[cfg is None] = (agg.get_inference_logs(), agg.get_dataset())
    (rows0, ds0), (rows1, ds1) = logs[True], logs[False]
    assert [set(r) for r in rows0] == [set(r) for r in rows1] and set(ds0) == set(ds1)
    assert not any("correction" in k for r in rows1 for k in r)
    plain = InferenceAggregatorConfig().build(info, 7, sht_factory=oracle_sht_factory)
    with pytest.raises(ValueError, match="step_diagnostics"):
        plain.record_batch(wins[0], step_diagnostics=StepDiagnostics(delta={"a": wins[0]["a"]}))


def test_metric_config(gold):
    info, delta, norm, want = _reference_case(gold)
    host = InferenceAggregatorConfig().build(info, 5, sht_factory=oracle_sht_factory)
    assert StepDiagnosticsMetricConfig() == StepDiagnosticsMetricConfig(correction_scalars=True, correction_maps=False)
    assert StepDiagnosticsMetricConfig.from_state(None) is None and StepDiagnosticsMetricConfig.from_state({}) is None
    assert StepDiagnosticsMetricConfig.from_state({"correction_maps": True}) == StepDiagnosticsMetricConfig(correction_maps=True)
    with pytest.raises(NotImplementedError, match="step_diagnostics"):
        StepDiagnosticsMetricConfig.from_state({"per_step": True})
    built = StepDiagnosticsMetricConfig(correction_maps=True).build(host, 5, True, norm)
    assert isinstance(built, CorrectionDeltaAggregator) and built.log_time_series
    assert not StepDiagnosticsMetricConfig().build(host, 5, False, norm).log_time_series
    assert StepDiagnosticsMetricConfig(correction_scalars=False).build(host, 5, True, norm) is None
    assert StepDiagnosticsMetricConfig().build(host, 5, True, None) is None                  # the default without a normaliser: none
    with pytest.raises(ValueError, match="normalizer"):
        StepDiagnosticsMetricConfig(correction_maps=True).build(host, 5, True, None)


# ---- the torch path against the reference's own outputs ---------------------------------------------------------------------------------
def _reference_case(gold):
    from ace_amd.dataset_info import DatasetInfo
    case, agg = gold["rollout"], gold["aggregator"]
    H, W = 8, 16
    info = DatasetInfo((H, W), lat=torch.linspace(-78.75, 78.75, H), lon=torch.arange(float(W)) * (360.0 / W))
    names = sorted(case["delta"])
    norm = StandardNormalizer({n: torch.tensor(0.0) for n in names}, {n: torch.tensor(case["stds"][n]) for n in names}, device="cpu")
    return info, case["delta"], norm, agg


def test_torch_path_matches_the_reference_aggregators(gold):
    info, delta, norm, want = _reference_case(gold)
    host = InferenceAggregatorConfig().build(info, want["n_timesteps"], sht_factory=oracle_sht_factory)
    agg = CorrectionDeltaAggregator(host, norm, want["n_timesteps"], record_scalars=True, record_maps=True, time_series=True)
    assert agg.summary_logs() == {} and agg.datasets() == {} and agg.series_rows() == []      # silent until data arrives
    agg.record_batch(None, 0)
    agg.record_batch(StepDiagnostics(delta={}), 0)
    assert not agg.has_data
    T = next(iter(delta.values())).shape[1]
    for sl, t0 in zip((slice(0, 2), slice(2, T)), want["i_time_start"]):
        agg.record_batch(StepDiagnostics(delta={k: v[:, sl] for k, v in delta.items()}), t0)
    ref = want["fp32"]
    logs, ds, series = agg.summary_logs(), agg.datasets(), agg.series_data()
    assert set(ds) == {"time_mean_norm_correction", "mean_norm_correction"}
    for n in delta:
        torch.testing.assert_close(torch.tensor(logs[f"time_mean_norm/correction_magnitude/{n}"]), ref["correction_magnitude"][n])
        torch.testing.assert_close(logs[f"time_mean_norm/correction_map/{n}"], ref["signed"][n])
        torch.testing.assert_close(ds["time_mean_norm_correction"][f"correction_map-{n}"], ref["signed"][n])
        for metric in ("weighted_correction_magnitude", "weighted_correction_std"):
            torch.testing.assert_close(series[metric][n], ref["series"][metric][n], equal_nan=True)
            assert torch.isnan(series[metric][n][[0, 4]]).all() and torch.isfinite(series[metric][n][1:4]).all()
            torch.testing.assert_close(ds["mean_norm_correction"][f"{metric}-{n}"], ref["series"][metric][n], equal_nan=True)
    rows = agg.series_rows()
    assert len(rows) == want["n_timesteps"] and set(rows[1]) == {f"mean_norm/{m}/{n}" for n in delta for m in series}
    # scalars only: no maps, no map dataset; without the series no series
    agg = CorrectionDeltaAggregator(host, norm, want["n_timesteps"], record_scalars=True, record_maps=False, time_series=False)
    agg.record_batch(StepDiagnostics(delta=delta), 0)
    assert set(agg.summary_logs()) == {f"time_mean_norm/correction_magnitude/{n}" for n in delta}
    assert agg.datasets() == {} and agg.series_rows() == []


def test_recording_raises(gold):
    info, delta, norm, want = _reference_case(gold)
    host = InferenceAggregatorConfig().build(info, 5, sht_factory=oracle_sht_factory)
    agg = CorrectionDeltaAggregator(host, norm, 5)
    agg.record_batch(StepDiagnostics(delta=delta), 0)
    fewer = {k: v for k, v in list(delta.items())[:-1]}
    with pytest.raises(ValueError, match="variable set must be constant"):
        agg.record_batch(StepDiagnostics(delta=fewer), 3)
    with pytest.raises(ValueError, match="sample count must be constant"):
        agg.record_batch(StepDiagnostics(delta={k: v[:1] for k, v in delta.items()}), 3)
    with pytest.raises(ValueError, match="no normalization constants"):
        CorrectionDeltaAggregator(host, norm, 5).record_batch(StepDiagnostics(delta={**delta, "unknown": delta["PRESsfc"]}), 0)
    with pytest.raises(ValueError, match="n_timesteps"):
        CorrectionDeltaAggregator(host, norm, 5).record_batch(StepDiagnostics(delta=delta), 3)


def test_run_inference_passes_the_record_only_when_asked(gold):
    """the loop hands ``out.step_diagnostics`` to an aggregator built with a correction aggregator, and calls any other as ever"""
    from ace_amd.inference import InferenceData, run_inference
    info, delta, norm, want = _reference_case(gold)
    fields = {k: v + 1.0 for k, v in delta.items()}
    ic = {k: v[:, :1] for k, v in fields.items()}

    def predict(state, forcing):
        return WindowData(fields, step_diagnostics=StepDiagnostics(delta=delta)), {k: v[:, -1:] for k, v in fields.items()}

    logs = {}
    for cfg in (None, StepDiagnosticsMetricConfig()):
        agg = InferenceAggregatorConfig(step_diagnostics=cfg).build(info, 4, sht_factory=oracle_sht_factory, normalize=norm)
        run_inference(predict, InferenceData(ic, [{}]), aggregator=agg)
        logs[cfg is None] = agg.get_inference_logs()
    assert not any("correction" in k for r in logs[True] for k in r)
    assert {f"mean_norm/weighted_correction_std/{n}" for n in delta} <= set(logs[False][1])
    assert {f"time_mean_norm/correction_magnitude/{n}" for n in delta} <= set(logs[False][-1])
    assert torch.isnan(torch.tensor(logs[False][0]["mean_norm/weighted_correction_std/PRESsfc"]))   # the initial condition's index


def test_flush_diagnostics_writes_the_correction_datasets(gold, tmp_path):
    """``flush_diagnostics`` writes the two correction datasets as ``.pt`` beside its neighbours, under the reference's stems"""
    import os
    info, delta, norm, want = _reference_case(gold)
    fields = {k: v + 1.0 for k, v in delta.items()}
    agg = InferenceAggregatorConfig(step_diagnostics=StepDiagnosticsMetricConfig(correction_maps=True)).build(
        info, 4, output_dir=str(tmp_path), save_diagnostics=True, sht_factory=oracle_sht_factory, normalize=norm)
    agg.record_initial_condition({k: v[:, :1] for k, v in fields.items()})
    agg.record_batch(fields, step_diagnostics=StepDiagnostics(delta=delta))
    agg.flush_diagnostics()
    written = set(os.listdir(tmp_path))
    assert {"time_mean_norm_correction_diagnostics.pt", "mean_norm_correction_diagnostics.pt", "mean_diagnostics.pt"} <= written
    maps = torch.load(tmp_path / "time_mean_norm_correction_diagnostics.pt", weights_only=True)
    assert set(maps) == {f"correction_map-{n}" for n in delta} and maps["correction_map-PRESsfc"].shape == (8, 16)
    series = torch.load(tmp_path / "mean_norm_correction_diagnostics.pt", weights_only=True)
    assert set(series) == {f"{m}-{n}" for n in delta for m in ("weighted_correction_magnitude", "weighted_correction_std")}
