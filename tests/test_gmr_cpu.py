"""Global-mean removal (ace_amd/global_mean_removal.py; fme/core/step/global_mean_removal.py) on the host: the configuration
rules, the transforms, a reference-written stepper state with the option loaded by ace_amd.load_stepper against the REAL
reference's rollouts (tests/golden/make_golden_gmr.py), and the rollout engine's host logic on the emulated C ABI
(tests/_fake_gmr.py) against Stepper.predict."""
import logging

import pytest
import torch

import ace_amd
from ace_amd.checkpoint import StepperOverrideConfig, load_stepper
from ace_amd.global_mean_removal import config_from_state
from ace_amd.registry import Module
from ace_amd.step import NormalizationConfig
from _fake_gmr import fake_gmr
from _util import load_golden, rel_max

CASES = ["shared", "per_channel", "subset"]
N_IN = {"shared": 6, "per_channel": 10, "subset": 5}          # 5 in_names + the synthetic channels


class _OracleModule(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self._net = net

    def forward(self, x):
        return self._net.forward(x)


def _with_oracle_network(stepper, n_in):
    from oracle.sfno import SFNOConfig, SFNOOracle
    cfg = SFNOConfig(in_chans=n_in, out_chans=4, img_shape=(8, 16), embed_dim=12, num_layers=2, operator_type="dhconv")
    stepper._step_obj.module = Module(_OracleModule(SFNOOracle(cfg, stepper.modules[0].state_dict(), dtype=torch.float32)), None)
    return stepper


def _base(**kw):
    names = ["f", "p", "q", "d"]
    norm = NormalizationConfig(means={k: 0.5 * i for i, k in enumerate(names)}, stds={k: 1.0 + i for i, k in enumerate(names)})
    return dict(builder=ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet", config={"embed_dim": 4, "num_layers": 1}),
                in_names=["f", "p", "q"], out_names=["p", "q", "d"], normalization=norm, **kw)


# ---- configuration
def test_configuration_rules(caplog):
    Shared, PerChannel = ace_amd.SharedGlobalMeanRemovalConfig, ace_amd.PerChannelGlobalMeanRemovalConfig
    assert Shared().field_names == ace_amd.DEFAULT_TEMPERATURE_FIELD_NAMES and Shared().reference_field == "surface_temperature"
    assert not Shared().append_as_input and PerChannel().field_names is None and not PerChannel().append_as_input
    with pytest.raises(ValueError, match="reference_field 'd'"):          # shared: the reference field has to be an input
        ace_amd.SingleModuleStepConfig(**_base(global_mean_removal=Shared(reference_field="d", field_names=["p"])))
    with pytest.raises(ValueError, match="field_name 'd' not in in_names"):     # per channel: an explicit output-only name
        ace_amd.SingleModuleStepConfig(**_base(global_mean_removal=PerChannel(field_names=["p", "d"])))
    for gmr in (Shared(reference_field="p", field_names=["p", "d", "nowhere"]), PerChannel(field_names=["p", "nowhere"])):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="ace_amd.global_mean_removal"):
            ace_amd.SingleModuleStepConfig(**_base(global_mean_removal=gmr))
        assert [r.getMessage() for r in caplog.records] == [
            "global_mean_removal field_name 'nowhere' is not in in_names or out_names and will have no effect"]
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="ace_amd.global_mean_removal"):
        ace_amd.SingleModuleStepConfig(**_base(global_mean_removal=PerChannel()))
        ace_amd.SingleModuleStepConfig(**_base(global_mean_removal=Shared(reference_field="p", field_names=["d"])))
    assert not caplog.records


def test_state_mapping_round_trip_and_refusals():
    import dataclasses
    for gmr in (ace_amd.SharedGlobalMeanRemovalConfig(reference_field="p", field_names=["p", "d"], append_as_input=True),
                ace_amd.PerChannelGlobalMeanRemovalConfig(field_names=["f"]), ace_amd.PerChannelGlobalMeanRemovalConfig()):
        state = dataclasses.asdict(gmr)
        assert state["kind"] in ("shared", "per_channel")
        cfg = ace_amd.SingleModuleStepConfig(**_base(global_mean_removal=state))
        assert cfg.global_mean_removal == gmr and type(cfg.global_mean_removal) is type(gmr)
        assert config_from_state(gmr) is gmr
    for bad in ({"x": 1}, {"kind": "zonal"}, {"kind": "shared", "reference_field": "p", "surprise": 1}, {"kind": "per_channel", "x": 1},
                "shared"):
        with pytest.raises(NotImplementedError):
            ace_amd.SingleModuleStepConfig(**_base(global_mean_removal=bad))
    with pytest.raises(NotImplementedError):          # the other two refused options stay refused
        ace_amd.SingleModuleStepConfig(**_base(input_dropout={"p": 0.1}))


def test_extra_channel_names_and_module_input_channels():
    info = ace_amd.DatasetInfo((4, 8))
    cases = [(None, []),
             (ace_amd.SharedGlobalMeanRemovalConfig(reference_field="p", field_names=["q", "d"]), []),
             (ace_amd.SharedGlobalMeanRemovalConfig(reference_field="p", field_names=["q", "d"], append_as_input=True), ["__gmr_extra__p"]),
             (ace_amd.PerChannelGlobalMeanRemovalConfig(append_as_input=True), ["__gmr_extra__f", "__gmr_extra__p", "__gmr_extra__q"]),
             (ace_amd.PerChannelGlobalMeanRemovalConfig(field_names=["q", "f"], append_as_input=True), ["__gmr_extra__q", "__gmr_extra__f"]),
             (ace_amd.PerChannelGlobalMeanRemovalConfig(field_names=["q", "f"]), [])]
    for gmr, extras in cases:
        stepper = ace_amd.Stepper.from_config(ace_amd.SingleModuleStepConfig(**_base(global_mean_removal=gmr)), info, device="cpu")
        step = stepper._step_obj
        assert (step.global_mean_removal is None) == (gmr is None)
        assert step.in_packer.names == ["f", "p", "q"] + extras
        assert step.module.torch_module.encoder[0].weight.shape[1] == 3 + len(extras)
        if gmr is not None:
            assert step.global_mean_removal.extra_channel_names == extras and step.global_mean_removal.n_extra_input_channels == len(extras)
    assert ace_amd.extra_channel_source_field("__gmr_extra__p") == "p" and ace_amd.extra_channel_source_field("p") is None


# ---- the transforms
def _normalizer():
    names = ["f", "p", "q", "d"]
    return NormalizationConfig(means={"f": 0.5, "p": 287.0, "q": 250.0, "d": 286.0}, stds={k: 2.0 + i for i, k in enumerate(names)}).build(names)


def _fields(B=3):
    g = torch.Generator().manual_seed(4)
    return {"f": torch.randn(B, 6, 10, generator=g), "p": 288.0 + 3.0 * torch.randn(B, 6, 10, generator=g) + torch.arange(B).view(B, 1, 1),
            "q": 251.0 + 4.0 * torch.randn(B, 6, 10, generator=g)}


def test_shared_transform_and_output_only_field():
    norm, x = _normalizer(), _fields()
    t = ace_amd.SharedGlobalMeanRemovalConfig(reference_field="p", field_names=["p", "q", "d", "nowhere"],
                                              append_as_input=True).build(norm, ["f", "p", "q"])
    shifted, state = t.forward_transform(x, None)
    assert isinstance(state, ace_amd.GlobalMeanRemovalState)
    offset = norm.means["p"] - x["p"].mean(dim=(1, 2))
    assert set(state.shifts) == {"p", "q", "d", "nowhere"} and all(torch.equal(s, offset) for s in state.shifts.values())
    assert torch.equal(shifted["f"], x["f"]) and set(shifted) == set(x)
    for n in ("p", "q"):
        assert torch.equal(shifted[n], x[n] + offset.view(-1, 1, 1))
    assert float((shifted["p"].mean(dim=(1, 2)) - 287.0).abs().max()) < 1e-4          # the reference field now sits on its climatology
    extras = t.extras_normalized(state)
    assert list(extras) == ["__gmr_extra__p"] and extras["__gmr_extra__p"].shape == (3, 6, 10)
    assert torch.equal(extras["__gmr_extra__p"], (-offset / norm.stds["p"]).view(-1, 1, 1).expand(3, 6, 10))
    # the inverse un-shifts what is in the output: the prognostic fields come back (where fp32 allows: the shift is a few units
    # on values of a few hundred, one rounding of the sum and one of the difference), the output-only field moves by -offset
    out = {"p": shifted["p"], "q": shifted["q"], "d": torch.full((3, 6, 10), 286.0), "h": torch.ones(3, 6, 10)}
    back = t.inverse_transform(out, state)
    for n in ("p", "q"):
        assert float((back[n] - x[n]).abs().max()) <= 2 * 2.0 ** -15           # ulp(512) / 2 per rounding, two roundings
    assert torch.equal(back["d"], 286.0 - offset.view(-1, 1, 1).expand(3, 6, 10)) and torch.equal(back["h"], out["h"])
    exact = {"p": torch.full((2, 4, 4), 280.0), "q": torch.full((2, 4, 4), 100.0)}     # exactly representable: an exact round trip
    s2, st2 = t.forward_transform(exact, None)
    assert torch.equal(s2["p"], torch.full((2, 4, 4), 287.0)) and torch.equal(s2["q"], torch.full((2, 4, 4), 107.0))
    assert all(torch.equal(v, exact[k]) for k, v in t.inverse_transform(s2, st2).items())
    with pytest.raises(ValueError, match="Reference field 'p'"):
        t.forward_transform({"q": x["q"]}, None)


def test_per_channel_transform():
    norm, x = _normalizer(), _fields()
    t = ace_amd.PerChannelGlobalMeanRemovalConfig(field_names=["q", "p"], append_as_input=True).build(norm, ["f", "p", "q"])
    shifted, state = t.forward_transform(x, None)
    assert list(state.shifts) == ["q", "p"] and torch.equal(shifted["f"], x["f"])
    for n in ("p", "q"):
        shift = norm.means[n] - x[n].mean(dim=(1, 2))
        assert torch.equal(state.shifts[n], shift) and torch.equal(shifted[n], x[n] + shift.view(-1, 1, 1))
        assert torch.equal(t.extras_normalized(state)["__gmr_extra__" + n], (-shift / norm.stds[n]).view(-1, 1, 1).expand(3, 6, 10))
    assert list(t.extras_normalized(state)) == ["__gmr_extra__q", "__gmr_extra__p"]
    back = t.inverse_transform({**shifted, "d": torch.zeros(3, 6, 10)}, state)
    assert float((back["p"] - x["p"]).abs().max()) <= 2 * 2.0 ** -15 and torch.equal(back["d"], torch.zeros(3, 6, 10))
    all_inputs = ace_amd.PerChannelGlobalMeanRemovalConfig().build(norm, ["f", "p", "q"])
    assert all_inputs.field_names == ["f", "p", "q"] and all_inputs.extra_channel_names == []
    # a field that is absent from the input is skipped, extras included
    _, partial = t.forward_transform({"p": x["p"]}, None)
    assert list(partial.shifts) == ["p"] and list(partial.extras) == ["__gmr_extra__p"]


def test_data_mask_is_refused():
    norm, x = _normalizer(), _fields()
    mask = {"p": torch.ones(3, dtype=torch.bool)}
    for cfg in (ace_amd.SharedGlobalMeanRemovalConfig(reference_field="p", field_names=["p"]), ace_amd.PerChannelGlobalMeanRemovalConfig()):
        with pytest.raises(NotImplementedError, match="data mask"):
            cfg.build(norm, ["f", "p", "q"]).forward_transform(x, mask)


# ---- against the reference's rollouts
@pytest.mark.parametrize("case", CASES)
def test_stepper_predict_vs_reference_rollout(case):
    g = load_golden("gen_gmr.pt")[case]
    loaded = load_stepper(g["state"], device="cpu")               # a reference-written state with the option loads
    st = loaded.stepper
    assert not any("global_mean_removal" in i for i in loaded.ignored)
    gmr = st._step_obj.global_mean_removal
    assert isinstance(gmr, ace_amd.SharedGlobalMeanRemoval if case == "shared" else ace_amd.PerChannelGlobalMeanRemoval)
    assert len(st._step_obj.in_packer.names) == N_IN[case]
    _with_oracle_network(st, N_IN[case])
    with torch.no_grad():
        out, state = st.predict(g["ic"], g["forcing"])
    assert set(out) == set(g["steps"][0]) and set(state) == {"Ts", "T_1"}
    for k in out:
        want = torch.stack([s[k] for s in g["steps"]], dim=1)
        assert rel_max(out[k], want) <= 1e-5, (case, k, rel_max(out[k], want))
    cfg = st._step_obj.config
    assert cfg.global_mean_removal is not None and cfg.global_mean_removal.kind == ("shared" if case == "shared" else "per_channel")


def test_checkpoint_loader_keeps_refusing_the_other_options():
    g = load_golden("gen_gmr.pt")["subset"]
    import copy
    state = copy.deepcopy(g["state"])
    state["config"]["step"]["config"]["input_dropout"] = {"rate": 0.1}
    with pytest.raises(NotImplementedError, match="input_dropout"):
        load_stepper(state, device="cpu")
    state = copy.deepcopy(g["state"])
    state["config"]["step"]["config"]["global_mean_removal"] = {"kind": "zonal"}
    with pytest.raises(NotImplementedError):
        load_stepper(state, device="cpu")


# ---- the engine's host logic on the emulated C ABI
@pytest.mark.parametrize("graph", [None, "step"])
@pytest.mark.parametrize("case", CASES)
def test_rollout_engine_vs_stepper_predict(case, graph):
    from ace_amd.rollout import RolloutEngine
    g = load_golden("gen_gmr.pt")[case]
    eng_st = load_stepper(g["state"], device="cpu").stepper
    ref_st = _with_oracle_network(load_stepper(g["state"], device="cpu").stepper, N_IN[case])
    with torch.no_grad():
        want, want_state = ref_st.predict(g["ic"], g["forcing"])
        with fake_gmr():
            eng = RolloutEngine(eng_st, batch=2, n_forward_steps=3, graph=graph)
            assert eng.x.shape == (2, N_IN[case], 8, 16)
            out, state = eng.predict(g["ic"], g["forcing"])
    assert set(out) == set(want)
    for k in out:
        assert rel_max(out[k], want[k]) <= 5e-6, (case, graph, k, rel_max(out[k], want[k]))
    for k in want_state:
        assert rel_max(state[k], want_state[k]) <= 5e-6, k
    # the engine's reduction is the stated fp64 one, Stepper.predict's on the CPU is t.mean: the last step's shifts agree to fp32
    last_in = {"Ts": want["Ts"][:, -2]}
    shift = eng._gmr["shift"]
    k = 0 if case == "shared" else eng._gmr["planes"].tolist().index(eng.in_names.index("Ts"))
    clim = float(eng_st.normalizer.means["Ts"])
    assert float((shift[:, k] - (clim - last_in["Ts"].mean(dim=(1, 2)))).abs().max()) <= 1e-4


def test_rollout_engine_multi_call_gets_its_own_shifts():
    """multi-call where the scaled forcing is itself a processed per_channel field: the re-evaluation's means, shifts and
    synthetic channels are those of ITS inputs (single_module.py:651-659 runs inside every wrapped call)"""
    from ace_amd.rollout import RolloutEngine
    g = load_golden("gen_gmr.pt")["per_channel"]
    mc = {"forcing_name": "co2", "forcing_multipliers": {"_doubled_co2": 2.0}, "output_names": ["h_3", "TMP2m"]}
    over = StepperOverrideConfig(multi_call=mc)
    eng_st = load_stepper(g["state"], over, device="cpu").stepper
    ref_st = _with_oracle_network(load_stepper(g["state"], over, device="cpu").stepper, N_IN["per_channel"])
    with torch.no_grad():
        want, _ = ref_st.predict(g["ic"], g["forcing"])
        with fake_gmr():
            out, _ = RolloutEngine(eng_st, batch=2, n_forward_steps=3, graph="step").predict(g["ic"], g["forcing"])
    assert {"h_doubled_co2_3", "TMP2m_doubled_co2"} <= set(out) and set(out) == set(want)
    for k in out:
        assert rel_max(out[k], want[k]) <= 5e-6, (k, rel_max(out[k], want[k]))
    assert float((want["h_doubled_co2_3"] - want["h_3"]).abs().max()) > 1e-3           # the scaled forcing was seen


def test_engine_without_the_option_makes_no_new_calls():
    """a stepper without global-mean removal runs on the emulation that does NOT know the new entries"""
    from ace_amd.rollout import RolloutEngine
    from _fake_sfno import fake_sfno
    g = load_golden("gen_step_options.pt")["stepper"]
    st = load_stepper(g["state"], StepperOverrideConfig(multi_call=None), device="cpu").stepper
    from _fake_hpx import fake_hpx
    with fake_hpx(), fake_sfno() as fake, torch.no_grad():
        assert not hasattr(type(fake), "ace_gmr_partials")
        eng = RolloutEngine(st, batch=2, n_forward_steps=3, graph="step")
        assert eng._gmr is None and eng.extra_names == []
        eng.predict(g["ic"], g["forcing"])


# ---- refusals
def _gmr_stepper(**kw):
    cfg = ace_amd.SingleModuleStepConfig(**_base(global_mean_removal=ace_amd.SharedGlobalMeanRemovalConfig(
        reference_field="p", field_names=["p", "d", "s"]), **kw))
    return ace_amd.Stepper.from_config(cfg, ace_amd.DatasetInfo((4, 8)), device="cpu")


def test_other_engines_refuse():
    from ace_amd.coupled_rollout import check_supported
    from ace_amd.ocean_rollout import OceanRolloutEngine
    import types
    with fake_gmr():
        stepper = _gmr_stepper()
        with pytest.raises(NotImplementedError, match=r"global_mean_removal.*Stepper\.predict"):
            OceanRolloutEngine.check_supported(stepper)
        plain = ace_amd.Stepper.from_config(ace_amd.SingleModuleStepConfig(**_base()), ace_amd.DatasetInfo((4, 8)), device="cpu")
        for pair in (types.SimpleNamespace(atmosphere=stepper, ocean=plain), types.SimpleNamespace(atmosphere=plain, ocean=stepper)):
            with pytest.raises(NotImplementedError, match=r"global_mean_removal.*Stepper\.predict"):
                check_supported(pair, 1, None)


def test_coupled_checkpoint_with_the_option_is_refused():
    from ace_amd.coupled import CoupledStepper
    g = load_golden("gen_gmr.pt")["subset"]
    plain = load_golden("gen_step_options.pt")["stepper"]["state"]
    with pytest.raises(NotImplementedError, match="global_mean_removal"):
        CoupledStepper.from_state({"ocean_state": plain, "atmosphere_state": g["state"], "config": {}}, device="cpu")


def test_rollout_engine_refuses_a_shifted_secondary_diagnostic():
    from ace_amd.rollout import RolloutEngine
    names = ["f", "p", "q", "d", "s"]
    norm = NormalizationConfig(means={k: 0.0 for k in names}, stds={k: 1.0 for k in names})
    base = {**_base(), "normalization": norm}
    sd = {"secondary_diagnostic_names": ["s"], "network": {"type": "MLP", "config": {"hidden_dim": 4, "depth": 2}}}
    cfg = ace_amd.SingleModuleStepConfig(**base, secondary_decoder=sd, global_mean_removal=ace_amd.SharedGlobalMeanRemovalConfig(
        reference_field="p", field_names=["p", "s"]))
    with fake_gmr():
        stepper = ace_amd.Stepper.from_config(cfg, ace_amd.DatasetInfo((4, 8)), device="cpu")
        with pytest.raises(NotImplementedError, match=r"\['s'\].*Stepper\.predict"):
            RolloutEngine(stepper, batch=1, n_forward_steps=2, graph=None)
        ok = ace_amd.SingleModuleStepConfig(**base, secondary_decoder=sd, global_mean_removal=ace_amd.SharedGlobalMeanRemovalConfig(
            reference_field="p", field_names=["p", "d"]))
        RolloutEngine(ace_amd.Stepper.from_config(ok, ace_amd.DatasetInfo((4, 8)), device="cpu"), batch=1, n_forward_steps=2, graph=None)
