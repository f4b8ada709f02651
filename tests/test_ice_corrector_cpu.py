"""The host side of the sea-ice corrector (ace_amd/ice_corrector.py): the configuration mirror and its refusals, the dispatch of
the step config's ``corrector``, a reference-style checkpoint through ``load_stepper`` and ``Stepper.predict`` on the CPU against the
reference's own rollout (tests/golden/gen_ice_rollout.pt), the refusals of the two engines that do not take an ice corrector, and
the host logic of ``FusedIceCorrector`` on an emulation of its kernels (tests/_fake_ice.py)."""
import copy
import datetime
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ace_amd  # noqa: E402
from ace_amd.ice_corrector import FusedIceCorrector, IceBudgetCorrectionConfig, IceCorrector, IceCorrectorConfig  # noqa: E402
from ace_amd.ocean_corrector import OceanCorrectorConfig, corrector_config_from_state  # noqa: E402
from _util import load_golden  # noqa: E402
from test_ice_corrector_ref_cpu import same_bits  # noqa: E402

SICONC = {"siconc": ["LSRCc", "LSNKc", "XPRTc"]}
SELECTOR = {"type": "ice_corrector", "config": {"budget_correction": {"corrected_variables": SICONC}}}


class Info:
    timestep = datetime.timedelta(hours=6)


# ---- the configuration ---------------------------------------------------------------------------------------------------
def test_config_round_trips_in_both_state_forms():
    import dataclasses
    a = IceCorrectorConfig.from_state(SELECTOR)
    b = IceCorrectorConfig.from_state(SELECTOR["config"])
    c = IceCorrectorConfig(budget_correction=IceBudgetCorrectionConfig(corrected_variables=SICONC))
    assert a == b == c and a.corrector_disabled_epochs == 0
    assert isinstance(a.budget_correction, IceBudgetCorrectionConfig)
    assert IceCorrectorConfig.from_state(dataclasses.asdict(a)) == a
    assert IceCorrectorConfig() == IceCorrectorConfig.from_state({}) == IceCorrectorConfig.from_state({"type": "ice_corrector", "config": {}})
    assert IceCorrectorConfig().budget_correction is None and IceBudgetCorrectionConfig().corrected_variables is None
    for nothing in (IceCorrectorConfig(), IceCorrectorConfig(budget_correction={"corrected_variables": None}),
                    IceCorrectorConfig(budget_correction={"corrected_variables": {}})):
        assert nothing.get_corrector(Info()) is None and nothing.unsupported(Info()) == []
    assert isinstance(a.get_corrector(Info(), ignore_unsupported=True), IceCorrector)


def test_corrector_disabled_epochs_rules():
    assert IceCorrectorConfig.from_state({"type": "ice_corrector", "config": {"corrector_disabled_epochs": 3}}).corrector_disabled_epochs == 3
    assert IceCorrectorConfig.from_state({**SELECTOR, "corrector_disabled_epochs": 0}) == IceCorrectorConfig.from_state(SELECTOR)
    with pytest.raises(ValueError, match="inside"):
        IceCorrectorConfig.from_state({**SELECTOR, "corrector_disabled_epochs": 2})
    with pytest.raises(ValueError, match="non-negative"):
        IceCorrectorConfig(corrector_disabled_epochs=-1)


def test_unknown_fields_and_wrong_types_raise():
    with pytest.raises(ValueError, match="unknown ice corrector fields"):
        IceCorrectorConfig.from_state({"budget_correction": None, "force_positive_names": []})
    with pytest.raises(ValueError, match="unknown corrector selector fields"):
        IceCorrectorConfig.from_state({**SELECTOR, "extra": 1})
    with pytest.raises(ValueError, match="unknown IceBudgetCorrectionConfig fields"):
        IceCorrectorConfig(budget_correction={"corrected_variables": SICONC, "cap": 1})
    with pytest.raises(ValueError, match="not an ice corrector"):
        IceCorrectorConfig.from_state({"type": "ocean_corrector", "config": {}})
    with pytest.raises(TypeError):
        IceCorrectorConfig(budget_correction=3)
    with pytest.raises(ValueError, match="three terms"):
        IceCorrectorConfig(budget_correction={"corrected_variables": {"siconc": ["LSRCc", "LSNKc"]}})


def test_dispatch_of_the_step_configs_corrector():
    assert isinstance(corrector_config_from_state(SELECTOR), IceCorrectorConfig)
    assert isinstance(corrector_config_from_state({"type": "ocean_corrector", "config": {}}), OceanCorrectorConfig)
    assert isinstance(corrector_config_from_state(None), ace_amd.AtmosphereCorrectorConfig)
    with pytest.raises(NotImplementedError):
        corrector_config_from_state({"type": "land_corrector", "config": {}})
    kw = dict(builder=ace_amd.ModuleSelector(type="Samudra", config={}), in_names=["siconc"], out_names=["siconc"],
              normalization=ace_amd.step.NormalizationConfig(means={"siconc": 0.0}, stds={"siconc": 1.0}))
    assert isinstance(ace_amd.SingleModuleStepConfig(corrector=SELECTOR, **kw).corrector, IceCorrectorConfig)
    cfg = IceCorrectorConfig.from_state(SELECTOR)
    assert ace_amd.SingleModuleStepConfig(corrector=cfg, **kw).corrector is cfg
    assert ace_amd.IceCorrectorConfig is IceCorrectorConfig and ace_amd.IceCorrector is IceCorrector
    assert ace_amd.IceBudgetCorrectionConfig is IceBudgetCorrectionConfig and ace_amd.FusedIceCorrector is FusedIceCorrector


def test_two_concentration_names_are_refused_at_build_time():
    cv = {"siconc": ["a", "b", "c"], "sea_ice_fraction": ["d", "e", "f"]}
    with pytest.raises(NotImplementedError, match="hash seed"):
        IceCorrectorConfig(budget_correction={"corrected_variables": cv})
    with pytest.raises(NotImplementedError, match="hash seed"):
        corrector_config_from_state({"type": "ice_corrector", "config": {"budget_correction": {"corrected_variables": cv}}})


def test_plan_order_masking_and_ignored_keys():
    cv = {"sisnmass": ["g", "h", "i"], "thetao_0": ["x", "y", "z"], "ocean_sea_ice_fraction": ["d", "e", "f"], "simass": ["a", "b", "c"]}
    plan = IceBudgetCorrectionConfig(corrected_variables=cv).plan()
    assert plan == [("simass", ("a", "b", "c"), False, False), ("ocean_sea_ice_fraction", ("d", "e", "f"), True, True),
                    ("sisnmass", ("g", "h", "i"), False, True)]
    assert IceBudgetCorrectionConfig(corrected_variables={"siconc": ["a", "b", "c"], "sisnmass": ["g", "h", "i"]}).plan() == [
        ("siconc", ("a", "b", "c"), True, False), ("sisnmass", ("g", "h", "i"), False, True)]
    assert IceBudgetCorrectionConfig(corrected_variables={"thetao_0": ["x", "y", "z"]}).plan() == []
    rec = load_golden("gen_ice_corrector_alone_00.pt")          # the reference ignored the unknown key too
    assert "not_a_sea_ice_variable" in rec["config"]["config"]["budget_correction"]["corrected_variables"]


def test_a_missing_field_raises_key_error():
    corrector = IceCorrectorConfig.from_state(SELECTOR).get_corrector(Info())
    z = torch.zeros(1, 2, 2)
    gen = {"LSRCc": z, "LSNKc": z, "XPRTc": z, "siconc": z}
    with pytest.raises(KeyError):
        corrector({}, gen, {}, None)
    with pytest.raises(KeyError):
        corrector({"siconc": z}, {k: v for k, v in gen.items() if k != "LSNKc"}, {}, None)
    out, _ = corrector({"siconc": z}, {k: v for k, v in gen.items() if k != "siconc"}, {}, None)      # the prognostic is rebuilt
    assert set(out) == set(gen)


def test_the_tensor_wide_flag_of_the_reference():
    """the issue's 1 x 2 x 2 example: violations survive with no trigger and are repaired everywhere by one pixel's trigger"""
    corrector = IceCorrectorConfig.from_state(SELECTOR).get_corrector(Info())
    inp = {"siconc": torch.full((1, 2, 2), 0.5)}
    gen = {"LSRCc": torch.full((1, 2, 2), -1e-6), "LSNKc": torch.full((1, 2, 2), 1e-6), "XPRTc": torch.zeros(1, 2, 2),
           "siconc": torch.zeros(1, 2, 2)}
    out, _ = corrector(inp, gen, {}, None)
    assert torch.equal(out["LSRCc"], gen["LSRCc"])
    gen["XPRTc"][0, 0, 0] = -1e-3
    out, _ = corrector(inp, gen, {}, None)
    assert out["LSRCc"].flatten()[1:].tolist() == [0.0, 0.0, 0.0] and float(out["LSRCc"][0, 0, 0]) > 0       # repaired at every pixel
    assert out["LSNKc"].flatten()[1:].tolist() == [0.0, 0.0, 0.0] and abs(float(out["siconc"][0, 0, 0])) < 1e-7


# ---- a reference-style checkpoint --------------------------------------------------------------------------------------------
def golden_stepper(device="cpu", edit=None):
    """the golden's checkpoint through load_stepper; ``edit``: a change to the stepper state before it is loaded"""
    case = load_golden("gen_ice_rollout.pt")
    state = copy.deepcopy(case["stepper"])
    state["step"]["module"] = {k: (v.float() if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
                               for k, v in state["step"]["module"].items()}
    di = state["dataset_info"]
    di["mask_provider"]["masks"] = {k: v.float() for k, v in di["mask_provider"]["masks"].items()}
    if edit is not None:
        edit(state)
    return ace_amd.load_stepper({"stepper": state}, device=device), case


class _FunctionalSamudra(torch.nn.Module):
    """TEST INFRASTRUCTURE for the suite without a GPU (Samudra has no CPU path): the architecture evaluated with
    torch.nn.functional in fp64 from the loaded module's parameters (tests/test_gpu_samudra.py: _f_samudra), rounded to fp32.  The
    host logic around the network - masking, normalisation, the corrector, the state that chains - is what the CPU test checks."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        from test_gpu_samudra import _f_samudra
        with torch.no_grad():
            return _f_samudra(x.double(), self.net).float()


@pytest.fixture(scope="module")
def cpu_rollout():
    from ace_amd.registry import Module
    loaded, case = golden_stepper()
    step = loaded.stepper._step_obj
    step.module = Module(_FunctionalSamudra(step.module.torch_module), None)
    out, _ = loaded.stepper.predict(case["initial_condition"], case["forcing"])
    return loaded, case, out


def test_load_stepper_builds_the_ice_corrector(cpu_rollout):
    loaded, case, _ = cpu_rollout
    corrector = loaded.stepper._step_obj._corrector
    assert isinstance(loaded.config.corrector, IceCorrectorConfig) and isinstance(corrector, IceCorrector)
    assert [p[0] for p in corrector.plan] == ["simass", "siconc", "sisnmass"] and corrector.timestep_seconds == 2 * 86400.0
    assert not loaded.ignored if hasattr(loaded, "ignored") else True


def test_predict_on_the_cpu_obeys_the_budget_and_follows_the_golden(cpu_rollout):
    loaded, case, out = cpu_rollout
    corrector = loaded.stepper._step_obj._corrector
    dt = corrector.timestep_seconds
    T = case["output"]["siconc"].shape[1]
    masker = loaded.stepper._input_process_func
    for name, terms, area, _ in corrector.plan:
        for s in range(T):
            # the state the step saw: the initial condition or the previous output, through the input masking
            old = masker({name: (case["initial_condition"][name][:, 0] if s == 0 else out[name][:, s - 1])})[name].double()
            b = [out[t][:, s].double() for t in terms]
            want = old + dt * ((b[0] + b[1]) + b[2])
            got = out[name][:, s].double()
            ok = ~torch.isnan(got)
            assert torch.equal(torch.isnan(want), ~ok), (name, s)
            # new = old + dt (s + k + t) to fp32 rounding: the stored terms are fp32 roundings of the fp64 ones (3 x 2^-24 of the
            # largest term's increment) and the sum is rounded once more (2^-24 of the result)
            scale = torch.stack([dt * x.abs() for x in b] + [want.abs()]).amax(dim=0)
            assert bool(((got - want).abs()[ok] <= 4 * 2.0 ** -24 * scale[ok] + 1e-30).all()), (name, s)
            # 0 <= siconc <= 1 (and 0 <= mass), as far as the reference's own fp64 arithmetic holds it: a stage moves the new mass
            # onto its bound with a handful of fp64 operations on the terms, so what it leaves is a residue of a few units of
            # 2^-53 of the largest term (the reference's golden rollout holds such pixels: -6.9e-18 where siconc is emptied),
            # not the 2^-24 of an fp32 rounding
            slack = 64 * 2.0 ** -53 * torch.maximum(scale, torch.ones_like(scale))[ok]
            low, high = float((got[ok] / slack).min()), float(((got[ok] - 1) / slack).max())
            print(f"ICEBOUNDS {name} step {s}: min {float(got[ok].min()):.3e} max {float(got[ok].max()):.9f} "
                  f"(lowest {low:.3f}, highest above one {high:.3f}, in units of the slack)")
            assert bool((got[ok] >= -slack).all()), (name, s)
            if area:
                assert bool((got[ok] <= 1 + slack).all()), (name, s)
    for k in case["output"]:      # the bar of tests/test_gpu_ocean_rollout.py (_close_to_reference) for fp32 fields
        out32 = case["output"][k].double()
        ref = out32 + case["output64_delta"][k].double() / case["output64_delta_scale"]
        got = out[k].double()
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), k
        ok = ~torch.isnan(ref)
        scale = ref[ok].abs().max()
        err = (got - ref)[ok].abs().max() / scale
        ref_err = (out32 - ref)[ok].abs().max() / scale
        print(f"ICEROLLOUT {k}: err {float(err):.3e} ref_err {float(ref_err):.3e} vs golden fp32 "
              f"{float((got - out32)[ok].abs().max() / scale):.3e}")
        assert err <= 2.0 * ref_err + 1e-6, (k, float(err), float(ref_err))


def test_fused_flag_changes_nothing_on_the_cpu(cpu_rollout):
    loaded, case, out = cpu_rollout
    corrector = loaded.stepper._step_obj._corrector
    assert corrector.fused and corrector.launches() == (0, 0)       # CPU tensors take the torch path


# ---- the engines that do not take it ---------------------------------------------------------------------------------------
def ice_corrector():
    return IceCorrectorConfig.from_state(SELECTOR).get_corrector(Info())


def test_sfno_engine_refuses_an_ice_corrector_before_the_device():
    from test_checkpoint_cpu import _reference_style_checkpoint
    from ace_amd.rollout import RolloutEngine
    ckpt, _ = _reference_style_checkpoint()
    stepper = ace_amd.load_stepper(copy.deepcopy(ckpt), device="cpu").stepper
    stepper._step_obj._corrector = ice_corrector()
    for graph in (None, "step", "window"):
        with pytest.raises(NotImplementedError, match="ice_corrector") as err:
            RolloutEngine(stepper, batch=1, n_forward_steps=2, graph=graph)
        assert "Stepper.predict" in str(err.value)


def test_coupled_engine_refuses_an_ice_corrector_before_the_device():
    from ace_amd.coupled_rollout import CoupledRolloutEngine
    from _coupled import B, coupled_checkpoint
    for realm in ("ocean", "atmosphere"):
        s = ace_amd.load_coupled_stepper(coupled_checkpoint(), device="cpu")
        getattr(s, realm)._step_obj._corrector = ice_corrector()
        with pytest.raises(NotImplementedError, match=f"ice_corrector.* on the {realm} component") as err:
            CoupledRolloutEngine(s, B, 2)
        assert "Stepper.predict" in str(err.value)


def test_ocean_engine_accepts_an_ice_corrector_up_to_the_device():
    """on a CPU stepper every refusal that needs no device has passed when the engine asks for an MI355X"""
    from ace_amd.ocean_rollout import OceanRolloutEngine
    loaded, _ = golden_stepper()
    with pytest.raises(RuntimeError, match="cuda"):
        OceanRolloutEngine(loaded.stepper, batch=2, n_forward_steps=2)


# ---- FusedIceCorrector's host logic on the emulation ------------------------------------------------------------------------------
def golden_case(name):
    rec = load_golden(f"gen_ice_corrector_{name}.pt")

    class I:
        timestep = datetime.timedelta(microseconds=rec["timestep_microseconds"])
    return rec, IceCorrectorConfig.from_state(rec["config"]).get_corrector(I())


@pytest.mark.parametrize("case", ["masked_111", "masked_010", "alone_11", "tiny", "nan", "mass_snow", "sea_ice_fraction"])
def test_fused_handle_on_the_emulation_is_the_reference(case):
    from _fake_ice import fake_ice
    rec, corrector = golden_case(case)
    inp = {k: v.clone() for k, v in rec["input"].items()}
    # outputs as time level 1 of (B, 3, H, W) windows: the planes are strided views, corrected in place
    windows = {k: torch.full((2, 3, 6, 9), 777.0) for k in rec["output"]}
    gen = {}
    for k, v in rec["output"].items():
        windows[k][:, 1] = v
        gen[k] = windows[k][:, 1]
    with fake_ice() as fake:
        h = corrector.handle(2, (6, 9), "cpu")
        assert corrector.handle(2, (6, 9), "cpu") is h and corrector.handle(1, (6, 9), "cpu") is not h      # one scratch per (device, B, H, W)
        assert h.scratch.numel() == fake.ace_ice_budget_scratch_bytes(2, 54) and h.scratch.data_ptr() % 16 == 0
        f = h.fields(inp, gen, {})
        assert f.nvars == len(corrector.plan)
        for v, (name, terms, area, masked) in enumerate(corrector.plan):
            assert (f.var[v].area_mode, f.var[v].masked) == (int(area), int(masked))
            assert f.var[v].old_mass.p == inp[name].data_ptr() and f.var[v].old_mass.stride == 54
            assert f.var[v].mass.p == gen[name].data_ptr() and f.var[v].mass.stride == 3 * 54
            assert [getattr(f.var[v], a).p for a in ("source", "sink", "transport")] == [gen[t].data_ptr() for t in terms]
        h.apply(f, 0)
        h.apply(h.fields(inp, gen, {}), 0)       # a second step: on the corrected terms, as a rollout would
        assert h.launches() == (2 * f.nvars, 2 * f.nvars) == corrector.launches()
        assert (fake.flags, fake.applies, fake.clears) == (2 * f.nvars, 2 * f.nvars, 2)
        assert [tuple(rec["paths"][p[0]]) for p in corrector.plan] == fake.calls[0]["paths"]
        assert fake.calls[0]["scratch"] == fake.calls[1]["scratch"] == h.scratch.data_ptr()
        assert fake.calls[0]["timestep"] == rec["timestep_seconds"]
    # the first application against the reference: redo it alone
    for k, v in rec["output"].items():
        windows[k][:, 1] = v
    with fake_ice():
        h.apply(h.fields(inp, gen, {}), 0)
    for k, want in rec["corrected"].items():
        assert same_bits(windows[k][:, 1], want), k
        assert bool((windows[k][:, 0] == 777.0).all() and (windows[k][:, 2] == 777.0).all()), k
    for k, v in rec["input"].items():
        assert same_bits(inp[k], v), k


def test_fused_handle_checks_layout_and_shared_fields():
    from _fake_ice import fake_ice
    rec, corrector = golden_case("alone_11")
    with fake_ice():
        h = FusedIceCorrector(corrector, 2, (6, 9), "cpu")
        gen = dict(rec["output"])
        with pytest.raises(KeyError):
            h.fields({}, gen, {})
        with pytest.raises(TypeError, match="float32"):
            h.fields({"siconc": rec["input"]["siconc"].double()}, gen, {})
        with pytest.raises(ValueError, match="contiguous rows"):
            h.fields(rec["input"], {**gen, "LSNKc": torch.zeros(2, 9, 6).transpose(1, 2)}, {})
        with pytest.raises(ValueError, match=r"\(2, 6, 9\)"):
            h.fields(rec["input"], {**gen, "LSNKc": torch.zeros(1, 6, 9)}, {})
        four = h.fields({"siconc": rec["input"]["siconc"][:, None]}, gen, {})       # (B, 1, H, W) is a plane too
        assert four.var[0].old_mass.p == rec["input"]["siconc"].data_ptr()

        class I:
            timestep = datetime.timedelta(hours=6)
        shared = IceCorrectorConfig(budget_correction={"corrected_variables": {"simass": ["a", "b", "c"], "sisnmass": ["d", "b", "e"]}})
        with pytest.raises(NotImplementedError, match=r"written by two corrected variables \(\['b'\]\).*fused = False"):
            FusedIceCorrector(shared.get_corrector(I()), 2, (6, 9), "cpu")
