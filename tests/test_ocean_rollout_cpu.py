"""The host side of the fused static masking (ace_amd/masking.py: the per-name plan of the masking kernels) against the reference's
own masking (tests/golden/gen_masking.pt), the torch route of CPU tensors, and the configurations ``OceanRolloutEngine`` refuses
before it touches a device."""
import copy

import pytest
import torch

from ace_amd.masking import SpatialMaskProvider, StaticSpatialMaskingConfig
from _util import load_golden
from test_ocean_corrector_cpu import samudra_ocean_state


@pytest.fixture(scope="module")
def gold():
    return load_golden("gen_masking.pt")


def _apply_plan(masker, data):
    """the reference's masking recomputed from the host plan alone: per name (mask key, fp32 fill) or untouched"""
    out = {}
    for (name, t), (key, fill) in zip(data.items(), masker.plan(list(data))):
        if key is None:
            out[name] = t
            continue
        hit = torch.round(masker._mask.masks[key]).to(torch.int64) == masker.mask_value
        out[name] = torch.where(hit.expand(t.shape), torch.tensor(fill, dtype=torch.float32), t)
    return out


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def test_host_plan_resolves_every_name_as_the_reference(gold):
    provider = SpatialMaskProvider(gold["masks"])
    for name, want in gold["lookup"].items():
        key = provider.mask_key_for(name)
        assert (key is None) == (want is None), name
        if key is not None:
            assert torch.equal(provider.masks[key], want), name
    for case in gold["cases"]:
        masker = StaticSpatialMaskingConfig.from_state(case["config"]).build(mask=provider, means=gold["means"])
        plan = dict(zip(gold["names"], masker.plan(gold["names"])))
        got = _apply_plan(masker, {n: gold["data"][n] for n in gold["names"]})
        for name, want in case["out"].items():
            assert torch.equal(got[name], want), (case["config"], name)
            if torch.equal(want, gold["data"][name]) and plan[name][0] is not None:
                # a masked name whose mask hits nowhere: the plan still names the mask the reference looked up
                assert provider.mask_key_for(name) == plan[name][0]
        excl = case["config"].get("exclude_names_and_prefixes") or []
        for name in gold["names"]:
            if any(name == e or name.startswith(e) for e in excl):
                assert plan[name] == (None, None), (case["config"], name)
        if case["config"]["fill_value"] == "mean":
            for name, (key, fill) in plan.items():
                if key is not None:
                    assert fill == float(gold["means"][name]), name
    out_masker = provider.build_output_spatial_masker()
    got = _apply_plan(out_masker, {n: gold["data"][n] for n in gold["names"]})
    for name, want in gold["output_masked"].items():
        assert _same(got[name], want), name
    assert all(f != f for k, f in out_masker.plan(gold["names"]) if k is not None)          # NaN fill


def test_level_variable_and_2d_masks_in_the_plan():
    masks = {"mask_2d": torch.ones(3, 4), "mask_0": torch.zeros(3, 4), "mask_thetao_1": torch.ones(3, 4)}
    provider = SpatialMaskProvider(masks)
    masker = StaticSpatialMaskingConfig(mask_value=0, fill_value=0.49).build(provider)
    plan = dict(zip(["thetao_0", "thetao_1", "thetao_2", "zos"], masker.plan(["thetao_0", "thetao_1", "thetao_2", "zos"])))
    f = float(torch.tensor(0.49, dtype=torch.float32))
    assert plan == {"thetao_0": ("mask_0", f), "thetao_1": ("mask_thetao_1", f), "thetao_2": (None, None), "zos": ("mask_2d", f)}


def test_cpu_tensors_keep_the_torch_path(gold):
    provider = SpatialMaskProvider(gold["masks"])
    for case in gold["cases"]:
        masker = StaticSpatialMaskingConfig.from_state(case["config"]).build(mask=provider, means=gold["means"])
        assert masker.fused and masker.route(gold["data"]) == "torch"
        out = masker(gold["data"])
        for k, v in case["out"].items():
            assert torch.equal(out[k], v)
        assert masker.launches() == 0


# ---- OceanRolloutEngine's refusals ----------------------------------------------------------------------------------------
def _stepper():
    from ace_amd.checkpoint import load_stepper
    return load_stepper(samudra_ocean_state(), device="cpu").stepper


def test_engine_refuses_an_sfno_stepper():
    from test_checkpoint_cpu import _reference_style_checkpoint
    from ace_amd.checkpoint import load_stepper
    from ace_amd.ocean_rollout import OceanRolloutEngine
    ckpt, _ = _reference_style_checkpoint()
    stepper = load_stepper(copy.deepcopy(ckpt), device="cpu").stepper
    with pytest.raises(NotImplementedError, match="RolloutEngine"):
        OceanRolloutEngine(stepper, batch=1, n_forward_steps=2)


@pytest.mark.parametrize("what, edit, match", [
    ("multi-call", lambda st: setattr(st, "_multi_call_config", object()), "multi-call"),
    ("secondary decoder", lambda st: setattr(st._step_obj, "secondary_decoder", object()), "secondary decoder"),
    ("labels", lambda st: setattr(st._step_obj.module, "_label_encoding", object()), "label"),
    ("atmosphere ocean", lambda st: setattr(st._step_obj, "_ocean", object()), "ocean"),
    ("prescribed prognostics", lambda st: st.replace_prescribed_prognostic_names(["sst"]), "prescribed"),
    ("atmosphere corrector", lambda st: setattr(st._step_obj, "_corrector", object()), "not an ocean corrector"),
])
def test_engine_refuses_unsupported_configurations_before_the_device(what, edit, match):
    from ace_amd.ocean_rollout import OceanRolloutEngine
    stepper = _stepper()
    edit(stepper)
    with pytest.raises(NotImplementedError, match=match) as err:
        OceanRolloutEngine(stepper, batch=1, n_forward_steps=2)
    assert "Stepper.predict" in str(err.value)


def test_engine_refuses_a_mask_that_is_not_a_plane():
    from ace_amd.ocean_rollout import OceanRolloutEngine
    stepper = _stepper()
    stepper._output_masking._mask._masks["mask_2d"] = torch.ones(1, 12, 24)
    with pytest.raises(NotImplementedError, match="2-D"):
        OceanRolloutEngine(stepper, batch=1, n_forward_steps=2)


def test_engine_needs_a_device_and_a_graph_mode():
    from ace_amd.ocean_rollout import OceanRolloutEngine
    stepper = _stepper()
    with pytest.raises(ValueError, match="graph"):
        OceanRolloutEngine(stepper, batch=1, n_forward_steps=2, graph="all")
    with pytest.raises(RuntimeError, match="cuda"):
        OceanRolloutEngine(stepper, batch=1, n_forward_steps=2)


def test_engine_predict_routes_samudra_steppers():
    import ace_amd
    from ace_amd.inference import EnginePredict
    assert ace_amd.OceanRolloutEngine is not None
    pred = EnginePredict(_stepper(), batch=1, graph=None)
    ic = {n: torch.zeros(1, 1, 12, 24) for n in ["sst", "thetao_0", "thetao_1", "thetao_2", "so_0", "HI", "ocean_sea_ice_fraction"]}
    forcing = {n: torch.zeros(1, 3, 12, 24) for n in ["land_fraction", "hfds"]}
    with pytest.raises(RuntimeError, match="OceanRolloutEngine"):        # a Samudra stepper reaches the ocean engine (no device here)
        pred(ic, forcing)
