"""The coupled stepper without a GPU: the torch path of ``Coupler`` and the configuration's name sets and errors against the
reference's own (tests/golden/gen_coupled.pt, emitted by fme/coupled/stepper.py through tests/golden/make_golden_coupled.py), the
order of a coupled rollout against a composition of ``Stepper.predict`` calls, the loader, and the host-side refusals of the two
native entries."""
import copy
import datetime

import pytest
import torch

import ace_amd
from ace_amd import coupled
from ace_amd.masking import SpatialMaskProvider
from ace_amd.ocean import Prescriber
from _coupled import N_INNER, N_OUTER, coupled_checkpoint, coupled_data, same, with_cpu_networks
from _util import checkpoint_case, load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("gen_coupled.pt")


@pytest.fixture(scope="module")
def tiny():
    return with_cpu_networks(ace_amd.load_coupled_stepper(coupled_checkpoint(), device="cpu")), coupled_data()


def _coupler(gold, case, fused=False):
    config = coupled.CoupledStepperConfig.from_state(case["config"])
    prescriber = Prescriber("surface_temperature", "ocean_fraction", 1, case["interpolate"])
    return coupled.Coupler(config, SpatialMaskProvider(gold["masks"][case["masks"]]), prescriber, (6, 8), fused=fused)


def test_torch_path_reproduces_the_reference_exchange_bitwise(gold):
    assert len(gold["exchange"]) >= 15
    for i, case in enumerate(gold["exchange"]):
        d = gold["inputs"][case["n_inner"]]
        coupler = _coupler(gold, case)
        forcings, ic = coupler.atmosphere_forcings(d["atmos_window"], d["ocean_state"], d["atmos_ic"])
        assert set(forcings) == set(case["atmosphere_forcings"]) | set(case["atmosphere_forcings_from_window"]), i
        for k, want in case["atmosphere_forcings"].items():
            assert same(forcings[k], want), (i, k)
        for k in case["atmosphere_forcings_from_window"]:
            assert forcings[k] is d["atmos_window"][k], (i, k)
        assert set(ic) == set(case["atmos_ic"])
        for k, want in case["atmos_ic"].items():
            assert same(ic[k], want), (i, k)
        ocean = coupler.ocean_forcings(d["ocean_window"], d["atmos_steps"], d["atmos_window"])
        assert set(ocean) == set(case["ocean_forcings"]) | set(case["ocean_forcings_from_window"]), i
        for k, want in case["ocean_forcings"].items():
            assert same(ocean[k], want), (i, k)
        assert coupler.launches() == 0


def test_name_sets_and_errors_are_the_references(gold):
    assert sum("error" in r for r in gold["configs"].values()) >= 12
    for name, want in gold["configs"].items():
        if "error" in want:
            with pytest.raises(ValueError) as err:
                coupled.CoupledStepperConfig.from_state(want["config"])
            assert str(err.value) == want["error"], name
            continue
        config = coupled.CoupledStepperConfig.from_state(want["config"])
        for prop, names in want["names"].items():
            assert set(getattr(config, prop)) == set(names), (name, prop)
        assert config.n_inner_steps == want["n_inner_steps"], name
        assert config.timestep.total_seconds() == want["timestep_seconds"], name


def test_durations_parse_without_pandas():
    td = datetime.timedelta
    for text, want in (("5D", td(days=5)), ("6h", td(hours=6)), ("P5D", td(days=5)), ("PT6H", td(hours=6)), ("1D12h", td(hours=36)),
                       ("P1DT12H", td(hours=36)), ("30min", td(minutes=30)), ("18h", td(hours=18))):
        assert coupled._parse_timedelta_plain(text) == want, text
        assert coupled.parse_timedelta(text) == want, text
    with pytest.raises(ValueError):
        coupled._parse_timedelta_plain("fortnight")


def test_config_state_round_trip_drops_the_deprecated_keys(gold):
    state = copy.deepcopy(gold["configs"]["predicted_ocean_sif_renamed"]["config"])
    config = coupled.CoupledStepperConfig.from_state(state)
    again = coupled.CoupledStepperConfig.from_state(config.get_state())
    assert again.get_state() == config.get_state()
    for prop in gold["configs"]["predicted_ocean_sif_renamed"]["names"]:
        assert set(getattr(again, prop)) == set(getattr(config, prop)), prop
    old = copy.deepcopy(state)
    old["sst_mask_name"] = "mask_2d"
    old["parameter_init"] = {"checkpoint_path": None}
    old["ocean"]["loss_contributions"] = {"n_steps": 1}
    old["atmosphere"]["loss_contributions"] = {"n_steps": 4}
    assert coupled.CoupledStepperConfig.from_state(old).get_state() == config.get_state()
    with pytest.raises(ValueError, match="unknown_key"):
        coupled.CoupledStepperConfig.from_state({**state, "unknown_key": 1})


def _composition(stepper, ic, forcing):
    """the coupled rollout written out with ``Stepper.predict`` on the two components and the (fixture-verified) torch path of
    ``Coupler`` spliced in"""
    coupler = coupled.Coupler(stepper.config, stepper.training_dataset_info.ocean_spatial_mask_provider,
                              stepper.atmosphere._step_obj._ocean.prescriber, (16, 32), fused=False)
    a_ic, o_ic = ic["atmosphere"], ic["ocean"]
    atmos, ocean = [], []
    for i in range(N_OUTER):
        window = {k: v[:, i * N_INNER:(i + 1) * N_INNER + 1] for k, v in forcing["atmosphere"].items()}
        a_forcing, a_ic = coupler.atmosphere_forcings(window, o_ic, a_ic)
        a_out, a_ic = stepper.atmosphere.predict(a_ic, a_forcing, N_INNER, compute_derived_forcings=False)
        atmos.append(a_out)
        steps = [{k: v[:, t] for k, v in a_out.items()} for t in range(N_INNER)]
        o_forcing = coupler.ocean_forcings({k: v[:, i:i + 2] for k, v in forcing["ocean"].items()}, steps, window)
        o_out, o_ic = stepper.ocean.predict(o_ic, o_forcing, 1, compute_derived_forcings=False)
        ocean.append(o_out)
    cat = lambda outs: {k: torch.cat([o[k] for o in outs], dim=1) for k in outs[0]}
    return {"atmosphere": cat(atmos), "ocean": cat(ocean)}


def test_rollout_order_is_the_composition_of_the_components(tiny):
    stepper, (ic, forcing) = tiny
    assert stepper.n_inner_steps == N_INNER and stepper.n_ic_timesteps == 1
    data, state = stepper.predict(ic, forcing)
    want = _composition(stepper, ic, forcing)
    for realm in ("atmosphere", "ocean"):
        assert set(data[realm]) == set(want[realm])
        for k, v in want[realm].items():
            assert same(data[realm][k], v), (realm, k)
        assert data[realm]["sst" if realm == "ocean" else "PRESsfc"].shape[1] == (N_OUTER if realm == "ocean" else N_OUTER * N_INNER)
    # the rollout is not degenerate: finite numbers over the ocean, which change from step to step
    sst = data["ocean"]["sst"]
    assert torch.isfinite(sst).float().mean() > 0.5 and not same(sst[:, 0], sst[:, 1])
    assert torch.isfinite(data["atmosphere"]["PRESsfc"]).all()
    assert set(state["atmosphere"]) == set(stepper.atmosphere.prognostic_names)
    assert set(state["ocean"]) == set(stepper.ocean.prognostic_names)
    assert same(state["ocean"]["sst"], sst[:, -1:])


def test_predict_generator_yields_in_the_references_order(tiny):
    stepper, (ic, forcing) = tiny
    with torch.no_grad():
        order = [(p.realm, p.step) for p in stepper.predict_generator(ic, forcing)]
    assert order == [("atmosphere", 0), ("atmosphere", 1), ("atmosphere", 2), ("ocean", 0),
                     ("atmosphere", 3), ("atmosphere", 4), ("atmosphere", 5), ("ocean", 1)]


def test_two_chained_predicts_equal_one(tiny):
    stepper, (ic, forcing) = tiny
    whole, end = stepper.predict(ic, forcing)
    first = {"atmosphere": {k: v[:, :N_INNER + 1] for k, v in forcing["atmosphere"].items()},
             "ocean": {k: v[:, :2] for k, v in forcing["ocean"].items()}}
    second = {"atmosphere": {k: v[:, N_INNER:] for k, v in forcing["atmosphere"].items()},
              "ocean": {k: v[:, 1:] for k, v in forcing["ocean"].items()}}
    a, state = stepper.predict(ic, first)
    b, end2 = stepper.predict(state, second)
    for realm in ("atmosphere", "ocean"):
        for k, v in whole[realm].items():
            assert same(torch.cat([a[realm][k], b[realm][k]], dim=1), v), (realm, k)
        for k, v in end[realm].items():
            assert same(end2[realm][k], v), (realm, k)


def _golden_component_states():
    """the two golden component checkpoints on one grid: the ACE2-like SFNO of gen_checkpoint.pt (8 x 16, 6 h) and the Samudra of
    gen_ocean_rollout.pt (convolutional: its weights hold on any grid), its dataset cut to the atmosphere's 8 x 16 and the
    atmosphere-generated DLWRFsfc made a next-step forcing, as the coupled configuration demands"""
    atmosphere = copy.deepcopy(checkpoint_case(load_golden("gen_checkpoint.pt"), "ace2_like")["state"])
    ocean = copy.deepcopy(load_golden("gen_ocean_rollout.pt")["stepper"])
    ds = ocean["dataset_info"]
    ds["horizontal_coordinates"] = atmosphere["dataset_info"]["horizontal_coordinates"]
    ds["mask_provider"]["masks"] = {k: v[4:12, 8:24].clone() for k, v in ds["mask_provider"]["masks"].items()}
    vc = ds["vertical_coordinate"]
    vc["mask"], vc["deptho"] = vc["mask"][4:12, 8:24].clone(), vc["deptho"][4:12, 8:24].clone()
    ocean["config"]["step"]["config"]["next_step_forcing_names"] = ["hfds", "DLWRFsfc"]
    return atmosphere, ocean


@pytest.mark.parametrize("with_dataset_info", [True, False])
def test_load_coupled_stepper_from_the_golden_component_checkpoints(tmp_path, with_dataset_info):
    atmosphere, ocean = _golden_component_states()
    state = {"config": {"ocean": {"timedelta": "5D", "stepper": ocean["config"], "loss_contributions": {}},
                        "atmosphere": {"timedelta": "6h", "stepper": atmosphere["config"]}, "sst_name": "sst",
                        "sst_mask_name": "mask_2d"},
             "atmosphere_state": atmosphere, "ocean_state": ocean}
    if with_dataset_info:
        state["dataset_info"] = {"ocean": ocean["dataset_info"], "atmosphere": atmosphere["dataset_info"]}
    path = tmp_path / "coupled.tar"
    torch.save({"stepper": state}, path)
    stepper = ace_amd.load_coupled_stepper(path, device="cpu")
    assert isinstance(stepper, ace_amd.CoupledStepper) and stepper.n_inner_steps == 20
    assert stepper.config.timestep == datetime.timedelta(days=5)
    assert set(stepper.config.ocean_to_atmosphere_forcing_names) == {"sst"}
    assert set(stepper.config.atmosphere_to_ocean_forcing_names) == {"DLWRFsfc"}
    assert stepper.config.atmosphere.stepper is stepper.atmosphere.config
    assert "mask_2d" in stepper.training_dataset_info.ocean_spatial_mask_provider.masks
    assert tuple(stepper.training_dataset_info.ocean.img_shape) == (8, 16)
    assert len(stepper.modules) == 2 and not any(m.training for m in stepper.modules)
    assert ace_amd.load_coupled_stepper(state, device="cpu").n_inner_steps == 20          # the stepper state itself, as a dict
    again = coupled.CoupledDatasetInfo.from_state(stepper.training_dataset_info.get_state())
    assert torch.equal(again.ocean_spatial_mask_provider.masks["mask_2d"],
                       stepper.training_dataset_info.ocean_spatial_mask_provider.masks["mask_2d"])


def test_the_stepper_refuses_what_the_engines_refuse():
    ckpt = coupled_checkpoint()
    bad = copy.deepcopy(ckpt)
    atmosphere = bad["stepper"]["atmosphere_state"]
    atmosphere["dataset_info"]["horizontal_coordinates"] = {"lat": torch.linspace(-80, 80, 8), "lon": torch.arange(16.0) * 22.5}
    builder = atmosphere["config"]["step"]["config"]["builder"]
    small = ace_amd.ModuleSelector(**builder).build(7, 6, ace_amd.DatasetInfo((8, 16)))           # the same network on 8 x 16
    atmosphere["step"]["module"] = {**{f"module.{k}": v for k, v in small.torch_module.state_dict().items()}, "label_encoding": None}
    with pytest.raises(ValueError, match="different grids"):
        ace_amd.load_coupled_stepper(bad, device="cpu")
    bad = copy.deepcopy(ckpt)
    info = bad["stepper"]["dataset_info"]
    info["ocean"] = {k: v for k, v in info["ocean"].items() if k != "mask_provider"}       # (the component state keeps its own)
    with pytest.raises(ValueError, match="ocean_spatial_mask_provider"):
        ace_amd.load_coupled_stepper(bad, device="cpu")
    bad = copy.deepcopy(ckpt)
    bad["stepper"]["config"]["ocean"]["timedelta"] = "12h"
    with pytest.raises(ValueError, match="Ocean timestep must match the dataset timestep"):
        ace_amd.load_coupled_stepper(bad, device="cpu")


def test_the_abi_refuses_on_the_host_before_any_launch():
    """the argument checks of the two coupler entries run before the first HIP call, so they hold without a GPU"""
    from ace_amd import _lib
    L = _lib.lib()
    t = [1] * 5                      # non-null tables (never read: every case below is refused or a no-op)
    nulls = [None] * 5
    for args, word in (((*nulls, 0, 0, 0, 1, 1, 4), "null argument"), ((*t, 0, 0, 0, 1, 1, 0), "hw"), ((*t, 0, 0, 0, 0, 1, 4), "n_inner"),
                       ((*t, 0, 0, 0, -3, 1, 4), "n_inner"), ((*t, coupled.MAX_NAMES + 1, 0, 0, 1, 1, 4), "npass"),
                       ((*t, 0, 3, 0, 1, 1, 4), "mode"), ((*t, 0, 0, 2, 1, 1, 4), "interpolate"), ((*t, 0, 0, 0, 1, 0, 4), "batch")):
        assert L.ace_couple_ocean_to_atmosphere(*args, None) == _lib.ACE_ERR_INVALID, args
        msg = L.ace_couple_last_error().decode()
        assert msg.startswith("ace_couple_ocean_to_atmosphere: ") and word in msg, msg
    for args, word in (((*nulls, 1, 1, 1, 4), "null argument"), ((*t, 1, 1, 1, 0), "hw"), ((*t, 1, 0, 1, 4), "n_inner"),
                       ((*t, coupled.MAX_NAMES + 1, 1, 1, 4), "nnames"), ((*t, 1, 1, 70000, 4), "batch")):
        assert L.ace_couple_atmosphere_to_ocean(*args, None) == _lib.ACE_ERR_INVALID, args
        msg = L.ace_couple_last_error().decode()
        assert msg.startswith("ace_couple_atmosphere_to_ocean: ") and word in msg, msg
    assert L.ace_couple_atmosphere_to_ocean(*nulls, 0, 1, 1, 4, None) == _lib.ACE_OK               # no names: a no-op
