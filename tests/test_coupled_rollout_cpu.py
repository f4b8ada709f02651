"""The coupled rollout engine without a GPU: the host-side argument checks of ace_couple_ocean_to_atmosphere_window, the host plan
(``plan_coupled_window``: which plane every input of every step reads, which levels every exchange writes) against the slicing of
``CoupledStepper.predict_generator`` written out in indices, and the refusals, all raised before any device work."""
import pytest
import torch

import ace_amd
from ace_amd import coupled, coupled_rollout
from ace_amd.coupled_rollout import CoupledRolloutEngine, Ref, plan_coupled_window
from _coupled import A_DIAG, A_FORCING, A_PROG, B, H, N_INNER, O_FORCING, O_NEXT_STEP, O_OUT, W, coupled_checkpoint, with_cpu_networks


def test_the_abi_refuses_on_the_host_before_any_launch():
    """the argument checks of the window entry run before the first HIP call, so they hold without a GPU"""
    from ace_amd import _lib
    L = _lib.lib()
    t = [1] * 5                      # non-null tables (never read: every case below is refused)
    nulls = [None] * 5
    for args, word in (((*nulls, 0, 0, 0, 1, 1, 4), "null argument"), ((*t[:4], None, 0, 0, 0, 1, 1, 4), "null argument"),
                       ((*t, 0, 0, 0, 1, 1, 0), "hw"), ((*t, 0, 0, 0, 1, 1, -4), "hw"), ((*t, 0, 0, 0, 0, 1, 4), "n_inner"),
                       ((*t, 0, 0, 0, -3, 1, 4), "n_inner"), ((*t, 0, 0, 0, 4097, 1, 4), "n_inner"),
                       ((*t, coupled.MAX_NAMES + 1, 0, 0, 1, 1, 4), "npass"), ((*t, -1, 0, 0, 1, 1, 4), "npass"),
                       ((*t, 0, 3, 0, 1, 1, 4), "mode"), ((*t, 0, -1, 0, 1, 1, 4), "mode"), ((*t, 0, 0, 2, 1, 1, 4), "interpolate"),
                       ((*t, 0, 0, -1, 1, 1, 4), "interpolate"), ((*t, 0, 0, 0, 1, 0, 4), "batch"), ((*t, 0, 0, 0, 1, 70000, 4), "batch")):
        assert L.ace_couple_ocean_to_atmosphere_window(*args, None) == _lib.ACE_ERR_INVALID, args
        msg = L.ace_couple_last_error().decode()
        assert msg.startswith("ace_couple_ocean_to_atmosphere_window: ") and word in msg, msg
    # the existing entry keeps its own name in its messages
    assert L.ace_couple_ocean_to_atmosphere(*t, 0, 3, 0, 1, 1, 4, None) == _lib.ACE_ERR_INVALID
    assert L.ace_couple_last_error().decode().startswith("ace_couple_ocean_to_atmosphere: ")


@pytest.fixture(scope="module")
def stepper():
    return ace_amd.load_coupled_stepper(coupled_checkpoint(), device="cpu")


MASKED = ("surface_temperature", "ocean_fraction", "sea_ice_fraction", "ocean_sea_ice_fraction")


@pytest.mark.parametrize("n_outer", [1, 3])
def test_the_plan_is_the_slicing_of_the_predict_generator(stepper, n_outer):
    """``CoupledStepper.predict_generator`` in indices: coupled step i cuts the atmosphere record at levels i n .. (i + 1) n, the
    ocean's fields are constant over that window, atmosphere step t of it reads window level t (t + 1 for a next-step forcing) and,
    as state, the prescribed initial condition (t = 0) or the previous output; the means are taken over the outputs of these n steps
    and over window levels 1 .. n of a shared forcing, into levels i, i + 1 of the ocean record."""
    n = N_INNER
    assert coupled_rollout._exchange_masks(stepper).keys() == set(MASKED)
    plan = plan_coupled_window(stepper.config, n_outer, MASKED)
    assert (plan.n_inner, plan.n_outer, plan.mode, plan.passed, plan.scratch) == (n, n_outer, coupled.OFRAC_FROM_OCEAN_SIF, [], [])
    assert plan.atmosphere.forcing == A_FORCING and plan.atmosphere.prognostic == A_PROG
    assert plan.atmosphere.target == ["surface_temperature"] and plan.ocean.forcing == O_FORCING and plan.ocean.target == []
    assert plan.supplied == {"atmosphere": {"surface_temperature", "ocean_fraction", "sea_ice_fraction"},
                             "ocean": {"hfds", "DLWRFsfc", "land_fraction", "DSWRFtoa"}}
    A, O = "atmosphere", "ocean"
    for i in range(n_outer):
        window = list(range(i * n, (i + 1) * n + 1))                            # atmos_record[:, i n : (i + 1) n + 1]
        ocean_state = (lambda k: Ref(O, "ic", k, 0)) if i == 0 else (lambda k: Ref(O, "out", k, i - 1))
        atmos_ic = Ref(A, "ic", "surface_temperature", 0) if i == 0 else Ref(A, "out", "surface_temperature", i * n - 1)
        # ---- ocean -> atmosphere: sources and the levels written
        sst, ic, of, si, raw = plan.o2a[i]
        assert (sst.src, sst.dst, sst.dst_levels, sst.mask) == (ocean_state("sst"), Ref(A, "target", "surface_temperature", window[0]),
                                                               n + 1, "surface_temperature")
        assert (ic.src, ic.dst, ic.dst_levels, ic.mask) == (atmos_ic, Ref(A, "prescribed", "surface_temperature", i), 1, None)
        assert (of.src, of.src_levels, of.dst, of.mask) == (Ref(A, "forcing", "land_fraction", window[0]), n + 1,
                                                            Ref(A, "forcing", "ocean_fraction", window[0]), "ocean_fraction")
        assert (si.src, si.dst, si.mask) == (ocean_state("ocean_sea_ice_fraction"), Ref(A, "forcing", "sea_ice_fraction", window[0]),
                                             "sea_ice_fraction")
        assert (raw.src, raw.dst, raw.mask) == (ocean_state("ocean_sea_ice_fraction"), None, None)      # no atmosphere input of that name
        written = plan.written(i)
        for key in ((A, "target", "surface_temperature"), (A, "forcing", "ocean_fraction"), (A, "forcing", "sea_ice_fraction")):
            assert written[key] == window, key
        assert written[(A, "prescribed", "surface_temperature")] == [i]
        # ---- the n atmosphere steps
        for t in range(n):
            s = i * n + t
            for name in A_FORCING:
                level = window[t + 1] if name == "DSWRFtoa" else window[t]      # next_step_forcing_names: ["DSWRFtoa"]
                assert plan.atmosphere_in(name, s) == Ref(A, "forcing", name, level), (name, s)
                assert level in (written.get((A, "forcing", name)) or window)
            for name in A_PROG:
                if t == 0 and name == "surface_temperature":
                    want = Ref(A, "prescribed", name, i)                         # the initial condition the exchange edited
                elif s == 0:
                    want = Ref(A, "ic", name, 0)
                else:
                    want = Ref(A, "out", name, s - 1)                            # the yielded output, untouched
                assert plan.atmosphere_in(name, s) == want, (name, s)
        # ---- atmosphere -> ocean
        means = {m.name: m for m in plan.a2o[i]}
        assert set(means) == {"hfds", "DLWRFsfc", "land_fraction", "DSWRFtoa"}
        for name, m in means.items():
            if name in A_DIAG:
                assert m.srcs == [Ref(A, "out", name, i * n + t) for t in range(n)], name              # atmos_steps[t][name]
            else:
                assert m.srcs == [Ref(A, "forcing", name, window[1 + t]) for t in range(n)], name      # atmos_window[name][:, 1 + t]
            assert m.dst == Ref(O, "forcing", name, i) and written[(O, "forcing", name)] == [i, i + 1]
            assert m.slot == (1 if name in O_NEXT_STEP else 0), name                                   # [NaN, mean] / [mean, NaN]
        # ---- the ocean step reads the level the mean was stored at, and the state of the previous step
        for name in O_FORCING:
            level = i + 1 if name in O_NEXT_STEP else i
            assert plan.ocean_in(name, i) == Ref(O, "forcing", name, level)
            if name in means:
                assert level == i + means[name].slot
        for name in O_OUT:
            assert plan.ocean_in(name, i) == ocean_state(name)
    assert plan.overrides() == {("surface_temperature", i * n): Ref("atmosphere", "prescribed", "surface_temperature", i)
                                for i in range(n_outer)}


def _config_state(a_forcing, o_forcing, o_prog, prediction):
    def component(builder, in_names, out_names, **extra):
        return {"step": {"type": "single_module", "config": dict(builder={"type": builder, "config": {}}, in_names=in_names,
                                                                 out_names=out_names, normalization={"network": {}}, **extra)}}
    a = component("SphericalFourierNeuralOperatorNet", a_forcing + ["surface_temperature"], ["surface_temperature", "hfds"],
                  ocean={"surface_temperature_name": "surface_temperature", "ocean_fraction_name": "ocean_fraction"})
    o = component("Samudra", o_forcing + o_prog, o_prog, next_step_forcing_names=["hfds"])
    return {"ocean": {"timedelta": "12h", "stepper": o}, "atmosphere": {"timedelta": "6h", "stepper": a}, "sst_name": "sst",
            "ocean_fraction_prediction": prediction}


def test_the_plan_of_the_carried_fraction_and_of_an_absent_destination():
    # carried: the atmosphere's own ocean fraction masked in place where it has a mask, left alone where it has none
    config = coupled.CoupledStepperConfig.from_state(_config_state(["ocean_fraction", "zos"], ["hfds"], ["sst", "zos"], None))
    for masked in ((), ("ocean_fraction",)):
        plan = plan_coupled_window(config, 2, masked)
        assert plan.mode == coupled.OFRAC_CARRIED and plan.passed == ["zos"] and plan.n_inner == 2
        own = Ref("atmosphere", "forcing", "ocean_fraction", 2)
        assert plan.o2a[1][2] == coupled_rollout.Slot(own, 3, own if masked else None, 3, "ocean_fraction" if masked else None)
        assert plan.o2a[1][3].dst == Ref("atmosphere", "forcing", "zos", 2) and plan.o2a[1][3].src == Ref("ocean", "out", "zos", 0)
        assert plan.supplied["atmosphere"] == {"surface_temperature", "zos"}          # the carried fraction is loaded, not supplied
    # a sea_ice_fraction the atmosphere has no input for: the kernel needs the destination, the engine gives it a scratch window
    prediction = {"sea_ice_fraction_name": "sea_ice_fraction", "land_fraction_name": "land_fraction"}
    config = coupled.CoupledStepperConfig.from_state(_config_state(["ocean_fraction", "land_fraction"], ["hfds"],
                                                                   ["sst", "sea_ice_fraction"], prediction))
    plan = plan_coupled_window(config, 1)
    assert plan.mode == coupled.OFRAC_FROM_SIF and plan.scratch == ["sea_ice_fraction"]
    assert plan.o2a[0][3].dst == Ref("atmosphere", "scratch", "sea_ice_fraction", 0) and plan.o2a[0][4].dst is None


def _refused(stepper, match, graph="step"):
    with pytest.raises(NotImplementedError, match=match) as err:
        CoupledRolloutEngine(stepper, B, 2, graph=graph)
    assert "CoupledStepper.predict" in str(err.value)


def test_every_refusal_comes_before_device_work(monkeypatch):
    """on steppers loaded onto the CPU, where any device work would fail differently: each refusal names
    ``CoupledStepper.predict``; a supported pair on the CPU raises the ocean engine's RuntimeError"""
    load = lambda ckpt=None: ace_amd.load_coupled_stepper(ckpt or coupled_checkpoint(), device="cpu")
    with pytest.raises(RuntimeError, match="runs on an MI355X") as err:
        CoupledRolloutEngine(load(), B, 2)
    assert str(err.value).startswith("OceanRolloutEngine")
    with pytest.raises(ValueError, match="graph must be"):
        CoupledRolloutEngine(load(), B, 2, graph="all")
    # -- what the component engines refuse
    _refused(with_cpu_networks(load()), "not of the SFNO family")                        # the CPU oracle as the atmosphere's module
    s = load()
    s.ocean._step_obj.module = with_cpu_networks(load()).ocean._step_obj.module
    _refused(s, "ocean engine refuses.*not Samudra")
    s = load()
    s.atmosphere._masks = True
    _refused(s, "atmosphere engine refuses.*static spatial masking")
    s = load()
    s.ocean._multi_call_config = object()
    _refused(s, "ocean engine refuses.*multi-call")
    # -- the coupled engine's own
    s = load()
    s.atmosphere._step_obj.module.torch_module.draw_noise = lambda *a: None
    _refused(s, "noise-conditioned")
    s = load()
    s.atmosphere._step_obj.module._label_encoding = object()
    _refused(s, "label-conditioned")
    s = load()
    s.atmosphere._multi_call_config = object()
    _refused(s, "multi-call diagnostics")
    s = load()
    s.atmosphere._step_obj.secondary_decoder = object()
    _refused(s, "secondary decoder")
    _refused(s, "secondary decoder", graph="window")
    s = load()
    provider = s.coupler._mask_provider
    provider._masks["mask_sea_ice_fraction"] = torch.ones(2, H, W)                        # a mask with a leading dimension
    _refused(s, "mask of 'sea_ice_fraction'.*not a 2-D")
    monkeypatch.setattr(coupled_rollout, "MAX_NAMES", 3)                                   # four averaged fields in the tiny pair
    _refused(load(), "4 exchanged fields.*ACE_COUPLE_MAX_NAMES")


def test_more_exchanged_fields_than_the_kernels_take():
    def config(n_fluxes):
        fluxes = [f"flux_{k}" for k in range(n_fluxes)]
        state = _config_state(["ocean_fraction"], ["hfds"], ["sst"], None)
        a = state["atmosphere"]["stepper"]["step"]["config"]
        o = state["ocean"]["stepper"]["step"]["config"]
        a["out_names"] = a["out_names"] + fluxes
        o["in_names"] = fluxes + o["in_names"]
        o["next_step_forcing_names"] = ["hfds"] + fluxes
        return coupled.CoupledStepperConfig.from_state(state)
    over = config(coupled.MAX_NAMES)                                                       # and hfds
    assert len(over.atmosphere_to_ocean_forcing_names) == coupled.MAX_NAMES + 1
    with pytest.raises(NotImplementedError, match="CoupledStepper.predict"):
        plan_coupled_window(over, 1)
    assert len(plan_coupled_window(config(coupled.MAX_NAMES - 1), 1).a2o[0]) == coupled.MAX_NAMES


def test_the_engines_build_the_same_tables_without_an_override():
    """``WindowEngine.in_plane`` with no override is the window layout of before; an override replaces exactly its (name, s)"""
    from ace_amd.rollout import WindowEngine
    eng = WindowEngine.__new__(WindowEngine)
    eng.ic = {"p": torch.zeros(B, 1, 2, 2)}
    eng.out = {"p": torch.arange(B * 3 * 4.0).reshape(B, 3, 2, 2)}
    eng.forcing = {"f": torch.arange(B * 4 * 4.0).reshape(B, 4, 2, 2), "g": torch.zeros(B, 4, 2, 2)}
    eng.next_step_forcing = {"g"}
    eng._in_override = {}
    plain = {(n, s): eng.in_plane(n, s) for n in ("p", "f", "g") for s in range(3)}
    assert plain[("p", 0)].data_ptr() == eng.ic["p"].data_ptr() and plain[("p", 2)].data_ptr() == eng.out["p"][:, 1].data_ptr()
    assert plain[("f", 1)].data_ptr() == eng.forcing["f"][:, 1].data_ptr()
    assert plain[("g", 1)].data_ptr() == eng.forcing["g"][:, 2].data_ptr()
    scratch = torch.zeros(B, 2, 2)
    eng._in_override = {("p", 2): scratch}
    for key, plane in plain.items():
        got = eng.in_plane(*key)
        assert got.data_ptr() == (scratch if key == ("p", 2) else plane).data_ptr(), key
