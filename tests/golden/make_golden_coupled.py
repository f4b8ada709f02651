"""tests/golden/gen_coupled.pt: the exchange of the coupled stepper and its configuration's name sets, emitted by the REAL
reference (fme/coupled/stepper.py) - build container only.

``fme.coupled.stepper`` imports on top of oracle/ref_loader.load_stepper_ref() with namespace packages for ``fme.coupled``,
``fme.coupled.data_loading``, ``fme.ace.data_loading`` and ``fme.core.generics`` and with ``Stepper``, ``TrainOutput``,
``process_prediction_generator_list`` and ``stack_list_of_tensor_dicts`` set on the ``fme.ace.stepper`` namespace from
``fme.ace.stepper.single_module``.  The unbound ``CoupledStepper._get_atmosphere_forcings`` / ``_get_ocean_forcings`` run on an
``object.__new__(CoupledStepper)`` that carries the real ``CoupledStepperConfig`` (built by ``CoupledStepperConfig.from_state``
through the real ``StepperConfig.from_state``), the real ``SpatialMaskProvider`` and the two ``TIME_DIM``s; the prescribed
initial surface temperature is the real ``Prescriber`` on time level 0 of the result, as ``_prescribe_ic_sst`` calls it.

Stored (data only, ``torch.load(weights_only=True)``):
  "inputs"    per n_inner: the atmosphere window, the ocean state, the atmosphere initial condition, the generated atmosphere
              steps and the ocean forcing window - B = 2 on 6 x 8, NaN, +-inf and +-0 in the ocean fields, the land fraction finite
  "masks"     two providers: "full" (mask_2d, the variable-specific mask_HI, the level mask_0; so_1 has no mask) and "sparse"
              (mask_HI only: the ocean fraction, sea ice and surface temperature are unmasked)
  "exchange"  cases over the three ocean-fraction modes, with and without sea_ice_fraction_name_in_atmosphere, both prescriber
              modes, n_inner in {1, 3}: the coupled config state and the reference's outputs
  "configs"   configurations with the reference's name sets (sorted lists) or the message of the ValueError it raises"""
import importlib
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader  # noqa: E402

B, H, W = 2, 6, 8
NAME_SETS = ["ocean_to_atmosphere_forcing_names", "atmosphere_to_ocean_forcing_names", "shared_forcing_exogenous_names",
             "atmosphere_forcing_window_names", "ocean_forcing_window_names", "atmosphere_forcing_exogenous_names",
             "ocean_forcing_exogenous_names", "ocean_next_step_forcing_names"]
SFNO = {"type": "SphericalFourierNeuralOperatorNet", "config": {"embed_dim": 8, "num_layers": 1}}


def load_coupled():
    ref = ref_loader.load_stepper_ref()
    for pkg in ["fme.coupled", "fme.coupled.data_loading", "fme.ace.data_loading", "fme.core.generics"]:
        if pkg not in sys.modules:
            ref_loader._ns(pkg, os.path.join(ref_loader.REF, *pkg.split(".")))
    ns = sys.modules["fme.ace.stepper"]
    for name in ["Stepper", "TrainOutput", "process_prediction_generator_list", "stack_list_of_tensor_dicts"]:
        setattr(ns, name, getattr(ref.module, name))
    return importlib.import_module("fme.coupled.stepper")


def stepper_state(in_names, out_names, **extra):
    names = sorted(set(in_names + out_names))
    return {"step": {"type": "single_module", "config": dict(
        builder=SFNO, in_names=list(in_names), out_names=list(out_names),
        normalization={"network": {"means": {n: 0.0 for n in names}, "stds": {n: 1.0 for n in names}}}, **extra)}}


A_PROG = ["surface_temperature", "PRESsfc"]
A_DIAG = ["LHTFLsfc", "PRATEsfc"]
O_PASS = ["zos", "HI", "so_0", "so_1"]


def coupled_state(sif=None, sif_in_atmosphere=None, interpolate=False, ocean_td="18h", atmosphere_td="6h", a_in=None, a_out=None,
                  o_in=None, o_out=None, a_extra=None, o_extra=None, sst_name="sst", ocean="default", land="land_fraction"):
    """The state of a CoupledStepperConfig.  sif: None (ocean fraction carried), "sea_ice_fraction" or "ocean_sea_ice_fraction"."""
    ice = [sif] if sif else ["ocean_sea_ice_fraction"]
    o_prog = ["sst"] + O_PASS + ice
    if a_in is None:
        a_in = ["land_fraction", "ocean_fraction", "DSWRFtoa"] + O_PASS + A_PROG
        if sif:
            a_in.append(sif_in_atmosphere or sif)
    if ocean == "default":
        ocean = {"surface_temperature_name": "surface_temperature", "ocean_fraction_name": "ocean_fraction", "interpolate": interpolate}
    a = stepper_state(a_in, a_out or (A_PROG + A_DIAG), ocean=ocean, **(a_extra or {}))
    o = stepper_state(o_in or (["DSWRFtoa", "hfgeou"] + A_DIAG + o_prog), o_out or o_prog,
                      **{"next_step_forcing_names": list(A_DIAG), **(o_extra or {})})
    ofp = None
    if sif:
        ofp = {"sea_ice_fraction_name": sif, "land_fraction_name": land, "sea_ice_fraction_name_in_atmosphere": sif_in_atmosphere}
    return {"ocean": {"timedelta": ocean_td, "stepper": o}, "atmosphere": {"timedelta": atmosphere_td, "stepper": a},
            "sst_name": sst_name, "ocean_fraction_prediction": ofp}


def special(x, g):
    """NaN, +-inf and +-0 at random pixels."""
    for value in (float("nan"), float("inf"), float("-inf"), 0.0, -0.0):
        x[torch.rand(x.shape, generator=g) < 0.06] = value
    return x


def inputs(n_inner, g):
    T = n_inner + 1
    r = lambda *s: torch.randn(*s, H, W, generator=g)
    u = lambda *s: torch.rand(*s, H, W, generator=g)
    ocean = {"sst": special(r(B, 1) * 3 + 285, g), "zos": special(r(B, 1), g), "HI": special(u(B, 1), g),
             "so_0": special(r(B, 1) + 34, g), "so_1": special(r(B, 1) + 35, g),
             "sea_ice_fraction": special(u(B, 1) * 1.2 - 0.1, g), "ocean_sea_ice_fraction": special(u(B, 1) * 1.2 - 0.1, g)}
    land = u(B, T)
    land[u(B, T) < 0.2] = 0.0
    land[u(B, T) < 0.2] = 1.0
    ofrac = u(B, T) * 1.2 - 0.1
    for value in (0.0, 0.5, 1.0, 1.5, -0.0):            # the halves round to even
        ofrac[u(B, T) < 0.08] = value
    window = {"land_fraction": land, "ocean_fraction": ofrac, "DSWRFtoa": r(B, T) * 100 + 300, "surface_temperature": r(B, T) + 280,
              "sea_ice_fraction": u(B, T), "ocean_sea_ice_fraction": u(B, T), "sea_ice_fraction_atm": u(B, T)}
    ic = {"surface_temperature": r(B, 1) * 5 + 280, "PRESsfc": r(B, 1) * 1000 + 1e5}
    steps = [{"surface_temperature": r(B) + 280, "PRESsfc": r(B) * 1000 + 1e5, "LHTFLsfc": r(B) * 40 + 80,
              "PRATEsfc": r(B) * 2e-5 + 3e-5} for _ in range(n_inner)]
    steps[0]["LHTFLsfc"][0, 0, 0] = float("nan")
    steps[-1]["LHTFLsfc"][0, 0, 1] = float("inf")
    steps[0]["PRATEsfc"][1, 2, 3] = float("-inf")
    ocean_window = {"hfgeou": r(B, 2) * 0.02 + 0.08, "DSWRFtoa": r(B, 2)}
    return {"atmos_window": window, "ocean_state": ocean, "atmos_ic": ic, "atmos_steps": steps, "ocean_window": ocean_window}


def main():
    cs = load_coupled()
    smp = importlib.import_module("fme.core.spatial_mask_provider")
    prescriber_mod = importlib.import_module("fme.core.prescriber")
    g = torch.Generator().manual_seed(21)
    m = lambda: (torch.rand(H, W, generator=g) < 0.7).float()
    masks = {"full": {"mask_2d": m(), "mask_HI": m(), "mask_0": m()}, "sparse": {"mask_HI": m()}}
    data = {n: inputs(n, g) for n in (1, 3)}

    variants = [(None, None), ("sea_ice_fraction", None), ("sea_ice_fraction", "sea_ice_fraction_atm"),
                ("ocean_sea_ice_fraction", None), ("ocean_sea_ice_fraction", "sea_ice_fraction_atm")]
    cases = []
    for n_inner, provider_name, interps in ((3, "full", (False, True)), (1, "sparse", (False,)), (1, "full", (True,))):
        for i, (sif, in_atm) in enumerate(variants):
            for interpolate in interps:
                state = coupled_state(sif, in_atm, interpolate, ocean_td=f"{6 * n_inner}h")
                config = cs.CoupledStepperConfig.from_state(state)
                assert config.n_inner_steps == n_inner
                self = object.__new__(cs.CoupledStepper)
                self._config = config
                self.atmosphere = types.SimpleNamespace(TIME_DIM=1)
                self.ocean = types.SimpleNamespace(TIME_DIM=1)
                self._ocean_spatial_mask_provider = smp.SpatialMaskProvider(masks[provider_name])
                d = data[n_inner]
                forcings = cs.CoupledStepper._get_atmosphere_forcings(self, d["atmos_window"], d["ocean_state"])
                level0 = {k: v[:, :1] for k, v in forcings.items()}
                prescriber = prescriber_mod.Prescriber("surface_temperature", "ocean_fraction", 1, interpolate)
                new_ic = prescriber(level0, d["atmos_ic"], level0)
                gen = {k: torch.stack([s[k] for s in d["atmos_steps"]], dim=1) for k in d["atmos_steps"][0]}
                window_forcings = {k: v[:, 1:] for k, v in d["atmos_window"].items()}
                ocean_forcings = cs.CoupledStepper._get_ocean_forcings(self, d["ocean_window"], gen, window_forcings)
                cases.append({"config": state, "n_inner": n_inner, "masks": provider_name, "interpolate": interpolate,
                              # the window's own names come back as the very tensors of the window: their names are enough
                              "atmosphere_forcings_from_window": sorted(k for k, v in forcings.items() if v is d["atmos_window"].get(k)),
                              "atmosphere_forcings": {k: v.contiguous().clone() for k, v in forcings.items()
                                                      if v is not d["atmos_window"].get(k)},
                              "atmos_ic": {k: v.clone() for k, v in new_ic.items()},
                              "ocean_forcings_from_window": sorted(k for k, v in ocean_forcings.items() if v is d["ocean_window"].get(k)),
                              "ocean_forcings": {k: v.clone() for k, v in ocean_forcings.items() if v is not d["ocean_window"].get(k)}})

    configs = {
        "carried": coupled_state(),
        "predicted_sif": coupled_state("sea_ice_fraction"),
        "predicted_ocean_sif_renamed": coupled_state("ocean_sea_ice_fraction", "sea_ice_fraction_atm", ocean_td="5D"),
        "iso_durations": coupled_state(ocean_td="P5D", atmosphere_td="PT6H"),
        "prescribed_ocean_prognostic": coupled_state(o_extra={"prescribed_prognostic_names": ["so_1"]}),
        "prescribed_atmosphere_prognostic": coupled_state(a_extra={"prescribed_prognostic_names": ["PRESsfc"]}),
        "no_ocean_config": coupled_state(ocean=None),
        "slab": coupled_state(ocean={"surface_temperature_name": "surface_temperature", "ocean_fraction_name": "ocean_fraction",
                                     "slab": {"mixed_layer_depth_name": "mld", "q_flux_name": "qflux"}}),
        "atmosphere_slower": coupled_state(ocean_td="3h"),
        "not_a_multiple": coupled_state(ocean_td="15h"),
        "duplicate_outputs": coupled_state(o_in=["hfgeou"] + A_DIAG[1:] + ["sst"] + O_PASS + ["ocean_sea_ice_fraction", "LHTFLsfc"],
                                           o_out=["sst"] + O_PASS + ["ocean_sea_ice_fraction", "LHTFLsfc"],
                                           o_extra={"next_step_forcing_names": A_DIAG[1:]}),
        "ocean_diagnostic_as_forcing": coupled_state(o_out=["sst"] + O_PASS + ["ocean_sea_ice_fraction", "mld_diag"],
                                                     a_in=["land_fraction", "ocean_fraction", "mld_diag"] + A_PROG),
        "missing_next_step": coupled_state(o_extra={"next_step_forcing_names": ["LHTFLsfc"]}),
        "sst_not_an_output": coupled_state(sst_name="tos"),
        "sif_not_prognostic": coupled_state("sea_ice_fraction", a_in=["land_fraction", "ocean_fraction", "DSWRFtoa"] + O_PASS + A_PROG,
                                            o_in=["hfgeou"] + A_DIAG + ["sst"] + O_PASS,
                                            o_out=["sst"] + O_PASS + ["sea_ice_fraction"]),
        "land_not_a_forcing": coupled_state("sea_ice_fraction", land="lfrac"),
        "sif_not_canonical": coupled_state("HI"),
        "prescribed_clobbered": coupled_state(a_extra={"prescribed_prognostic_names": ["surface_temperature"]}),
    }
    results = {}
    for name, state in configs.items():
        try:
            config = cs.CoupledStepperConfig.from_state(state)
        except ValueError as err:
            results[name] = {"config": state, "error": str(err)}
            continue
        results[name] = {"config": state, "names": {p: sorted(getattr(config, p)) for p in NAME_SETS},
                         "n_inner_steps": config.n_inner_steps, "timestep_seconds": config.timestep.total_seconds()}
    for name, r in results.items():
        print(name, "->", r.get("error") or r["n_inner_steps"])

    rec = {"inputs": data, "masks": masks, "exchange": cases, "configs": results}
    path = os.path.join(HERE, "gen_coupled.pt")
    torch.save(rec, path)
    torch.load(path, weights_only=True)
    print("wrote", path, os.path.getsize(path), "bytes,", len(cases), "exchange cases")


if __name__ == "__main__":
    main()
