#!/usr/bin/env python
"""The coupled emulator at the shipped shapes - 1 degree (180 x 360), B = 1, n_inner = 20 (a 5 day ocean step over a 6 h atmosphere
step), the SFNO atmosphere of bench.py --hooks (44 in / 50 out channels, atmosphere corrector, prescribed-SST ocean hook), the
Samudra ocean of tools/bench_ocean_step.py (19 levels, input + output masking, the shipped ocean corrector), the shipped exchange
name lists of tools/bench_coupler.py (nine atmosphere -> ocean next-step forcings plus the shared land_fraction, the ocean's
ocean_sea_ice_fraction as the atmosphere's sea_ice_fraction, interpolate: false as bench.py --hooks) - seeded weights, one MI355X.

Writes profiles/coupled_rollout_bench.json, ms per coupled step (= 20 atmosphere steps + the exchange + 1 ocean step):
  coupled_stepper_predict   ``CoupledStepper.predict`` over a window of ``--steps`` coupled steps
  engine_none / _step / _window   ``CoupledRolloutEngine.run_window`` on loaded buffers, per graph mode
  components   ``RolloutEngine`` (20 steps) and ``OceanRolloutEngine`` (1 step) alone on the same steppers in the same graph mode,
               as 20 x atmosphere step + 1 x ocean step: what a coupled step costs with no exchange at all
Every path is warmed by whole windows, then the paths are alternated round by round (all see the same box in the same minute),
device events around ``--iters`` windows each; the medians over ``--rounds`` are reported with the rounds beside them.  No ratio is
asserted.  Needs an MI355X; there is no CPU timing."""
import argparse
import datetime
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

B, N_INNER = 1, 20


def atmosphere(dev, seed=0):
    """bench.py's --hooks stepper with the ocean's nine forcings among its diagnostics"""
    import numpy as np

    import ace_amd
    import bench
    import bench_ocean_step as bos
    from ace_amd.step import NormalizationConfig
    forcing, prog, diag = bench.hook_names()
    diag = [d for d in diag if not d.startswith("diag_")] + [n for n in bos.FORCING if n not in diag]
    diag += [f"diag_{k}" for k in range(len(diag), bench.N_DIAGNOSTIC)]
    assert len(diag) == bench.N_DIAGNOSTIC and set(bos.FORCING) <= set(diag)
    in_names, out_names = forcing + prog, prog + diag
    means = {k: 0.1 for k in in_names + out_names}
    stds = {k: 1.1 for k in in_names + out_names}
    means.update({"PRESsfc": 1.0e5, "surface_temperature": 288.0, "HGTsfc": 300.0, "DSWRFtoa": 340.0})
    stds.update({"PRESsfc": 1.0e3, "surface_temperature": 10.0, "HGTsfc": 100.0, "DSWRFtoa": 100.0})
    for k in range(8):
        means[f"specific_total_water_{k}"], stds[f"specific_total_water_{k}"] = 3.0e-3, 1.0e-4
        means[f"air_temperature_{k}"], stds[f"air_temperature_{k}"] = 250.0, 5.0
    cfg = ace_amd.SingleModuleStepConfig(
        builder=ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet", config=bench.ACE2),
        in_names=in_names, out_names=out_names, normalization=NormalizationConfig(means=means, stds=stds),
        ocean={"surface_temperature_name": "surface_temperature", "ocean_fraction_name": "ocean_fraction"},
        corrector={"conserve_dry_air": True, "moisture_budget_correction": "advection_and_precipitation",
                   "force_positive_names": ["PRATEsfc"] + [f"specific_total_water_{k}" for k in range(8)],
                   "total_energy_budget_correction": {"method": "constant_temperature", "constant_unaccounted_heating": 0.0}})
    lat, _ = np.polynomial.legendre.leggauss(bench.IMG[0])
    lat = torch.tensor(np.degrees(np.arcsin(lat)), dtype=torch.float32)
    ak = torch.linspace(0.0, 2.0e4, 9).flip(0) * torch.linspace(0.0, 1.0, 9)
    bk = torch.linspace(0.0, 1.0, 9)
    info = ace_amd.DatasetInfo(bench.IMG, lat=lat, lon=torch.arange(bench.IMG[1]) * (360.0 / bench.IMG[1]), ak=ak, bk=bk)
    torch.manual_seed(seed)
    stepper = ace_amd.Stepper.from_config(cfg, info, device=dev)
    stepper.set_eval()
    return stepper, info


def coupled_stepper(dev):
    import bench_ocean_step as bos
    from ace_amd import coupled
    from ace_amd.checkpoint import load_stepper
    state = bos.stepper_state(ohc=False)["stepper"]
    state["config"]["step"]["config"]["next_step_forcing_names"] = bos.FORCING + ["land_fraction"]
    ocean = load_stepper(state, device=dev)
    atmos, atmos_info = atmosphere(dev)
    config = coupled.CoupledStepperConfig(
        ocean=coupled.ComponentConfig("5D", ocean.stepper.config), atmosphere=coupled.ComponentConfig("6h", atmos.config),
        ocean_fraction_prediction={"sea_ice_fraction_name": "ocean_sea_ice_fraction", "land_fraction_name": "land_fraction",
                                   "sea_ice_fraction_name_in_atmosphere": "sea_ice_fraction"})
    assert config.n_inner_steps == N_INNER and set(config.atmosphere_to_ocean_forcing_names) == set(bos.FORCING)
    assert config.shared_forcing_exogenous_names == ["land_fraction"]
    stepper = coupled.CoupledStepper(config, ocean.stepper, atmos, coupled.CoupledDatasetInfo(ocean.dataset_info, atmos_info))
    stepper.set_eval()
    return stepper


def window_data(stepper, n_outer, dev, seed=3):
    import bench_ocean_step as bos
    g = torch.Generator().manual_seed(seed)
    cfg = stepper.config
    H, W = bos.H, bos.W
    a_mean = {k: float(v) for k, v in stepper.atmosphere._step_obj.normalizer.means.items()}
    a_std = {k: float(v) for k, v in stepper.atmosphere._step_obj.normalizer.stds.items()}
    draw = lambda name, nt: (torch.randn(B, nt, H, W, generator=g) * 0.1 * a_std.get(name, 1.0) + a_mean.get(name, 1.0)).to(dev)
    ic = {"atmosphere": {k: draw(k, 1) for k in stepper.atmosphere.prognostic_names},
          "ocean": {k: (torch.randn(B, 1, H, W, generator=g) * 0.1 + (285.0 if k == "sst" else 1.0)).to(dev)
                    for k in stepper.ocean.prognostic_names}}
    ic["ocean"]["ocean_sea_ice_fraction"] = torch.rand(B, 1, H, W, generator=g).to(dev) * 0.5
    Ta, To = n_outer * N_INNER + 1, n_outer + 1
    forcing = {"atmosphere": {k: draw(k, Ta) for k in cfg.atmosphere_forcing_window_names},
               "ocean": {k: torch.randn(B, To, H, W, generator=g).to(dev) for k in cfg.ocean_forcing_window_names}}
    forcing["atmosphere"]["land_fraction"] = torch.rand(B, Ta, H, W, generator=g).to(dev) * 0.5
    return ic, forcing


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2, help="coupled steps per window")
    ap.add_argument("--iters", type=int, default=2, help="windows per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coupled_rollout_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_coupled_rollout needs an MI355X: nothing is timed on the CPU")
    from ace_amd.coupled_rollout import CoupledRolloutEngine
    from ace_amd.ocean_rollout import OceanRolloutEngine
    from ace_amd.rollout import RolloutEngine
    dev = torch.device("cuda", 0)
    n_outer = args.steps
    stepper = coupled_stepper(dev)
    ic, forcing = window_data(stepper, n_outer, dev)
    paths = {"coupled_stepper_predict": lambda: stepper.predict(ic, forcing)}
    engines = {}
    for mode in (None, "step", "window"):
        name = mode or "none"
        eng = engines[name] = CoupledRolloutEngine(stepper, B, n_outer, graph=mode)
        eng.load(ic, forcing)
        paths[f"engine_{name}"] = eng.run_window
        # the components alone, on windows of their own filled from the coupled engine's buffers (so every field is there)
        a = RolloutEngine(stepper.atmosphere, B, N_INNER, graph=mode)
        o = OceanRolloutEngine(stepper.ocean, B, 1, graph=mode)
        eng.run_window()
        torch.cuda.synchronize()
        for part, whole in ((a, eng.atmosphere), (o, eng.ocean)):
            part.load({k: v for k, v in whole.ic.items()},
                      {k: v[:, :part.T + 1] for k, v in {**whole.forcing, **whole.target}.items()})
        paths[f"atmosphere_engine_{name}"] = a.run_window
        paths[f"ocean_engine_{name}"] = o.run_window
    per = {k: (1 if k.startswith(("atmosphere_engine", "ocean_engine")) else n_outer) for k in paths}
    with torch.no_grad():
        for fn in paths.values():                       # warm-up: whole windows of every path (captures included)
            fn()
            fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in paths}
        for _ in range(args.rounds):
            for k, fn in paths.items():                 # alternated
                rounds[k].append(timed(fn, args.iters) / per[k])
    med = {k: statistics.median(v) for k, v in rounds.items()}
    result = {"grid": [180, 360], "batch": B, "n_inner": N_INNER, "coupled_steps_per_window": n_outer, "iters": args.iters,
              "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
              "unit": "ms per coupled step (20 atmosphere steps + the exchange + 1 ocean step)",
              "atmosphere": "SFNO, bench.py --hooks (44 in / 50 out, atmosphere corrector, prescribed-SST ocean hook)",
              "ocean": "Samudra, 19 levels, input + output masking, the shipped ocean corrector (tools/bench_ocean_step.py)",
              "exchange_launches_per_window": {k: e.launches() for k, e in engines.items()},
              "coupled_stepper_predict_ms": round(med["coupled_stepper_predict"], 3), "rows": [],
              "rounds_ms": {k: [round(x, 3) for x in v] for k, v in rounds.items()}}
    for name in engines:
        a_ms, o_ms, e_ms = med[f"atmosphere_engine_{name}"] / N_INNER, med[f"ocean_engine_{name}"], med[f"engine_{name}"]
        parts = N_INNER * a_ms + o_ms
        result["rows"].append({
            "graph": name, "engine_ms": round(e_ms, 3), "atmosphere_step_ms": round(a_ms, 4), "ocean_step_ms": round(o_ms, 3),
            "components_ms": round(parts, 3), "overhead_over_components_ms": round(e_ms - parts, 3),
            "overhead_over_components": round(e_ms / parts - 1.0, 4),
            "coupled_stepper_predict_over_engine": round(med["coupled_stepper_predict"] / e_ms, 3)})
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
