"""The exchange of the coupled stepper (ace_amd/coupled.py, csrc/coupler.hip) at 1 degree, B = 1, n_inner = 20 and the shipped CM4
name lists: nine atmosphere -> ocean next-step forcings plus the shared land_fraction, the ocean's ocean_sea_ice_fraction as the
atmosphere's sea_ice_fraction, interpolate: true.  Writes profiles/coupler_bench.json:

  call_ms     one ``Coupler.atmosphere_forcings`` / ``Coupler.ocean_forcings`` call, fused and on the torch path, the two paths
              alternated round by round, device events around ``--iters`` calls (host work of the call included: it is in the stream)
  kernel_us   the native entry alone on prebuilt tables, back to back, device events around ``--iters`` launches
  bytes       what each kernel has to move, from the shapes; bound_us = bytes / 8 TB/s; fraction_of_8TBs = bound_us / kernel_us
  tiny_pair   the tiny coupled pair of the test suite over 2 coupled steps: the largest relative difference of the fused rollout
              from the torch-path one, and of the torch-path device run from the CPU oracle on the atmosphere's first steps

Needs an MI355X; there is no CPU timing."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, B, N_INNER = 180, 360, 1, 20
A2O = ["DLWRFsfc", "DSWRFsfc", "ULWRFsfc", "USWRFsfc", "LHTFLsfc", "SHTFLsfc", "PRATEsfc", "eastward_surface_wind_stress",
       "northward_surface_wind_stress"]
A_PROG = ["surface_temperature", "PRESsfc"]
O_PROG = ["sst", "zos", "thetao_0", "so_0", "ocean_sea_ice_fraction", "HI"]
PEAK = 8.0e12


def config_state():
    def stepper(builder, in_names, out_names, **extra):
        return {"step": {"type": "single_module", "config": dict(builder={"type": builder, "config": {}}, in_names=in_names,
                                                                 out_names=out_names, normalization={"network": {}}, **extra)}}
    a = stepper("SphericalFourierNeuralOperatorNet", ["land_fraction", "ocean_fraction", "sea_ice_fraction", "DSWRFtoa"] + A_PROG,
                A_PROG + A2O, ocean={"surface_temperature_name": "surface_temperature", "ocean_fraction_name": "ocean_fraction",
                                     "interpolate": True})
    o = stepper("Samudra", ["land_fraction"] + A2O + O_PROG, O_PROG, next_step_forcing_names=A2O + ["land_fraction"])
    return {"ocean": {"timedelta": "5D", "stepper": o}, "atmosphere": {"timedelta": "6h", "stepper": a}, "sst_name": "sst",
            "ocean_fraction_prediction": {"sea_ice_fraction_name": "ocean_sea_ice_fraction", "land_fraction_name": "land_fraction",
                                          "sea_ice_fraction_name_in_atmosphere": "sea_ice_fraction"}}


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def tiny_pair(dev):
    import ace_amd
    from _coupled import N_INNER as TINY_INNER, coupled_checkpoint, coupled_data, with_cpu_networks
    from _util import rel_max
    stepper = ace_amd.load_coupled_stepper(coupled_checkpoint(), device=dev)
    ic, forcing = coupled_data()
    to = lambda d: {realm: {k: v.to(dev) for k, v in fields.items()} for realm, fields in d.items()}
    fused, _ = stepper.predict(to(ic), to(forcing))
    stepper.coupler.fused = False
    plain, _ = stepper.predict(to(ic), to(forcing))
    cpu = with_cpu_networks(ace_amd.load_coupled_stepper(coupled_checkpoint(), device="cpu"))
    with torch.no_grad():
        steps = [p for p, _ in zip(cpu.predict_generator(ic, forcing), range(TINY_INNER))]
    diff = lambda a, b: rel_max(a.nan_to_num(), b.nan_to_num())
    return {"what": "tests/_coupled.py: 16 x 32, B = 2, 2 coupled steps, n_inner = 3",
            "fused_vs_torch_path_max_rel": {realm: max(diff(fused[realm][k], v) for k, v in plain[realm].items()) for realm in plain},
            "torch_path_device_vs_cpu_oracle_atmosphere_first_steps_max_rel":
                max(diff(plain["atmosphere"][k][:, t], steps[t].data[k]) for k in steps[0].data for t in range(TINY_INNER))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coupler_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_coupler needs an MI355X: nothing is timed on the CPU")
    from ace_amd import _lib, coupled
    from ace_amd.masking import SpatialMaskProvider
    from ace_amd.ocean import Prescriber
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    config = coupled.CoupledStepperConfig.from_state(config_state())
    assert config.n_inner_steps == N_INNER and set(config.atmosphere_to_ocean_forcing_names) == set(A2O)
    assert config.shared_forcing_exogenous_names == ["land_fraction"]
    T = N_INNER + 1
    mask = (torch.rand(H, W, generator=g) < 0.7).float()
    r = lambda *s: torch.randn(*s, H, W, generator=g).to(dev)
    window = {"land_fraction": torch.rand(B, T, H, W, generator=g).to(dev), "DSWRFtoa": r(B, T)}
    ocean_state = {k: r(B, 1) for k in O_PROG}
    atmos_ic = {k: r(B, 1) for k in A_PROG}
    steps = [{k: r(B) for k in A_PROG + A2O} for _ in range(N_INNER)]
    couplers = {path: coupled.Coupler(config, SpatialMaskProvider({"mask_2d": mask}),
                                      Prescriber("surface_temperature", "ocean_fraction", 1, True), (H, W), fused=path == "fused")
                for path in ("fused", "torch")}
    calls = {"ocean_to_atmosphere": lambda c: c.atmosphere_forcings(window, ocean_state, atmos_ic),
             "atmosphere_to_ocean": lambda c: c.ocean_forcings({}, steps, window)}
    call_ms = {name: {path: [] for path in couplers} for name in calls}
    for name, call in calls.items():
        for c in couplers.values():
            timed(lambda: call(c), args.warmup)
        for _ in range(args.rounds):
            for path, c in couplers.items():          # alternated: both paths see the same box in the same minute
                call_ms[name][path].append(timed(lambda: call(c), args.iters))
    launches = couplers["fused"].launches()
    assert launches == 2 * (args.warmup + args.rounds * args.iters) and couplers["torch"].launches() == 0

    # ---- the native entries alone, on prebuilt tables
    from ace_amd.aggregator import _plane_table, _upload
    L, stream, hw = _lib.lib(), _lib.current_stream(), H * W
    mask_dev = mask.to(dev)
    sst, ic, sif, land = ocean_state["sst"], atmos_ic["surface_temperature"], ocean_state["ocean_sea_ice_fraction"], window["land_fraction"]
    out = torch.empty(B, 1 + 1 + T + T + 1, H, W, device=dev)
    keys = ["0", "1", "2", "3", "4"]
    srcs = dict(zip(keys, [sst, ic, land, sif, sif]))
    dsts = dict(zip(keys, [out[:, 0:1], out[:, 1:2], out[:, 2:2 + T], out[:, 2 + T:2 + 2 * T], out[:, 2 + 2 * T:]]))
    values, off = _plane_table(keys, srcs, dsts)
    m = mask_dev.data_ptr()
    table = _upload(values + [m, 0, m, m, m], torch.int64, dev)
    a = table.data_ptr()
    o2a = lambda: L.ace_couple_ocean_to_atmosphere(a + off["gen"], a + off["gen_strides"], a + off["target"], a + off["target_strides"],
                                                   a + off["end"], 0, coupled.OFRAC_FROM_OCEAN_SIF, 1, N_INNER, B, hw, stream)
    names = A2O + ["land_fraction"]
    block = torch.empty(len(names), B, 2, H, W, device=dev)
    planes = [steps[t][k] for k in A2O for t in range(N_INNER)] + [land[:, 1 + t] for t in range(N_INNER)]
    values2, off2 = _plane_table(names, {k: block[i] for i, k in enumerate(names)})
    table2 = _upload(values2 + [p.data_ptr() for p in planes] + [p.stride(0) for p in planes], torch.int64, dev)
    slot = torch.ones(len(names), dtype=torch.int32, device=dev)
    a2, n = table2.data_ptr(), len(planes)
    a2o = lambda: L.ace_couple_atmosphere_to_ocean(a2 + off2["end"], a2 + off2["end"] + 8 * n, a2 + off2["gen"], a2 + off2["gen_strides"],
                                                   slot.data_ptr(), len(names), N_INNER, B, hw, stream)
    assert o2a() == 0 and a2o() == 0, L.ace_couple_last_error()
    kernel_us = {}
    for name, fn in (("ocean_to_atmosphere", o2a), ("atmosphere_to_ocean", a2o)):
        timed(fn, args.warmup)
        kernel_us[name] = [1e3 * timed(fn, args.iters) for _ in range(args.rounds)]
    plane = 4 * B * hw
    bytes_ = {
        # reads: sst, initial temperature, sea ice, land x T, the mask once per masked field (sst, raw sea ice, sea ice, ocean
        # fraction; broadcast over batch and time); writes: sst, initial temperature, raw sea ice, sea ice x T, ocean fraction x T
        "ocean_to_atmosphere": plane * (3 + T) + 4 * hw * 4 + plane * (3 + 2 * T),
        "atmosphere_to_ocean": plane * len(names) * N_INNER + plane * len(names) * 2,
    }
    med = statistics.median
    result = {"grid": [H, W], "batch": B, "n_inner": N_INNER, "device": torch.cuda.get_device_name(0), "iters": args.iters,
              "warmup": args.warmup, "rounds": args.rounds,
              "names": {"atmosphere_to_ocean": A2O, "shared": ["land_fraction"], "ocean_to_atmosphere": ["sst", "ocean_sea_ice_fraction"],
                        "ocean_fraction_prediction": "ocean_sea_ice_fraction -> sea_ice_fraction", "interpolate": True},
              "rows": []}
    for name in calls:
        k_us = med(kernel_us[name])
        bound_us = 1e6 * bytes_[name] / PEAK
        result["rows"].append({
            "exchange": name,
            "call_ms": {path: round(med(v), 4) for path, v in call_ms[name].items()},
            "call_ms_rounds": {path: [round(x, 4) for x in v] for path, v in call_ms[name].items()},
            "native_launches_per_call": {"fused": 1, "torch": 0},
            "kernel_us_back_to_back": round(k_us, 2), "kernel_us_rounds": [round(x, 2) for x in kernel_us[name]],
            "bytes": bytes_[name], "bytes_bound_us": round(bound_us, 2), "fraction_of_8TBs": round(bound_us / k_us, 4)})
    result["tiny_pair"] = tiny_pair(dev)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
