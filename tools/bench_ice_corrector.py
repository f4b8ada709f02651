#!/usr/bin/env python
"""The sea-ice budget corrector at 1 degree (180 x 360), B = 1, on one MI355X, in two configurations: the shipped one (siconc with
LSRCc / LSNKc / XPRTc, fme/ace/test_ice_train.py) and all three variables (simass, siconc, sisnmass).  Three measurements, each after
a warm-up, each a host clock around work that ends in a device synchronise:
  call     ``IceCorrector.__call__`` fused (ace_ice_budget_apply: two launches per variable, flags on the device) against
           ``fused = False`` (the reference's ~60 torch ops per variable in fp64, with a host readback per ``torch.any``), in the same
           process on the same device, alternating; both on a fresh copy of the same seeded step output, and compared bit for bit
  launches ``FusedIceCorrector.apply`` alone on resolved planes, many calls per synchronise, with the bytes its passes move (flags:
           4 planes read; apply: 4 read, 4 written; the mask byte) over that time.  No share of the 8 TB/s peak is claimed where a
           launch takes less than 10 microseconds: that is launch latency, not bandwidth
  engine   an ``OceanRolloutEngine`` step (graph="window", T = 4, the Samudra of tools/bench_ocean_step.py) with the three-variable
           corrector and with none
Writes profiles/ice_corrector_bench.json and prints it as one JSON line.
usage: python tools/bench_ice_corrector.py [--iters 30] [--warmup 5] [--no-engine]"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

H, W, B = 180, 360, 1
HBM = 8e12
TIMESTEP = datetime.timedelta(hours=6)
TERMS = {"simass": ["SIMSRC", "SIMSNK", "SIMXPRT"], "siconc": ["LSRCc", "LSNKc", "XPRTc"], "sisnmass": ["SNSRC", "SNSNK", "SNXPRT"]}
SCALE = {"simass": 40.0, "siconc": 1.0, "sisnmass": 7.0}
CONFIGS = {"shipped_siconc": ["siconc"], "three_variables": ["simass", "siconc", "sisnmass"]}


def corrector_state(names):
    return {"type": "ice_corrector", "config": {"budget_correction": {"corrected_variables": {n: TERMS[n] for n in names}}}}


def step_data(names, dev, seed=1):
    """a step's input and output whose every stage has work: old masses in [0, 1] x scale with open water, increments of +- 0.3"""
    g = torch.Generator().manual_seed(seed)
    dt = TIMESTEP.total_seconds()
    inp, gen = {}, {}
    for n in names:
        c = SCALE[n]
        old = torch.rand(B, H, W, generator=g) * c
        old[:, :, :40] = 0.0
        inp[n] = old.to(dev)
        for term, (mean, std) in zip(TERMS[n], ((0.1, 0.1), (-0.1, 0.1), (0.0, 0.15))):
            gen[term] = ((torch.randn(B, H, W, generator=g) * std + mean) * c / dt).to(dev)
        gen[n] = torch.zeros(B, H, W, device=dev)
    return inp, gen


def wall(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def bench_call(names, dev, iters, warmup):
    from ace_amd.ice_corrector import IceCorrectorConfig

    class Info:
        timestep = TIMESTEP
    corrector = IceCorrectorConfig.from_state(corrector_state(names)).get_corrector(Info())
    inp, pristine = step_data(names, dev)
    gen = {k: v.clone() for k, v in pristine.items()}

    def restore():
        for k, v in pristine.items():
            gen[k].copy_(v)

    def call(fused):
        corrector.fused = fused
        restore()
        return corrector(inp, gen, {}, None)[0]
    fused_out = {k: v.clone() for k, v in call(True).items()}
    torch_out = {k: v.clone() for k, v in call(False).items()}
    torch.cuda.synchronize()
    same = all(torch.equal(fused_out[k].view(torch.int32), torch_out[k].view(torch.int32)) for k in fused_out)
    t_restore = wall(restore, iters, warmup)
    t_fused, t_torch = [], []
    for _ in range(3):                  # alternate the two
        t_fused.append(wall(lambda: call(True), iters, warmup))
        t_torch.append(wall(lambda: call(False), iters, warmup))
    med = lambda rows: statistics.median(r[0] for r in rows)
    out = {"fused_call_seconds": med(t_fused) - t_restore[0], "torch_call_seconds": med(t_torch) - t_restore[0],
           "restore_seconds_subtracted": t_restore[0], "fused_call_min_max": [min(r[1] for r in t_fused), max(r[2] for r in t_fused)],
           "torch_call_min_max": [min(r[1] for r in t_torch), max(r[2] for r in t_torch)], "bitwise_equal": same,
           "launches_per_fused_call": 2 * len(names), "flag_clearings_per_fused_call": 1,
           "host_readbacks_per_torch_call": len(corrector.plan) + sum(a + m for _, _, a, m in corrector.plan)}
    out["speedup"] = out["torch_call_seconds"] / out["fused_call_seconds"]
    # the launches alone, on resolved planes
    h = corrector.handle(B, (H, W), dev)
    fields = h.fields(inp, gen, {})
    stream = torch.cuda.current_stream().cuda_stream
    reps = 50

    def launches():
        for _ in range(reps):
            h.apply(fields, stream)
    restore()
    t = wall(launches, iters, warmup)
    per_call = t[0] / reps
    nbytes = len(names) * (4 + 8) * 4 * H * W * B + (len(names) > 1) * len(names) * H * W * B
    per_launch = per_call / (2 * len(names) + 1)
    latency_bound = per_launch < 10e-6
    out.update({"apply_seconds": per_call, "apply_min_max": [t[1] / reps, t[2] / reps], "apply_bytes": nbytes,
                "apply_bytes_per_second": nbytes / per_call, "seconds_per_launch": per_launch, "latency_bound": latency_bound,
                "share_of_8TBps_peak": None if latency_bound else nbytes / per_call / HBM})
    return out


def engine_state(names):
    from ace_amd.samudra import Samudra
    out = [n for v in names for n in (v, *TERMS[v])] if names else [n for v in CONFIGS["three_variables"] for n in (v, *TERMS[v])]
    inn = ["DSWRFsfc"] + out
    torch.manual_seed(0)
    cfg = {"ch_width": [200, 250, 300, 400], "dilation": [1, 2, 4, 8], "n_layers": [1, 1, 1, 1], "norm": "instance"}
    net = Samudra(len(inn), len(out), **cfg)
    g = torch.Generator().manual_seed(1)
    mask = (torch.rand(H, W, generator=g) > 0.3).float()
    dt = TIMESTEP.total_seconds()
    means, stds = {"DSWRFsfc": 180.0}, {"DSWRFsfc": 90.0}
    for v in CONFIGS["three_variables"]:
        c = SCALE[v]
        means[v], stds[v] = 0.45 * c, 0.3 * c
        for term, (m, s) in zip(TERMS[v], ((0.1, 0.1), (-0.1, 0.1), (0.0, 0.15))):
            means[term], stds[term] = m * c / dt, s * c / dt
    return {"stepper": {
        "config": {"input_masking": {"mask_value": 0, "fill_value": 0.0},
                   "step": {"type": "single_module", "config": {
                       "builder": {"type": "Samudra", "config": cfg}, "in_names": inn, "out_names": out,
                       "normalization": {"network": {"means": means, "stds": stds}}, "ocean": None,
                       "corrector": corrector_state(names) if names else None}}},
        "dataset_info": {"img_shape": [H, W], "timestep": TIMESTEP // datetime.timedelta(microseconds=1),
                         "mask_provider": {"masks": {"mask_2d": mask}}},
        "step": {"module": {**{f"module.{k}": v for k, v in net.state_dict().items()}, "label_encoding": None}}}}, inn, out


def bench_engine(dev, iters, warmup, T=4):
    from ace_amd.checkpoint import load_stepper
    from ace_amd.ocean_rollout import OceanRolloutEngine
    res = {}
    for label, names in (("with_corrector", CONFIGS["three_variables"]), ("without_corrector", [])):
        state, inn, out = engine_state(names)
        stepper = load_stepper(state, device=dev).stepper
        g = torch.Generator().manual_seed(2)
        ic = {n: (torch.rand(B, 1, H, W, generator=g) * SCALE.get(n, 1e-6)).to(dev) for n in out}
        forcing = {"DSWRFsfc": (torch.randn(B, T + 1, H, W, generator=g) * 90.0 + 180.0).to(dev)}
        eng = OceanRolloutEngine(stepper, batch=B, n_forward_steps=T, graph="window")
        eng.predict(ic, forcing)
        t = wall(eng.run_window, iters, warmup)
        res[label] = {"step_seconds": t[0] / T, "min_max": [t[1] / T, t[2] / T], "steps_per_window": T}
        del eng, stepper
    res["corrector_seconds_per_step"] = res["with_corrector"]["step_seconds"] - res["without_corrector"]["step_seconds"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-engine", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ice_corrector needs an MI355X: nothing is measured without one")
    dev = torch.device("cuda", 0)
    from ace_amd import build
    result = {"device": torch.cuda.get_device_name(0), "shape": [B, H, W], "timestep_seconds": TIMESTEP.total_seconds(),
              "kernel_source_sha256": build.source_sha256()[:12], "iters": args.iters, "warmup": args.warmup,
              "clock": "host perf_counter around work ending in a device synchronise; medians", "configurations": {}}
    for label, names in CONFIGS.items():
        result["configurations"][label] = bench_call(names, dev, args.iters, args.warmup)
    if not args.no_engine:
        result["engine_step"] = bench_engine(dev, max(5, args.iters // 3), args.warmup)
    path = os.path.join(ROOT, "profiles", "ice_corrector_bench.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
