#!/usr/bin/env python
"""The inference aggregator's cost against the rollout it reduces, at BASELINE.json configs[1] (bench.py's ACE2-shape SFNO, 1 degree
180 x 360, B = 1, T = 40 steps per window, the shipped output names: 36 prognostic + 14 diagnostic), on one MI355X.  In ms per
window, timed with host syncs around each call after an untimed warm-up:
  - one window of EnginePredict (the static-buffer engine, graph "step", outputs copied out as run_inference receives them);
  - InferenceAggregator.record_batch on that window, fused (csrc/diag.hip) and on the torch path (fused = False);
and the fused overhead as a fraction of the window's rollout time (target: at most 2 %).
Writes one JSON file and prints it.  usage: python tools/bench_aggregator.py [--steps 40] [--iters 5] [--out profiles/aggregator_bench.json]

--paired times the evaluator aggregator instead (ace_amd/evaluator/): InferenceEvaluatorAggregator.record_batch on the same window
against a perturbed copy of it as target, fused (one ace_diag_paired_window per window) and on the torch path, alternated call by
call on the same device, beside the rollout-window time; the JSON (default profiles/evaluator_aggregator_bench.json) states the
aggregator's share of a window for both paths.  No speed-up is a target."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402


def timed(fn, dev, iters):
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


@torch.no_grad()
def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--paired", action="store_true", help="time the evaluator aggregator (paired windows)")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "evaluator_aggregator_bench.json" if args.paired else "aggregator_bench.json")
    import ace_amd
    from ace_amd.aggregator import InferenceAggregatorConfig
    from ace_amd.inference import EnginePredict

    dev = torch.device("cuda", 0)
    T, B = args.steps, 1
    stepper, forcing_names, prog, diag = bench.build_stepper(dev, seed=0)
    g = torch.Generator().manual_seed(0)
    H, W = bench.IMG
    ic = {n: torch.randn(B, 1, H, W, generator=g).to(dev) for n in prog}
    forcing = {n: torch.randn(B, T + 1, H, W, generator=g).to(dev) for n in forcing_names}
    predict = EnginePredict(stepper, batch=B, graph="step")
    with torch.no_grad():
        out, _ = predict(ic, forcing)                                 # builds the engine and captures its step
    window_ms, window_all = timed(lambda: predict(ic, forcing), dev, args.iters)

    lat, _ = np.polynomial.legendre.leggauss(H)
    info = ace_amd.DatasetInfo(bench.IMG, lat=torch.tensor(np.degrees(np.arcsin(lat))), lon=torch.arange(W) * (360.0 / W))
    if args.paired:
        return paired(args, dev, stepper, info, out, window_ms, window_all)
    res = {}
    for fused in (True, False):
        agg = InferenceAggregatorConfig().build(info, (args.iters + 1) * T)
        agg.fused = fused
        agg.record_batch(out)                                         # untimed: tables, SHT plan, accumulators
        ms, all_ms = timed(lambda: agg.record_batch(out), dev, args.iters)
        res["fused" if fused else "torch"] = {"record_batch_ms": round(ms, 3), "all_ms": [round(v, 3) for v in all_ms],
                                              "route": agg.route(out)}
        if fused:
            agg2 = InferenceAggregatorConfig().build(info, T)
            agg2.record_batch(out)
            res["fused"]["native_launches_per_window"] = agg2.launches()
            res["fused"]["spectrum_names"] = len(out) - len(agg2.omitted)
    bytes_read = sum(v.numel() * 4 for v in out.values())
    result = {
        "workload": f"inference aggregator at BASELINE configs[1]: 1 degree {H}x{W}, B={B}, T={T}, {len(out)} output names",
        "device": torch.cuda.get_device_name(0),
        "window_bytes": bytes_read,
        "engine_predict_window_ms": round(window_ms, 3),
        "engine_predict_all_ms": [round(v, 3) for v in window_all],
        "fused": res["fused"],
        "torch": res["torch"],
        "fused_overhead_fraction": round(res["fused"]["record_batch_ms"] / window_ms, 5),
        "torch_overhead_fraction": round(res["torch"]["record_batch_ms"] / window_ms, 5),
        "target_fused_overhead_fraction": 0.02,
        "timing": "median of --iters host-synchronised calls after one untimed call",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


def paired(args, dev, stepper, info, out, window_ms, window_all):
    from ace_amd.evaluator import InferenceEvaluatorAggregatorConfig
    T, B = args.steps, 1
    H, W = bench.IMG
    g = torch.Generator().manual_seed(1)
    target = {n: x + 0.01 * torch.randn(x.shape, generator=g).to(dev) for n, x in out.items()}
    aggs = {}
    for fused in (True, False):
        agg = InferenceEvaluatorAggregatorConfig().build(info, 0, (args.iters + 1) * T, normalize=stepper.normalizer)
        agg.fused = fused
        agg.record_batch(out, target)                                 # untimed: tables, SHT plan, accumulators
        aggs[fused] = agg
    times = {True: [], False: []}
    for _ in range(args.iters):                                       # alternated: both paths see the same machine state
        for fused in (True, False):
            _, ts = timed(lambda: aggs[fused].record_batch(out, target), dev, 1)
            times[fused] += ts
    res = {}
    for fused, key in ((True, "fused"), (False, "torch")):
        ms = float(np.median(times[fused]))
        res[key] = {"record_batch_ms": round(ms, 3), "all_ms": [round(v, 3) for v in times[fused]],
                    "route": aggs[fused].route(out, target), "share_of_window": round(ms / window_ms, 5)}
    one = InferenceEvaluatorAggregatorConfig().build(info, 0, T, normalize=stepper.normalizer)
    one.record_batch(out, target)
    res["fused"]["native_launches_per_window"] = one.launches()
    res["fused"]["spectrum_names_per_side"] = len(out) - len(one.omitted)
    result = {
        "workload": f"inference evaluator aggregator at BASELINE configs[1]: 1 degree {H}x{W}, B={B}, T={T}, {len(out)} output names, "
                    "every name paired with a target",
        "device": torch.cuda.get_device_name(0),
        "window_bytes_read": 2 * sum(v.numel() * 4 for v in out.values()),
        "engine_predict_window_ms": round(window_ms, 3),
        "engine_predict_all_ms": [round(v, 3) for v in window_all],
        "fused": res["fused"],
        "torch": res["torch"],
        "skipped_metrics": one.skipped,
        "timing": "median of --iters host-synchronised calls per path, the two paths alternated call by call, after one untimed call",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
