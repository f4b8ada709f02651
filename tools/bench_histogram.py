#!/usr/bin/env python
"""The evaluator's histogram metric (ace_amd/evaluator/, csrc/hist.hip) at 1 degree 180 x 360, 40 paired names, B = 1, T = 40 steps
per window, on one MI355X: InferenceEvaluatorAggregator.record_batch with the histogram as the only metric, fused (one
ace_diag_hist_window per window) and on the torch path, alternated call by call on the same device, once on Gaussian fields and
once on zero-inflated ones (a cubed half-Gaussian on 8 % of the pixels, exact zeros elsewhere: precipitation).  In ms per window,
host syncs around each call after an untimed warm-up window; every timed window repeats the warm-up's values, so no range doubles
inside the timing.  The per-kernel split comes from a kernel trace of one fused window.  The floor is both sides streamed twice
(range pass and binning pass) at the plain-copy rate of DESIGN.md, 6.29 TB/s.  No time is a target.
Writes one JSON file and prints it.  usage: python tools/bench_histogram.py [--steps 40] [--names 40] [--iters 5] [--out ...]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

COPY_RATE = 6.29e12            # bytes / s, DESIGN.md
H, W = 180, 360


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def fields(kind, names, T, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = {}
    for i, n in enumerate(names):
        x = torch.randn(1, T, H, W, generator=g, device=dev)
        if kind == "zero_inflated":
            wet = torch.rand(1, T, H, W, generator=g, device=dev) < 0.08
            x = torch.where(wet, 3e-4 * x.abs() ** 3, torch.zeros((), device=dev))
        else:
            x = (1.0 + i) * x + 10.0 * i
        out[n] = x
    return out


def build(info, n_steps, fused):
    from ace_amd.evaluator import HistogramMetricConfig, InferenceEvaluatorAggregatorConfig, MetricConfig, PowerSpectrumMetricConfig, \
        ZonalMeanMetricConfig
    off = lambda: MetricConfig(enabled=False)                                  # noqa: E731
    agg = InferenceEvaluatorAggregatorConfig(
        mean_denorm=off(), mean_norm=off(), step_means=[], ensembles=[], power_spectrum=PowerSpectrumMetricConfig(enabled=False),
        zonal_mean=ZonalMeanMetricConfig(enabled=False), time_mean_denorm=off(), time_mean_norm=off(), annual=off(), enso_index=off(),
        enso_coefficient=off(), ipo_index=off(), histogram=HistogramMetricConfig(enabled=True)).build(
            info, 0, n_steps, normalize=lambda d: d)
    agg.fused = fused
    return agg


def kernel_split(record, dev):
    """GPU time per kernel of one fused window, in microseconds"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        record()
        torch.cuda.synchronize(dev)
    out = {}
    for e in prof.key_averages():
        if "hist_" in e.key:
            out[e.key.split("(")[0].split("::")[-1]] = round(float(getattr(e, "device_time_total", None) or e.cuda_time_total), 1)
    return out


@torch.no_grad()
def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--names", type=int, default=40)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "histogram_bench.json"))
    args = ap.parse_args(argv)
    import ace_amd

    dev = torch.device("cuda", 0)
    T = args.steps
    names = [f"v{i:02d}" for i in range(args.names)]
    lat, _ = np.polynomial.legendre.leggauss(H)
    info = ace_amd.DatasetInfo((H, W), lat=torch.tensor(np.degrees(np.arcsin(lat))), lon=torch.arange(W) * (360.0 / W))
    window_bytes = 2 * len(names) * T * H * W * 4
    floor_ms = 2 * window_bytes / COPY_RATE * 1e3
    cases = {}
    for kind in ("gaussian", "zero_inflated"):
        gen, tgt = fields(kind, names, T, dev, 0), fields(kind, names, T, dev, 1)
        aggs = {fused: build(info, (args.iters + 2) * T, fused) for fused in (True, False)}
        for agg in aggs.values():
            agg.record_batch(gen, tgt)                                # untimed: state, tables, the first window's range
        times = {True: [], False: []}
        for _ in range(args.iters):                                   # alternated: both paths see the same machine state
            for fused in (True, False):
                times[fused].append(timed(lambda: aggs[fused].record_batch(gen, tgt), dev))
        fds, tds = aggs[True].get_dataset()["histogram"], aggs[False].get_dataset()["histogram"]
        try:
            split = kernel_split(lambda: aggs[True].record_batch(gen, tgt), dev)
        except Exception as err:                                      # a box without a kernel tracer still reports the times
            split = {"error": repr(err)}
        res = {key: {"record_batch_ms": round(float(np.median(times[fused])), 3), "all_ms": [round(v, 3) for v in times[fused]],
                     "route": aggs[fused].route(gen, tgt)} for fused, key in ((True, "fused"), (False, "torch"))}
        res["fused"]["kernels_us"] = split
        res["fused"]["ratio_to_floor"] = round(res["fused"]["record_batch_ms"] / floor_ms, 2)
        res["paths_agree_bitwise"] = all(torch.equal(fds[k], tds[k]) for k in tds)
        res["exact_zero_fraction"] = round(float(sum((x == 0).float().mean() for x in gen.values()) / len(gen)), 4)
        cases[kind] = res
        del gen, tgt, aggs
        torch.cuda.empty_cache()
    result = {
        "workload": f"histogram metric alone: 1 degree {H}x{W}, B=1, T={T}, {len(names)} paired names, 200 bins",
        "device": torch.cuda.get_device_name(0),
        "window_bytes_both_sides": window_bytes,
        "floor_ms_both_sides_streamed_twice_at_6.29TBps": round(floor_ms, 3),
        "gaussian": cases["gaussian"],
        "zero_inflated": cases["zero_inflated"],
        "fused_zero_inflated_over_gaussian": round(cases["zero_inflated"]["fused"]["record_batch_ms"]
                                                   / cases["gaussian"]["fused"]["record_batch_ms"], 3),
        "timing": "median of --iters host-synchronised calls per path, the two paths alternated call by call, after one untimed call",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
