#!/usr/bin/env python
"""The evaluator's trend, enso_coefficient and near_zero_fraction metrics (ace_amd/evaluator/, csrc/regress.hip) at 1 degree
180 x 360, 50 paired names, B = 1, T = 40 steps per window, on one MI355X: InferenceEvaluatorAggregator.record_batch with these three
as the only metrics (trend and the ENSO coefficient on every name, the near-zero fraction with maps on every name), fused (one
ace_diag_regress_window per window) and on the torch path, alternated call by call on the same device.  In ms per window, host
syncs around each call after one untimed warm-up window, and for the fused path also --burst windows enqueued back to back under
one synchronise (what a rollout sees: the host does not wait).  The kernel times come from a trace of one further fused window.
The traffic bound is both sides read once (2 x names x T planes of 259 KB) at the HBM peak of MI355X_MICROARCH (8 TB/s) and at the
plain-copy rate of DESIGN.md (6.29 TB/s); the achieved fraction is the bound over the kernel time.  No time is a target.
Writes one JSON file and prints it.  usage: python tools/bench_regress.py [--steps 40] [--names 50] [--iters 5] [--burst 8] [--out ...]"""
import argparse
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12              # bytes / s
COPY_RATE = 6.29e12            # bytes / s, DESIGN.md
H, W = 180, 360
STEP = datetime.timedelta(days=10)


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def fields(names, T, dev, seed):
    """even names Gaussian, odd names zero-inflated (precipitation-like)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    out = {}
    for i, n in enumerate(names):
        x = torch.randn(1, T, H, W, generator=g, device=dev)
        if i % 2:
            wet = torch.rand(1, T, H, W, generator=g, device=dev) < 0.08
            x = torch.where(wet, 3e-4 * x.abs() ** 3, torch.zeros((), device=dev))
        out[n] = x
    return out


def build(info, names, n_steps, index, fused):
    from ace_amd.evaluator import EnsoCoefficientMetricConfig, InferenceEvaluatorAggregatorConfig, MetricConfig, \
        NearZeroFractionMetricConfig, PowerSpectrumMetricConfig, TrendMetricConfig, ZonalMeanMetricConfig
    off = lambda: MetricConfig(enabled=False)                                  # noqa: E731
    agg = InferenceEvaluatorAggregatorConfig(
        mean_denorm=off(), mean_norm=off(), step_means=[], ensembles=[], power_spectrum=PowerSpectrumMetricConfig(enabled=False),
        zonal_mean=ZonalMeanMetricConfig(enabled=False), time_mean_denorm=off(), time_mean_norm=off(), annual=off(), enso_index=off(),
        ipo_index=off(), trend=TrendMetricConfig(enabled=True), enso_coefficient=EnsoCoefficientMetricConfig(index=index),
        near_zero_fraction=NearZeroFractionMetricConfig(enabled=True, variables=list(names), include_maps=True)).build(
            info, 1, n_steps, normalize=lambda d: d)
    assert "enso_coefficient" not in agg.skipped
    agg.fused = fused
    return agg


def kernel_split(record, dev):
    """GPU time per kernel of one fused window, in microseconds, from the device-side events of a trace"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        record()
        torch.cuda.synchronize(dev)
    out = {}
    for e in prof.events():
        if e.device_type == DeviceType.CUDA and ("regress_" in e.name or "diag_paired" in e.name):
            key = "regress_window_kernel" if "regress_window" in e.name else "regress_frac_kernel" if "regress_" in e.name \
                else "diag_paired_kernels (the evaluator's paired pass, made for every window whatever is on)"
            out[key] = round(out.get(key, 0.0) + float(e.time_range.elapsed_us()), 1)
    return out


@torch.no_grad()
def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--names", type=int, default=50)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--burst", type=int, default=8, help="fused windows enqueued back to back under one synchronise")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regress_bench.json"))
    args = ap.parse_args(argv)
    import ace_amd
    from ace_amd.timeaxis import TimeAxis

    dev = torch.device("cuda", 0)
    T = args.steps
    names = [f"v{i:02d}" for i in range(args.names)]
    lat, _ = np.polynomial.legendre.leggauss(H)
    info = ace_amd.DatasetInfo((H, W), timestep=STEP, lat=torch.tensor(np.degrees(np.arcsin(lat))), lon=torch.arange(W) * (360.0 / W))
    n_windows = args.iters + 2 + args.burst
    n_time = 1 + n_windows * T
    axis = TimeAxis.regular((2001, 1, 1), STEP, n_time)
    index = torch.randn(1, n_time, generator=torch.Generator().manual_seed(2))
    window_bytes = 2 * len(names) * T * H * W * 4
    gen, tgt = fields(names, T, dev, 0), fields(names, T, dev, 1)
    aggs = {fused: build(info, names, n_windows * T, index, fused) for fused in (True, False)}
    seen = {True: 0, False: 0}

    def record(fused):
        i = seen[fused]
        aggs[fused].record_batch(gen, tgt, time=axis[:, 1 + i * T:1 + (i + 1) * T])
        seen[fused] += 1
    for fused, agg in aggs.items():
        ic = {n: x[:, :1] for n, x in tgt.items()}
        agg.record_initial_condition(ic, ic)
        record(fused)                                                 # untimed: state, tables, code objects
    times = {True: [], False: []}
    for _ in range(args.iters):                                       # alternated: both paths see the same machine state
        for fused in (True, False):
            times[fused].append(timed(lambda: record(fused), dev))
    burst_ms = timed(lambda: [record(True) for _ in range(args.burst)], dev) / args.burst
    for _ in range(args.burst):
        record(False)
    before = aggs[True].launches()
    try:
        split = kernel_split(lambda: record(True), dev)
    except Exception as err:                                          # a box without a kernel tracer still reports the times
        split = {"error": repr(err)}
        record(True)
    record(False)                                                     # both paths have now seen the same windows
    calls = aggs[True].launches() - before
    fds, tds = aggs[True].get_dataset(), aggs[False].get_dataset()
    nz_equal = all(torch.equal(fds["near_zero_fraction"][k], v) for k, v in tds["near_zero_fraction"].items())
    trend_err = max(float((fds["trend"][n] - tds["trend"][n]).abs().max() / tds["trend"][n].abs().max()) for n in names)
    enso_err = max(float((fds["enso_coefficient"][n].double() - tds["enso_coefficient"][n].double()).abs().max()
                         / tds["enso_coefficient"][n].abs().max()) for n in names)
    res = {key: {"record_batch_ms": round(float(np.median(times[fused])), 3), "all_ms": [round(v, 3) for v in times[fused]],
                 "route": aggs[fused].route(gen, tgt)} for fused, key in ((True, "fused"), (False, "torch"))}
    res["fused"]["kernels_us"] = split
    res["fused"]["native_calls_per_window"] = calls
    res["fused"]["record_batch_ms_in_a_burst"] = round(burst_ms, 3)
    kernel_ms = sum(v for k, v in split.items() if k.startswith("regress_")) / 1e3 if "error" not in split else None
    result = {
        "workload": f"trend + enso_coefficient + near_zero_fraction (maps) alone: 1 degree {H}x{W}, B=1, T={T}, {len(names)} paired names",
        "device": torch.cuda.get_device_name(0),
        "window_bytes_both_sides": window_bytes,
        "traffic_bound_ms_at_8TBps_peak": round(window_bytes / HBM_PEAK * 1e3, 4),
        "traffic_bound_ms_at_6.29TBps_copy_rate": round(window_bytes / COPY_RATE * 1e3, 4),
        "fused": res["fused"],
        "torch": res["torch"],
        "torch_over_fused": round(res["torch"]["record_batch_ms"] / res["fused"]["record_batch_ms"], 1),
        "regress_kernels_ms": None if kernel_ms is None else round(kernel_ms, 4),
        "achieved_fraction_of_hbm_peak": None if not kernel_ms else round(window_bytes / HBM_PEAK * 1e3 / kernel_ms, 3),
        "achieved_fraction_of_copy_rate": None if not kernel_ms else round(window_bytes / COPY_RATE * 1e3 / kernel_ms, 3),
        "near_zero_maps_agree_bitwise": nz_equal,
        "trend_max_relative_difference": trend_err,
        "enso_max_relative_difference_fp64_fused_vs_fp32_torch": enso_err,
        "timing": "median of --iters host-synchronised calls per path, the two paths alternated call by call, after one untimed call; "
                  "the burst figure is --burst fused windows under one synchronise; kernel times from the device events of a trace of one "
                  "further fused window",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
