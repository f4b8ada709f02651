#!/usr/bin/env python
"""The evaluator's seasonal, annual, enso_index and ipo_index metrics (ace_amd/evaluator/ ``_Calendar``, csrc/calendar.hip) at 1
degree 180 x 360, 50 paired names (one of them ``sst``, which the two index metrics read), B = 1, T = 40 steps per window, on one
MI355X: InferenceEvaluatorAggregator.record_batch with these four as the only metrics, fused (one ace_diag_calendar_window per
window) and on the torch path, alternated call by call on the same device.  In ms per window, host syncs around each call after one
untimed warm-up window, and for the fused path also --burst windows enqueued back to back under one synchronise (what a rollout
sees: the host does not wait).  The kernel times come from a trace of one further fused window.  The traffic bound is both sides
read once (2 x names x T planes of 259 KB) at the HBM peak of MI355X_MICROARCH (8 TB/s) and at the plain-copy rate of DESIGN.md
(6.29 TB/s); the achieved fraction is the bound over the kernel time.  The torch path is the baseline, not the code under test, and
no time is a target.
Writes one JSON file and prints it.  usage: python tools/bench_calendar.py [--steps 40] [--names 50] [--iters 5] [--burst 8] [--out ...]"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench_regress import COPY_RATE, HBM_PEAK, H, W, fields, timed  # noqa: E402

STEP = datetime.timedelta(days=10)
RECORD_STEPS = 2960                # time levels the aggregators are built for: 29600 days, past the 80 x 365 the tripole index asks for


def build(info, n_steps, fused):
    from ace_amd.evaluator import AnnualMetricConfig, EnsoIndexMetricConfig, InferenceEvaluatorAggregatorConfig, IpoIndexMetricConfig, \
        MetricConfig, PowerSpectrumMetricConfig, SeasonalMetricConfig, ZonalMeanMetricConfig
    off = lambda: MetricConfig(enabled=False)                                  # noqa: E731
    agg = InferenceEvaluatorAggregatorConfig(
        mean_denorm=off(), mean_norm=off(), step_means=[], ensembles=[], power_spectrum=PowerSpectrumMetricConfig(enabled=False),
        zonal_mean=ZonalMeanMetricConfig(enabled=False), time_mean_denorm=off(), time_mean_norm=off(), enso_coefficient=off(),
        seasonal=SeasonalMetricConfig(enabled=True), annual=AnnualMetricConfig(), enso_index=EnsoIndexMetricConfig(),
        ipo_index=IpoIndexMetricConfig()).build(info, 1, n_steps, normalize=lambda d: d)
    assert agg.skipped == [] and len(agg._calendar.on()) == 4
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
        if e.device_type == DeviceType.CUDA and ("calendar_" in e.name or "diag_paired" in e.name):
            key = "calendar_window_kernel" if "calendar_window" in e.name else "calendar_series_kernel" if "calendar_" in e.name \
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calendar_bench.json"))
    args = ap.parse_args(argv)
    import ace_amd
    from ace_amd.timeaxis import TimeAxis

    dev = torch.device("cuda", 0)
    T = args.steps
    names = ["sst"] + [f"v{i:02d}" for i in range(1, args.names)]
    lat, _ = np.polynomial.legendre.leggauss(H)
    info = ace_amd.DatasetInfo((H, W), timestep=STEP, lat=torch.tensor(np.degrees(np.arcsin(lat))), lon=torch.arange(W) * (360.0 / W))
    n_windows = args.iters + 2 + args.burst
    n_steps = max(RECORD_STEPS, n_windows * T)
    axis = TimeAxis.regular((2001, 1, 1), STEP, 1 + n_steps, calendar="noleap")
    window_bytes = 2 * len(names) * T * H * W * 4
    gen, tgt = fields(names, T, dev, 0), fields(names, T, dev, 1)
    aggs = {fused: build(info, n_steps, fused) for fused in (True, False)}
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
    before = aggs[True].calendar_launches()
    try:
        split = kernel_split(lambda: record(True), dev)
    except Exception as err:                                          # a box without a kernel tracer still reports the times
        split = {"error": repr(err)}
        record(True)
    record(False)                                                     # both paths have now seen the same windows
    calls = aggs[True].calendar_launches() - before
    cals = {fused: aggs[fused]._calendar for fused in aggs}
    series_err = max(float(((cals[True]._raw(s, r, n) - cals[False]._raw(s, r, n).double()).abs().max()
                            / cals[False]._raw(s, r, n).abs().max().clamp_min(1e-30))) for s in (0, 1) for r, n in cals[True]._have[s])
    fm, tm = cals[True]._seasonal_means(), cals[False]._seasonal_means()
    season_err = max(float((fm[n][s] - tm[n][s]).abs().max() / tm[n][s].abs().max().clamp_min(1e-30)) for n in fm for s in (0, 1))
    res = {key: {"record_batch_ms": round(float(np.median(times[fused])), 3), "all_ms": [round(v, 3) for v in times[fused]],
                 "route": aggs[fused].route(gen, tgt)} for fused, key in ((True, "fused"), (False, "torch"))}
    res["fused"]["kernels_us"] = split
    res["fused"]["calendar_calls_per_window"] = calls
    res["fused"]["record_batch_ms_in_a_burst"] = round(burst_ms, 3)
    kernel_ms = sum(v for k, v in split.items() if k.startswith("calendar_")) / 1e3 if "error" not in split else None
    result = {
        "workload": f"seasonal + annual + enso_index + ipo_index alone: 1 degree {H}x{W}, B=1, T={T}, {len(names)} paired names (sst among them)",
        "device": torch.cuda.get_device_name(0),
        "window_bytes_both_sides": window_bytes,
        "traffic_bound_ms_at_8TBps_peak": round(window_bytes / HBM_PEAK * 1e3, 4),
        "traffic_bound_ms_at_6.29TBps_copy_rate": round(window_bytes / COPY_RATE * 1e3, 4),
        "fused": res["fused"],
        "torch": res["torch"],
        "torch_over_fused": round(res["torch"]["record_batch_ms"] / res["fused"]["record_batch_ms"], 1),
        "calendar_kernels_ms": None if kernel_ms is None else round(kernel_ms, 4),
        "achieved_fraction_of_hbm_peak": None if not kernel_ms else round(window_bytes / HBM_PEAK * 1e3 / kernel_ms, 3),
        "achieved_fraction_of_copy_rate": None if not kernel_ms else round(window_bytes / COPY_RATE * 1e3 / kernel_ms, 3),
        "regional_series_max_relative_difference_fp64_fused_vs_fp32_torch": series_err,
        "seasonal_means_max_relative_difference_fp64_fused_vs_fp32_torch": season_err,
        "timing": "median of --iters host-synchronised calls per path, the two paths alternated call by call, after one untimed call; "
                  "the burst figure is --burst fused windows under one synchronise; kernel times from the device events of a trace of one "
                  "further fused window; both paths also make the evaluator's paired pass, which is in record_batch_ms and not in "
                  "calendar_kernels_ms",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
