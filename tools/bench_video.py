#!/usr/bin/env python
"""The evaluator's video metric (ace_amd/evaluator/video.py, csrc/video.hip) at 1 degree 180 x 360 on one MI355X: windows of 50
paired names of which ``VideoMetricConfig.variables`` keeps 8, B = 2, T = 40 steps per window, n_forward_steps = 400, extended
videos on (8 x 401 x 64800 x 48 bytes = 10 GB of accumulators per aggregator).  InferenceEvaluatorAggregator.record_batch with the
video as the only metric, fused (one ace_diag_video_window per window) and on the torch path of the same module, alternated call
by call on the same device, in ms per window with host syncs around each call, after one untimed warm-up window (which also
allocates the accumulators).  The first pass visits fresh slots (the kernel assigns), the second pass the same slots again (it
accumulates); the two are reported apart.  record_batch also makes the evaluator's paired pass over all 50 names on either path,
so the kernel time is taken apart from it, from a trace of one further window of each kind.  Traffic counted: the kept planes of
both sides read once plus the accumulator bytes written, and for the accumulating pass also the accumulator bytes read; the
achieved fraction is that over the kernel time against the HBM peak of 8 TB/s.  No time is a target.
Writes one JSON file and prints it.  usage: python tools/bench_video.py [--steps 40] [--windows 10] [--names 50] [--keep 8] [--out ...]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12              # bytes / s
H, W, B = 180, 360, 2


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def build(info, keep, n_steps, fused, video=True):
    from ace_amd.evaluator import InferenceEvaluatorAggregatorConfig, MetricConfig, PowerSpectrumMetricConfig, VideoMetricConfig, \
        ZonalMeanMetricConfig
    off = lambda: MetricConfig(enabled=False)                                  # noqa: E731
    agg = InferenceEvaluatorAggregatorConfig(
        mean_denorm=off(), mean_norm=off(), step_means=[], ensembles=[], power_spectrum=PowerSpectrumMetricConfig(enabled=False),
        zonal_mean=ZonalMeanMetricConfig(enabled=False), time_mean_denorm=off(), time_mean_norm=off(), annual=off(), enso_index=off(),
        enso_coefficient=off(), ipo_index=off(),
        video=VideoMetricConfig(enabled=video, enable_extended_videos=True, variables=list(keep))).build(
            info, 1, n_steps, normalize=lambda d: d)
    agg.fused = fused
    return agg


def kernel_us(record, dev):
    """GPU time of the video kernel of one fused window, in microseconds, from the device-side events of a trace"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        record()
        torch.cuda.synchronize(dev)
    return round(sum(float(e.time_range.elapsed_us()) for e in prof.events()
                     if e.device_type == DeviceType.CUDA and "video_window" in e.name), 1)


@torch.no_grad()
def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--names", type=int, default=50)
    ap.add_argument("--keep", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_bench.json"))
    args = ap.parse_args(argv)
    import ace_amd

    dev = torch.device("cuda", 0)
    T, nwin = args.steps, args.windows
    names = [f"v{i:02d}" for i in range(args.names)]
    keep = names[::max(1, args.names // args.keep)][:args.keep]
    lat, _ = np.polynomial.legendre.leggauss(H)
    info = ace_amd.DatasetInfo((H, W), lat=torch.tensor(np.degrees(np.arcsin(lat))), lon=torch.arange(W) * (360.0 / W))
    g = torch.Generator(device=dev).manual_seed(0)
    gen = {n: 280.0 + 15.0 * torch.randn(B, T, H, W, generator=g, device=dev) for n in names}
    tgt = {n: x + 2.0 * torch.randn(B, T, H, W, generator=g, device=dev) for n, x in gen.items()}
    aggs = {fused: build(info, keep, nwin * T, fused) for fused in (True, False)}
    bare = {fused: build(info, keep, nwin * T, fused, video=False) for fused in (True, False)}      # what record_batch costs without it

    def record_bare(fused, window):
        bare[fused]._n_seen = 1 + window * T
        bare[fused].record_batch(gen, tgt)

    def record(fused, window):
        aggs[fused]._n_seen = 1 + window * T                              # the second pass visits the same slots again
        aggs[fused].record_batch(gen, tgt)
    for fused in aggs:
        record(fused, 0)                                                  # untimed: the accumulators, tables, code objects
        record_bare(fused, 0)
    times = {(fused, kind): [] for fused in aggs for kind in ("assign", "accumulate", "bare")}
    for w in range(1, nwin - 1):                                          # fresh slots; alternated: all see the same machine state
        for fused in (True, False):
            times[fused, "assign"].append(timed(lambda: record(fused, w), dev))
            times[fused, "bare"].append(timed(lambda: record_bare(fused, w), dev))
    before = aggs[True].launches()
    split = {}
    try:
        split["assign"] = kernel_us(lambda: record(True, nwin - 1), dev)
    except Exception as err:                                              # a box without a kernel tracer still reports the times
        split["error"] = repr(err)
        record(True, nwin - 1)
    calls = aggs[True].launches() - before
    record(False, nwin - 1)
    for w in range(0, nwin - 1):                                          # the same slots again
        for fused in (True, False):
            times[fused, "accumulate"].append(timed(lambda: record(fused, w), dev))
    if "error" not in split:
        split["accumulate"] = kernel_us(lambda: record(True, nwin - 1), dev)
    else:
        record(True, nwin - 1)
    record(False, nwin - 1)                                               # both paths have now seen the same windows
    fds, tds = aggs[True].get_dataset()["video"], aggs[False].get_dataset()["video"]
    worst = {k: float((fds[k][..., 1:, :, :] - tds[k][..., 1:, :, :]).abs().max()) for k in (keep[0], f"bias_{keep[0]}", f"rmse_{keep[0]}")}
    extrema_equal = all(torch.equal(fds[f"{k}_{n}"], tds[f"{k}_{n}"]) for k in ("min_err", "max_err") for n in keep)
    hw, k = H * W, len(keep)
    read_window = k * 2 * B * T * hw * 4
    acc = k * T * hw * 48
    traffic = {"assign": read_window + acc, "accumulate": read_window + 2 * acc}
    res = {}
    for kind in ("assign", "accumulate"):
        f, t = float(np.median(times[True, kind])), float(np.median(times[False, kind]))
        fv, tv = f - float(np.median(times[True, "bare"])), t - float(np.median(times[False, "bare"]))
        us = split.get(kind)
        res[kind] = {"fused_record_batch_ms": round(f, 3), "torch_record_batch_ms": round(t, 3),
                     "fused_video_share_ms": round(fv, 3), "torch_video_share_ms": round(tv, 3), "torch_over_fused_video_share": round(tv / fv, 1),
                     "fused_all_ms": [round(v, 3) for v in times[True, kind]], "torch_all_ms": [round(v, 3) for v in times[False, kind]],
                     "video_kernel_us": us, "traffic_bytes": traffic[kind],
                     "traffic_bound_ms_at_8TBps_peak": round(traffic[kind] / HBM_PEAK * 1e3, 4),
                     "achieved_fraction_of_hbm_peak": None if not us else round(traffic[kind] / HBM_PEAK * 1e6 / us, 3)}
    result = {
        "workload": f"video (extended) alone: 1 degree {H}x{W}, B={B}, T={T}, {k} of {len(names)} paired names kept, "
                    f"n_forward_steps={nwin * T}",
        "device": torch.cuda.get_device_name(0),
        "accumulator_bytes": k * (1 + nwin * T) * hw * 48,
        "route": {"fused": aggs[True].route(gen, tgt), "torch": aggs[False].route(gen, tgt)},
        "native_calls_per_window": calls,
        "record_batch_ms_without_the_video": {"fused": round(float(np.median(times[True, "bare"])), 3),
                                              "torch": round(float(np.median(times[False, "bare"])), 3)},
        "first_pass_assign": res["assign"],
        "second_pass_accumulate": res["accumulate"],
        "trace": split,
        "max_abs_difference_fused_vs_torch": worst,
        "extrema_agree_exactly": extrema_equal,
        "timing": "median of host-synchronised record_batch calls per path, the two paths alternated call by call, after one untimed "
                  "window; record_batch includes the evaluator's paired pass over all names, so the same call on an aggregator "
                  "without the video is timed alongside and the video's share is the difference of the medians; the kernel time is the "
                  "video kernel alone, from the device events of a trace of one further fused window of each kind",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
