#!/usr/bin/env python
"""The evaluator's ensemble metrics and step means (ace_amd/evaluator/ ``_Ensembles``, ``_StepMeans``, csrc/ensemble.hip) at 1 degree
180 x 360, 50 paired names, 1 initial condition x 8 members, T = 40 steps per window, on one MI355X:
InferenceEvaluatorAggregator.record_batch of the window that holds step 20, with one EnsembleMetricConfig(step=20) and the
reference's two default step means (step 20, denorm and norm) as the only metrics, fused (the paired pass and one
ace_diag_ensemble_step) and on the torch path, alternated call by call on the same device.  Step 20 lies in one window of a record, so
every call is the first window of an aggregator of its own, built and given its initial condition outside the timed region; the
timed call therefore includes the allocation of that aggregator's accumulators (from torch's caching allocator after the untimed
warm-up).  In ms per window, host syncs around each call after one untimed warm-up aggregator per path.  The kernel's own time comes from a
trace of one further fused window; its traffic is both sides of the selected step read once (2 x names x members planes of 259 KB),
reported as a fraction of the HBM peak of MI355X_MICROARCH (8 TB/s).  The torch path is the baseline, not the code under test, and no
time is a target.
Writes one JSON file and prints it.  usage: python tools/bench_ensemble.py [--steps 40] [--names 50] [--members 8] [--iters 5] [--out ...]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench_regress import HBM_PEAK, H, W, timed  # noqa: E402

STEP = 20


def build(info, names, n_steps, members, fused):
    from ace_amd.evaluator import EnsembleMetricConfig, InferenceEvaluatorAggregatorConfig, MetricConfig, PowerSpectrumMetricConfig, \
        StepMeanMetricConfig, ZonalMeanMetricConfig
    from ace_amd.normalizer import StandardNormalizer
    off = lambda: MetricConfig(enabled=False)                                  # noqa: E731
    norm = StandardNormalizer({n: 0.1 * i for i, n in enumerate(names)}, {n: 1.0 + 0.05 * i for i, n in enumerate(names)}, device="cpu")
    agg = InferenceEvaluatorAggregatorConfig(
        mean_denorm=off(), mean_norm=off(), power_spectrum=PowerSpectrumMetricConfig(enabled=False),
        zonal_mean=ZonalMeanMetricConfig(enabled=False), time_mean_denorm=off(), time_mean_norm=off(), annual=off(), enso_index=off(),
        enso_coefficient=off(), ipo_index=off(),
        step_means=[StepMeanMetricConfig(step=STEP), StepMeanMetricConfig(step=STEP, target="norm")],
        ensembles=[EnsembleMetricConfig(step=STEP)]).build(info, 1, n_steps, normalize=norm, n_ensemble_per_ic=members)
    assert agg.skipped == []
    agg.fused = fused
    return agg


def fields(names, members, T, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return {n: torch.randn(members, T, H, W, generator=g, device=dev) for n in names}


def kernel_us(record, dev):
    """GPU time of the ensemble kernel in one fused window, in microseconds, from the device-side events of a trace"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        record()
        torch.cuda.synchronize(dev)
    return round(sum(float(e.time_range.elapsed_us()) for e in prof.events()
                     if e.device_type == DeviceType.CUDA and "ensemble_step" in e.name), 1)


@torch.no_grad()
def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--names", type=int, default=50)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.json"))
    args = ap.parse_args(argv)
    import ace_amd

    dev = torch.device("cuda", 0)
    T, E = args.steps, args.members
    names = [f"v{i:02d}" for i in range(args.names)]
    lat, _ = np.polynomial.legendre.leggauss(H)
    info = ace_amd.DatasetInfo((H, W), lat=torch.tensor(np.degrees(np.arcsin(lat))), lon=torch.arange(W) * (360.0 / W))
    gen, tgt = fields(names, E, T, dev, 0), fields(names, E, T, dev, 1)
    ic = {n: x[:, :1] for n, x in tgt.items()}

    def fresh(fused):
        agg = build(info, names, T, E, fused)
        agg.record_initial_condition(ic, ic)
        return agg
    for fused in (True, False):
        fresh(fused).record_batch(gen, tgt)                           # untimed: tables, code objects, the allocator's blocks
    times = {True: [], False: []}
    for _ in range(args.iters):                                       # alternated: both paths see the same machine state
        for fused in (True, False):
            agg = fresh(fused)
            times[fused].append(timed(lambda: agg.record_batch(gen, tgt), dev))
    aggs = {fused: fresh(fused) for fused in (True, False)}
    before = aggs[True].launches()
    try:
        k_us = kernel_us(lambda: aggs[True].record_batch(gen, tgt), dev)
    except Exception as err:                                          # a box without a kernel tracer still reports the times
        k_us = None
        print("no kernel trace:", repr(err), file=sys.stderr)
        aggs[True] = fresh(True)
        before = aggs[True].launches()
        aggs[True].record_batch(gen, tgt)
    aggs[False].record_batch(gen, tgt)                                # both paths have now seen the same window
    calls = aggs[True].launches() - before - 1                        # less the paired pass
    logs = {fused: aggs[fused].get_summary_logs() for fused in aggs}
    assert sorted(logs[True]) == sorted(logs[False])
    diff = max(abs(logs[True][k] - logs[False][k]) / max(abs(logs[False][k]), 1e-30) for k in logs[True] if "/crps/" in k)
    step_bytes = 2 * len(names) * E * H * W * 4
    res = {key: {"record_batch_ms": round(float(np.median(times[fused])), 3), "all_ms": [round(v, 3) for v in times[fused]],
                 "route": aggs[fused].route(gen, tgt)} for fused, key in ((True, "fused"), (False, "torch"))}
    result = {
        "workload": f"one ensemble entry (step {STEP}) + step means (step {STEP}, denorm and norm) alone: 1 degree {H}x{W}, 1 initial "
                    f"condition x {E} members, T={T}, {len(names)} paired names; the window that holds step {STEP}",
        "device": torch.cuda.get_device_name(0),
        "fused": res["fused"],
        "torch": res["torch"],
        "torch_over_fused": round(res["torch"]["record_batch_ms"] / res["fused"]["record_batch_ms"], 1),
        "ensemble_step_calls_per_window": calls,
        "ensemble_step_kernel_us": k_us,
        "ensemble_step_bytes_both_sides": step_bytes,
        "traffic_bound_us_at_8TBps_peak": round(step_bytes / HBM_PEAK * 1e6, 2),
        "achieved_fraction_of_hbm_peak": None if not k_us else round(step_bytes / HBM_PEAK * 1e6 / k_us, 3),
        "crps_max_relative_difference_fp64_fused_vs_fp32_torch": diff,
        "timing": "median of --iters host-synchronised calls per path, each the first window of a fresh aggregator built outside the timed "
                  "region, the two paths alternated call by call, after one untimed aggregator per path; "
                  "the kernel time from the device events of a trace of one further fused window; both paths also make the evaluator's "
                  "paired pass over the whole window (the step means are a column of it), which is in record_batch_ms and not in "
                  "ensemble_step_kernel_us",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
