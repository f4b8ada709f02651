#!/usr/bin/env python
"""Corrector step diagnostics at the ACE2 shape (bench.py's network with its ACE2-style names and hooks: 44 inputs, 50 outputs,
180 x 360, B = 1, the ace2_like corrector at 8 layers and a prescribed-SST ocean) on one MI355X.  Timed with events after a warm-up:
  - RolloutEngine ms per step with step_diagnostics=True against the same engine without it, in this process, alternated, in
    graph="step" and graph="window";
  - the correction aggregator's record_batch per window on its fused path against its torch path on the same device and deltas;
  - ace_diag_correction_window alone (both launches, events around the C-ABI call on tables built once) with the bytes it reads
    and writes - the deltas once, the weight row per plane, the two fp64 maps read and written, the fp64 partials written and
    read back - as a fraction of the 8 TB/s HBM peak.
Writes profiles/step_diagnostics_bench.json and prints it as one JSON line.
usage: python tools/bench_step_diagnostics.py [--steps 40] [--iters 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402

PEAK_HBM_GBS = 8000.0


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_alone(delta, stds, weights, n_time, iters):
    """ms of one ace_diag_correction_window call on device tables built once, and the bytes it moves"""
    from ace_amd import _lib
    from ace_amd.aggregator import _check
    names = list(delta)
    views = [delta[n] for n in names]
    K = len(views)
    B, T, H, W = views[0].shape
    hw, dev = H * W, views[0].device
    L = _lib.lib()
    i64 = dict(dtype=torch.int64, device=dev)
    ptrs = torch.tensor([v.data_ptr() for v in views], **i64)
    strides = torch.tensor([s for v in views for s in v.stride()[:2]], **i64)
    std_t = torch.tensor([stds[n] for n in names], dtype=torch.float32, device=dev)
    rows = torch.arange(K, dtype=torch.int32, device=dev)
    wrows = torch.zeros(K, dtype=torch.int32, device=dev)
    npartial = int(L.ace_diag_correction_partial_doubles(K, B, T, hw))
    partial = torch.empty(npartial, dtype=torch.float64, device=dev)
    sgn, mag = (torch.zeros(K, hw, dtype=torch.float64, device=dev) for _ in range(2))
    series = torch.zeros(2, K, n_time, dtype=torch.float64, device=dev)
    stream = _lib.current_stream()

    def call():
        _check(L.ace_diag_correction_window(ptrs.data_ptr(), strides.data_ptr(), std_t.data_ptr(), rows.data_ptr(), wrows.data_ptr(),
                                            weights.data_ptr(), weights.shape[0], partial.data_ptr(), sgn.data_ptr(), mag.data_ptr(),
                                            series.data_ptr(), K, n_time, 0, K, B, T, hw, stream))

    ms = timed(call, iters)
    moved = {"deltas": 4 * K * B * T * hw, "weights": 4 * K * hw, "maps_read_and_written": 2 * 2 * 8 * K * hw,
             "partials_written_and_read": 2 * 8 * npartial, "series": 2 * 2 * 8 * K * T}
    return ms, moved


def window_data(stepper, forcing_names, prog, T, dev, seed=3):
    norm = stepper._step_obj.normalizer
    g = torch.Generator().manual_seed(seed)

    def field(n, nt):
        x = float(norm.means[n]) + 0.1 * float(norm.stds[n]) * torch.randn(1, nt, *bench.IMG, generator=g)
        return (x.clamp(0.0, 1.0) if n.endswith("_fraction") else x).to(dev)

    ic = {n: field(n, 1) for n in prog}
    forcing = {n: field(n, T + 1) for n in forcing_names}
    forcing["surface_temperature"] = field("surface_temperature", T + 1)      # the ocean's prescribed SST target
    return ic, forcing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_diagnostics_bench.json"))
    args = ap.parse_args()
    from ace_amd.aggregator import InferenceAggregatorConfig
    from ace_amd.rollout import RolloutEngine
    from ace_amd.step_diagnostics import CorrectionDeltaAggregator, StepDiagnostics
    dev = torch.device("cuda", 0)
    T = args.steps
    stepper, forcing_names, prog, diag = bench.build_stepper(dev, 0, hooks=True)
    ic, forcing = window_data(stepper, forcing_names, prog, T, dev)
    result = {"shape": {"img": list(bench.IMG), "batch": 1, "n_in": len(forcing_names) + len(prog), "n_out": len(prog) + len(diag),
                        "steps": T, "iters": args.iters, "rounds": args.rounds},
              "device": torch.cuda.get_device_name(0), "engine": {}}
    delta = None
    for graph in ("step", "window"):
        engines = {flag: RolloutEngine(stepper, batch=1, n_forward_steps=T, graph=graph, step_diagnostics=flag) for flag in (False, True)}
        for eng in engines.values():
            eng.load(ic, forcing)
        ms = {False: [], True: []}
        for _ in range(args.rounds):                      # alternated: the two engines see the same clocks
            for flag, eng in engines.items():
                ms[flag].append(timed(eng.run_window, args.iters) / T)
        rec = engines[True]._recorder
        row = {"ms_per_step_without": min(ms[False]), "ms_per_step_with": min(ms[True]), "all_without": ms[False], "all_with": ms[True],
               "K": len(rec.names), "names": rec.names,
               "snapshot_bytes_per_step": 2 * 4 * len(rec.names) * rec.hw, "delta_bytes_per_window": 3 * 4 * len(rec.names) * T * rec.hw}
        row["extra_ms_per_step"] = row["ms_per_step_with"] - row["ms_per_step_without"]
        row["extra_fraction"] = row["extra_ms_per_step"] / row["ms_per_step_without"]
        # the spread between rounds of one engine: a difference under it is not distinguishable from noise
        row["spread_ms_per_step"] = max(max(ms[f]) - min(ms[f]) for f in ms)
        row["distinguishable_from_noise"] = bool(row["extra_ms_per_step"] > row["spread_ms_per_step"])
        result["engine"][graph] = row
        delta = {k: v.clone() for k, v in rec.delta().items()}
        del engines
        torch.cuda.empty_cache()

    # the aggregator on one window of real deltas
    info = stepper._dataset_info
    host = InferenceAggregatorConfig().build(info, 2 * T)
    diags = StepDiagnostics(delta=delta)
    agg_ms = {}
    for fused in (True, False):
        agg = CorrectionDeltaAggregator(host, stepper.normalizer, 2 * T, record_scalars=True, record_maps=True)
        agg.fused = fused
        agg.record_batch(diags, 0)                        # the accumulators and tables exist

        def record(a=agg):
            a._n_steps, a._n_batches = 0, [0] * a._n_time
            a.record_batch(diags, 0)

        agg_ms["fused" if fused else "torch"] = timed(record, args.iters)
        assert agg._path == ("fused" if fused else "torch")
    K = len(delta)
    stds = {n: float(stepper.normalizer.stds[n]) for n in delta}
    weights = host.weights_for(next(iter(delta)), dev).reshape(1, -1).contiguous()
    kernel_ms, moved = kernel_alone(delta, stds, weights, 2 * T, 20 * args.iters)
    total = sum(moved.values())
    result["aggregator"] = {"record_batch_ms_fused": agg_ms["fused"], "record_batch_ms_torch": agg_ms["torch"],
                            "speedup": agg_ms["torch"] / agg_ms["fused"], "K": K, "steps": T,
                            "kernel_ms": kernel_ms, "kernel_bytes": total, "kernel_bytes_by_part": moved,
                            "kernel_gbs": total / (kernel_ms * 1e-3) / 1e9,
                            "kernel_fraction_of_hbm_peak": total / (kernel_ms * 1e-3) / 1e9 / PEAK_HBM_GBS}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
