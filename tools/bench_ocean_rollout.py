#!/usr/bin/env python
"""Rollout windows of the CM4 piControl uncoupled ocean (tools/bench_ocean_step.py's shipped configuration: Samudra, 19 levels, the
shipped in / out names, input masking, the shipped ocean_corrector) at 1 degree (180 x 360), B = 1 and 2, T = 40 steps per window
(the shipped evaluator's window), seeded weights, on one MI355X.  Per step, in ms, timed with events after a warm-up window:
  - Stepper.predict with the static masking on the torch path (fused = False) and on the HIP path (fused = True);
  - OceanRolloutEngine in the graph modes None / "step" / "window" (run_window on loaded buffers);
  - the captured Samudra forward alone (CapturedSamudraForward replays) - the floor the engine's "step" mode is held against;
  - the masking kernels alone: the engine's ace_mask_pack_normalize (input masking + normalise + pack + staging) and
    ace_mask_planes (output masking in place) of one step, with the bytes they move and the fraction of 8 TB/s;
  - with --launches: kernel launches per step from `rocprofv3 --kernel-trace --stats` runs of their own (one- and two-window runs,
    the difference over T), rocprofv3 on PATH.
Prints one JSON line.  usage: python tools/bench_ocean_rollout.py [--steps 40] [--iters 3] [--launches]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench_ocean_step as bos  # noqa: E402

HBM = 8e12


def window_data(B, T, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    ic = {n: (torch.randn(B, 1, bos.H, bos.W, generator=g) + (285.0 if n == "sst" else 1.0)).to(dev) for n in bos.OUT}
    forcing = {n: torch.randn(B, T + 1, bos.H, bos.W, generator=g).to(dev) for n in bos.IN if n not in bos.OUT}
    forcing["land_fraction"] = forcing["land_fraction"].abs().clamp(max=1.0) * 0.5
    return ic, forcing


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


def stepper(dev):
    from ace_amd.checkpoint import load_stepper
    return load_stepper(bos.stepper_state(ohc=False), device=dev).stepper


def child(mode, B, T, windows):
    """the engine alone, for the kernel trace: `windows` windows after construction (graph capture included in both runs)"""
    from ace_amd.ocean_rollout import OceanRolloutEngine
    dev = torch.device("cuda", 0)
    st = stepper(dev)
    ic, forcing = window_data(B, T, dev)
    eng = OceanRolloutEngine(st, batch=B, n_forward_steps=T, graph=None if mode == "none" else mode)
    eng.load(ic, forcing)
    for _ in range(windows):
        eng.run_window()
    torch.cuda.synchronize()


def launches(mode, B, T):
    counts = []
    for windows in (1, 2):
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
                   os.path.abspath(__file__), "--child", mode, "--B", str(B), "--steps", str(T), "--windows", str(windows)]
            subprocess.run(cmd, check=True, capture_output=True, timeout=900)
            total = 0
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                with open(path) as f:
                    total += sum(int(row["Calls"]) for row in csv.DictReader(f))
            counts.append(total)
    return (counts[1] - counts[0]) / T


def masking_kernels(eng, iters):
    """ms of one step's ace_mask_pack_normalize and ace_mask_planes (kernels only, the engine's own tables), bytes moved"""
    from ace_amd import _lib
    from ace_amd.masking import _check
    L = _lib.lib()
    B, HW = eng.B, eng.HW
    srcs, src_strides, stage, stage_strides = eng._pack_addr[0]
    hits = eng._in_hits

    def pack():
        _check(L.ace_mask_pack_normalize(srcs, src_strides, eng._in_idx.data_ptr(), hits.data_ptr(), hits.shape[0],
                                         eng._in_fill.data_ptr(), stage, stage_strides, eng.in_mean.data_ptr(),
                                         eng.in_std.data_ptr(), eng.x.data_ptr(), len(eng.in_names), eng._nplanes, B, HW,
                                         _lib.current_stream()))
    a, st = eng._omask_addr[0], eng._omask_strides.data_ptr()

    def outmask():
        _check(L.ace_mask_planes(a, st, a, st, eng._out_idx.data_ptr(), eng._out_hits.data_ptr(), eng._out_hits.shape[0],
                                 eng._out_fill.data_ptr(), len(eng._out_names_masked), B, HW, _lib.current_stream()))
    idx = eng._in_idx.cpu()
    n_masked_in = int((idx >= 0).sum())
    # pack: every source read, every packed plane written, staged planes written, hit bytes of the masked planes
    pack_bytes = B * HW * (4 * eng._nplanes + 4 * len(eng.in_names) + 4 * (len(eng.stage) + len(eng.stage_next)) + n_masked_in)
    # output masking: read + write of each masked plane, its hit bytes
    out_bytes = B * HW * len(eng._out_names_masked) * (4 + 4 + 1)
    return timed(pack, iters * 10), pack_bytes, timed(outmask, iters * 10), out_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--child", choices=["none", "step", "window"])
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--windows", type=int, default=1)
    args = ap.parse_args()
    T = args.steps
    if args.child:
        return child(args.child, args.B, T, args.windows)
    from ace_amd.ocean_rollout import OceanRolloutEngine
    dev = torch.device("cuda", 0)
    st = stepper(dev)
    result = {"model": "Samudra + ocean_corrector (shipped), input + output masking", "grid": [bos.H, bos.W], "levels": bos.L,
              "in_channels": len(bos.IN), "out_channels": len(bos.OUT), "steps_per_window": T, "iters": args.iters,
              "device": torch.cuda.get_device_name(0), "unit": "ms per step", "rows": []}
    maskers = (st._input_process_func, st._output_masking)
    for B in (1, 2):
        ic, forcing = window_data(B, T, dev)
        row = {"batch": B}
        with torch.no_grad():
            inp, gen, _ = bos.data(B, dev)
            net_in = {n: inp[n] for n in bos.IN}
            for fused in (False, True):       # one step's input + output masking on the eager path (bench_ocean_step's masking_ms)
                for m in maskers:
                    m.fused = fused
                row[f"eager_masking_{'fused' if fused else 'torch'}_ms"] = timed(lambda: (maskers[0](net_in), maskers[1](gen)),
                                                                                 args.iters * 10)
            del inp, gen, net_in
            for fused in (False, True):
                for m in maskers:
                    m.fused = fused
                row[f"predict_masking_{'fused' if fused else 'torch'}_ms"] = timed(lambda: st.predict(ic, forcing), args.iters) / T
            for mode in (None, "step", "window"):
                eng = OceanRolloutEngine(st, batch=B, n_forward_steps=T, graph=mode)
                eng.load(ic, forcing)
                row[f"engine_{mode or 'none'}_ms"] = timed(eng.run_window, args.iters) / T
                if mode == "step":
                    cap = eng._captured
                    row["captured_forward_ms"] = timed(lambda: cap.graph.replay(), args.iters * 10)
                    pk_ms, pk_bytes, om_ms, om_bytes = masking_kernels(eng, args.iters)
                    row["mask_pack_normalize"] = {"ms": pk_ms, "bytes": pk_bytes,
                                                  "fraction_of_8TBs": round(pk_bytes / HBM / (pk_ms * 1e-3), 4)}
                    row["mask_planes_output"] = {"ms": om_ms, "bytes": om_bytes,
                                                 "fraction_of_8TBs": round(om_bytes / HBM / (om_ms * 1e-3), 4)}
                del eng
                torch.cuda.empty_cache()
        if args.launches:
            row["launches_per_step"] = {m: launches(m, B, T) for m in ("none", "step", "window")}
        for k, v in list(row.items()):
            if isinstance(v, float):
                row[k] = round(v, 4)
            elif isinstance(v, dict) and "ms" in v:
                v["ms"] = round(v["ms"], 4)
        result["rows"].append(row)
        del ic, forcing
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
