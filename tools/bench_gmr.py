#!/usr/bin/env python
"""Global-mean removal at the ACE2 shape (bench.py's network and its ACE2-style names: 44 inputs, 50 outputs, 180 x 360, B = 1)
on one MI355X, for ``shared`` with the default temperature field names (reference field surface_temperature, 10 of the 11 names
present) and for ``per_channel`` over all 44 inputs, both without synthetic channels so that the network is the one of the stepper
without the option.  Timed with events after a warm-up, in ms:
  - RolloutEngine per step (graph="step") with the option, and the same stepper configuration without it, in this process;
  - the three kernels of csrc/gmr.hip alone on the engine's own tables (ace_gmr_partials, ace_gmr_pack_normalize,
    ace_gmr_unpack_denormalize), and the plain ace_pack_normalize / ace_unpack_denormalize they replace;
  - the same transform as torch ops captured in a hipGraph: forward_transform (fused=False: t.mean) -> normalize -> pack and
    unpack -> denormalize -> inverse_transform of one step on static tensors, against the capture of the same glue without the
    option (the difference is what the option costs as torch ops);
  - Stepper.predict per step with the host class fused / unfused and without the option (eager, not captured);
  - with --trace: the glue kernels' own durations from `rocprofv3 --kernel-trace --stats` runs of their own (one child process
    per configuration that runs the engine's windows), rocprofv3 on PATH.  The event timings above are intervals between
    back-to-back launches on data the caches hold; the trace gives the kernels inside the rollout.
Writes profiles/gmr_bench.json and prints it as one JSON line.
usage: python tools/bench_gmr.py [--steps 8] [--iters 3] [--trace]"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402


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


def build(dev, gmr, seed=0):
    import ace_amd
    from ace_amd.step import NormalizationConfig
    forcing, prog, diag = bench.hook_names()
    names = forcing + prog + diag
    means, stds = {k: 0.1 for k in names}, {k: 1.1 for k in names}
    means["surface_temperature"], stds["surface_temperature"] = 288.0, 10.0
    means["TMP2m"], stds["TMP2m"] = 287.0, 10.0
    for k in range(8):
        means[f"air_temperature_{k}"], stds[f"air_temperature_{k}"] = 250.0, 5.0
    cfg = ace_amd.SingleModuleStepConfig(
        builder=ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet", config=bench.ACE2),
        in_names=forcing + prog, out_names=prog + diag, normalization=NormalizationConfig(means=means, stds=stds),
        global_mean_removal=gmr)
    torch.manual_seed(seed)
    stepper = ace_amd.Stepper.from_config(cfg, ace_amd.DatasetInfo(bench.IMG), device=dev)
    stepper.set_eval()
    return stepper, forcing, prog, means, stds


def window_data(forcing, prog, means, stds, T, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    field = lambda n, nt: (means[n] + stds[n] * torch.randn(1, nt, *bench.IMG, generator=g)).to(dev)      # noqa: E731
    return {n: field(n, 1) for n in prog}, {n: field(n, T + 1) for n in forcing}


def kernels(eng, iters):
    """ms of one step's glue launches on the engine's own tables"""
    from ace_amd import _lib
    L, stream = _lib.lib(), _lib.current_stream()
    nin, nout, B, HW = len(eng.in_names), len(eng.out_names), eng.B, eng.HW
    src, strides, dst = eng._src_ptr_addr[1], eng._src_stride_addr[1], eng._dst_ptr_addr[1]
    out = {}
    out["ace_pack_normalize"] = timed(lambda: _lib.check(L.ace_pack_normalize(
        src, strides, eng.in_mean.data_ptr(), eng.in_std.data_ptr(), eng.x.data_ptr(), B, nin, HW, stream)), iters)
    out["ace_unpack_denormalize"] = timed(lambda: _lib.check(L.ace_unpack_denormalize(
        eng.y.data_ptr(), eng.out_mean.data_ptr(), eng.out_std.data_ptr(), dst, eng._dst_strides.data_ptr(), B, nout, HW, stream)), iters)
    g = eng._gmr
    if g is not None:
        nextra = len(eng.extra_names)
        out["ace_gmr_partials"] = timed(lambda: _lib.check(L.ace_gmr_partials(
            src, strides, g["planes"].data_ptr(), nin, g["partials"].data_ptr(), B, g["K"], HW, stream)), iters)
        out["ace_gmr_pack_normalize"] = timed(lambda: _lib.check(L.ace_gmr_pack_normalize(
            src, strides, eng.in_mean.data_ptr(), eng.in_std.data_ptr(), g["in_idx"].data_ptr(), g["partials"].data_ptr(),
            g["clim"].data_ptr(), g["extra_idx"].data_ptr() if nextra else None, g["extra_std"].data_ptr() if nextra else None,
            eng.x.data_ptr(), g["shift"].data_ptr(), B, nin, nextra, g["K"], HW, stream)), iters)
        out["ace_gmr_unpack_denormalize"] = timed(lambda: _lib.check(L.ace_gmr_unpack_denormalize(
            eng.y.data_ptr(), eng.out_mean.data_ptr(), eng.out_std.data_ptr(), dst, eng._dst_strides.data_ptr(),
            g["out_idx"].data_ptr(), g["shift"].data_ptr(), B, nout, g["K"], HW, stream)), iters)
        out["reduced_bytes"] = 4 * g["K"] * B * HW
    return out


def captured_torch_glue(stepper, ic, forcing, iters):
    """ms of one step's glue as torch ops replayed from a hipGraph: (forward_transform ->) normalize -> pack, then
    unpack -> denormalize (-> inverse_transform) of a static network output"""
    step = stepper._step_obj
    gmr = step.global_mean_removal
    if gmr is not None:
        gmr = step.config.global_mean_removal.build(step.normalizer, list(step.in_names), fused=False)
    inputs = {**{n: v[:, 0] for n, v in ic.items()}, **{n: v[:, 0] for n, v in forcing.items()}}
    y = torch.randn(1, len(step.out_names), *bench.IMG, device=next(iter(inputs.values())).device)
    norm = step.normalizer

    def glue():
        state = None
        x = inputs
        if gmr is not None:
            x, state = gmr.forward_transform(x, None)
        x = norm.normalize(x)
        if gmr is not None:
            x = {**x, **gmr.extras_normalized(state)}
        packed = step.in_packer.pack(x, axis=-3)
        out = norm.denormalize(step.out_packer.unpack(y, axis=-3))
        if gmr is not None:
            out = gmr.inverse_transform(out, state)
        return packed, out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        glue()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        keep = glue()      # noqa: F841  (the captured outputs stay alive with the graph)
    return timed(graph.replay, iters)


GLUE_KERNELS = ("gmr_partials_kernel", "gmr_pack_normalize_kernel", "gmr_unpack_denormalize_kernel", "pack_normalize_kernel",
                "unpack_denormalize_kernel")


def gmr_configs():
    import ace_amd
    return {"none": None, "shared": ace_amd.SharedGlobalMeanRemovalConfig(),
            "per_channel": ace_amd.PerChannelGlobalMeanRemovalConfig()}


def child(name, T, windows):
    """the engine alone, for the kernel trace"""
    from ace_amd.rollout import RolloutEngine
    dev = torch.device("cuda", 0)
    stepper, forcing_names, prog, means, stds = build(dev, gmr_configs()[name])
    ic, forcing = window_data(forcing_names, prog, means, stds, T, dev)
    eng = RolloutEngine(stepper, batch=1, n_forward_steps=T, graph=None)
    eng.load(ic, forcing)
    for _ in range(windows):
        eng.run_window()
    torch.cuda.synchronize()


def kernel_trace(name, T, windows=3):
    """kernel name -> {"calls", "mean_us"} of the stepper-glue kernels in a traced run of the engine (graph=None)"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--child", name, "--steps", str(T), "--windows", str(windows)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=400)
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    # whole identifiers: "gmr_pack_normalize_kernel" also ends in "pack_normalize_kernel"
                    found = re.search(r"(\w+_kernel)\b", row["Name"])
                    if found and found.group(1) in GLUE_KERNELS:
                        out[found.group(1)] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmr_bench.json"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps, args.windows)
    from ace_amd.rollout import RolloutEngine
    dev = torch.device("cuda", 0)
    T = args.steps
    configs = gmr_configs()
    result = {"shape": {"img": list(bench.IMG), "batch": 1, "n_in": bench.N_FORCING + bench.N_PROGNOSTIC,
                        "n_out": bench.N_PROGNOSTIC + bench.N_DIAGNOSTIC, "steps": T, "iters": args.iters},
              "device": torch.cuda.get_device_name(0), "configs": {}}
    for name, gmr in configs.items():
        stepper, forcing_names, prog, means, stds = build(dev, gmr)
        ic, forcing = window_data(forcing_names, prog, means, stds, T, dev)
        eng = RolloutEngine(stepper, batch=1, n_forward_steps=T, graph="step")
        eng.load(ic, forcing)
        row = {"engine_ms_per_step": timed(eng.run_window, args.iters) / T,
               "kernels_ms": kernels(eng, 20 * args.iters),
               "captured_torch_glue_ms": captured_torch_glue(stepper, ic, forcing, 10 * args.iters)}
        with torch.no_grad():
            row["predict_ms_per_step"] = timed(lambda: stepper.predict(ic, forcing), args.iters) / T
            if gmr is not None:
                stepper._step_obj.global_mean_removal.fused = False
                row["predict_unfused_ms_per_step"] = timed(lambda: stepper.predict(ic, forcing), args.iters) / T
                stepper._step_obj.global_mean_removal.fused = True
                g = eng._gmr
                row["K"], row["shifted_inputs"] = g["K"], int((g["in_idx"] >= 0).sum())
                row["shifted_outputs"] = int((g["out_idx"] >= 0).sum())
        result["configs"][name] = row
        del eng, stepper
        torch.cuda.empty_cache()
    base = result["configs"]["none"]
    for name in ("shared", "per_channel"):
        row, k = result["configs"][name], result["configs"][name]["kernels_ms"]
        row["fused_glue_ms"] = k["ace_gmr_partials"] + k["ace_gmr_pack_normalize"] + k["ace_gmr_unpack_denormalize"]
        row["fused_glue_extra_ms"] = row["fused_glue_ms"] - (k["ace_pack_normalize"] + k["ace_unpack_denormalize"])
        row["torch_glue_extra_ms"] = row["captured_torch_glue_ms"] - base["captured_torch_glue_ms"]
        row["engine_extra_ms_per_step"] = row["engine_ms_per_step"] - base["engine_ms_per_step"]
    if args.trace:      # after this process is done with the device's timing: one traced child per configuration
        for name in configs:
            result["configs"][name]["traced_kernels"] = kernel_trace(name, T)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
