#!/usr/bin/env python
"""One step of the CM4 piControl uncoupled ocean (configs/baselines/cm4-piControl/uncoupled-ocean: Samudra, 19 levels, the shipped
in / out names, input masking, the shipped ocean_corrector) at 1 degree (180 x 360), B = 1 and 2, seeded weights, on one MI355X,
timed in three parts with events after a warm-up: the static masking (input fill + output NaN), the Samudra forward (normalise,
pack, network, unpack, denormalise), and the corrector - fused (ace_ocean_phys_*: O1 / O2) and as torch ops on the GPU.  Two
corrector configurations: the shipped one (force positive so_* and HI, sea-ice fraction without rebalance: O1 only) and the
shipped one plus the heat-content budget (flux from an input hfds: O1 + O2).  Reports the bytes O1 + O2 move (each plane they
read or write once, the static dz / mask tables once per sample) against 8 TB/s, and the launches per corrector call from
`rocprofv3 --kernel-trace --stats` runs of its own (--launches; rocprofv3 must be on PATH).  Prints one JSON line.
usage: python tools/bench_ocean_step.py [--iters 20] [--warmup 5] [--launches]"""
import argparse
import csv
import datetime
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

H, W, L = 180, 360, 19
FORCING = ["DLWRFsfc", "DSWRFsfc", "ULWRFsfc", "USWRFsfc", "LHTFLsfc", "SHTFLsfc", "PRATEsfc", "eastward_surface_wind_stress",
           "northward_surface_wind_stress"]
LEV = lambda p: [f"{p}_{k}" for k in range(L)]
OUT = ["sst", "zos"] + LEV("so") + LEV("thetao") + LEV("uo") + LEV("vo") + ["ocean_sea_ice_fraction", "HI"]
IN = FORCING + ["land_fraction"] + OUT
HBM = 8e12


def corrector_config(ohc: bool):
    cfg = {"force_positive_names": LEV("so") + ["HI"],
           "sea_ice_fraction_correction": {"sea_ice_fraction_name": "ocean_sea_ice_fraction", "land_fraction_name": "land_fraction",
                                           "remove_negative_ocean_fraction": False}}
    if ohc:
        cfg["ocean_heat_content_correction"] = {"method": "scaled_temperature"}
    return {"type": "ocean_corrector", "config": cfg}


def stepper_state(ohc: bool):
    from ace_amd.samudra import Samudra
    torch.manual_seed(0)
    net = Samudra(len(IN), len(OUT), ch_width=[200, 250, 300, 400], dilation=[1, 2, 4, 8], n_layers=[1, 1, 1, 1], norm="instance")
    g = torch.Generator().manual_seed(1)
    idepth = torch.cat([torch.zeros(1), torch.cumsum(torch.linspace(5.0, 500.0, L), 0)])
    deptho = torch.rand(H, W, generator=g) * 6000.0
    deptho[torch.rand(H, W, generator=g) < 0.3] = 0.0
    mask = (deptho.unsqueeze(-1) > idepth[:-1]).float()
    masks = {"mask_2d": mask[..., 0], **{f"mask_{k}": mask[..., k] for k in range(L)}}
    names = sorted(set(IN) | set(OUT))
    return {"stepper": {
        "config": {"input_masking": {"mask_value": 0, "fill_value": 0.0, "exclude_names_and_prefixes": ["land_fraction"]},
                   "step": {"type": "single_module", "config": {
                       "builder": {"type": "Samudra", "config": {"ch_width": [200, 250, 300, 400], "dilation": [1, 2, 4, 8],
                                                                 "n_layers": [1, 1, 1, 1], "norm": "instance"}},
                       "in_names": IN, "out_names": OUT,
                       "normalization": {"network": {"means": {n: 0.0 for n in names}, "stds": {n: 1.0 for n in names}}},
                       "ocean": None, "corrector": corrector_config(ohc)}}},
        "dataset_info": {"horizontal_coordinates": {"lat": torch.linspace(-89.5, 89.5, H), "lon": torch.arange(W) * 1.0},
                         "timestep": datetime.timedelta(days=5) // datetime.timedelta(microseconds=1),
                         "mask_provider": {"masks": masks}, "vertical_coordinate": {"idepth": idepth, "mask": mask, "deptho": deptho}},
        "step": {"module": {**{f"module.{k}": v for k, v in net.state_dict().items()}, "label_encoding": None}}}}


def data(B, dev, seed=2):
    g = torch.Generator().manual_seed(seed)
    inp = {n: (torch.randn(B, H, W, generator=g) + (285.0 if n == "sst" else 1.0)).to(dev) for n in IN}
    inp["land_fraction"] = torch.rand(B, H, W, generator=g).to(dev) * 0.5
    inp["hfds"] = (20.0 * torch.randn(B, H, W, generator=g)).to(dev)       # the heat budget's flux (heat-content variant only)
    gen = {n: (torch.randn(B, H, W, generator=g) + (285.0 if n == "sst" else 1.0)).to(dev) for n in OUT}
    forcing = {n: inp[n] for n in FORCING + ["land_fraction"]}
    return inp, gen, forcing


def o_bytes(corrector, B):
    """bytes O1 + O2 move per call: every plane read (and written) once per sample, the static tables once per sample"""
    plane = 4 * H * W * B
    n = 2 * len(corrector.force_positive_names) + 2        # read + write; sea-ice fraction read + write
    if "ocean_heat_content_correction" in corrector.corrections:
        n += 2 * L + 3 + 1 + 1 + 1          # O1: thetao of output and input, dz (L), mask0, mask_ohc, flux, land (sea-surface fraction)
        n += 2 * L + 2                      # O2: thetao read + write, sst read + write
    return n * plane


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def child(mode, ohc, B, iters):
    """the corrector alone, for the kernel trace: iters calls"""
    from ace_amd.checkpoint import load_stepper
    dev = torch.device("cuda", 0)
    corrector = load_stepper(stepper_state(ohc), device="cpu").stepper._step_obj._corrector
    corrector.fused = mode == "fused"
    inp, gen, forcing = data(B, dev)
    torch.cuda.synchronize()
    for _ in range(iters):
        corrector(inp, gen, forcing)
    torch.cuda.synchronize()


def launches(ohc, B, mode):
    """kernel launches per corrector call: (calls of a 20-call run - calls of a 10-call run) / 10"""
    counts = []
    for iters in (10, 20):
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
                   sys.executable, os.path.abspath(__file__), "--child", mode, "--B", str(B), "--iters", str(iters)] + (["--ohc"] if ohc else [])
            subprocess.run(cmd, check=True, capture_output=True, timeout=600)
            total = 0
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                with open(path) as f:
                    total += sum(int(row["Calls"]) for row in csv.DictReader(f))
            counts.append(total)
    return (counts[1] - counts[0]) / 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--child", choices=["fused", "torch"])
    ap.add_argument("--ohc", action="store_true")
    ap.add_argument("--B", type=int, default=1)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.ohc, args.B, args.iters)
    from ace_amd.checkpoint import load_stepper
    dev = torch.device("cuda", 0)
    result = {"model": "Samudra + ocean_corrector", "grid": [H, W], "levels": L, "in_channels": len(IN), "out_channels": len(OUT),
              "device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rows": []}
    for ohc in (False, True):
        stepper = load_stepper(stepper_state(ohc), device=dev).stepper
        step = stepper._step_obj
        corrector = step._corrector
        net = step.module
        for B in (1, 2):
            inp, gen, forcing = data(B, dev)
            row = {"corrector": "shipped + heat content" if ohc else "shipped", "batch": B, "corrections": corrector.corrections}
            with torch.no_grad():
                net_in = {n: inp[n] for n in IN}
                row["masking_ms"] = timed(lambda: (stepper._input_process_func(net_in), stepper._output_masking(gen)), args.iters,
                                          args.warmup)

                def forward():
                    x = step.in_packer.pack(step.normalizer.normalize(net_in), axis=-3)
                    return step.normalizer.denormalize(step.out_packer.unpack(net(x), axis=-3))
                row["samudra_forward_ms"] = timed(forward, args.iters, args.warmup)
                g0 = {k: v.clone() for k, v in gen.items()}

                def fused():
                    corrector(inp, g0, forcing)
                corrector.fused = True
                row["corrector_fused_ms"] = timed(fused, args.iters, args.warmup)
                corrector.fused = False
                row["corrector_torch_ms"] = timed(lambda: corrector(inp, gen, forcing), args.iters, args.warmup)
                corrector.fused = True
            nbytes = o_bytes(corrector, B)
            row["fused_bytes"] = nbytes
            row["fused_bytes_bound_us"] = round(nbytes / HBM * 1e6, 2)
            row["fused_fraction_of_8TBs"] = round(nbytes / HBM / (row["corrector_fused_ms"] * 1e-3), 4)
            if args.launches:
                row["launches_per_call"] = {m: launches(ohc, B, m) for m in ("fused", "torch")}
            for k in ("masking_ms", "samudra_forward_ms", "corrector_fused_ms", "corrector_torch_ms"):
                row[k] = round(row[k], 4)
            result["rows"].append(row)
            del inp, gen, forcing, g0
        del stepper, step, corrector, net
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
