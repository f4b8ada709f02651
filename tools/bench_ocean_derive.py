#!/usr/bin/env python
"""The ocean's derived variables (ace_amd/ocean_derived_variables.py: OceanDeriveFn.window, csrc/ocean_derive.hip) on one MI355X
at 1 degree 180 x 360, the 19 depth levels of tools/bench_ocean_step.py (the shipped Samudra layout), B = 1, T = 40 steps per
window, all seven outputs, the tendency of the first step taken against the initial condition:
  * ``window`` on the fused path (one ace_ocean_derive_window) and on the module's own torch path (``fused=False``: concatenate the
    initial condition, the reference's op sequence, drop the first time level), alternated call by call on the same device, in ms
    per window with host syncs around each call after --warmup untimed windows;
  * the kernel alone between device events around --launches back-to-back C calls, for the library's own t_chunk and for a sweep;
  * counted from the shapes, not measured: the bytes the kernel has to move once (every input plane, the dz table once, every
    output), and its share of the HBM peak (8 TB/s) at the kernel's time.  A chunk's first step re-reads the thetao levels of the
    step before it; those bytes are listed apart.
Both paths' outputs are compared at the timed shape (the surface variables bitwise, the heat budget to the fp32 rounding of the
torch path).  No time is a target.  Writes one JSON file and prints it.
usage: python tools/bench_ocean_derive.py [--steps 40] [--iters 10] [--warmup 3] [--launches 20] [--out ...]"""
import argparse
import ctypes
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, L = 180, 360, 19
HBM_PEAK = 8.0e12
STEP = datetime.timedelta(days=5)
DATA = [f"thetao_{k}" for k in range(L)] + ["hfds_total_area", "ocean_sea_ice_fraction", "sea_ice_volume"]
FORCING = ["land_fraction", "hfgeou"]


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, out


def geometry():
    from ace_amd.insolation import LatLonGrid
    from ace_amd.ocean_corrector import DepthCoordinate
    g = torch.Generator().manual_seed(1)
    idepth = torch.cat([torch.zeros(1), torch.cumsum(torch.linspace(5.0, 500.0, L), 0)])
    deptho = torch.rand(H, W, generator=g) * 6000.0
    deptho[torch.rand(H, W, generator=g) < 0.3] = 0.0
    mask = (deptho.unsqueeze(-1) > idepth[:-1]).float()
    grid = LatLonGrid(torch.linspace(-89.5, 89.5, H), torch.arange(W) + 0.5)
    return DepthCoordinate(idepth, mask, deptho), grid


@torch.no_grad()
def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3, help="untimed windows per path before the timed ones")
    ap.add_argument("--launches", type=int, default=20, help="back-to-back kernel launches per device-event timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ocean_derive_bench.json"))
    args = ap.parse_args(argv)
    from ace_amd import _lib
    from ace_amd.ocean_derived_variables import OceanDeriveFn

    dev = torch.device("cuda", 0)
    T = args.steps
    depth, grid = geometry()
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)                                           # noqa: E731
    u = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g, device=dev)                    # noqa: E731
    mask = depth.mask.to(dev)
    series = {}
    for k in range(L):
        series[f"thetao_{k}"] = (r(1, T + 1, H, W) * 2.0 + 14.0 - 0.6 * k).where(mask[..., k] > 0, float("nan"))
    series.update({"hfds_total_area": r(1, T + 1, H, W) * 40 + 3, "ocean_sea_ice_fraction": u(0.05, 1.0, 1, T + 1, H, W),
                   "sea_ice_volume": u(0.01, 5.0, 1, T + 1, H, W)})
    forcing = {"land_fraction": u(0.0, 0.9, 1, 1, H, W).expand(1, T + 1, H, W).contiguous(), "hfgeou": r(1, T + 1, H, W) * 0.02 + 0.08}
    ic = {k: v[:, :1].contiguous() for k, v in series.items()}
    data = {k: v[:, 1:].contiguous() for k, v in series.items()}
    fns = {"fused": OceanDeriveFn(depth, STEP, grid, fused=True), "torch": OceanDeriveFn(depth, STEP, grid, fused=False)}
    times = {k: [] for k in fns}
    last = {}
    for i in range(args.warmup + args.iters):                       # alternated: both paths see the same machine state
        for key, fn in fns.items():
            ms, last[key] = timed(lambda: fn.window(data, ic, forcing, 1, T), dev)
            if i >= args.warmup:
                times[key].append(ms)
    assert fns["fused"].launches == args.warmup + args.iters and fns["torch"].launches == 0
    from ace_amd._lib import OCEAN_DERIVE_OUTPUTS
    assert [k for k in last["fused"] if k not in data] == list(OCEAN_DERIVE_OUTPUTS) == [k for k in last["torch"] if k not in data]
    agree = {}
    for n in OCEAN_DERIVE_OUTPUTS:
        a, b = last["fused"][n], last["torch"][n]
        assert torch.equal(torch.isnan(a), torch.isnan(b)), n
        ok = ~torch.isnan(b)
        agree[n] = {"bitwise": bool(torch.equal(a[ok].view(torch.int32), b[ok].view(torch.int32))),
                    "max_abs_diff_over_max_abs": float((a[ok].double() - b[ok].double()).abs().max() / b[ok].double().abs().max())}
    for n in ("net_energy_flux_into_ocean_column", "sea_ice_fraction", "hfds"):
        assert agree[n]["bitwise"], n
    assert agree["ocean_heat_content"]["max_abs_diff_over_max_abs"] < (L + 3) * 2.0 ** -24
    assert agree["HI"]["max_abs_diff_over_max_abs"] < 1e-4

    # the kernel alone: the descriptor the fused path filled for this window, launched back to back
    fn = fns["fused"]
    desc = next(iter(fn._plans.values()))[1]
    lib = _lib.lib()
    kernel = {}
    for t_chunk in (0, 1, 2, 3, 4, 5, 8, 10, 20, T):
        desc.t_chunk = t_chunk
        runs = []
        for _ in range(args.iters + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                rc = lib.ace_ocean_derive_window(ctypes.byref(desc), _lib.current_stream())
            b.record()
            torch.cuda.synchronize(dev)
            assert rc == 0, lib.ace_ocean_derive_last_error().decode()
            runs.append(a.elapsed_time(b) / args.launches)
        kernel[str(t_chunk)] = [round(x, 5) for x in runs[1:]]
    desc.t_chunk = 0
    med = lambda v: float(np.median(v))                                  # noqa: E731
    hw = H * W
    planes_in = L * T + L + 5 * T                                        # thetao steps, the head, five surface fields
    static = (L + 2) * hw * 4                                            # dz, mask0, area_m2 (once; dz is re-read from cache)
    once = (planes_in + 7 * T) * hw * 4 + static
    nchunk = -(-hw // 1024)
    lib_chunk = max(1, min(T, T * nchunk // 512))                        # csrc/ocean_derive.hip: TARGET_GROUPS
    reread = (-(-T // lib_chunk) - 1) * L * hw * 4
    k_ms = med(kernel["0"])
    result = {
        "workload": f"ocean derived variables: 1 degree {H}x{W}, {L} levels, B=1, T={T}, all seven outputs, with head",
        "device": torch.cuda.get_device_name(0),
        "window_ms": {k: round(med(v), 4) for k, v in times.items()},
        "window_all_ms": {k: [round(x, 4) for x in v] for k, v in times.items()},
        "torch_over_fused": round(med(times["torch"]) / med(times["fused"]), 2),
        "fused_is_faster": med(times["fused"]) < med(times["torch"]),
        "launches_per_window": {"fused": 1},
        "kernel_alone_ms": round(k_ms, 5),
        "kernel_alone_ms_by_t_chunk": {k: round(med(v), 5) for k, v in kernel.items()},
        "kernel_alone_all_ms": kernel,
        "library_t_chunk": lib_chunk,
        "bytes_counted_from_shapes": {"moved_once": once, "of_which_read": once - 7 * T * hw * 4, "of_which_written": 7 * T * hw * 4,
                                      "thetao_re_read_at_chunk_starts": reread,
                                      "dz_table_re_read_per_step_from_cache": L * hw * 4},
        "kernel_bytes_per_second": round(once / (k_ms * 1e-3), 1),
        "share_of_hbm_peak_8TBps": round(once / (k_ms * 1e-3) / HBM_PEAK, 4),
        "bound": "bandwidth (the least time is bytes over the HBM peak; the arithmetic is two fp64 operations per thetao value)",
        "fused_against_torch_path": agree,
        "timing": "window: median of --iters host-synchronised OceanDeriveFn.window calls per path, the paths alternated call by "
                  "call, after --warmup untimed calls each; the kernel alone between device events around --launches back-to-back "
                  "launches, per launch, median of --iters after one untimed round",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert result["fused_is_faster"], result["window_ms"]


if __name__ == "__main__":
    main()
