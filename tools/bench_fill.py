#!/usr/bin/env python
"""The masked-spectrum fill (ace_amd/fill.py, csrc/fill.hip) at 1 degree 180 x 360, B = 1, T = 40 steps per window, on the Samudra
output list (thetao, so, uo, vo on 19 levels and zos: 77 names, every one masked - a land mask per level that grows with depth and
"mask_2d" at the surface), on one MI355X.  Three measurements, each the median of --iters repeats after an untimed warm-up, the two
sides of a comparison alternated repeat by repeat:
  * ace_diag_fill_planes on all 77 names (both launches: the plane means of the names with an interior, the tiles) against the
    torch.stack of the same names, which it replaces - device events around each;
  * the bytes the fill needs - one read of every source plane and one write of dst, computed from the shapes - over its time, as a
    fraction of the 8 TB/s HBM peak (the means pass reads the planes of names with an interior a second time; that read is the
    call's own cost and is not added to the bytes);
  * InferenceEvaluatorAggregator.record_batch with the spectrum as the only metric and the fill on, fused against the torch path
    (``smooth_flood_fill`` per name and side) - a host clock around calls that end in a device synchronise.
No time is a target.  Writes one JSON file and prints it.
usage: python tools/bench_fill.py [--steps 40] [--levels 19] [--iters 5] [--out ...]"""
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
H, W = 180, 360


def land(level: int, levels: int) -> torch.Tensor:
    """1 = ocean: smooth continents from a fixed seed, growing with depth"""
    g = torch.Generator().manual_seed(5)
    z = torch.randn(1, 1, H, W, generator=g)
    for _ in range(6):
        z = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(z, (6, 6, 0, 0), mode="circular"), (1, 13), 1)
        z = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(z, (0, 0, 6, 6), mode="replicate"), (13, 1), 1)
    z = (z[0, 0] - z.mean()) / z.std()
    return (z < 0.5 - 0.8 * level / max(levels - 1, 1)).float()


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def host_ms(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def build(info, n_steps, fused):
    from ace_amd.evaluator import InferenceEvaluatorAggregatorConfig, MetricConfig, PowerSpectrumMetricConfig, ZonalMeanMetricConfig
    off = lambda: MetricConfig(enabled=False)                                  # noqa: E731
    agg = InferenceEvaluatorAggregatorConfig(
        mean_denorm=off(), mean_norm=off(), step_means=[], ensembles=[], power_spectrum=PowerSpectrumMetricConfig(fill_masked=True),
        zonal_mean=ZonalMeanMetricConfig(enabled=False), time_mean_denorm=off(), time_mean_norm=off(), annual=off(), enso_index=off(),
        enso_coefficient=off(), ipo_index=off()).build(info, 0, n_steps, normalize=lambda d: d)
    agg.fused = fused
    return agg


@torch.no_grad()
def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--levels", type=int, default=19)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_bench.json"))
    args = ap.parse_args(argv)
    import ace_amd
    from ace_amd.masking import SpatialMaskProvider

    dev = torch.device("cuda", 0)
    T = args.steps
    names = [f"{v}_{k}" for v in ("thetao", "so", "uo", "vo") for k in range(args.levels)] + ["zos"]
    masks = {f"mask_{k}": land(k, args.levels) for k in range(args.levels)}
    masks["mask_2d"] = masks["mask_0"]
    lat, _ = np.polynomial.legendre.leggauss(H)
    info = ace_amd.DatasetInfo((H, W), lat=torch.tensor(np.degrees(np.arcsin(lat))), lon=torch.arange(W) * (360.0 / W),
                               mask_provider=SpatialMaskProvider(masks))
    g = torch.Generator(device=dev).manual_seed(0)

    def window(shift):
        out = {}
        for i, n in enumerate(names):
            x = 10.0 + i + shift + torch.randn(1, T, H, W, generator=g, device=dev)
            out[n] = x.where(info.mask_provider.get_mask_tensor_for(n).to(dev) != 0, torch.full((), float("nan"), device=dev))
        return out
    gen, tgt = window(0.0), window(0.1)

    # ---- the fill call against the torch.stack it replaces
    probe = build(info, T, True)
    for n in names:
        probe._omitted(n)
    fields = [gen[n] for n in names]
    fill = lambda: probe._spectrum_input(names, fields, dev)[0]                # noqa: E731
    stack = lambda: torch.stack(fields)                                        # noqa: E731
    for fn in (fill, stack):
        fn()
    torch.cuda.synchronize(dev)
    times = {"fill": [], "stack": []}
    for _ in range(args.iters):
        for key, fn in (("fill", fill), ("stack", stack)):
            ms, out = event_ms(fn)
            times[key].append(ms)
            del out
    layers = probe._fill.stacks(dev)[0]
    with_interior = sum(bool((layers[probe._fill.row(info.mask_provider.mask_key_for(n), None, dev)] == 5).any()) for n in names)
    fill_ms, stack_ms = float(np.median(times["fill"])), float(np.median(times["stack"]))
    fill_bytes = 2 * len(names) * T * H * W * 4
    del probe, fields
    torch.cuda.empty_cache()

    # ---- record_batch, the spectrum alone, fused against torch
    aggs = {fused: build(info, (args.iters + 2) * T, fused) for fused in (True, False)}
    for agg in aggs.values():
        agg.record_batch(gen, tgt)
    rec = {True: [], False: []}
    for _ in range(args.iters):
        for fused in (True, False):
            rec[fused].append(host_ms(lambda: aggs[fused].record_batch(gen, tgt), dev))
    fds, tds = aggs[True].get_dataset()["power_spectrum"], aggs[False].get_dataset()["power_spectrum"]
    worst = max(float((fds[n].double() - tds[n].double()).abs().max() / tds[n].double().abs().max()) for n in tds)
    fused_ms, torch_ms = float(np.median(rec[True])), float(np.median(rec[False]))
    result = {
        "workload": f"masked-spectrum fill: 1 degree {H}x{W}, B=1, T={T}, {len(names)} names, all masked ({len(masks)} masks)",
        "device": torch.cuda.get_device_name(0),
        "names_with_an_interior": with_interior,
        "fill_call": {"ms": round(fill_ms, 3), "all_ms": [round(v, 3) for v in times["fill"]],
                      "bytes_one_read_one_write": fill_bytes,
                      "fraction_of_8TBps": round(fill_bytes / (fill_ms * 1e-3) / HBM_PEAK, 3)},
        "torch_stack": {"ms": round(stack_ms, 3), "all_ms": [round(v, 3) for v in times["stack"]]},
        "fill_over_stack": round(fill_ms / stack_ms, 3),
        "record_batch_spectrum_only": {
            "fused_ms": round(fused_ms, 2), "torch_ms": round(torch_ms, 2), "torch_over_fused": round(torch_ms / fused_ms, 2),
            "fused_all_ms": [round(v, 2) for v in rec[True]], "torch_all_ms": [round(v, 2) for v in rec[False]],
            "routes": [aggs[True].route(gen, tgt), aggs[False].route(gen, tgt)],
            "filled_names": len(aggs[True].filled), "omitted_names": len(aggs[True].omitted),
            "launches_per_window_fused": aggs[True].launches() // (args.iters + 1),
            "largest_spectrum_difference_over_max": worst},
        "timing": "median of --iters repeats after one untimed call; fill and stack by device events, record_batch by a host "
                  "clock around synchronised calls; the two sides of each comparison alternated repeat by repeat",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
