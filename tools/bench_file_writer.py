#!/usr/bin/env python
"""The region- and time-selected file writers (ace_amd/data_writer.py: FileWriter, csrc/region.hip) at the shape of
tools/bench_data_writer.py - 1 degree 180 x 360, 50 names in the window, B = 1, T = 40 six-hourly steps per window - on one MI355X:
``append_batch`` per window of
  * box:            a 20 x 40 box (lon0 = 200: the 16-byte path) of 8 names;
  * box_lon0_190:   the same box ten columns to the west (lon0 = 190: pixels loaded one by one);
  * box_coarsen_4:  the first box with TimeCoarsen(4);
  * jja_globe:      MonthSelector(["JJA"]) over the whole globe, 8 names, every timed window inside the season;
each on the fused path (one ace_diag_region_segments per window, then one copy of the kept record) and on the module's own torch
path, alternated call by call on the same device, in ms per window with host syncs around each call after --warmup untimed windows,
and the bytes each moved to the host per window.  The fused path's bytes are asserted to be the kept record exactly:
names * B * n_kept * nlat_r * nlon_r * 4.  The kernel alone (means only, no copy) is timed between device events around --launches
back-to-back C calls.  Counted from the shapes, not measured: the bytes the result needs (requested) and the bytes of the 64-byte
and 128-byte lines the row fragments of the box touch (fetched, if every touched line is fetched once).  No time is a target.
Writes one JSON file and prints it.
usage: python tools/bench_file_writer.py [--steps 40] [--names 50] [--iters 6] [--warmup 2] [--launches 20] [--out ...]"""
import argparse
import datetime
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 180, 360
STEP = datetime.timedelta(hours=6)
KEPT_NAMES = 8


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def touched_bytes(region, steps, names, line):
    """bytes of the ``line``-byte lines that the rows of the box touch, planes taken as starting on a line boundary"""
    lat0, h, lon0, w = region
    n = 0
    for i in range(lat0, lat0 + h):
        first, last = (i * W + lon0) * 4, (i * W + lon0 + w) * 4 - 1
        n += last // line - first // line + 1
    return n * line * steps * names


@torch.no_grad()
def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--names", type=int, default=50)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2, help="untimed windows per writer before the timed ones")
    ap.add_argument("--launches", type=int, default=20, help="back-to-back kernel launches per device-event timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "file_writer_bench.json"))
    args = ap.parse_args(argv)
    from ace_amd import _lib
    from ace_amd import data_writer as DW
    from ace_amd.timeaxis import TimeAxis

    dev = torch.device("cuda", 0)
    T, names = args.steps, [f"v{i:02d}" for i in range(args.names)]
    kept_names = names[::max(1, len(names) // KEPT_NAMES)][:KEPT_NAMES]
    g = torch.Generator(device=dev).manual_seed(0)
    data = {n: torch.randn(1, T, H, W, generator=g, device=dev) for n in names}
    n_windows = args.iters + args.warmup
    axis = TimeAxis.regular((2001, 6, 1), STEP, 1 + n_windows * T)                 # 80 days from 1 June by default: inside JJA
    coords = {"lat": np.arange(-89.5, 90.0), "lon": np.arange(0.5, 360.0)}
    tmp = tempfile.TemporaryDirectory()
    box = dict(lat_extent=(-10, 10), lon_extent=(200, 240))
    cases = {
        "box": dict(names=kept_names, **box),
        "box_lon0_190": dict(names=kept_names, lat_extent=(-10, 10), lon_extent=(190, 230)),
        "box_coarsen_4": dict(names=kept_names, time_coarsen=DW.TimeCoarsenConfig(4), **box),
        "jja_globe": dict(names=kept_names, time_selection=DW.MonthSelector(["JJA"])),
    }
    writers = {}
    for case, kw in cases.items():
        for fused in (True, False):
            w = DW.FileWriterConfig(case, **kw).build(os.path.join(tmp.name, f"{case}{int(fused)}"), coords=coords)
            w.reducer.fused = fused
            writers[f"{case}_{'fused' if fused else 'torch'}"] = w
    times = {k: [] for k in writers}
    moved = {k: [] for k in writers}
    kept = {}
    last = {}

    def append(key, i):
        w = writers[key]
        before = w.reducer.bytes_to_host
        w.append_batch(data, time=axis[:, 1 + i * T:1 + (i + 1) * T])
        moved[key].append(w.reducer.bytes_to_host - before)
        last[key] = w._records[-1]
        kept[key] = tuple(next(iter(last[key].values())).shape)
        w._records.clear()                                          # the window's cost is what is timed, not a year on the host
        w._times.clear()
    for i in range(args.warmup):
        for key in writers:
            append(key, i)                                            # untimed: tables, staging, pinned memory, code objects
    for i in range(args.warmup, n_windows):                           # alternated: every writer sees the same machine state
        for key in writers:
            times[key].append(timed(lambda: append(key, i), dev))
    routes = {k: w.reducer.last_path for k, w in writers.items()}
    agree, exact = {}, {}
    for case in cases:
        f, t = last[case + "_fused"], last[case + "_torch"]
        agree[case] = all(torch.equal(f[n].view(torch.int32), t[n].view(torch.int32)) for n in kept_names)
        b, n_kept, h, w_ = kept[case + "_fused"]
        exact[case] = len(kept_names) * b * n_kept * h * w_ * 4
        assert all(m == exact[case] for m in moved[case + "_fused"]), (case, moved[case + "_fused"], exact[case])
        assert routes[case + "_fused"] == "fused" and routes[case + "_torch"] == "torch"

    # the kernel alone: means only, through the reducer's own tables
    lib = _lib.lib()
    kernel, traffic = {}, {}
    for case in cases:
        wr = writers[case + "_fused"]
        red, f = wr.reducer, wr._factor
        region = red.region or (0, H, 0, W)
        n_kept = kept[case + "_fused"][1]
        N = len(kept_names)
        base = red._table.data_ptr()
        rows_at = base + 8 * 3 * N
        runs = []
        for _ in range(args.iters + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                rc = lib.ace_diag_region_segments(base, base + 8 * N, rows_at, rows_at + 4 * N, None, red._dev["means"].data_ptr(),
                                                  N, n_kept, N, 1, T, H, W, *region, _lib.current_stream())
            b.record()
            torch.cuda.synchronize(dev)
            assert rc == 0, lib.ace_diag_last_error().decode()
            runs.append(a.elapsed_time(b) / args.launches)
        kernel[case] = [round(x, 5) for x in runs[1:]]
        src_steps = n_kept * f
        requested = N * src_steps * region[1] * region[3] * 4
        traffic[case] = {"requested_bytes": requested, "written_bytes": exact[case],
                         "bytes_of_touched_64B_lines": touched_bytes(region, src_steps, N, 64),
                         "bytes_of_touched_128B_lines": touched_bytes(region, src_steps, N, 128)}
    med = lambda v: float(np.median(v))                                  # noqa: E731
    result = {
        "workload": f"file writers: 1 degree {H}x{W}, B=1, T={T} six-hourly steps, {len(names)} names in the window, "
                    f"{len(kept_names)} kept",
        "device": torch.cuda.get_device_name(0),
        "window_bytes": len(names) * T * H * W * 4,
        "cases": {k: {kk: (vv.__dict__ if dataclasses_like(vv) else vv) for kk, vv in kw.items()} for k, kw in cases.items()},
        "kept_record_shape": {c: list(kept[c + "_fused"]) for c in cases},
        "append_batch_ms": {k: round(med(v), 3) for k, v in times.items()},
        "append_batch_all_ms": {k: [round(x, 3) for x in v] for k, v in times.items()},
        "torch_over_fused": {c: round(med(times[c + "_torch"]) / med(times[c + "_fused"]), 2) for c in cases},
        "bytes_to_host_per_window": {k: int(np.median(v)) for k, v in moved.items()},
        "bytes_to_host_fused_exact_names_B_kept_h_w_4": exact,
        "kept_bytes_over_window_bytes": {c: round(exact[c] / (len(names) * T * H * W * 4), 5) for c in cases},
        "route": routes,
        "fused_and_torch_agree_bitwise": agree,
        "kernel_alone_ms_means_only": {c: round(med(v), 5) for c, v in kernel.items()},
        "kernel_alone_all_ms": kernel,
        "traffic_counted_from_shapes": traffic,
        "timing": "median of --iters host-synchronised append_batch calls per writer, the writers alternated call by call, after "
                  "--warmup untimed calls each; the kernel alone between device events around --launches back-to-back launches, "
                  "per launch, median of --iters after one untimed round",
    }
    tmp.cleanup()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


def dataclasses_like(v):
    import dataclasses
    return dataclasses.is_dataclass(v) and not isinstance(v, type)


if __name__ == "__main__":
    main()
