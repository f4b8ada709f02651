#!/usr/bin/env python
"""The data writers (ace_amd/data_writer.py, csrc/timeseg.hip) at 1 degree 180 x 360, 50 names, B = 1, T = 40 six-hourly steps per
window, on one MI355X: ``append_batch`` per window of
  * ``TensorFileWriter`` alone - every step of every name copied to the host, the only writer there was;
  * ``MonthlyDataWriter``, fused (one ace_diag_time_segments per window, then one copy of the reduced record) and on the torch path;
  * ``TimeCoarsen(4)`` over a writer that drops what it is handed, fused and on the torch path;
alternated call by call on the same device, in ms per window with host syncs around each call after --warmup untimed windows, and
the bytes each moved to the host per window.  The kernel alone (sums and means of blocks of 4 steps, no copy) is timed with device
events around the C call; the traffic bound is one read of the window (names x T planes of 259 KB) at the HBM peak of
MI355X_MICROARCH (8 TB/s), the achieved fraction the bound over the kernel time.  No time is a target.
Writes one JSON file and prints it.  usage: python tools/bench_data_writer.py [--steps 40] [--names 50] [--iters 15] [--warmup 3] [--out ...]"""
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

HBM_PEAK = 8.0e12              # bytes / s
H, W = 180, 360
STEP = datetime.timedelta(hours=6)
ROLLOUT_WINDOW_MS = 200.9      # the 40-step rollout window README.md quotes


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


class Drop:
    def append_batch(self, batch):
        pass


@torch.no_grad()
def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--names", type=int, default=50)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3, help="untimed windows per writer before the timed ones")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_writer_bench.json"))
    args = ap.parse_args(argv)
    from ace_amd import _lib
    from ace_amd import data_writer as DW
    from ace_amd.inference import TensorFileWriter
    from ace_amd.timeaxis import TimeAxis

    dev = torch.device("cuda", 0)
    T, names = args.steps, [f"v{i:02d}" for i in range(args.names)]
    g = torch.Generator(device=dev).manual_seed(0)
    data = {n: torch.randn(1, T, H, W, generator=g, device=dev) for n in names}
    window_bytes = len(names) * T * H * W * 4
    n_windows = args.iters + args.warmup
    axis = TimeAxis.regular((2001, 1, 1), STEP, 1 + n_windows * T)
    tmp = tempfile.TemporaryDirectory()

    def monthly(fused):
        w = DW.MonthlyDataWriter(os.path.join(tmp.name, f"m{int(fused)}"), "monthly_mean_predictions")
        w.reducer.fused = fused
        return w

    def coarsen(fused):
        w = DW.TimeCoarsen(Drop(), 4)
        w.reducer.fused = fused
        return w

    raw = TensorFileWriter(os.path.join(tmp.name, "raw"))
    writers = {"tensor_file_writer": raw, "monthly_fused": monthly(True), "monthly_torch": monthly(False),
               "time_coarsen_4_fused": coarsen(True), "time_coarsen_4_torch": coarsen(False)}
    times = {k: [] for k in writers}
    moved = {k: [] for k in writers}

    def append(key, i):
        w = writers[key]
        if key == "tensor_file_writer":
            w.append_batch(data)
            moved[key].append(sum(x.numel() * 4 for x in w._windows[-1].values()))
            w._windows.clear()                                        # the host copy is what is timed, not the 19 GB of a year
            return
        before = w.reducer.bytes_to_host
        w.append_batch(data, time=axis[:, 1 + i * T:1 + (i + 1) * T])
        moved[key].append(w.reducer.bytes_to_host - before)
    for i in range(args.warmup):
        for key in writers:
            append(key, i)                                            # untimed: tables, staging, pinned memory, code objects
    for i in range(args.warmup, n_windows):                           # alternated: every writer sees the same machine state
        for key in writers:
            times[key].append(timed(lambda: append(key, i), dev))
    routes = {k: getattr(getattr(w, "reducer", None), "last_path", None) for k, w in writers.items()}
    mf, mt = writers["monthly_fused"], writers["monthly_torch"]
    monthly_equal = all(torch.equal(mf._totals[n].view(torch.int64), mt._totals[n].view(torch.int64)) for n in names)

    # the kernel alone: blocks of 4 steps, sums and means, through the reducer's own tables
    red = DW.SegmentReducer()
    edges = np.arange(0, T + 1, 4, dtype=np.int64)[None]
    red(data, names, edges)
    nseg, N, HW = edges.shape[1] - 1, len(names), H * W
    base = red._table.data_ptr()
    rows_at = base + 8 * 3 * N
    lib = _lib.lib()
    kernel = []
    for _ in range(args.iters + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = lib.ace_diag_time_segments(base, base + 8 * N, rows_at, rows_at + 4 * N, red._dev["sums"].data_ptr(),
                                        red._dev["means"].data_ptr(), N, nseg, N, 1, T, HW, _lib.current_stream())
        b.record()
        torch.cuda.synchronize(dev)
        assert rc == 0, lib.ace_diag_last_error().decode()
        kernel.append(a.elapsed_time(b))
    kernel_ms = float(np.median(kernel[1:]))
    written = N * nseg * HW * 12
    result = {
        "workload": f"data writers: 1 degree {H}x{W}, B=1, T={T} six-hourly steps, {len(names)} names",
        "device": torch.cuda.get_device_name(0),
        "window_bytes": window_bytes,
        "append_batch_ms": {k: round(float(np.median(v)), 3) for k, v in times.items()},
        "append_batch_all_ms": {k: [round(x, 3) for x in v] for k, v in times.items()},
        "append_batch_fraction_of_the_rollout_window": {k: round(float(np.median(v)) / ROLLOUT_WINDOW_MS, 4) for k, v in times.items()},
        "rollout_window_ms_quoted_in_README": ROLLOUT_WINDOW_MS,
        "bytes_to_host_per_window_median": {k: int(np.median(v)) for k, v in moved.items()},
        "bytes_to_host_whole_run": {k: int(np.sum(v)) for k, v in moved.items()},
        "route": routes,
        "monthly_totals_fused_and_torch_agree_bitwise": monthly_equal,
        "torch_over_fused": {k: round(float(np.median(times[k + "_torch"])) / float(np.median(times[k + "_fused"])), 2)
                             for k in ("monthly", "time_coarsen_4")},
        "kernel_alone_ms_blocks_of_4_sums_and_means": round(kernel_ms, 4),
        "kernel_alone_all_ms": [round(x, 4) for x in kernel[1:]],
        "kernel_bytes_written": written,
        "traffic_bound_ms_one_read_at_8TBps_peak": round(window_bytes / HBM_PEAK * 1e3, 4),
        "achieved_fraction_of_hbm_peak_reads_only": round(window_bytes / HBM_PEAK * 1e3 / kernel_ms, 3),
        "achieved_fraction_of_hbm_peak_reads_and_writes": round((window_bytes + written) / HBM_PEAK * 1e3 / kernel_ms, 3),
        "timing": "median of --iters host-synchronised append_batch calls per writer, the writers alternated call by call, after "
                  "--warmup untimed calls each; the kernel alone between device events, median of --iters after one untimed launch",
    }
    tmp.cleanup()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
