"""The contract of ``ace_diag_time_segments`` (include/ace_sfno.h) in plain numpy fp64, written from the header: for plane j, sample
b, segment s and pixel p, with lo / hi the edges s and s + 1 of sample b clamped to [0, steps]:  acc = 0.0;  for t ascending from lo
to hi - 1: acc += (double)x[b][t][p];  sums[rows[j]][b][s][p] = acc and means[...] = (float)(acc / (double)(hi - lo)), NaN for an empty
segment.  A plane whose row is out of range writes nothing.  tests/test_timeseg_ref_cpu.py holds this statement to the reference."""
import numpy as np


def time_segments(planes, rows, nrows, edges, sums=None, means=None):
    """planes: list of (B, T, hw) fp32 arrays; edges: int (B, nseg + 1); sums / means: (nrows, B, nseg, hw) arrays assigned in
    place (``None``: not produced).  Returns (sums, means)."""
    edges = np.asarray(edges, dtype=np.int64)
    nseg = edges.shape[1] - 1
    for x, r in zip(planes, rows):
        if x is None or r < 0 or r >= nrows:
            continue
        B, T, hw = x.shape
        e = np.clip(edges, 0, T)
        for b in range(B):
            for s in range(nseg):
                lo, hi = int(e[b, s]), int(e[b, s + 1])
                acc = np.zeros(hw, np.float64)
                with np.errstate(invalid="ignore"):                  # inf + -inf: NaN, as on the device
                    for t in range(lo, hi):
                        acc = acc + x[b, t].astype(np.float64)
                if sums is not None:
                    sums[r, b, s] = acc
                if means is not None:
                    with np.errstate(invalid="ignore", divide="ignore"):
                        means[r, b, s] = (acc / np.float64(max(hi - lo, 0))).astype(np.float32)
    return sums, means


def block_edges(B, T, factor):
    """the edge table of the time coarsening: blocks of ``factor`` steps"""
    return np.broadcast_to(np.arange(0, T + 1, factor), (B, T // factor + 1)).copy()


def month_edges(months):
    """the edge table of the monthly writer for the month indices (B, T) of a window, ascending along T: (month_min, edges), segment
    s the steps of month month_min + s"""
    months = np.asarray(months)
    lo, hi = int(months.min()), int(months.max())
    want = lo + np.arange(hi - lo + 2)
    return lo, np.stack([np.searchsorted(row, want, side="left") for row in months])
