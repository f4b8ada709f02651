"""The contract of ``ace_diag_region_segments`` (include/ace_sfno.h) in plain numpy fp64, written from the header: for plane j, sample
b, segment s and region pixel (i, k), with lo / hi the two bounds of segment s of sample b, each clamped to [0, steps]:  acc = 0.0;
for t ascending from lo to hi - 1: acc += (double)x[b][t][lat0 + i][lon0 + k];  sums[rows[j]][b][s][i][k] = acc and means[...] =
(float)(acc / (double)(hi - lo)), NaN for an empty segment (hi <= lo).  Segments need not touch and may overlap.  A plane that is
``None`` or whose row is out of range writes nothing.  tests/test_region_ref_cpu.py holds this statement to tests/_timeseg_ref.py."""
import numpy as np


def region_segments(planes, rows, nrows, bounds, region, sums=None, means=None):
    """planes: list of (B, T, nlat, nlon) fp32 arrays (or ``None``); bounds: int (B, nseg, 2); region: (lat0, nlat_r, lon0, nlon_r);
    sums / means: (nrows, B, nseg, nlat_r, nlon_r) arrays assigned in place (``None``: not produced).  Returns (sums, means)."""
    bounds = np.asarray(bounds, dtype=np.int64)
    nseg = bounds.shape[1]
    lat0, nlat_r, lon0, nlon_r = region
    for x, r in zip(planes, rows):
        if x is None or r < 0 or r >= nrows:
            continue
        B, T = x.shape[:2]
        assert 0 <= lat0 and 1 <= nlat_r and lat0 + nlat_r <= x.shape[2] and 0 <= lon0 and 1 <= nlon_r and lon0 + nlon_r <= x.shape[3]
        e = np.clip(bounds, 0, T)
        for b in range(B):
            for s in range(nseg):
                lo, hi = int(e[b, s, 0]), int(e[b, s, 1])
                acc = np.zeros((nlat_r, nlon_r), np.float64)
                with np.errstate(invalid="ignore"):                  # inf + -inf: NaN, as on the device
                    for t in range(lo, hi):
                        acc = acc + x[b, t, lat0:lat0 + nlat_r, lon0:lon0 + nlon_r].astype(np.float64)
                if sums is not None:
                    sums[r, b, s] = acc
                if means is not None:
                    with np.errstate(invalid="ignore", divide="ignore"):
                        means[r, b, s] = (acc / np.float64(max(hi - lo, 0))).astype(np.float32)
    return sums, means


def bounds_of_edges(edges):
    """the bounds table of touching segments: (B, nseg + 1) edges -> (B, nseg, 2)"""
    edges = np.asarray(edges, dtype=np.int64)
    return np.stack([edges[:, :-1], edges[:, 1:]], axis=-1)
