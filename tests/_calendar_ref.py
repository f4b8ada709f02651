"""The header contract of ``ace_diag_calendar_window`` (include/ace_sfno.h) in plain numpy fp64, written from the header: the binned
sums in the stated order (b, then t; a step added to its own bin only, nothing multiplied) and the regional series (mode 0: the
fp32 product of region and weight row, zero-weight pixels out, NaN propagating; mode 1: the region alone, NaN pixels out).  The
pixel sums of the series are numpy's, in another order than the kernel's waves: the GPU tests allow 1e-12 of ``series_scale``.
tests/test_calendar_ref_cpu.py holds it to the reference's formulas; the GPU tests hold the kernel to it."""
import numpy as np


def _taking_part(x, j, rows, nrows):
    return x is not None and 0 <= rows[j] < nrows


def calendar_window(gen, target, rows, nrows, bin=None, nbins=0, bins=None, regions=None, srow=None, mode=None, weights=None,
                    wrows=None, series=None, t0=0, t_begin=0, scale=None):
    """One call, in place on ``bins`` (2, nrows, nbins, hw) fp64 and ``series`` (2, nsrows, B, n_time) fp64 (either may be None:
    that part is off).  gen / target: lists of (B, T, hw) fp32 arrays, a target entry may be None.  bin (B, T) int; regions
    (nreg, hw) fp32, srow (nplanes, nreg) int, mode (nreg,) int; weights (nw, hw) fp32, wrows (nplanes,) int.  ``scale``, when
    given, has the shape of ``series`` and receives sum |w x| / sum w of every assigned entry."""
    for side, planes in enumerate((gen, target)):
        for j, x in enumerate(planes):
            if not _taking_part(x, j, rows, nrows):
                continue
            x = np.asarray(x, dtype=np.float32)
            B, T, hw = x.shape
            xd = x.astype(np.float64)
            if bins is not None:
                for m in range(nbins):
                    acc = np.zeros(hw, dtype=np.float64)
                    for b in range(B):
                        for t in range(t_begin, T):
                            if bin[b, t] == m:
                                with np.errstate(all="ignore"):
                                    acc = acc + xd[b, t]
                    if t_begin < T:
                        with np.errstate(all="ignore"):
                            bins[side, rows[j], m] += acc
            if series is None or regions is None or not 0 <= wrows[j] < weights.shape[0]:
                continue
            for r in range(regions.shape[0]):
                s = srow[j][r]
                if not 0 <= s < series.shape[1]:
                    continue
                reg = np.asarray(regions[r], dtype=np.float32)
                w = reg if mode[r] == 1 else reg * np.asarray(weights[wrows[j]], dtype=np.float32)      # the product in fp32
                wd = w.astype(np.float64)
                for b in range(B):
                    for t in range(t_begin, T):
                        take = w != 0
                        if mode[r] == 1:
                            take = take & ~np.isnan(x[b, t])
                        with np.errstate(all="ignore"):
                            num, den = (wd[take] * xd[b, t][take]).sum(), wd[take].sum()
                            series[side, s, b, t0 + t] = num / den
                            if scale is not None:
                                scale[side, s, b, t0 + t] = np.abs(wd[take] * np.nan_to_num(xd[b, t][take], nan=0.0, posinf=0.0,
                                                                                              neginf=0.0)).sum() / np.abs(den)
