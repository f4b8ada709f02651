"""The header contract of ``ace_diag_regress_window`` (include/ace_sfno.h) in plain numpy fp64, written from the header: the maps in
the stated order (k, then b, then t; product rounded, then added), the integer below-eps counts and the area-weighted fractions.
tests/test_regress_ref_cpu.py holds it to the reference's formulas; the GPU tests hold the kernel to it."""
import numpy as np


def regress_window(gen, target, rows, nrows, coef=None, slot=None, nmaps=0, maps=None, eps=None, weights=None, wrows=None,
                   below_count=None, below_frac=None, t_begin=0):
    """One call, in place on ``maps`` (2, nrows, nmaps, hw) fp64, ``below_count`` (2, nrows, hw) int64 and ``below_frac`` (2, nrows)
    fp64.  gen / target: lists of (B, T, hw) fp32 arrays, a target entry may be None.  coef (nterms, B, T) fp64, slot (nterms, B)
    int; eps: None (indicator off) or (nplanes,) fp32; weights (nw, hw) fp32, wrows (nplanes,) int."""
    nterms = 0 if coef is None else coef.shape[0]
    for side, planes in enumerate((gen, target)):
        for j, x in enumerate(planes):
            r = rows[j]
            if x is None or r < 0 or r >= nrows:
                continue
            x = np.asarray(x, dtype=np.float32)
            B, T, hw = x.shape
            if t_begin >= T:
                continue
            xd = x.astype(np.float64)
            if nterms > 0:
                for m in range(nmaps):
                    acc = np.zeros(hw, dtype=np.float64)
                    for k in range(nterms):
                        for b in range(B):
                            if slot[k, b] != m:
                                continue
                            for t in range(t_begin, T):
                                with np.errstate(all="ignore"):
                                    acc = acc + np.float64(coef[k, b, t]) * xd[b, t]
                    with np.errstate(all="ignore"):
                        maps[side, r, m] += acc
            if eps is not None and 0 <= wrows[j] < weights.shape[0]:
                w = np.asarray(weights[wrows[j]], dtype=np.float32)
                live = w != 0
                wd = w.astype(np.float64)
                den = wd[live].sum()
                f = np.float64(0.0)
                for b in range(B):
                    for t in range(t_begin, T):
                        below = x[b, t] <= np.float32(eps[j])                  # fp32 compare; NaN is not below
                        below_count[side, r] += below.astype(np.int64)
                        with np.errstate(all="ignore"):
                            f = f + wd[below & live].sum() / den
                below_frac[side, r] += f


def map_scale(planes, rows, nrows, coef, slot, nmaps, t_begin=0):
    """sum |c x| per (row, map, pixel) of one side: the scale the maps' error bar is a fraction of"""
    hw = next(x for x in planes if x is not None).shape[-1]
    out = np.zeros((nrows, nmaps, hw), dtype=np.float64)
    for j, x in enumerate(planes):
        if x is None or not 0 <= rows[j] < nrows:
            continue
        xd = np.abs(np.nan_to_num(np.asarray(x, dtype=np.float64), nan=0.0, posinf=0.0, neginf=0.0))
        for k in range(coef.shape[0]):
            for b in range(x.shape[0]):
                if 0 <= slot[k, b] < nmaps:
                    for t in range(t_begin, x.shape[1]):
                        out[rows[j], slot[k, b]] += abs(coef[k, b, t]) * xd[b, t]
    return out
