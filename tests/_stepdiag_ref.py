"""TEST INFRASTRUCTURE: a numpy fp64 statement of the three contracts of csrc/stepdiag.hip (include/ace_sfno.h, "Corrector step
diagnostics"): the snapshot copy, the in-place fp32 delta and the correction metrics of a window of deltas."""
import numpy as np


def snapshot(src: np.ndarray) -> np.ndarray:
    return np.array(src, dtype=np.float32, copy=True)


def delta(out: np.ndarray, snap: np.ndarray) -> np.ndarray:
    """fl32(out - snap): one IEEE fp32 subtraction per element"""
    return (out.astype(np.float32) - snap.astype(np.float32)).astype(np.float32)


def normalised(d: np.ndarray, std) -> np.ndarray:
    """n = fl32(d / std), the correctly rounded fp32 quotient, widened to fp64"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (d.astype(np.float32) / np.float32(std)).astype(np.float64)


def correction_window(deltas, stds, rows, wrows, weights, signed, magnitude, series, t0):
    """deltas: per plane j a (B, T, hw) fp32 array; weights (nw, hw) fp32; signed, magnitude (nrows, hw) and series
    (2, nrows, n_time) fp64, updated in place as ``ace_diag_correction_window`` updates them."""
    nrows, nw = signed.shape[0], weights.shape[0]
    for j, d in enumerate(deltas):
        r, wr = int(rows[j]), int(wrows[j])
        if not (0 <= r < nrows and 0 <= wr < nw):
            continue
        n = normalised(d, stds[j])
        B, T, hw = n.shape
        w = weights[wr].astype(np.float64)
        sel = w != 0
        acc_n, acc_a = np.zeros(hw), np.zeros(hw)
        for b in range(B):                       # b outer, t inner, one running accumulator
            for t in range(T):
                acc_n = acc_n + n[b, t]
                acc_a = acc_a + np.abs(n[b, t])
        signed[r] += acc_n
        magnitude[r] += acc_a
        ww = w[sel]
        for t in range(T):
            sa = ss = 0.0
            for b in range(B):
                x = n[b, t][sel]
                if ww.size == 0:
                    a = s = np.nan
                else:
                    m = (ww * x).sum() / ww.sum()
                    a = (ww * np.abs(x)).sum() / ww.sum()
                    s = np.sqrt((ww * (x - m) ** 2).sum() / ww.sum())
                sa, ss = sa + a, ss + s
            series[0, r, t0 + t] += sa / B
            series[1, r, t0 + t] += ss / B
