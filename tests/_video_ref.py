"""The contract of ``ace_diag_video_window`` (include/ace_sfno.h) in plain numpy fp64, written from the header: for plane j, step t,
slot u = t0 + t and pixel p, with g_b, y_b the fp32 values of sample b, d_b = g_b - y_b formed in fp32, everything else widened
to fp64 and every sum over b ascending from 0.0 with rounded products:
  mean[0][row][u] += (sum g_b) / B            mean[1][row][u] += (sum y_b) / B
  sq[0][row][u] += (sum g_b g_b) / B          sq[1][row][u] += (sum y_b y_b) / B          sq[2][row][u] += (sum d_b d_b) / B
  err[0][row][u] = min(err[0][row][u], min_b d_b)          err[1][row][u] = max(err[1][row][u], max_b d_b)
with NaN from any NaN on either side of a min or max; ``assign`` stores the window's values instead.  A plane without a target
updates mean[0] and sq[0] only, a plane whose row is out of range nothing.  ``derived`` states what ``dataset()`` of
ace_amd/evaluator/video.py forms from the accumulators (fme/ace/aggregator/inference/video.py:363-441).
tests/test_video_ref_cpu.py holds this statement to the reference."""
import numpy as np


def new_buffers(nrows, n_time, hw, extended=True):
    """(mean, sq, err) as the family allocates them: zeros, and +inf / -inf for the extrema"""
    mean = np.zeros((2, nrows, n_time, hw), np.float64)
    if not extended:
        return mean, None, None
    err = np.empty((2, nrows, n_time, hw), np.float32)
    err[0], err[1] = np.inf, -np.inf
    return mean, np.zeros((3, nrows, n_time, hw), np.float64), err


def _nan_min(a, b):
    return np.where(np.isnan(a) | np.isnan(b), np.float32(np.nan), np.minimum(a, b))


def _nan_max(a, b):
    return np.where(np.isnan(a) | np.isnan(b), np.float32(np.nan), np.maximum(a, b))


def video_window(gens, tgts, rows, mean, sq, err, t0, assign=False):
    """gens / tgts: lists of (B, T, hw) fp32 arrays (a target may be ``None``); mean / sq / err updated in place"""
    nrows = mean.shape[1]
    assert (sq is None) == (err is None)
    for g, y, r in zip(gens, tgts, rows):
        if g is None or r < 0 or r >= nrows:
            continue
        B, T, hw = g.shape
        sl = slice(t0, t0 + T)
        Bd = np.float64(B)

        def put(buf, c, total):
            with np.errstate(invalid="ignore"):
                buf[c, r, sl] = total / Bd if assign else buf[c, r, sl] + total / Bd

        def total(values):
            acc = np.zeros((T, hw), np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                for b in range(B):
                    acc = acc + values[b]
            return acc
        g64 = g.astype(np.float64)
        put(mean, 0, total(g64))
        if sq is not None:
            put(sq, 0, total(g64 * g64))
        if y is None:
            continue
        y64 = y.astype(np.float64)
        put(mean, 1, total(y64))
        if sq is None:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            d = (g - y).astype(np.float32)                           # the error in fp32
            d64 = d.astype(np.float64)
            put(sq, 1, total(y64 * y64))
            put(sq, 2, total(d64 * d64))
            mn, mx = np.full((T, hw), np.inf, np.float32), np.full((T, hw), -np.inf, np.float32)
            for b in range(B):
                mn, mx = _nan_min(mn, d[b]), _nan_max(mx, d[b])
            err[0, r, sl] = mn if assign else _nan_min(err[0, r, sl], mn)
            err[1, r, sl] = mx if assign else _nan_max(err[1, r, sl], mx)
    return mean, sq, err


def derived(mean, sq, err, row, n, paired=True):
    """the dataset variables of one name from its accumulators and the visit counts ``n`` (n_time,): ``name`` (2, n_time, hw)
    [prediction, target] and, with sq / err, ``bias``, ``rmse``, ``min_err``, ``max_err``, ``gen_var`` (n_time, hw)"""
    n = np.asarray(n, np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        gen = mean[0, row] / n
        tgt = mean[1, row] / n if paired else np.full_like(gen, np.nan)
        out = {"name": np.stack([gen, tgt])}
        if sq is not None and paired:
            out["bias"] = gen - tgt
            out["rmse"] = np.sqrt(sq[2, row] / n)
            out["min_err"] = err[0, row].astype(np.float64)
            out["max_err"] = err[1, row].astype(np.float64)
            out["gen_var"] = (sq[0, row] / n - gen ** 2) / (sq[1, row] / n - tgt ** 2)
    return out
