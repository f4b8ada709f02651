"""A plain numpy statement of what include/ace_sfno.h promises for ``ace_diag_hist_window``, written from the header: one dynamic
histogram per (side, row).  tests/test_hist_ref_cpu.py holds it to the reference's own ComparedDynamicHistograms
(tests/golden/gen_histogram.pt) bitwise; the GPU kernel tests are judged by it."""
import numpy as np

EPS = np.float32(1.0e-6)


class Hist:
    def __init__(self, n_bins: int):
        self.n = int(n_bins)
        self.lo = self.hi = float("nan")
        self.counts = np.zeros(self.n, dtype=np.int64)
        self.dropped = 0

    def add(self, values) -> bool:
        """one window's unmasked values (fp32, any shape); False when the window is dropped"""
        v = np.asarray(values, dtype=np.float32).ravel()
        if v.size == 0 or not np.isfinite(v).all():
            self.dropped += 1
            return False
        with np.errstate(all="ignore"):
            vmin, vmax = float(np.float32(v.min() - EPS)), float(np.float32(v.max() + EPS))      # step 1: the epsilon in fp32
            lo, hi, nleft, nright = self.lo, self.hi, 0, 0
            if not (np.isfinite(vmin) and np.isfinite(vmax)):
                self.dropped += 1
                return False
            if np.isnan(lo):                                                                    # step 2
                lo, hi = vmin, vmax
            else:
                while vmin < lo:
                    lo, nleft = hi - 2.0 * (hi - lo), nleft + 1
                while vmax > hi:
                    hi, nright = lo + 2.0 * (hi - lo), nright + 1
            step = (hi - lo) / self.n                                                           # step 3
            flo, fbin = np.float32(lo), np.float32((lo + step) - lo)
            if not (fbin > 0 and np.isfinite(fbin) and np.isfinite(flo)):
                self.dropped += 1
                return False
            c, half = self.counts, self.n // 2
            for i in range(nleft + nright):
                merged, c = c[0::2] + c[1::2], np.zeros(self.n, dtype=np.int64)
                if i < nleft:
                    c[half:] = merged
                else:
                    c[:half] = merged
            q = (v - flo) / fbin                                                                # step 4, fp32 throughout
            assert q.dtype == np.float32
            idx = np.where(~(q < np.float32(self.n)), self.n - 1, np.where(q < 0, 0, np.trunc(np.clip(q, 0, self.n)))).astype(np.int64)
        self.lo, self.hi, self.counts = lo, hi, c + np.bincount(idx, minlength=self.n)
        return True

    @property
    def edges(self) -> np.ndarray:
        return np.linspace(self.lo, self.hi, self.n + 1)


def trim_zero_bins(counts, edges):
    """fme/core/histogram.py:52-71"""
    nz = np.nonzero(counts > 0)[0]
    return counts[nz[0]:nz[-1] + 1], edges[nz[0]:nz[-1] + 2]


def quantile(edges, counts, probability: float) -> float:
    """fme/core/metrics.py:355-385"""
    cdf = np.concatenate([[0.0], np.cumsum(counts) / np.sum(counts)])
    i = int(np.argmax(cdf > probability)) - 1
    return float(edges[i] + (edges[i + 1] - edges[i]) * (probability - cdf[i]) / (cdf[i + 1] - cdf[i]))


def percentile(h: Hist, p: float = 99.9999) -> float:
    c, e = trim_zero_bins(h.counts, h.edges)
    return quantile(e, c, p / 100.0)
