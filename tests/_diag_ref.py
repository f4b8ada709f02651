"""A plain fp64 statement of what include/ace_sfno.h promises for ``ace_diag_window`` and ``ace_diag_spectrum``, written from the
header and the reference's formulas (fme/core/metrics.py weighted_mean / weighted_std / spherical_power_spectrum,
fme/ace/aggregator/inference/time_mean.py), not from the kernels.  CPU only; tests/test_diag_ref_cpu.py pins it against the
aggregator's torch path run in fp64.

Inputs are fp32 (complex64) tensors: their widenings to fp64, the products ``w * x`` and the squares are exact in fp64, so the only
errors of this module are the roundings of the sums.  Planes of at most ``FSUM_LIMIT`` pixels are summed with ``math.fsum``
(correctly rounded); larger ones with torch's pairwise fp64 sums (about log2(n) roundings)."""
import math
from typing import Optional, Sequence, Tuple

import torch

FSUM_LIMIT = 100_000
NAN = float("nan")


def _sum(v: torch.Tensor) -> float:
    return math.fsum(v.tolist()) if v.numel() <= FSUM_LIMIT else float(v.sum())


def moments_ref(x: torch.Tensor, w: torch.Tensor) -> Tuple[float, float, float]:
    """(weighted mean, weighted std sqrt(wmean((x - wmean x)^2)), weighted mean of |x|) of one plane over its pixels of non-zero
    weight; all NaN when there is none (the reference's 0 / 0)."""
    x, w = x.reshape(-1).double(), w.reshape(-1).double()
    keep = w != 0
    if not bool(keep.any()):
        return NAN, NAN, NAN
    x, w = x[keep], w[keep]
    wsum = _sum(w)
    mean = _sum(w * x) / wsum
    d = x - mean
    var = _sum(w * d * d) / wsum
    return mean, math.sqrt(var), _sum(w * x.abs()) / wsum


def window_ref(fields: Sequence[torch.Tensor], weights: torch.Tensor, wrows: Sequence[int], rows: Sequence[int], B: int, T: int,
               t0: int, t_begin: int, do_tsum: bool, series: torch.Tensor, tsum: Optional[torch.Tensor]) -> torch.Tensor:
    """``fields[j]``: (B, T, hw) fp32 (any strides); ``weights``: (nw, hw) fp32; ``series``: fp64 (2, nrows, n_time) and ``tsum``:
    fp64 (nrows, hw), both updated in place.  Returns the (2, nplanes, T) scale of each series entry's error bar: the batch mean of
    the weighted mean of |x| (0) and of |weighted mean| (1); NaN where the series entry is NaN."""
    nrows, nw = series.shape[1], weights.shape[0]
    scale = torch.full((2, len(fields), T), NAN, dtype=torch.float64)
    for j, f in enumerate(fields):
        r, wr = int(rows[j]), int(wrows[j])
        if not (0 <= r < nrows and 0 <= wr < nw):
            continue                                    # contributes to nothing
        assert f.dtype == torch.float32 and tuple(f.shape[:2]) == (B, T)
        for t in range(T):
            sm = ss = sa = sabs = 0.0
            for b in range(B):                           # batch mean in sample order
                m, s, a = moments_ref(f[b, t], weights[wr])
                sm, ss, sa, sabs = sm + m, ss + s, sa + a, sabs + abs(m)
            series[0, r, t0 + t] += sm / B
            series[1, r, t0 + t] += ss / B
            scale[0, j, t], scale[1, j, t] = sa / B, sabs / B
        if do_tsum:
            acc = torch.zeros(f.shape[-1], dtype=torch.float64)
            for b in range(B):
                for t in range(t_begin, T):
                    acc += f[b, t].double()
            tsum[r] += acc
    return scale


def add_scale(bar: torch.Tensor, scale: torch.Tensor, rows: Sequence[int], t0: int) -> None:
    """accumulate ``window_ref``'s scales into ``bar`` (2, nrows, n_time), laid out as the series"""
    for j, r in enumerate(rows):
        if 0 <= int(r) < bar.shape[1] and not bool(torch.isnan(scale[:, j]).all()):
            bar[:, int(r), t0:t0 + scale.shape[2]] += scale[:, j]


def series_errors(got: torch.Tensor, ref: torch.Tensor, bar: torch.Tensor) -> Tuple[float, float]:
    """The largest error of the means and of the stds as multiples of their bars: ``|got - ref| / (1e-12 * sum w|x| / sum w)`` and
    ``|got - ref| / (1e-12 * ref + 1e-14 * |wmean|)``; <= 1 passes.  NaNs must be in the same places (else inf)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if not torch.equal(torch.isnan(got), torch.isnan(ref)):
        return math.inf, math.inf
    ok = ~torch.isnan(ref)
    err = (got - ref).abs()
    lim = torch.stack([1e-12 * bar[0], 1e-12 * ref[1].abs() + 1e-14 * bar[1]])
    ratio = torch.where(ok & (err > 0), err / lim.clamp_min(1e-320), torch.zeros_like(err))
    return float(ratio[0].max()), float(ratio[1].max())


def spectrum_ref(coeffs: torch.Tensor, rows: Sequence[int], spec: torch.Tensor) -> None:
    """``coeffs``: complex (nnames, planes, L, M); ``spec``: fp64 (nrows, L), ``spec[rows[j]][l] += sum over planes, m of re^2 +
    im^2`` in place."""
    nrows = spec.shape[0]
    for j in range(coeffs.shape[0]):
        r = int(rows[j])
        if not 0 <= r < nrows:
            continue
        c = torch.view_as_real(coeffs[j].to(torch.complex128))              # (planes, L, M, 2)
        p = (c * c).permute(1, 0, 2, 3).reshape(c.shape[1], -1)            # squares of fp32 values: exact
        for l in range(p.shape[0]):
            spec[r, l] += _sum(p[l])


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """fp64 tensors equal bit for bit, NaNs in the same places."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    if a.shape != b.shape or not torch.equal(na, nb):
        return False
    zero = torch.zeros((), dtype=a.dtype)
    return torch.equal(torch.where(na, zero, a).view(torch.int64), torch.where(nb, zero, b).view(torch.int64))
