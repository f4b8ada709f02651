"""A plain fp64 statement of what include/ace_sfno.h promises for ``ace_diag_paired_window``, written from the header and the
reference's formulas (fme/core/metrics.py:63-224 weighted_mean / weighted_std / weighted_mean_bias / root_mean_squared_error /
gradient_magnitude_percent_diff with weighted_nanmean; the zonal nan-mean of fme/core/distributed/non_distributed.py:136-137; the
time sums of fme/ace/aggregator/inference/time_mean.py:103-124), not from the kernel.  CPU only; tests/test_diag_paired_ref_cpu.py
pins it against the evaluator aggregator's torch path run in fp64.

Inputs are fp32: their widenings, the products ``w * x`` and the differences of the gradient stencils are exact in fp64, and sums of
planes of at most ``_diag_ref.FSUM_LIMIT`` pixels are correctly rounded (``math.fsum``)."""
import math
from typing import Optional, Sequence

import torch

from _diag_ref import NAN, _sum, moments_ref

NSERIES = 6          # mean gen, std gen, mean target, bias, rmse, gradient-magnitude percent diff


def grad_mag_mean_ref(x: torch.Tensor, w: torch.Tensor):
    """the weighted nan-mean of sqrt(gy^2 + gx^2), torch.gradient with unit spacing (one-sided at all four edges, no wrap), over
    the pixels of non-zero weight whose gradient is not NaN"""
    gy, gx = torch.gradient(x.double(), dim=(-2, -1))
    g = torch.sqrt(gy * gy + gx * gx).reshape(-1)
    w = w.reshape(-1).double()
    keep = (w != 0) & ~torch.isnan(g)
    if not bool(keep.any()):
        return NAN
    return _sum(w[keep] * g[keep]) / _sum(w[keep])


def sample_ref(x: torch.Tensor, y: Optional[torch.Tensor], w: torch.Tensor):
    """the six per-sample values of one (H, W) pair and the natural scale of each one's error bar"""
    m, s, a = moments_ref(x, w)
    vals, scale = [m, s, NAN, NAN, NAN, NAN], [a, abs(m), NAN, NAN, NAN, NAN]
    if y is None:
        return vals, scale
    wf, keep = w.reshape(-1).double(), w.reshape(-1) != 0
    if not bool(keep.any()):
        return vals, scale
    xd, yd, wk = x.reshape(-1).double()[keep], y.reshape(-1).double()[keep], wf[keep]
    wsum = _sum(wk)
    d = xd - yd
    vals[2], scale[2] = _sum(wk * yd) / wsum, _sum(wk * yd.abs()) / wsum
    vals[3], scale[3] = _sum(wk * d) / wsum, _sum(wk * d.abs()) / wsum
    vals[4] = math.sqrt(_sum(wk * d * d) / wsum)
    scale[4] = vals[4]
    gg, gt = grad_mag_mean_ref(x, w), grad_mag_mean_ref(y, w)
    vals[5] = 100.0 * (gg - gt) / gt if gt != 0 else (NAN if gg == gt or gg != gg else math.copysign(math.inf, gg - gt))
    scale[5] = 100.0 * (abs(gg) + abs(gt)) / abs(gt) if gt != 0 else NAN
    return vals, scale


def paired_window_ref(gen: Sequence[torch.Tensor], target: Sequence[Optional[torch.Tensor]], weights: torch.Tensor,
                      wrows: Sequence[int], rows: Sequence[int], B: int, T: int, t0: int, t_begin: int, do_maps: bool, zt0: int,
                      factor: int, series: torch.Tensor, tsum: Optional[torch.Tensor], zonal: Optional[torch.Tensor],
                      zbar: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``gen[j]`` / ``target[j]`` (or None): (B, T, H, W) fp32 (any strides); ``weights``: (nw, H, W) fp32; ``series``: fp64
    (6, nrows, n_time), ``tsum``: fp64 (2, nrows, H * W), ``zonal``: fp64 (2, nrows, nslots, H), all updated in place; ``zbar``
    (like ``zonal``) accumulates the row nan-means of |x| / (B * factor), the scale of zonal's error bar.  Returns the
    (6, nplanes, T) scales of the series entries' error bars (NaN where an entry has none)."""
    nrows, nw = series.shape[1], weights.shape[0]
    scale = torch.full((NSERIES, len(gen), T), NAN, dtype=torch.float64)
    for j, f in enumerate(gen):
        r, wr = int(rows[j]), int(wrows[j])
        if not (0 <= r < nrows and 0 <= wr < nw):
            continue                                    # contributes to nothing
        y = target[j]
        for t in range(T):
            tot, sc = [0.0] * NSERIES, [0.0] * NSERIES
            for b in range(B):                           # batch mean in sample order
                v, s = sample_ref(f[b, t], None if y is None else y[b, t], weights[wr])
                tot = [a + c for a, c in zip(tot, v)]
                sc = [a + c for a, c in zip(sc, s)]
            for k in range(NSERIES if y is not None else 2):
                series[k, r, t0 + t] += tot[k] / B
                scale[k, j, t] = sc[k] / B
        if not do_maps:
            continue
        for side, x in enumerate((f, y)):
            if x is None:
                continue
            acc = torch.zeros(f.shape[-2] * f.shape[-1], dtype=torch.float64)
            for b in range(B):
                for t in range(T):
                    if t >= t_begin:
                        acc += x[b, t].reshape(-1).double()
                    slot = (zt0 + t) // factor
                    if slot < zonal.shape[2]:
                        xd = x[b, t].double()
                        zonal[side, r, slot] += xd.nanmean(dim=-1) / (B * factor)
                        if zbar is not None:
                            zbar[side, r, slot] += xd.abs().nanmean(dim=-1).nan_to_num(0.0) / (B * factor)
            tsum[side, r] += acc
    return scale


def paired_series_errors(got: torch.Tensor, ref: torch.Tensor, bar: torch.Tensor):
    """The largest error of each of the six series as a multiple of its bar, 1e-12 * its natural scale (mean gen: wmean |x|; std:
    itself, plus 1e-14 |wmean x|; mean target: wmean |y|; bias: wmean |d|; rmse: itself; percent diff: 100 (G + Gt) / Gt, the
    two gradient means' relative errors carried through the quotient); <= 1 passes.  NaNs must be in the same places."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if not torch.equal(torch.isnan(got), torch.isnan(ref)):
        return [math.inf] * NSERIES
    lim = 1e-12 * bar.clone()
    lim[1] = 1e-12 * ref[1].abs() + 1e-14 * bar[1]
    out = []
    for k in range(NSERIES):
        ok = ~torch.isnan(ref[k]) & ~torch.isinf(ref[k])
        err = (got[k] - ref[k]).abs()
        ratio = torch.where(ok & (err > 0), err / lim[k].nan_to_num(0.0).clamp_min(1e-320), torch.zeros_like(err))
        out.append(float(ratio.max()) if ratio.numel() else 0.0)
    return out


def add_paired_scale(bar: torch.Tensor, scale: torch.Tensor, rows: Sequence[int], t0: int) -> None:
    for j, r in enumerate(rows):
        if 0 <= int(r) < bar.shape[1]:
            bar[:, int(r), t0:t0 + scale.shape[2]] += scale[:, j].nan_to_num(0.0)
