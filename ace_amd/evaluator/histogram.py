"""The ``histogram`` metric of the evaluator: the dynamic histograms' formulas and ``_Histograms``."""
import math
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from ..aggregator import _check, _upload, _upload_planes

HIST_BINS = 200                                                           # histogram.py:59
HIST_PERCENTILES = (99.9999,)


def trim_zero_bins(counts, edges):
    """fme/core/histogram.py:52-71: the empty bins at both ends removed"""
    mask = counts > 0
    first, last = int(np.argmax(mask)), len(mask) - int(np.argmax(mask[::-1]))
    return counts[first:last], edges[first:last + 1]


def histogram_quantile(edges, counts, probability: float) -> float:
    """fme/core/metrics.py:355-385: the inverse CDF, linear inside a bin"""
    cdf = np.cumsum(counts)
    cdf = np.insert(cdf / cdf[-1], 0, 0)
    i = int(np.argmax(cdf > probability)) - 1
    return float(edges[i] + (edges[i + 1] - edges[i]) * (probability - cdf[i]) / (cdf[i + 1] - cdf[i]))


class _Histograms:
    """ComparedDynamicHistograms(n_bins=200, percentiles=[99.9999]) (fme/core/histogram.py:336-509) behind the reference's
    HistogramAggregator and its ``variables`` filter (histogram.py:50-82, build_context.py:19-46): per paired name and side one
    dynamic histogram of every unmasked value of every window of ``record_batch``.  The statement both paths follow is the header
    contract of ``ace_diag_hist_window`` (include/ace_sfno.h): the range starts at (min - 1e-6, max + 1e-6) of the first window,
    doubles towards whichever side a later window overflows, pairs of bins merging, and a value goes to bin
    int((x - float(lo)) / float(bin)) with the division in fp32 - by a 0-dim tensor on the torch path, because torch on a GPU turns
    a division by a Python scalar into a multiplication by its reciprocal, which moves values across bin edges.

    The NaN mask of a name is the NaN pattern of the target's first sample and step at the first window, for both sides
    (fme/core/histogram.py:241-264); it is kept as a device plane and never reduced to a flag.  One difference from the reference:
    a window whose unmasked values hold a non-finite value, or whose range is degenerate in fp32, is skipped and counted
    (``dropped_windows``) at every window; the reference skips it once it has edges (fme/core/histogram.py:181-183) but on a first
    window keeps the poisoned edges.  The torch path reads minima, maxima and counts back per name, as the reference does; the
    fused path reads nothing back before ``dataset`` / ``logs``, which report nothing before the first window."""
    needs_time = uses_time = needs_norm = False
    counted = True                                                        # its calls are part of ``launches()``

    def __init__(self, config):
        self.label = config.name or "histogram"
        self._only = None if config.variables is None else frozenset(config.variables)
        self._pct_only = None if config.percentile_variables is None else set(config.percentile_variables)
        self._names: Optional[List[str]] = None
        self._masks: Dict[str, torch.Tensor] = {}                         # name -> bool (1, 1, H, W), True where removed
        self._host: Dict[str, List[Dict[str, Any]]] = {}                   # torch path: name -> [generated, target] states
        self._range = self._counts = self._dropped = self._mask_planes = self._table = None     # fused path

    @property
    def recorded(self) -> bool:
        return self._names is not None

    def _select(self, gen, tgt):
        """_check_overlapping_keys (fme/core/histogram.py:357-372) after the variable filter"""
        keep = lambda d: {k: v for k, v in d.items() if self._only is None or k in self._only}      # noqa: E731
        gen, tgt = keep(gen), keep(tgt)
        current = set(tgt).intersection(gen)
        if self._names is None:
            if not current:
                raise ValueError("No overlapping keys between target and prediction variables. "
                                 f"target: {tgt.keys()}, prediction: {gen.keys()}")
            self._names = sorted(current)
            for n in self._names:
                self._masks[n] = tgt[n][:1, :1].isnan()
        elif current != set(self._names):
            raise ValueError("Available comparison variables provided to record_batch differ from initial call to record_batch.  "
                             f"initial: {set(self._names)}, current: {current}")
        return gen, tgt

    def record(self, w) -> int:
        gen, tgt = self._select(w.gen, w.tgt)
        return self._record_fused(gen, tgt) if w.fused else self._record_torch(gen, tgt)

    # ---- the torch path -----------------------------------------------------------------------------------------------
    def _record_torch(self, gen, tgt) -> int:
        for n in self._names:
            states = self._host.setdefault(n, [{"lo": math.nan, "hi": math.nan, "counts": np.zeros(HIST_BINS, np.int64),
                                               "dropped": 0} for _ in range(2)])
            for st, x in zip(states, (gen[n], tgt[n])):
                v = torch.masked_select(x, ~self._masks[n].to(x.device).expand(x.shape))
                if v.numel() == 0 or not bool(torch.isfinite(v).all()):
                    st["dropped"] += 1
                    continue
                vmin, vmax = float(v.min() - 1.0e-6), float(v.max() + 1.0e-6)     # the epsilon in the tensor's precision
                lo, hi, nleft, nright = st["lo"], st["hi"], 0, 0
                if math.isnan(lo):
                    lo, hi = vmin, vmax
                else:
                    while vmin < lo:
                        lo, nleft = hi - 2 * (hi - lo), nleft + 1
                    while vmax > hi:
                        hi, nright = lo + 2 * (hi - lo), nright + 1
                with np.errstate(all="ignore"):
                    edges = np.linspace(lo, hi, HIST_BINS + 1)
                flo = torch.tensor(float(edges[0]), dtype=v.dtype, device=v.device)
                fbin = torch.tensor(float(edges[1] - edges[0]), dtype=v.dtype, device=v.device)
                if not (float(fbin) > 0 and math.isfinite(float(fbin)) and math.isfinite(float(flo))):
                    st["dropped"] += 1
                    continue
                c = st["counts"]
                for i in range(nleft + nright):
                    merged, c = c[0::2] + c[1::2], np.zeros(HIST_BINS, np.int64)
                    c[HIST_BINS // 2 if i < nleft else 0:][:HIST_BINS // 2] = merged
                idx = ((v - flo) / fbin).clamp(0, HIST_BINS - 1).int()            # past the last edge: the last bin
                st.update(lo=lo, hi=hi, counts=c + torch.bincount(idx, minlength=HIST_BINS).cpu().numpy())
        return 0

    # ---- the fused path -----------------------------------------------------------------------------------------------
    def _record_fused(self, gen, tgt) -> int:
        """one ``ace_diag_hist_window`` for both sides and all names of fields with contiguous planes; returns the launches made"""
        from .. import _lib
        names = self._names
        n, first = len(names), gen[names[0]]
        dev, (B, T, H, W) = first.device, first.shape
        if self._range is None:
            self._range = torch.full((2, n, 2), math.nan, dtype=torch.float64, device=dev)
            self._counts = torch.zeros(2, n, HIST_BINS, dtype=torch.int64, device=dev)
            self._dropped = torch.zeros(2, n, dtype=torch.int32, device=dev)
            self._mask_planes = torch.stack([self._masks[nm].reshape(H * W) for nm in names]).to(torch.uint8).contiguous()
            self._rows = _upload(list(range(n)), torch.int32, dev)
        masks = np.asarray([self._mask_planes.data_ptr() + i * H * W for i in range(n)], np.int64)      # from at["end"]
        at, _ = _upload_planes(names, gen, tgt, dev, [masks])
        lib = _lib.lib()
        scratch = torch.empty(int(lib.ace_diag_hist_scratch_bytes(n, B, T, H * W)), dtype=torch.uint8, device=dev)
        _check(lib.ace_diag_hist_window(at["gen"], at["gen_strides"], at["target"], at["target_strides"], self._rows.data_ptr(),
                                        at["end"], scratch.data_ptr(), self._range.data_ptr(), self._counts.data_ptr(),
                                        self._dropped.data_ptr(), n, HIST_BINS, n, B, T, H * W, _lib.current_stream()))
        return 1

    # ---- results ------------------------------------------------------------------------------------------------------
    def _state(self):
        """name -> ([target, prediction] int64 counts (2, n_bins), fp64 edges (2, n_bins + 1), dropped windows)"""
        out = {}
        if self._range is not None:
            rng, cnt, drop = self._range.cpu().numpy(), self._counts.cpu().numpy(), self._dropped.cpu().numpy()
        for i, n in enumerate(self._names):
            if self._range is not None:
                sides = [(rng[s, i, 0], rng[s, i, 1], cnt[s, i], int(drop[s, i])) for s in (1, 0)]
            else:
                sides = [(st["lo"], st["hi"], st["counts"], st["dropped"]) for st in reversed(self._host[n])]
            with np.errstate(all="ignore"):
                edges = np.stack([np.linspace(lo, hi, HIST_BINS + 1) for lo, hi, _, _ in sides])
            out[n] = (np.stack([c for _, _, c, _ in sides]), edges, sum(d for _, _, _, d in sides))
        return out

    def dataset(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """fme/core/histogram.py:480-509 under the label: ``<name>`` (2, n_bins) int64 and ``<name>_bin_edges`` (2, n_bins + 1) fp64,
        the leading axis source = [target, prediction]"""
        if not self.recorded:
            return {}
        ds = {}
        for n, (counts, edges, _) in self._state().items():
            ds[n] = torch.from_numpy(counts.copy())
            ds[f"{n}_bin_edges"] = torch.from_numpy(edges.copy())
        return {self.label: ds}

    def logs(self) -> Dict[str, Dict[str, Any]]:
        """fme/core/histogram.py:446-478 under the label: ``<source>/<p>th-percentile/<name>`` floats, ``<name>`` the trimmed
        densities and edges of both sources (the reference's figure), ``dropped_windows/<name>`` when any window was skipped.  A
        source without a recorded value has no percentile and an empty density."""
        if not self.recorded:
            return {}
        logs: Dict[str, Any] = {}
        for n, (counts, edges, dropped) in self._state().items():
            fig = {}
            for s, source in enumerate(("target", "prediction")):
                if counts[s].sum() == 0:
                    fig[f"{source}_density"], fig[f"{source}_bin_edges"] = torch.zeros(0, dtype=torch.float64), \
                        torch.zeros(0, dtype=torch.float64)
                    continue
                c, e = trim_zero_bins(counts[s], edges[s])
                fig[f"{source}_density"] = torch.from_numpy(c / np.sum(c * np.diff(e)))       # _normalize_histogram
                fig[f"{source}_bin_edges"] = torch.from_numpy(e.copy())
                if self._pct_only is None or n in self._pct_only:
                    for p in HIST_PERCENTILES:
                        logs[f"{source}/{p}th-percentile/{n}"] = histogram_quantile(e, c, p / 100.0)
            logs[n] = fig
            if dropped:
                logs[f"dropped_windows/{n}"] = dropped
        return {self.label: logs}
