"""The paired pass of the evaluator (``_Paired``: series, time means, zonal means) and the power spectrum (``_Spectrum``)."""
import math
from typing import Any, Dict, List, Mapping, Optional

import torch

from ..aggregator import _check, _grow, _grow_rows, _upload_planes
from .common import _channel_mean, _wmean, _wstd

LABELS = ("mean", "mean_norm", "time_mean", "time_mean_norm", "power_spectrum", "zonal_mean")    # the blocks, in reporting order
SERIES = ("weighted_mean_gen", "weighted_std_gen", "weighted_mean_target", "weighted_bias", "weighted_rmse",
          "weighted_grad_mag_percent_diff")                               # the rows of the fused series accumulator
NORM_SERIES = SERIES[:5]                                                  # reduced.py:248-255: the percent diff is denorm-only
_SHIFTED = ("weighted_mean_gen", "weighted_mean_target")                  # (v - mu) / sigma; the others v / sigma


def _grad_mag_mean(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """metrics.py:200-210 with weighted_nanmean (metrics.py:93-115)"""
    gy, gx = torch.gradient(x, dim=(-2, -1))
    g = torch.sqrt(gy ** 2 + gx ** 2)
    denom = torch.where(torch.isnan(g), torch.zeros((), dtype=w.dtype, device=w.device), w.expand(g.shape)).sum(dim=(-2, -1))
    return (g * w).nansum(dim=(-2, -1)) / denom


def zonal_coarsening(n_timesteps: int, max_size: int):
    """zonal_mean.py:89-127: (coarsening factor, number of slots)"""
    max_size = min(int(max_size), 2 ** 15, n_timesteps)
    if n_timesteps > max_size:
        factor = int(math.ceil(n_timesteps / max_size))
        return factor, n_timesteps // factor
    return 1, n_timesteps


def spectrum_bias_scores(gen: torch.Tensor, target: torch.Tensor, directional: bool = True) -> Dict[str, float]:
    """spectrum.py:218-276 for one name"""
    ratio = gen / target - 1
    pos = float(ratio[ratio > 0].sum() / target.shape[0])
    neg = float(ratio[ratio < 0].sum() / target.shape[0])
    out = {"smallest_scale_norm_bias": float(ratio[-1])}
    if directional:
        out["positive_norm_bias"], out["negative_norm_bias"] = pos, neg
    out["mean_abs_norm_bias"] = abs(pos) + abs(neg)
    return out


class _TorchState:
    """The torch path's accumulators of ``_Paired``: the reference's formulas in torch ops on the window and on ``normalize`` of it."""

    def __init__(self, p):
        self._p = p
        self._series: Dict[str, Dict[str, Dict[str, torch.Tensor]]] = {"denorm": {}, "norm": {}}
        self._tsum: Dict[str, List[Dict[str, torch.Tensor]]] = {"denorm": [{}, {}], "norm": [{}, {}]}
        self._zon: List[Dict[str, torch.Tensor]] = [{}, {}]

    def record(self, w, zonal: bool) -> int:
        p, agg = self._p, self._p._agg
        sl = slice(w.i_time_start, w.i_time_start + w.T)
        for kind, time_mean in (("denorm", "time_mean"), ("norm", "time_mean_norm")):
            series, maps = kind in p.series_kinds, w.with_maps and time_mean in p._labels
            if not (series or maps):
                continue
            g, t = w.kind(kind)
            if series:
                vals: Dict[str, Dict[str, torch.Tensor]] = {m: {} for m in (SERIES if kind == "denorm" else NORM_SERIES)}
                for n, x in g.items():
                    wt = agg.weights_for(n, x.device).to(x.dtype)
                    vals["weighted_mean_gen"][n] = _wmean(x, wt)
                    vals["weighted_std_gen"][n] = _wstd(x, wt)
                for n, y in t.items():
                    x, wt = g[n], agg.weights_for(n, y.device).to(y.dtype)
                    vals["weighted_mean_target"][n] = _wmean(y, wt)
                    vals["weighted_bias"][n] = _wmean(x - y, wt)                          # metrics.py:146-168
                    vals["weighted_rmse"][n] = _wmean(torch.square(x - y), wt).sqrt()    # metrics.py:171-197
                    if kind == "denorm":                                                  # metrics.py:213-224
                        gt, gg = _grad_mag_mean(y, wt), _grad_mag_mean(x, wt)
                        vals["weighted_grad_mag_percent_diff"][n] = 100 * (gg - gt) / gt
                for metric, d in vals.items():
                    tot = self._series[kind].setdefault(metric, {})
                    for n, v in d.items():
                        if n not in tot:
                            tot[n] = torch.zeros(agg._n_time, dtype=v.dtype, device=v.device)
                        tot[n][sl] += v.mean(dim=0)                                       # reduced.py:201-211
            if maps:
                part = slice(1, None) if w.i_time_start == 0 else slice(0, None)
                for side, d in enumerate((g, t)):
                    acc = self._tsum[kind][side]
                    for n, x in d.items():
                        s = x[:, part].sum(dim=1).sum(dim=0)
                        acc[n] = s if n not in acc else acc[n] + s
        if zonal:
            z0 = w.i_time_start - p._zon_first
            slots = torch.arange(z0, z0 + w.T, device=w.device) // agg._factor
            keep = slots < agg._n_slots
            for side, d in enumerate((w.gen, w.tgt)):
                for n, x in d.items():
                    zm = x.nanmean(dim=-1)                                                # non_distributed.py:136-137
                    acc = self._zon[side]
                    if n not in acc:
                        acc[n] = torch.zeros(x.shape[0], agg._n_slots, x.shape[2], dtype=x.dtype, device=x.device)
                    acc[n].index_add_(1, slots[keep], zm[:, keep] / agg._factor)
        return 0

    def series(self, kind: str, out) -> None:
        for metric in out:
            tot = self._series[kind].get(metric, {})
            for n in sorted(tot):
                counts = torch.tensor(self._p._n_batches, dtype=torch.int32, device=tot[n].device)
                out[metric][n] = self._p._agg._reduce_mean(tot[n] / counts)

    def time_means(self, n: str, steps: int, samples: int) -> Dict[str, Any]:
        reduce = self._p._agg._reduce_mean
        return {kind: (reduce(gs[n] / steps / samples), reduce(ts[n] / steps / samples) if n in ts else None)
                for kind, (gs, ts) in self._tsum.items() if n in gs}

    def stored(self, x: torch.Tensor) -> torch.Tensor:
        return x                                                          # a map of the dataset keeps the window's dtype

    def zonal(self, n: str) -> Optional[torch.Tensor]:
        if n in self._zon[0] and n in self._zon[1]:
            return torch.stack([self._zon[0][n].mean(dim=0), self._zon[1][n].mean(dim=0)])
        return None


class _FusedState:
    """The fused path's accumulators of ``_Paired``, rows by ``agg._rows``: ``_series`` (6, rows, n_time), ``_tsum`` (2, rows, H W) and
    ``_zon`` (2, rows, slots, H) in fp64, fed by one ``ace_diag_paired_window`` per window; the ``_norm`` outputs are formed from them
    at ``get_*`` time (module docstring of the package)."""

    def __init__(self, p):
        self._p, self._rows = p, p._agg._rows
        self._series = self._tsum = self._zon = None

    def record(self, w, zonal: bool) -> int:
        from .. import _lib
        p, agg = self._p, self._p._agg
        dev, B, T, (H, W) = w.device, w.B, w.T, agg._shape
        names = list(w.gen)
        n = len(names)
        if _grow_rows(self, names, dev, _series=lambda R: (len(SERIES), R, agg._n_time), _tsum=lambda R: (2, R, H * W),
                      _zon=lambda R: (2, R, agg._n_slots if "zonal_mean" in p._labels else 1, H)):
            agg._tables.clear()
        wrows = agg._weight_rows(names, dev)
        rows = agg._row_table(names, dev)
        at, _ = _upload_planes(names, w.gen, w.tgt, dev)
        lib = _lib.lib()
        partial = torch.empty(int(lib.ace_diag_paired_partial_doubles(n, B, T, H, W)), dtype=torch.float64, device=dev)
        series, n_time, t0 = self._series, agg._n_time, w.i_time_start
        if not p.series_kinds:                                            # the window's series go to scratch
            series, n_time, t0 = torch.empty(len(SERIES), len(self._rows), T, dtype=torch.float64, device=dev), T, 0
        _check(lib.ace_diag_paired_window(
            at["gen"], at["gen_strides"], at["target"], at["target_strides"], rows.data_ptr(), wrows.data_ptr(),
            agg._wplanes.data_ptr(), agg._wplanes.shape[0], partial.data_ptr(), self._tsum.data_ptr(), self._zon.data_ptr(),
            series.data_ptr(), len(self._rows), n_time, t0, 1 if w.i_time_start == 0 else 0, 1 if w.with_maps else 0,
            w.i_time_start - p._zon_first if zonal else 0, agg._factor if zonal else 1, self._zon.shape[2], n, B, T, H, W,
            _lib.current_stream()))
        return 1

    def series(self, kind: str, out) -> None:
        p, agg = self._p, self._p._agg
        dev = self._series.device
        counts = torch.tensor(p._n_batches, dtype=torch.float64, device=dev)
        for i, metric in enumerate(SERIES):
            if metric not in out:
                continue
            side = "gen" if metric in ("weighted_mean_gen", "weighted_std_gen") else "target"
            for n in sorted(p._present[side]):
                if kind == "norm" and not agg._has_stats(n):
                    continue
                tot = self._series[i, self._rows[n]]
                if kind == "norm":
                    mu, sigma = agg._stats[n]
                    if metric in _SHIFTED:                    # a record without the name adds 0 to the normalised total as well
                        tot = tot - mu * torch.tensor(p._present[side][n], dtype=torch.float64, device=dev)
                    tot = tot / sigma
                out[metric][n] = agg._reduce_mean((tot / counts).float())

    def time_means(self, n: str, steps: int, samples: int) -> Dict[str, Any]:
        agg, div = self._p._agg, steps * samples
        g = agg._reduce_mean((self._tsum[0, self._rows[n]] / div).reshape(agg._shape))
        t = agg._reduce_mean((self._tsum[1, self._rows[n]] / div).reshape(agg._shape)) if n in self._p._pair_names else None
        out = {"denorm": (g, t)}
        if agg._has_stats(n):
            mu, sigma = agg._stats[n]
            out["norm"] = ((g - mu) / sigma, None if t is None else (t - mu) / sigma)
        return out

    def stored(self, x: torch.Tensor) -> torch.Tensor:
        return x.float()

    def zonal(self, n: str) -> Optional[torch.Tensor]:
        return self._zon[:, self._rows[n]].float() if n in self._rows else None


class _Paired:
    """``mean`` / ``mean_norm`` (reduced.py:221-348), ``time_mean`` / ``time_mean_norm`` (time_mean.py:246-444) and ``zonal_mean``
    (zonal_mean.py:50-355) of every window, the initial condition included (it feeds the series only).  ``series_kinds``: the kinds
    ("denorm", "norm") whose series something reads - a ``mean`` label, or a step mean, which is a column of them.  The accumulators
    are a ``_TorchState`` or a ``_FusedState``, whichever path the first window takes; the counts stay here, on the host."""
    needs_time = uses_time = False
    counted = True

    def __init__(self, agg, labels: Mapping[str, str], series_kinds):
        self._agg, self._labels = agg, labels
        self.series_kinds = set(series_kinds) | {k for k, key in (("denorm", "mean"), ("norm", "mean_norm")) if key in labels}
        self.needs_norm = "norm" in self.series_kinds or "time_mean_norm" in labels
        self._state = None
        self._n_batches = [0] * agg._n_time                               # per time index (reduced.py: _n_batches)
        self._present: Dict[str, Dict[str, List[int]]] = {"gen": {}, "target": {}}     # name -> records per time index
        self._tm_names: List[str] = []
        self._pair_names: List[str] = []
        self._tm_steps = self._zon_steps = 0
        self._tm_samples = self._zon_first = None                         # samples of the first window; first zonal time index

    def record(self, w) -> int:
        if self._state is None:
            self._state = (_FusedState if w.fused else _TorchState)(self)
        zonal = w.with_maps and "zonal_mean" in self._labels
        if zonal and self._zon_first is None:
            self._zon_first = w.i_time_start
        made = self._state.record(w, zonal)
        steps = range(w.i_time_start, w.i_time_start + w.T)
        if self.series_kinds:
            for side, d in (("gen", w.gen), ("target", w.tgt)):
                for n in d:
                    seen = self._present[side].setdefault(n, [0] * self._agg._n_time)
                    for i in steps:
                        seen[i] += 1
            for i in steps:
                self._n_batches[i] += 1
        if w.with_maps:
            if self._tm_samples is None:                                              # time_mean.py:127-146
                self._tm_samples = w.B
            self._tm_steps = w.T - 1 if w.i_time_start == 0 else self._tm_steps + w.T
            self._tm_names += [n for n in w.gen if n not in self._tm_names]
            # the maps' pairs: an initial condition that is its own target feeds the series only
            self._pair_names += [n for n in w.tgt if n not in self._pair_names]
            if zonal:
                self._zon_steps += w.T
        return made

    # ---- results --------------------------------------------------------------------------------------------------------
    def _series_data(self, kind: str = "denorm") -> Dict[str, Dict[str, torch.Tensor]]:
        """reduced.py:34-55, 213-218: metric -> name -> (n_timesteps,) series (sorted names), total / per-index count."""
        if not any(self._n_batches):
            raise ValueError("No batches have been recorded.")
        out: Dict[str, Dict[str, torch.Tensor]] = {m: {} for m in sorted(SERIES if kind == "denorm" else NORM_SERIES)}
        self._state.series(kind, out)
        return out

    def _time_means(self):
        """time_mean.py:151-162 for both sides: kind -> name -> (gen, target or None) (H, W) maps, fp64 (fused; the norm maps formed
        from the denormalised ones) or in the window's dtype (torch)."""
        if self._tm_steps == 0 or not self._tm_names:
            raise ValueError("No data recorded.")
        out: Dict[str, Dict[str, Any]] = {"denorm": {}, "norm": {}}
        for n in sorted(self._tm_names):
            for kind, maps in self._state.time_means(n, self._tm_steps, self._tm_samples).items():
                out[kind][n] = maps
        return out

    def _time_mean_logs(self, kind: str, maps) -> Dict[str, Any]:
        """time_mean.py:339-401 without the label"""
        logs: Dict[str, Any] = {}
        rmse_all, all_nan = {}, set()
        for n, (g, t) in maps.items():
            logs[f"gen_map/{n}"] = g.float().cpu()
            if t is None:
                continue
            w = self._agg.weights_for(n, g.device).to(g.dtype)
            rmse_all[n] = float(_wmean(torch.square(g - t), w).sqrt())
            if bool(torch.isnan(t).all()):
                all_nan.add(n)
            logs[f"rmse/{n}"] = rmse_all[n]
            if kind == "denorm":
                logs[f"bias_map/{n}"] = (g - t).float().cpu()
                logs[f"bias/{n}"] = float(_wmean(g - t, w))
        if kind == "norm":
            cm = _channel_mean(rmse_all, None, self._agg._channel_mean_names, all_nan)
            if cm is None:
                raise ValueError("All target variables are NaN; cannot compute channel mean.")
            logs["rmse/channel_mean"] = cm
        return logs

    def _zonal(self) -> Dict[str, torch.Tensor]:
        """zonal_mean.py:268-306: name -> (2, n_slots, H) [generated, target]; a slot that no window completed is NaN (the
        reference's 0 / 0)."""
        if self._zon_first is None:
            raise RuntimeError("No data recorded")
        done = self._zon_steps // self._agg._factor
        out = {}
        for n in sorted(self._pair_names):
            z = self._state.zonal(n)
            if z is None:
                continue
            z = z.clone()
            z[:, done:] = float("nan")
            out[n] = torch.stack([self._agg._reduce_mean(z[0]), self._agg._reduce_mean(z[1])])
        return out

    def _kinds(self, mean: str, norm: str):
        return [(kind, self._labels[key]) for kind, key in (("denorm", mean), ("norm", norm)) if key in self._labels]

    def dataset(self) -> Dict[str, Dict[str, torch.Tensor]]:
        ds: Dict[str, Dict[str, torch.Tensor]] = {}
        for kind, label in self._kinds("mean", "mean_norm"):
            ds[label] = {f"{m}-{n}": v.cpu() for m, d in self._series_data(kind).items() for n, v in d.items()}
        maps = self._time_means() if self._kinds("time_mean", "time_mean_norm") else None
        for kind, label in self._kinds("time_mean", "time_mean_norm"):
            d = ds[label] = {}
            for n, (g, t) in maps[kind].items():
                if t is not None:
                    d[f"bias_map-{n}"] = self._state.stored(g - t).cpu()
                    d[f"gen_map-{n}"] = self._state.stored(g).cpu()
        if "zonal_mean" in self._labels:
            d = ds[self._labels["zonal_mean"]] = {}
            for n, z in self._zonal().items():
                d[f"gen-{n}"] = z[0].cpu()
                d[f"error-{n}"] = (z[0] - z[1]).cpu()
        return ds

    def logs(self) -> Dict[str, Dict[str, Any]]:
        logs: Dict[str, Dict[str, Any]] = {}
        maps = self._time_means() if self._kinds("time_mean", "time_mean_norm") else None
        for kind, label in self._kinds("time_mean", "time_mean_norm"):
            logs[label] = self._time_mean_logs(kind, maps[kind])
        if "zonal_mean" in self._labels:
            d = logs[self._labels["zonal_mean"]] = {}
            for n, z in self._zonal().items():
                d[f"gen/{n}"] = z.cpu()
                d[f"error/{n}"] = (z[0] - z[1]).cpu()
        return logs


class _Spectrum:
    """``power_spectrum`` (spectrum.py:112-276): the mean spectra of prediction and target over samples and steps and their bias
    scores, of the names whose mask has no zeros (``agg.omitted`` lists the others) and, with ``fill_masked`` - the reference's
    behaviour, off by default - of the masked names with a valid pixel too, flood-filled first (``agg.filled``; ace_amd/fill.py).
    Torch path: the running mean of metrics.py:388-408 per name; fused path: per chunk of names one SHT and one
    ``ace_diag_spectrum`` for each side, adding to ``_spec`` (2, rows, lmax) fp64, rows by ``agg._rows``; with ``fill_masked`` one
    ``ace_diag_fill_planes`` builds the SHT's input in place of the ``torch.stack``, three launches per chunk and side."""
    needs_time = uses_time = needs_norm = False
    counted = True

    def __init__(self, agg, label: str, directional: bool):
        self._agg, self.label, self._directional = agg, label, bool(directional)
        self._counts: List[Dict[str, int]] = [{}, {}]                     # per side, name -> samples x steps recorded
        self._t_spec: List[Dict[str, torch.Tensor]] = [{}, {}]
        self._spec = None

    def record(self, w) -> int:
        agg, made = self._agg, 0
        sht, BT = agg._get_sht(), w.B * w.T
        for side, d in enumerate((w.gen, w.tgt)):
            names = [n for n in d if not agg._omitted(n)]
            if w.fused:
                made += self._record_fused(w, side, [d[n] for n in names], names, sht)
            for n in names:
                old = self._counts[side].get(n, 0)
                if not w.fused:
                    mean_ps = torch.mean(torch.sum(abs(sht(agg._fill_torch(n, d[n]))) ** 2, dim=-1), dim=(0, 1))      # metrics.py:388-408
                    acc = self._t_spec[side]
                    acc[n] = mean_ps if n not in acc else (BT * mean_ps + old * acc[n]) / (BT + old)
                self._counts[side][n] = old + BT
        return made

    def _record_fused(self, w, side: int, fields, names, sht) -> int:
        from .. import _lib
        agg, dev, (H, W), L, M = self._agg, w.device, self._agg._shape, sht.lmax, sht.mmax
        if self._spec is None or self._spec.shape[1] < len(agg._rows):
            self._spec = _grow(self._spec, (2, len(agg._rows), L), torch.float64, dev)
        k = max(1, agg.spectrum_chunk_bytes // (w.B * w.T * (H * W * 4 + L * M * 8)))
        acc = self._spec.data_ptr() + side * self._spec.shape[1] * L * 8
        total = 0
        for c0 in range(0, len(names), k):
            chunk = names[c0:c0 + k]
            planes, made = agg._spectrum_input(chunk, fields[c0:c0 + k], dev)
            coeffs = sht(planes)                                                  # (k, B, T, L, M) complex64
            _check(_lib.lib().ace_diag_spectrum(coeffs.data_ptr(), agg._row_table(chunk, dev).data_ptr(), acc, self._spec.shape[1],
                                                len(chunk), w.B * w.T, L, M, _lib.current_stream()))
            total += 2 + made
        return total

    def _spectra(self) -> Dict[str, torch.Tensor]:
        """spectrum.py:67-77, 207-215: name -> (2, lmax) [prediction, target] mean spectra; the target row of a name without a
        target is NaN."""
        out = {}
        for n in sorted(self._counts[0]):
            sides = []
            for side in (0, 1):
                cnt = self._counts[side].get(n)
                if cnt is None:
                    sides.append(None)
                elif self._spec is not None:
                    sides.append(self._agg._reduce_mean((self._spec[side, self._agg._rows[n]] / cnt).float()))
                else:
                    sides.append(self._agg._reduce_mean(self._t_spec[side][n].clone()))
            if sides[1] is None:
                sides[1] = torch.full_like(sides[0], float("nan"))
            out[n] = torch.stack(sides)
        return out

    def dataset(self) -> Dict[str, Dict[str, torch.Tensor]]:
        return {self.label: {n: v.cpu() for n, v in self._spectra().items()}}

    def logs(self) -> Dict[str, Dict[str, Any]]:
        logs: Dict[str, Any] = {}
        for n, s in self._spectra().items():
            logs[n] = s.cpu()
            if not bool(torch.isnan(s[1]).all()):
                for k, v in spectrum_bias_scores(s[0].double().cpu(), s[1].double().cpu(), self._directional).items():
                    logs[f"{k}/{n}"] = v
        return {self.label: logs}
