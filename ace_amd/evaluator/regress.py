"""The ``trend``, ``enso_coefficient`` and ``near_zero_fraction`` metrics of the evaluator (``_Regress``)."""
import math
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from ..aggregator import _check, _grow, _grow_rows, _upload_planes
from .common import _check_time, _only, _wmean

SECONDS_PER_YEAR = 365.25 * 24 * 60 * 60                                 # trend.py:21-25: a fixed Julian year
TREND_EPOCH = (2000, 1, 1)                                                # trend.py:26-32
MAX_REGRESS_MAPS = 8                                                      # ACE_DIAG_REGRESS_MAX_MAPS (include/ace_sfno.h)


class _Regress:
    """The three metrics that are per-pixel sums over time: ``trend`` (TrendEvaluatorAggregator, trend.py:46-194),
    ``enso_coefficient`` (EnsoCoefficientEvaluatorAggregator, enso_coefficient.py:61-244) and ``near_zero_fraction``
    (NearZeroFractionAggregator, near_zero_fraction.py:97-216).  The torch path states the reference's formulas in the reference's
    dtypes (trend fp64, the ENSO covariance fp32, the indicator in the field's dtype); the fused path feeds all that are on from one
    ``ace_diag_regress_window`` per window (csrc/regress.hip; the header contract in include/ace_sfno.h): term 0 = 1 -> map 0 (sum y),
    term 1 = t in years -> map 1 (sum t y), term 2 = the index -> map 2 + b (sample b's covariance), eps per plane for the indicator
    (NaN for a plane outside the near-zero variables: nothing is below NaN).  n, sum t, sum t^2, the per-sample sum of index^2 and
    the record counts stay on the host in fp64.

    The ENSO index is the caller's (B, n_ic_steps + n_forward_steps) table; each row is made zero-mean over its time levels in fp64
    (enso_coefficient.py:408-410) and rounded to fp32, as the reference rounds each window's values (enso_coefficient.py:141-145);
    both paths regress on those fp32 numbers.  A row with a non-finite value is left out, the reference's ``None`` series.  The
    reference records the ENSO sums at every step of a window but drops, as the time mean does, the first step of a window at time
    index 0 from the trend and the near-zero fraction; the fused path then makes a second call for the ENSO term alone."""
    needs_norm = False
    counted = True                                                        # its calls are part of ``launches()``

    def __init__(self, agg, trend, enso, nzf):
        self._agg = agg
        self.trend, self.enso, self.nzf = trend, enso, nzf
        self._n = self._sum_t = self._sum_tt = 0.0
        self._index = self._valid = None
        if enso is not None:
            idx = torch.as_tensor(enso.index).detach().to("cpu", torch.float64)
            if idx.dim() != 2 or idx.shape[1] != agg._n_time:
                raise ValueError(f"enso_coefficient.index must be (samples, {agg._n_time} time levels), got {tuple(idx.shape)}")
            self._valid = [bool(torch.isfinite(row).all()) for row in idx]
            self._index = (idx - idx.mean(dim=1, keepdim=True)).float()
            self._ivar64 = [0.0] * idx.shape[0]
        self._recorded = False
        self._tnames: List[List[str]] = [[], []]                              # per side, the names of each metric seen so far
        self._enames: List[List[str]] = [[], []]
        self._znames: List[List[str]] = [[], []]
        self._zcount = 0                                                  # (sample, step) entries behind the fractions and maps
        # torch path
        self._t_sum_y: List[Dict[str, torch.Tensor]] = [{}, {}]
        self._t_sum_ty: List[Dict[str, torch.Tensor]] = [{}, {}]
        self._t_cov: List[Dict[int, Dict[str, torch.Tensor]]] = [{}, {}]
        self._t_ivar: Dict[int, torch.Tensor] = {}
        self._t_frac: List[Dict[str, torch.Tensor]] = [{}, {}]
        self._t_cells: List[Dict[str, torch.Tensor]] = [{}, {}]
        # fused path: _maps (2, rows, nmaps, H W) fp64, _count (2, rows, H W) int64, _frac (2, rows) fp64
        self._rows: Dict[str, int] = {}
        self._maps = self._count = self._frac = None
        self._nmaps = 0

    @property
    def needs_time(self) -> bool:
        return self.trend is not None

    uses_time = needs_time

    def without_time(self):
        raise ValueError("the trend metric needs the window's time axis: record_batch(prediction, target, time=...)")

    def _eps_for(self, name: str) -> float:
        return self.nzf.per_variable_eps.get(name, self.nzf.eps)

    def _prepare(self, gen, tgt, i_time_start, time):
        """the host side of a window: the name lists of each metric, the years and the index values of its steps"""
        B, T = next(iter(gen.values())).shape[:2]
        begin = 1 if i_time_start == 0 else 0
        years = None
        if self.trend is not None:
            if time is None:
                self.without_time()
            _check_time(time, B, T)
            years = time.microseconds_since(TREND_EPOCH).astype("float64") / 1.0e6 / SECONDS_PER_YEAR
            part = years[:, begin:]
            self._n += part.size
            self._sum_t += float(part.sum())
            self._sum_tt += float((part * part).sum())
        index = None
        if self.enso is not None:
            if B != self._index.shape[0]:
                raise ValueError("number of index series must match number of samples")
            index = self._index[:, i_time_start:i_time_start + T]
            for b in range(B):
                if self._valid[b]:
                    self._ivar64[b] += float((index[b].double() ** 2).sum())
        names = {"trend": [_only(d, self.trend.variables) if self.trend is not None and T > begin else [] for d in (gen, tgt)],
                 "enso": [list(d) if self.enso is not None else [] for d in (gen, tgt)],
                 "nzf": [_only(d, self.nzf.variables) if self.nzf is not None and T > begin else [] for d in (gen, tgt)]}
        for key, seen in (("trend", self._tnames), ("enso", self._enames), ("nzf", self._znames)):
            for side in (0, 1):
                seen[side] += [n for n in names[key][side] if n not in seen[side]]
        if self.nzf is not None:
            self._zcount += B * (T - begin)
        self._recorded = True
        return B, T, begin, years, index, names

    def record(self, w) -> int:
        prepared = self._prepare(w.gen, w.tgt, w.i_time_start, w.time)
        return (self._record_fused if w.fused else self._record_torch)(w, *prepared)

    # ---- the torch path -----------------------------------------------------------------------------------------------
    def _record_torch(self, w, B, T, begin, years, index, names) -> int:
        for side, d in enumerate((w.gen, w.tgt)):
            if names["trend"][side]:                                          # trend.py:104-147
                dev = d[names["trend"][side][0]].device
                t = torch.tensor(years[:, begin:], dtype=torch.float64, device=dev)[:, :, None, None]
                for n in names["trend"][side]:
                    y = d[n][:, begin:].to(torch.float64)
                    cy, cty = y.sum(dim=(0, 1)), (t * y).sum(dim=(0, 1))
                    sy, sty = self._t_sum_y[side], self._t_sum_ty[side]
                    sy[n], sty[n] = (sy[n] + cy, sty[n] + cty) if n in sy else (cy, cty)
            for b in range(B if names["enso"][side] else 0):                  # enso_coefficient.py:136-168
                if not self._valid[b]:
                    continue
                first = d[names["enso"][side][0]]
                iw = index[b].to(device=first.device, dtype=torch.float32)
                if side == 0:
                    self._t_ivar[b] = self._t_ivar.get(b, torch.tensor(0.0, dtype=torch.float32, device=first.device)) + (iw ** 2).sum()
                cov = self._t_cov[side].setdefault(b, {})
                for n in names["enso"][side]:
                    c = (d[n][b] * iw.view(T, 1, 1)).sum(dim=0)                # data_index_covariance, enso_coefficient.py:418-437
                    cov[n] = cov[n] + c if n in cov else c
            for n in names["nzf"][side]:                                      # near_zero_fraction.py:147-186
                x = d[n][:, begin:]
                below = (x <= torch.tensor(self._eps_for(n), dtype=torch.float32, device=x.device)).to(x.dtype)
                frac = _wmean(below, self._agg.weights_for(n, x.device).to(x.dtype))
                acc = self._t_frac[side]
                acc[n] = acc.get(n, frac.new_zeros(())) + frac.sum()
                if self.nzf.include_maps:
                    cells = below.sum(dim=1).sum(dim=0)
                    self._t_cells[side][n] = self._t_cells[side][n] + cells if n in self._t_cells[side] else cells
        return 0

    # ---- the fused path -----------------------------------------------------------------------------------------------
    def _record_fused(self, w, B, T, begin, years, index, names) -> int:
        """one ``ace_diag_regress_window`` for all the metrics that are on, both sides and all names (fields with contiguous
        planes); returns the launches made"""
        from .. import _lib
        agg, gen, tgt, dev, HW = self._agg, w.gen, w.tgt, w.device, w.HW
        base_e = 2 if self.trend is not None else 0
        nmaps = base_e + (B if self.enso is not None else 0)
        if nmaps > MAX_REGRESS_MAPS:
            raise ValueError(f"the fused trend / enso_coefficient pass keeps 2 + samples maps per pixel in registers, at most "
                             f"{MAX_REGRESS_MAPS}: {B} samples with the ENSO coefficient on need {nmaps}; record fewer samples per "
                             "window or take the torch path (fused = False)")
        if self._maps is not None and nmaps != self._nmaps:
            raise ValueError("the number of samples changed between windows")
        planes = [n for n in gen if any(n in names[k][s] for k in names for s in (0, 1))]
        self._nmaps = nmaps
        if _grow_rows(self, planes, dev, _maps=lambda R: (2, R, max(1, nmaps), HW), _frac=lambda R: (2, R)):
            self._count = _grow(self._count, self._maps.shape[:2] + (HW,), torch.int64, dev)
        if not planes:
            return 0
        n = len(planes)
        wrows = agg._weight_rows(planes, dev)
        # a plane takes part in every term of the call; what a metric's variable filter excludes is left out at get_* time
        calls = []
        if self.trend is not None or self.nzf is not None or (self.enso is not None and begin == 0):
            calls.append((begin, self.trend is not None, self.enso is not None and begin == 0, self.nzf is not None))
        if self.enso is not None and begin == 1:
            calls.append((0, False, True, False))
        lib = _lib.lib()
        made = 0
        for t_begin, do_trend, do_enso, do_nzf in calls:
            coef, slot = [], []
            if do_trend:
                coef += [np.ones((B, T)), years]
                slot += [[0] * B, [1] * B]
            if do_enso:
                coef.append(index.double().numpy())
                slot.append([base_e + b if self._valid[b] else -1 for b in range(B)])
            nterms = len(coef)
            eps = [self._eps_for(nm) if nm in self.nzf.variables else math.nan for nm in planes] if do_nzf else []
            # one pinned blob: the plane table, then from its end the coefficients, the rows, the slots and the eps
            at, (p_coef, p_rows, p_slot, p_eps) = _upload_planes(planes, gen, tgt, dev, [
                np.asarray(coef, np.float64), np.asarray([self._rows[nm] for nm in planes], np.int32), np.asarray(slot, np.int32),
                np.asarray(eps, np.float32)])
            partial = None
            if do_nzf:
                partial = torch.empty(int(lib.ace_diag_regress_partial_doubles(n, B, T, HW)), dtype=torch.float64, device=dev)
            _check(lib.ace_diag_regress_window(
                at["gen"], at["gen_strides"], at["target"], at["target_strides"], p_rows, p_coef if nterms else None,
                p_slot if nterms else None, self._maps.data_ptr() if nterms else None, p_eps if do_nzf else None,
                wrows.data_ptr(), agg._wplanes.data_ptr(), agg._wplanes.shape[0], partial.data_ptr() if do_nzf else None,
                self._count.data_ptr(), self._frac.data_ptr(), self._maps.shape[1], nterms, nmaps if nterms else 0, t_begin, n,
                B, T, HW, _lib.current_stream()))
            made += 1
        return made

    # ---- results ------------------------------------------------------------------------------------------------------
    def _trends(self) -> Dict[str, List[Optional[torch.Tensor]]]:
        """trend.py:163-194: name -> [target, prediction] fp64 (H, W) slopes (None for a side the name was not recorded on)"""
        n, st, stt = self._n, self._sum_t, self._sum_tt
        denom = n * stt - st * st
        out: Dict[str, List[Optional[torch.Tensor]]] = {}
        for side, slot in ((1, 0), (0, 1)):
            for name in sorted(self._tnames[side]):
                if self._maps is not None:
                    sy, sty = self._maps[side, self._rows[name], 0], self._maps[side, self._rows[name], 1]
                else:
                    sy, sty = self._t_sum_y[side][name], self._t_sum_ty[side][name]
                slope = self._agg._reduce_mean(((n * sty - st * sy) / denom).reshape(self._agg._shape))
                out.setdefault(name, [None, None])[slot] = slope
        return {k: v for k, v in out.items() if v[1] is not None}

    def _coefficients(self) -> Dict[str, List[Optional[torch.Tensor]]]:
        """enso_coefficient.py:170-244: name -> [target, prediction] (H, W) coefficients, the mean over the samples that have a
        series of covariance / sum of index^2; fp32 on the torch path, fp64 on the fused path"""
        out: Dict[str, List[Optional[torch.Tensor]]] = {}
        samples = [b for b, ok in enumerate(self._valid) if ok]
        base_e = 2 if self.trend is not None else 0
        for side, slot in ((1, 0), (0, 1)):
            for name in sorted(self._enames[side]):
                if self._maps is not None:
                    per = [self._maps[side, self._rows[name], base_e + b] / self._ivar64[b] for b in samples]
                else:
                    per = [self._t_cov[side][b][name] / self._t_ivar[b] for b in samples if name in self._t_cov[side].get(b, {})]
                if per:
                    c = torch.stack(per, dim=0).mean(dim=0).reshape(self._agg._shape)
                    out.setdefault(name, [None, None])[slot] = self._agg._reduce_mean(c)
        return {k: v for k, v in out.items() if v[1] is not None}

    def _fractions(self):
        """near_zero_fraction.py:209-225: name -> [gen, target] scalar fractions and, with include_maps, per-cell fraction maps"""
        fr: Dict[str, List[Optional[float]]] = {}
        maps: Dict[str, List[Optional[torch.Tensor]]] = {}
        for side in (0, 1):
            for name in sorted(self._znames[side]):
                if self._maps is not None:
                    f = self._frac[side, self._rows[name]] / self._zcount
                    cells = self._count[side, self._rows[name]].to(torch.float32)
                else:
                    f = self._t_frac[side][name] / self._zcount
                    cells = self._t_cells[side].get(name)
                fr.setdefault(name, [None, None])[side] = float(self._agg._reduce_mean(f))
                if self.nzf.include_maps:
                    maps.setdefault(name, [None, None])[side] = self._agg._reduce_mean((cells / self._zcount).reshape(self._agg._shape))
        return fr, maps

    def _rmse(self, name, gen_map, target_map) -> float:
        w = self._agg.weights_for(name, gen_map.device).to(gen_map.dtype)
        return float(_wmean(torch.square(gen_map - target_map), w).sqrt())

    def dataset(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """label -> variables.  trend (trend.py:252-276) and enso_coefficient (enso_coefficient.py:308-329): ``<name>`` (2, H, W), the
        leading axis source = [target, prediction], NaN where a name has no target; near_zero_fraction with include_maps
        (near_zero_fraction.py:284-300): ``gen_map-<name>``, ``target_map-<name>``, ``error_map-<name>``."""
        ds: Dict[str, Dict[str, torch.Tensor]] = {}
        if not self._recorded:
            return ds
        pair = lambda t, g: torch.stack([torch.full_like(g, math.nan) if t is None else t, g]).cpu()      # noqa: E731
        if self.trend is not None and self._n > 0:
            ds[self.trend.name or "trend"] = {n: pair(t, g) for n, (t, g) in self._trends().items()}
        if self.enso is not None:
            ds[self.enso.name or "enso_coefficient"] = {n: pair(t, g) for n, (t, g) in self._coefficients().items()}
        if self.nzf is not None and self._zcount > 0:
            d = ds[self.nzf.name or "near_zero_fraction"] = {}
            for n, (g, t) in self._fractions()[1].items():
                if g is None:
                    continue
                d[f"gen_map-{n}"] = g.cpu()
                if t is not None:
                    d[f"target_map-{n}"] = t.cpu()
                    d[f"error_map-{n}"] = (g - t).cpu()
        return ds

    def logs(self) -> Dict[str, Dict[str, Any]]:
        """label -> logs: trend.py:204-239, enso_coefficient.py:246-306 and near_zero_fraction.py:269-282 with tensors where the
        reference logs images.  ``maps/<name>`` (2, H, W) [target, generated], ``difference_map/<name>`` and
        ``weighted_rmse/<name>`` from the fp32 casts; ``coefficient_maps/<name>``, ``coefficient_difference_map/<name>``,
        ``rmse/<name>``; ``gen/<name>``, ``gen_minus_target/<name>`` and with include_maps ``gen_target_map/<name>`` (2, H, W)
        [generated, target], ``error_map/<name>`` (``gen_map/<name>`` for a name without a target)."""
        logs: Dict[str, Dict[str, Any]] = {}
        if not self._recorded:
            return logs
        if self.trend is not None and self._n > 0:
            d = logs[self.trend.name or "trend"] = {}
            for n, (t, g) in self._trends().items():
                if t is None:
                    continue
                d[f"maps/{n}"] = torch.stack([t, g]).cpu()
                d[f"difference_map/{n}"] = (g - t).cpu()
                d[f"weighted_rmse/{n}"] = self._rmse(n, g.to(torch.float32), t.to(torch.float32))
        if self.enso is not None:
            d = logs[self.enso.name or "enso_coefficient"] = {}
            for n, (t, g) in self._coefficients().items():
                if t is None:
                    continue
                d[f"coefficient_maps/{n}"] = torch.stack([t, g]).cpu()
                d[f"coefficient_difference_map/{n}"] = (g - t).cpu()
                d[f"rmse/{n}"] = self._rmse(n, g, t)
        if self.nzf is not None and self._zcount > 0:
            d = logs[self.nzf.name or "near_zero_fraction"] = {}
            fr, maps = self._fractions()
            for n, (g, t) in fr.items():
                if g is None:
                    continue
                d[f"gen/{n}"] = g
                if t is not None:
                    d[f"gen_minus_target/{n}"] = g - t
            for n, (g, t) in maps.items():
                if g is None:
                    continue
                if t is None:
                    d[f"gen_map/{n}"] = g.cpu()
                else:
                    d[f"gen_target_map/{n}"] = torch.stack([g, t]).cpu()
                    d[f"error_map/{n}"] = (g - t).cpu()
        return logs
