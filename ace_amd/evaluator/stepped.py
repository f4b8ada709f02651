"""The ``step_means`` and ``ensembles`` metrics of the evaluator: entries that each report one step."""
from typing import Any, Dict, List, Optional, Sequence

import torch

from ..aggregator import _check, _grow, _grow_rows, _upload, _upload_planes
from .common import _channel_mean, _wmean

ENSEMBLE_CRPS_ALPHA = 0.95                                                # one_step/ensemble.py:80
PRESCRIBED_MSE_RTOL = 1e-6                                                # one_step/ensemble.py:20-23
MAX_ENSEMBLE_MEMBERS = 32                                                 # ACE_DIAG_ENSEMBLE_MAX_MEMBERS (include/ace_sfno.h)
ENSEMBLE_METRICS = ("crps", "ensemble_mean_rmse", "ssr_bias")             # sorted, as _get_data walks them (ensemble.py:296)


def ssr_bias(total_unbiased_mse: torch.Tensor, total_variance: torch.Tensor) -> torch.Tensor:
    """SSRBiasMetric.get (one_step/ensemble.py:150-173): spread / skill - 1 per pixel from the totals of mse - variance / E and of
    the variance.  The unbiased MSE is clamped at 0 before the square root (the correction can go slightly negative with few
    members); zero skill gives -1 by convention (the limit for spread -> 0 at non-zero skill); a prescribed cell - variance
    exactly 0 and unbiased MSE at most PRESCRIBED_MSE_RTOL x the field's largest clamped MSE - is a 0 / 0 and reports 0."""
    spread = total_variance.sqrt()
    skill = torch.clamp(total_unbiased_mse, min=0.0).sqrt()
    ssr = torch.where(skill > 0, spread / skill - 1, torch.full_like(spread, -1.0))
    mse_floor = PRESCRIBED_MSE_RTOL * skill.square().max()
    prescribed = (total_variance == 0) & (total_unbiased_mse <= mse_floor)
    return torch.where(prescribed, torch.zeros_like(spread), ssr)




class _Stepped:
    """What the two families share: ``_entries()`` yields (label, key -> float or map) per entry that has something to report."""
    needs_time = uses_time = False
    counted = True

    @property
    def needs_norm(self) -> bool:
        return "norm" in self.kinds

    def logs(self) -> Dict[str, Dict[str, Any]]:
        return {label: dict(sorted(data.items())) for label, data in self._entries()}

    def dataset(self) -> Dict[str, Dict[str, torch.Tensor]]:
        return {label: {k.replace("/", "-"): v if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=torch.float64)
                        for k, v in data.items()} for label, data in self._entries()}


class _StepMeans(_Stepped):
    """``step_means`` (MeanAggregator behind StepMeanMetricConfig, one_step/reduced.py:24-249): the column of the ``mean`` series at
    time index ``step + n_ic_steps - 1`` of the paired family - the sample-mean ``weighted_rmse``, ``weighted_bias`` and
    ``weighted_grad_mag_percent_diff`` of that step, averaged over the records that held it - so there is nothing to accumulate
    beyond what the paired pass (or the torch path's series) already holds; the norm form is the norm series' column.  Only
    ``record_batch`` feeds it, as in the reference (main.py:602-603, 660-661): an entry whose index lies inside the initial
    condition, or whose window has not come yet, reports nothing.  Which targets are entirely NaN (left out of the channel mean,
    reduced_metrics.py:101-110) is decided on the device at the first record of the selected step and read at ``get_*`` time."""

    def __init__(self, agg, configs: Sequence, paired):
        self._agg, self._paired = agg, paired
        self.configs = list(configs)
        self.kinds = {c.target for c in self.configs}
        self._nan: Dict[int, Any] = {}                                    # entry -> (names, device bool (names,))

    def index(self, c) -> int:
        return c.step + self._agg.n_ic_steps - 1

    def record(self, w) -> int:
        tgt = w.tgt
        for i, c in enumerate(self.configs):
            k = self.index(c) - w.i_time_start
            if c.target == "norm" and i not in self._nan and 0 <= k < w.T and self.index(c) >= self._agg.n_ic_steps:
                names = list(tgt)                                           # one stacked reduction over the names
                self._nan[i] = (names, torch.stack([tgt[n][:, k] for n in names]).isnan().flatten(1).all(dim=1))
        return 0

    def _entries(self):
        agg = self._agg
        series: Dict[str, Any] = {}
        for i, c in enumerate(self.configs):
            ti = self.index(c)
            if ti < agg.n_ic_steps or self._paired._n_batches[ti] == 0:
                continue
            if c.target not in series:
                series[c.target] = self._paired._series_data(c.target)
            metrics = ("weighted_rmse", "weighted_bias", "weighted_grad_mag_percent_diff") if c.target == "denorm" else \
                ("weighted_rmse",)
            data: Dict[str, float] = {}
            for metric in metrics:
                column = series[c.target][metric]                           # one read of the column per metric
                values = dict(zip(column, torch.stack([v[ti] for v in column.values()]).tolist())) if column else {}
                for n, v in values.items():
                    if c.variables is None or n in c.variables:
                        data[f"{metric}/{n}"] = v
                if c.target == "norm":
                    names, flags = self._nan.get(i, ([], None))
                    nan_targets = set() if flags is None else {n for n, f in zip(names, flags.tolist()) if f}
                    cm = _channel_mean(values, c.channel_mean_names, agg._channel_mean_names, nan_targets)
                    if cm is None:
                        raise ValueError("All target variables are NaN; cannot compute channel mean.")
                    data[f"{metric}/channel_mean"] = cm
            yield c.name, data


class _Ensembles(_Stepped):
    """``ensembles`` (SelectStepEnsembleAggregator over _EnsembleAggregator, one_step/ensemble.py:176-441): per entry and name the
    per-pixel CRPS (``get_crps`` with alpha = 0.95, fme/core/ensemble.py:4-44), ensemble-mean RMSE and spread-skill-ratio bias at
    the window step whose global time index equals the entry's ``step`` - no ``n_ic_steps`` term, unlike ``_StepMeans`` - averaged
    over the records that held it.  The samples of a window are ``n_ic x n_members``, sample ``b = i * n_members + e``
    (``unfold_ensemble_dim``, fme/core/tensors.py:135-155), and the target is unfolded the same way: member ``e`` is compared with
    its own target plane.  The torch path restates CRPSMetric, EnsembleMeanRMSEMetric and SSRBiasMetric in torch ops on the
    window's dtype (and on ``normalize`` of the window for a norm entry); the fused path makes one ``ace_diag_ensemble_step`` per
    entry whose step lies in the window (csrc/ensemble.hip; the header contract in include/ace_sfno.h): four fp64 maps per entry
    and name - the sums of crps, sqrt(mse), mse - var / E and var - stay on the device until ``get_*``, where a norm entry is
    formed from them (crps / sigma, rmse / sigma, (mse, var) / sigma^2; a name without statistics is dropped).  An entry whose
    window has not come yet reports nothing.

    Logs (ensemble.py:291-352, tensors where the reference logs figures): ``<label>/<metric>/<name>`` the area-weighted mean of the
    map, with ``log_mean_maps`` ``<label>/<metric>/mean_map/<name>`` the (H, W) map, with ``target="norm"``
    ``<label>/<metric>/channel_mean``."""

    def __init__(self, agg, configs: Sequence, n_members: int):
        self._agg = agg
        self.configs = list(configs)
        self.kinds = {c.target for c in self.configs}
        self.n_members = int(n_members)
        self.calls = 0
        self._n = [0] * len(self.configs)                                 # records per entry (_n_batches)
        # torch path: entry -> name -> [crps, rmse, unbiased mse, variance] totals; entry -> name -> 0-dim bool, target all NaN
        self._t: List[Dict[str, List[torch.Tensor]]] = [{} for _ in self.configs]
        self._t_nan: List[Optional[Dict[str, torch.Tensor]]] = [None] * len(self.configs)
        # fused path: _maps (entries, 4, rows, H W) fp64, _seen (entries, rows) int32
        self._rows: Dict[str, int] = {}
        self._maps = self._seen = None

    def _selected(self, i_time_start: int, T: int):
        return [(i, c.step - i_time_start) for i, c in enumerate(self.configs) if i_time_start <= c.step < i_time_start + T]

    def record(self, w) -> int:
        todo = self._selected(w.i_time_start, w.T)
        return (self._record_fused if w.fused else self._record_torch)(w, todo) if todo else 0

    # ---- the torch path -----------------------------------------------------------------------------------------------
    def _record_torch(self, w, todo) -> int:
        E, B = self.n_members, w.B
        eps = (1.0 - ENSEMBLE_CRPS_ALPHA) / 2.0
        for i, k in todo:
            gen, tgt = w.kind(self.configs[i].target)
            unfold = lambda x: x[:, k:k + 1].reshape(B // E, E, 1, *x.shape[2:])      # noqa: E731  [batch, ensemble, time, H, W]
            for n, yb in tgt.items():
                g, y = unfold(gen[n]), unfold(yb)
                e0, e1 = torch.triu_indices(E, E, offset=1, device=g.device)
                internal = -0.5 * (g[:, e0] - g[:, e1]).abs().mean(dim=1)
                crps = (torch.mean(torch.abs(g - y), dim=1) + (1.0 - eps) * internal).mean(dim=(0, 1))
                mse = ((g.mean(dim=1, keepdim=True) - y) ** 2).mean(dim=(0, 1, 2))
                var = g.var(dim=1, unbiased=True).mean(dim=(0, 1))
                parts = [crps, mse.sqrt(), mse - var / E, var]
                tot = self._t[i].get(n)
                self._t[i][n] = parts if tot is None else [a + b for a, b in zip(tot, parts)]
            if self._t_nan[i] is None:
                self._t_nan[i] = {n: torch.isnan(unfold(y)).all() for n, y in tgt.items()}
            self._n[i] += 1
        return 0

    # ---- the fused path -----------------------------------------------------------------------------------------------
    def _record_fused(self, w, todo) -> int:
        """one ``ace_diag_ensemble_step`` per entry whose step lies in the window, for all paired names (fields with contiguous
        planes); returns the calls made"""
        from .. import _lib
        gen, tgt, dev, B, T = w.gen, w.tgt, w.device, w.B, w.T
        H, W = self._agg._shape
        E, HW = self.n_members, H * W
        if not 2 <= E <= MAX_ENSEMBLE_MEMBERS:
            raise ValueError(f"the fused ensemble pass keeps the members of a pixel in registers, at most {MAX_ENSEMBLE_MEMBERS}: "
                             f"{E} members per initial condition need the torch path (fused = False)")
        names = list(tgt)
        if _grow_rows(self, names, dev, _maps=lambda R: (len(self.configs), 4, R, HW)):
            self._seen = _grow(self._seen, (len(self.configs), self._maps.shape[2]), torch.int32, dev)
        at, _ = _upload_planes(names, gen, tgt, dev)
        rows32 = _upload([self._rows[n] for n in names], torch.int32, dev)
        lib = _lib.lib()
        pair_weight = 0.5 * (1.0 - (1.0 - ENSEMBLE_CRPS_ALPHA) / 2.0)
        for i, k in todo:
            _check(lib.ace_diag_ensemble_step(
                at["gen"], at["gen_strides"], at["target"], at["target_strides"], rows32.data_ptr(), self._maps.data_ptr(),
                self._seen.data_ptr(), self._maps.shape[2], i, len(self.configs), pair_weight, k, len(names), B // E, E, T, HW,
                _lib.current_stream()))
            self._n[i] += 1
        self.calls += len(todo)
        return len(todo)

    # ---- results ------------------------------------------------------------------------------------------------------
    def _maps_of(self, i: int):
        """entry i: name -> (crps, ensemble_mean_rmse, ssr_bias) (H, W) maps, and the names whose target is all NaN"""
        agg, c, nb = self._agg, self.configs[i], self._n[i]
        out: Dict[str, Any] = {}
        if self._maps is not None:
            seen = self._seen[i].tolist()
            nan_targets = {n for n, r in self._rows.items() if not seen[r]}
            for n, r in sorted(self._rows.items()):
                crps, rmse, umse, var = self._maps[i, :, r]
                if c.target == "norm":
                    if not agg._has_stats(n):
                        continue
                    sigma = agg._stats[n][1]
                    crps, rmse, umse, var = crps / sigma, rmse / sigma, umse / (sigma * sigma), var / (sigma * sigma)
                out[n] = (crps / nb, rmse / nb, ssr_bias(umse, var))
        else:
            nan_targets = {n for n, f in (self._t_nan[i] or {}).items() if bool(f)}
            for n, (crps, rmse, umse, var) in sorted(self._t[i].items()):
                out[n] = (crps / nb, rmse / nb, ssr_bias(umse, var))
        shape = agg._shape
        return {n: tuple(agg._reduce_mean(m.reshape(shape)) for m in maps) for n, maps in out.items()}, nan_targets

    def _entries(self):
        agg = self._agg
        for i, c in enumerate(self.configs):
            if self._n[i] == 0:
                continue
            maps, nan_targets = self._maps_of(i)
            data: Dict[str, Any] = {}
            for j, metric in enumerate(ENSEMBLE_METRICS):
                values = {}
                for n, per in maps.items():
                    m = per[j]
                    values[n] = float(_wmean(m, agg.weights_for(n, m.device).to(m.dtype)))
                    if c.variables is None or n in c.variables:
                        data[f"{metric}/{n}"] = values[n]
                        if c.log_mean_maps:
                            data[f"{metric}/mean_map/{n}"] = m.cpu()
                if c.target == "norm":
                    cm = _channel_mean(values, c.channel_mean_names, agg._channel_mean_names, nan_targets)
                    if cm is not None:
                        data[f"{metric}/channel_mean"] = cm
            yield c.name, data
