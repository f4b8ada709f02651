"""``InferenceEvaluatorAggregator``: validation, routing and the public ``get_*`` methods over the list of metric families."""
import contextlib
import logging
from typing import Any, Dict, List, Mapping, Optional, Sequence

import torch

from ..aggregator import InferenceAggregator, TensorMapping, _flat
from .calendar import _Calendar
from .common import Window
from .config import (EnsembleMetricConfig, EnsoCoefficientMetricConfig, HistogramMetricConfig, InferenceSummary, MetricConfig,
                     NearZeroFractionMetricConfig, StepMeanMetricConfig, TrendMetricConfig, VideoMetricConfig)
from .histogram import _Histograms
from .paired import LABELS, _Paired, _Spectrum, zonal_coarsening
from .regress import _Regress
from .stepped import _Ensembles, _StepMeans
from .video import _Video


class InferenceEvaluatorAggregator(InferenceAggregator):
    """main.py:526-732 for the sub-aggregators of the module docstring.  Weights, masks, routing and the SHT are the parent's."""

    def __init__(self, dataset_info, n_ic_steps: int, n_forward_steps: int, normalize, labels: Optional[Mapping[str, str]] = None,
                 skipped: Sequence[str] = (), zonal_mean_max_size: int = 4096, channel_mean_names: Optional[Sequence[str]] = None,
                 report_directional_bias: bool = True, output_dir: Optional[str] = None, save_diagnostics: bool = False,
                 sht_factory=None, spectrum_chunk_bytes: int = 256 << 20, histogram: Optional[HistogramMetricConfig] = None,
                 trend: Optional[TrendMetricConfig] = None, enso_coefficient: Optional[EnsoCoefficientMetricConfig] = None,
                 near_zero_fraction: Optional[NearZeroFractionMetricConfig] = None,
                 calendar: Optional[Mapping[str, MetricConfig]] = None, step_means: Sequence[StepMeanMetricConfig] = (),
                 ensembles: Sequence[EnsembleMetricConfig] = (), n_ensemble_per_ic: int = 1, fill_masked: bool = False,
                 video: Optional[VideoMetricConfig] = None, video_max_bytes: int = 32 << 30):
        super().__init__(dataset_info, n_ic_steps + n_forward_steps, True, output_dir, save_diagnostics, sht_factory,
                         spectrum_chunk_bytes, fill_masked_spectrum=fill_masked)
        self.n_ensemble_per_ic = int(n_ensemble_per_ic)
        self.n_ic_steps = int(n_ic_steps)
        self.skipped = list(skipped)
        labels = {k: k for k in LABELS} if labels is None else labels
        self._labels = {k: labels[k] for k in LABELS if k in labels}
        self._log_series = "mean" in self._labels or "mean_norm" in self._labels
        self._channel_mean_names = None if channel_mean_names is None else list(channel_mean_names)
        owner = getattr(normalize, "__self__", normalize)
        self._normalize_fn = normalize if callable(normalize) else getattr(normalize, "normalize", None)
        self._stats = None
        if hasattr(owner, "means") and hasattr(owner, "stds") and not getattr(owner, "fill_nans_on_normalize", False):
            self._stats = {n: (float(owner.means[n]), float(owner.stds[n])) for n in owner.means if n in owner.stds}
        self._factor, self._n_slots = zonal_coarsening(self._n_time, zonal_mean_max_size)
        # the metric families, in the order a window goes through them; a step mean is a column of the paired pass's series
        self._paired = _Paired(self, self._labels, {c.target for c in step_means})
        self._families: List[Any] = [self._paired]
        if video is not None and video.enabled:
            self._families.append(_Video(self, video, video_max_bytes))
        if histogram is not None and histogram.enabled:
            self._families.append(_Histograms(histogram))
        on = [None if m is None or not m.enabled else m for m in (trend, enso_coefficient, near_zero_fraction)]
        if any(m is not None for m in on):
            self._families.append(_Regress(self, *on))
        if calendar:
            self._families.append(_Calendar(self, calendar, dataset_info))
        if step_means:
            self._families.append(_StepMeans(self, step_means, self._paired))
        # main.py:560-562, 604-621: with one member per initial condition the ensemble entries are neither recorded nor reported
        if ensembles and self.n_ensemble_per_ic > 1:
            self._families.append(_Ensembles(self, ensembles, self.n_ensemble_per_ic))
        if "power_spectrum" in self._labels:
            self._families.append(_Spectrum(self, self._labels["power_spectrum"], report_directional_bias))
        self._need_norm = any(f.needs_norm for f in self._families)

    def _family(self, cls):
        return next((f for f in self._families if isinstance(f, cls)), None)

    _regress = property(lambda self: self._family(_Regress))             # what the tests and the benchmarks reach for
    _calendar = property(lambda self: self._family(_Calendar))
    _video = property(lambda self: self._family(_Video))
    _ensembles = property(lambda self: self._family(_Ensembles))

    # ---- routing ------------------------------------------------------------------------------------------------------
    def route(self, prediction: TensorMapping, target: Optional[TensorMapping] = None) -> str:
        """"fused" when recording this pair runs the HIP kernels, "torch" when it runs the torch ops."""
        if self._need_norm and self._stats is None:
            return "torch"
        return super().route({**{f"p:{k}": v for k, v in prediction.items()}, **{f"t:{k}": v for k, v in (target or {}).items()}})

    def launches(self) -> int:
        """Native launches made so far: one ``ace_diag_paired_window`` per window, one ``ace_diag_video_window`` per window of
        ``record_batch`` when the video is on, one ``ace_diag_hist_window`` per window of ``record_batch`` when the histogram is
        on, one ``ace_diag_regress_window`` per window of ``record_batch`` when any of
        trend, enso_coefficient and near_zero_fraction is on (a second one for the ENSO term of a window at time index 0), and
        one ``ace_diag_ensemble_step`` per ensemble entry and window that holds its step, and per spectrum chunk of either side
        one forward SHT and one ``ace_diag_spectrum`` - three with ``power_spectrum.fill_masked``: one ``ace_diag_fill_planes``
        ahead of them."""
        return self._launches

    def calendar_launches(self) -> int:
        """``ace_diag_calendar_window`` calls made so far (C-ABI calls, not kernel launches): one per window of ``record_batch``
        when any of seasonal, annual, enso_index and ipo_index is on.  Counted apart from ``launches``, whose total the metrics
        above define."""
        return sum(f.calls for f in self._families if not f.counted)

    @property
    def needs_time(self) -> bool:
        """True when ``record_batch`` raises without the window's time axis: the trend metric regresses against it, and a strict
        calendar metric (a ``SeasonalMetricConfig`` is strict unless told otherwise) groups the steps by it."""
        return any(f.needs_time for f in self._families)

    @property
    def uses_time(self) -> bool:
        """True when ``record_batch`` takes the window's time axis if it is given one: ``needs_time``, or a non-strict calendar
        metric is on (annual, enso_index and ipo_index are by default), which a ``record_batch`` without ``time`` drops with a
        warning and lists in ``skipped``."""
        return any(f.uses_time for f in self._families)

    def _without_time(self):
        """``record_batch`` came without a time axis: a family that cannot do without raises, the others (on by default) are dropped
        with one warning and their metrics listed in ``skipped``, as an unsupported metric is at build time."""
        dropped = [f for f in self._families if f.uses_time]
        names = [n for f in dropped for n in f.without_time()]
        logging.warning("record_batch was given no time axis; metrics not supported without it, omitting: " + ", ".join(names))
        self.skipped += [n for n in names if n not in self.skipped]
        self._families = [f for f in self._families if f not in dropped]

    # ---- recording ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def record_initial_condition(self, initial_condition: TensorMapping, target: Optional[TensorMapping] = None):
        """main.py:629-666: the initial condition (name -> (B, H, W) or (B, n_ic_steps, H, W)) feeds the series only; without
        ``target`` it is its own target (main.py:638-646).  Returns no per-step logs (reading them back would synchronise)."""
        if self._n_seen != 0:
            raise RuntimeError("record_initial_condition may only be called once, before recording any batches")
        fix = lambda d: {k: (v if v.dim() == 4 else v.unsqueeze(1)) for k, v in d.items()}      # noqa: E731
        gen = fix(initial_condition)
        if not gen:
            raise ValueError("data is empty")
        tgt = gen if target is None else fix(target)
        n = next(iter(gen.values())).shape[1]
        if n != self.n_ic_steps:
            raise ValueError(f"Expected {self.n_ic_steps} initial condition steps, but got {n}")
        if self._paired.series_kinds:
            self._record_pair(gen, tgt, 0, with_maps=False)
        self._n_seen = n
        return []

    @torch.no_grad()
    def record_batch(self, prediction: TensorMapping, target: TensorMapping, time=None, step_diagnostics=None):
        """main.py:579-627: a paired window, each name -> (B, T, H, W), at time index ``i_time_start`` = the steps seen so far;
        ``time``: the ``TimeAxis`` (B, T) of the window's steps, needed when ``needs_time``; ``step_diagnostics``: the window's
        ``StepDiagnostics``, recorded before the other metrics (main.py:588-592).  Returns no per-step logs and does not
        synchronise."""
        if len(prediction) == 0:
            raise ValueError("No prediction values in data")
        if len(target) == 0:
            raise ValueError("No target values in data")
        B, n = next(iter(prediction.values())).shape[:2]
        if B % self.n_ensemble_per_ic != 0:
            raise ValueError(f"a window of {B} samples is not a multiple of n_ensemble_per_ic = {self.n_ensemble_per_ic}")
        self._record_step_diagnostics(step_diagnostics)
        if self.uses_time and time is None:
            self._without_time()
        if self.uses_time:
            from ..timeaxis import as_time_axis
            time = as_time_axis(time)
        self._record_pair(dict(prediction), dict(target), self._n_seen, with_maps=True, time=time)
        self._n_seen += n
        return []

    def _record_pair(self, gen: Dict[str, torch.Tensor], tgt: Dict[str, torch.Tensor], i_time_start: int, with_maps: bool,
                     time=None):
        first = next(iter(gen.values()))
        B, T = first.shape[:2]
        if i_time_start + T > self._n_time:
            raise ValueError(f"steps {i_time_start}..{i_time_start + T - 1} are past the aggregator's n_timesteps {self._n_time}")
        if tuple(first.shape[-2:]) != self._shape:
            raise ValueError(f"fields of shape {tuple(first.shape[-2:])} on an aggregator of {self._shape}")
        for n, y in tgt.items():
            if n not in gen:
                raise ValueError(f"target name '{n}' has no prediction")
            if y.shape != gen[n].shape:
                raise RuntimeError(f"Tensors in target and gen must have the same shape, but got {tuple(y.shape)} and "
                                   f"{tuple(gen[n].shape)} for the tensor '{n}'.")
        zonal = with_maps and "zonal_mean" in self._labels
        if zonal and T < self._factor:
            raise ValueError(f"a window of {T} steps is shorter than the zonal mean's time coarsening factor {self._factor}")
        fused = self._pick(gen, tgt) == "fused"
        if fused:
            W, given = first.shape[-1], gen
            gen = {n: _flat(x, W) for n, x in given.items()}
            tgt = {n: (gen[n] if y is given[n] else _flat(y, W)) for n, y in tgt.items()}
        if with_maps:
            for n in gen:                                  # ``omitted`` lists a masked name whether or not the spectrum is on
                self._omitted(n)
        window = Window(gen, tgt, i_time_start, time, with_maps, fused, self._normalize_fn)
        with torch.cuda.device(first.device) if fused else contextlib.nullcontext():
            for family in self._families if with_maps else [self._paired]:      # the initial condition feeds the series only
                made = family.record(window)
                self._launches += made if family.counted else 0

    # ---- results --------------------------------------------------------------------------------------------------------
    def _has_stats(self, name: str) -> bool:
        return self._stats is not None and name in self._stats

    @torch.no_grad()
    def get_dataset(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """get_reduced_diagnostics with the reference's variable keys (CPU tensors): ``mean`` / ``mean_norm``:
        ``<metric>-<name>`` (T,); ``time_mean`` / ``time_mean_norm``: ``bias_map-<name>``, ``gen_map-<name>`` (H, W);
        ``power_spectrum``: ``<name>`` (2, lmax) with the leading source axis [prediction, target]; ``zonal_mean``:
        ``gen-<name>``, ``error-<name>`` (n_slots, H)."""
        out = self._blocks("dataset")
        if self._correction is not None:
            out.update(self._correction.datasets())
        return out

    def _blocks(self, which: str) -> Dict[str, Dict[str, Any]]:
        """label -> block of every family's ``dataset()`` or ``logs()``, the paired labels first in their reporting order (the
        spectrum reports between the time means and the zonal mean, and records last), then the families in list order"""
        out: Dict[str, Dict[str, Any]] = {}
        for family in self._families:
            out.update(getattr(family, which)())
        return {label: out[label] for label in (*self._labels.values(), *out) if label in out}

    @torch.no_grad()
    def get_summary(self) -> InferenceSummary:
        """main.py:668-676: the logs of the sub-aggregators that are not time series, and ``loss`` =
        ``time_mean_norm/rmse/channel_mean``."""
        logs = {f"{label}/{k}": v for label, block in self._blocks("logs").items() for k, v in block.items()}
        if self._correction is not None:
            logs.update(self._correction.summary_logs())
        key = self._labels.get("time_mean_norm")
        return InferenceSummary(logs=logs, loss=logs.get(f"{key}/rmse/channel_mean") if key else None)

    def get_summary_logs(self) -> Dict[str, Any]:
        return self.get_summary().logs

    @torch.no_grad()
    def get_inference_logs(self) -> List[Dict[str, Any]]:
        """to_inference_logs (main.py:751-772): one dict per time index with ``<label>/forecast_step`` and
        ``<label>/<metric>/<name>`` floats for both ``mean`` labels; the summary logs go in the last dict."""
        rows: List[Dict[str, Any]] = [{} for _ in range(self._n_time if self._log_series else 1)]
        for kind, label in self._paired._kinds("mean", "mean_norm"):
            series = {f"{m}/{n}": v.cpu().tolist() for m, d in self._paired._series_data(kind).items() for n, v in d.items()}
            for i, row in enumerate(rows):
                row[f"{label}/forecast_step"] = i
                for k in sorted(series):
                    row[f"{label}/{k}"] = series[k][i]
        if self._correction is not None and self._log_series:
            for row, extra in zip(rows, self._correction.series_rows()):
                row.update(extra)
        rows[-1].update(self.get_summary_logs())
        return rows
