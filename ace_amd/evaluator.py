"""The inference evaluator aggregator on a lat-lon grid (fme/ace/aggregator/inference/main.py:186-361, 526-732): a rollout
compared against a target record, for ``ace_amd.inference.run_evaluator``.  Built sub-aggregators, under the reference's labels:

  * ``mean`` / ``mean_norm`` (reduced.py:221-348): per time index ``weighted_rmse``, ``weighted_bias``, ``weighted_mean_gen``,
    ``weighted_mean_target``, ``weighted_std_gen`` and, denormalised only (reduced.py:248-255), ``weighted_grad_mag_percent_diff``;
  * ``time_mean`` / ``time_mean_norm`` (time_mean.py:246-444): the time-mean maps of both sides, their bias map, RMSE and bias, and
    ``time_mean_norm/rmse/channel_mean``, which ``get_summary`` returns as the inference ``loss`` (main.py:668-676);
  * ``power_spectrum`` (spectrum.py:112-276): the mean spectra of prediction and target and their bias scores;
  * ``zonal_mean`` (zonal_mean.py:50-355): time-latitude maps of both sides and of their difference, coarsened in time;
  * ``histogram`` (histogram.py:12-82 on fme/core/histogram.py:121-509), off by default and built from a ``HistogramMetricConfig``
    only: a 200-bin dynamic histogram of every paired name for prediction and target over the windows of ``record_batch``, the
    99.9999th percentiles of both, and the trimmed densities as tensors where the reference logs a figure (``_Histograms``);
  * ``trend`` (trend.py:46-314), off by default and built from a ``TrendMetricConfig`` only: the per-pixel least-squares slope of
    every name against time in years since 2000-01-01 (a fixed 365.25-day year) for target and prediction, in fp64, and the
    area-weighted RMSE between the two maps.  It needs the time axis of each window: ``record_batch(..., time=)``, which
    ``inference.run_evaluator`` hands to an aggregator whose ``needs_time`` is set;
  * ``enso_coefficient`` (enso/enso_coefficient.py:61-500), built from an ``EnsoCoefficientMetricConfig`` that carries an
    ``index``: per pixel the regression coefficient of every name on a zero-mean index series, per sample, averaged over the
    samples, for target and prediction, and the area-weighted RMSE of the two maps.  The one stated difference: the reference looks
    the index up in its own monthly Nino 3.4 table, which is not shipped here; the caller supplies the index values at every time
    level of every sample, a row with a non-finite value standing for the reference's sample without a series.  Without an index
    the metric is skipped, as it always was;
  * ``near_zero_fraction`` (near_zero_fraction.py:20-300), off by default and built from a ``NearZeroFractionMetricConfig`` only:
    the area-weighted fraction of cells ``<= eps`` of the named variables for the prediction and its difference from the target's,
    and with ``include_maps`` the per-cell fractions (``_Regress`` holds these three);
  * ``annual`` (annual.py:24-455), ``enso_index`` (enso/dynamic_index.py:36-399) and ``ipo_index`` (ipo/ipo_index.py:90-400), on by
    default, and ``seasonal`` (seasonal.py:22-265), off by default, built from their typed configurations only
    (``AnnualMetricConfig``, ``EnsoIndexMetricConfig``, ``IpoIndexMetricConfig``, ``SeasonalMetricConfig``): per-sample yearly
    global means with their RMSE and fair CRPS over years; the Nino 3.4 index (monthly anomalies, 5-month running mean) with its
    standard deviation, power spectrum and band powers; the tripole index with its 13-year low pass (needs ``scipy.signal``);
    seasonal mean maps with bias, anomaly, R2 and area-mean RMSE (``_Calendar`` holds these four).  They group the steps of
    ``record_batch`` by the calendar of ``time=``; a non-strict one that gets no time axis is dropped with a warning and listed
    in ``skipped`` (``uses_time``), a strict one raises (``needs_time``).  As in the reference, annual and enso_index need a
    record of more than 730 days, ipo_index of more than 80 x 365 days, and the two indices need lat and lon;
  * ``step_means`` (one_step/reduced.py:24-249), built from ``StepMeanMetricConfig`` entries only: ``weighted_rmse``,
    ``weighted_bias`` and ``weighted_grad_mag_percent_diff`` of the snapshot at time index ``step + n_ic_steps - 1``, or with
    ``target="norm"`` the normalised RMSE and its ``channel_mean`` (``_StepMeans``: a column of the ``mean`` series, which is
    then recorded even with ``mean_denorm`` and ``mean_norm`` off);
  * ``ensembles`` (one_step/ensemble.py:74-505), built from ``EnsembleMetricConfig`` entries only and recorded only when
    ``build(..., n_ensemble_per_ic=E)`` has ``E > 1``: the samples of a window are ``n_ic x E`` members (sample ``b = i E + e``),
    and at the step whose time index equals ``step`` - no ``n_ic_steps`` term - the per-pixel almost-fair CRPS (alpha = 0.95),
    ensemble-mean RMSE and spread-skill-ratio bias, their area-weighted means, with ``log_mean_maps`` the maps and with
    ``target="norm"`` the channel means (``_Ensembles``).

Not built, skipped at build time with one warning and listed in ``skipped`` as the reference's non-strict path does
(main.py:143-153): a ``step_means`` or ``ensembles`` entry given as a bare ``MetricConfig`` (the defaults; listed under the field's
name) or whose ``step`` exceeds ``n_forward_steps`` (listed under its own name), an ``annual``, ``enso_index`` or ``ipo_index``
given as a bare ``MetricConfig`` or whose record is too short, an ``enso_coefficient`` without an index or over a record of 1800 days or less, a ``trend`` over fewer
than two forward steps.  ``video``, a ``seasonal``, ``histogram``, ``trend`` or ``near_zero_fraction`` enabled through a bare
``MetricConfig``, the reference-data paths (``annual.reference_data`` among them), a ``variables`` filter on any metric but the
histogram, the trend, the near-zero fraction, annual and seasonal, HEALPix grids and ``strict=True`` on a skipped metric raise
``NotImplementedError``.  As in ace_amd/aggregator.py, tensors and floats stand where the
reference logs images and figures, and a name whose mask has zeros is left out of the spectrum and listed in ``omitted``.

Paired metrics cover the names present in both mappings, ``weighted_mean_gen`` / ``weighted_std_gen`` every generated name; a target
name without a prediction is refused (the reference indexes ``gen[name]`` for every target name, reduced.py:190-196).

Two paths compute the same thing.  The torch path (``fused = False``, any device) is the reference's formulas in torch ops on the
window and on ``normalize`` of the window.  The fused path (CUDA fp32 windows) makes one ``ace_diag_paired_window`` call per window
(csrc/diag.hip: every quantity above from one pass over each plane, a band's halo rows re-read through the cache; fp64, fixed
order, no atomics, no host synchronisation) and per
spectrum chunk one SHT and one ``ace_diag_spectrum`` for each side, and with the histogram on one ``ace_diag_hist_window`` per window
(csrc/hist.hip: range, update and binning passes on device-resident state, integer counts bitwise equal to the torch path's, nothing
read back before ``get_*``), and with any of trend, enso_coefficient and near_zero_fraction on one ``ace_diag_regress_window`` per
window for the three together (csrc/regress.hip: every plane read once, the fp64 sums of a pixel kept in registers), and with any
of seasonal, annual, enso_index and ipo_index on one ``ace_diag_calendar_window`` per window for the four together
(csrc/calendar.hip: every plane read once for the seasonal sums and the regional means, which stay on the device until ``get_*``),
and per ensemble entry one ``ace_diag_ensemble_step`` in the window that holds its step (csrc/ensemble.hip: the members of a pixel in
registers, the target planes streamed, four fp64 maps per name that stay on the device until ``get_*``).
It never normalises a field: ``normalize`` is (x - mu) / sigma
per name (fme/core/normalizer.py:213-227), every per-sample quantity is linear in it (rmse / sigma, bias / sigma, (mean - mu) /
sigma, std / sigma, and the time-mean RMSE / sigma), so the ``_norm`` outputs are formed from the denormalised fp64 accumulators at
``get_*`` time.  Names without statistics are dropped from the ``_norm`` outputs, as ``normalize`` drops them
(normalizer.py:159).  A normaliser that fills NaNs (not linear) or exposes no statistics takes the torch path.

The one deliberate difference from the reference: the zonal mean adds each step at its coarsened slot ``(t - t_first) // factor``
scaled by 1 / factor, which equals the reference's buffer-carry form (zonal_mean.py:192-266) whenever every window has at least
``factor`` steps; a shorter window raises ``ValueError`` where the reference silently drops it (zonal_mean.py:181-190).  Zonal
accumulator memory: names x 2 x slots x H x 8 bytes (40 names, 4096 slots, 180 latitudes: 472 MB; the default
``zonal_mean_max_size`` only coarsens past 4096 steps)."""
import dataclasses
import datetime
import itertools
import logging
import math
import os
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence

import torch

from .aggregator import InferenceAggregator, TensorMapping, _check, _flat, _grow, _is_healpix, _plane_table, _upload

SERIES = ("weighted_mean_gen", "weighted_std_gen", "weighted_mean_target", "weighted_bias", "weighted_rmse",
          "weighted_grad_mag_percent_diff")                               # the rows of the fused series accumulator
NORM_SERIES = SERIES[:5]                                                  # reduced.py:248-255: the percent diff is denorm-only
_SHIFTED = ("weighted_mean_gen", "weighted_mean_target")                  # (v - mu) / sigma; the others v / sigma


@dataclasses.dataclass
class MetricConfig:
    """The fields every metric configuration of the reference shares (e.g. reduced.py:506-512)."""
    enabled: bool = True
    strict: bool = False
    variables: Optional[List[str]] = None
    name: Optional[str] = None


@dataclasses.dataclass
class ZonalMeanMetricConfig(MetricConfig):
    zonal_mean_max_size: int = 4096                                       # zonal_mean.py:357-363


@dataclasses.dataclass
class PowerSpectrumMetricConfig(MetricConfig):
    report_directional_bias: bool = True                                  # spectrum.py:317-322


@dataclasses.dataclass
class HistogramMetricConfig(MetricConfig):
    """histogram.py:12-45.  ``variables``: record these names only; ``percentile_variables``: emit the percentile scalars for these
    names only (the densities are still logged for every recorded name)."""
    enabled: bool = False
    strict: bool = True
    name: Optional[str] = "histogram"
    percentile_variables: Optional[List[str]] = None

    def __post_init__(self):
        if self.variables is not None and self.percentile_variables is not None:
            extra = set(self.percentile_variables) - set(self.variables)
            if extra:
                raise ValueError(f"percentile_variables contains names not in variables: {sorted(extra)}")


@dataclasses.dataclass
class TrendMetricConfig(MetricConfig):
    """trend.py:279-314.  ``variables``: compute trends for these names only."""
    enabled: bool = False
    strict: bool = False
    name: Optional[str] = "trend"


@dataclasses.dataclass
class NearZeroFractionMetricConfig(MetricConfig):
    """near_zero_fraction.py:20-94: the area-weighted fraction of cells ``<= eps`` of ``variables`` (``per_variable_eps``
    overriding ``eps`` per name); ``include_maps``: also the per-cell fraction maps."""
    enabled: bool = False
    strict: bool = True
    variables: List[str] = dataclasses.field(default_factory=list)
    name: Optional[str] = "near_zero_fraction"
    eps: float = 0.0
    per_variable_eps: Dict[str, float] = dataclasses.field(default_factory=dict)
    include_maps: bool = False

    def __post_init__(self):                                              # near_zero_fraction.py:61-80
        if not self.enabled:
            return
        if not self.variables:
            raise ValueError("NearZeroFractionMetricConfig is enabled but no variables were given; specify the variables to "
                             "compute the metric for.")
        if self.eps < 0:
            raise ValueError(f"NearZeroFractionMetricConfig.eps must be >= 0, got {self.eps}.")
        negative = {var: value for var, value in self.per_variable_eps.items() if value < 0}
        if negative:
            raise ValueError(f"NearZeroFractionMetricConfig.per_variable_eps values must be >= 0, got {negative}.")


@dataclasses.dataclass
class EnsoCoefficientMetricConfig(MetricConfig):
    """enso_coefficient.py:440-500 with the index supplied by the caller: ``index`` is a (B, n_ic_steps + n_forward_steps) tensor of
    index values at every time level of every sample (the reference looks them up in its own monthly Nino 3.4 table, which is not
    shipped here); ``None`` leaves the metric skipped."""
    enabled: bool = True
    strict: bool = False
    name: Optional[str] = "enso_coefficient"
    index: Optional[Any] = None


@dataclasses.dataclass
class AnnualMetricConfig(MetricConfig):
    """annual.py:423-455.  ``variables``: annual means of these names only; ``reference_data`` is a netCDF path and is refused."""
    name: Optional[str] = "annual"
    reference_data: Optional[str] = None
    report_crps: bool = True
    report_rmse: bool = True


@dataclasses.dataclass
class EnsoIndexMetricConfig(MetricConfig):
    """enso/dynamic_index.py:358-399"""
    name: Optional[str] = "enso_index"


@dataclasses.dataclass
class IpoIndexMetricConfig(MetricConfig):
    """ipo/ipo_index.py:374-400"""
    name: Optional[str] = "ipo_index"


@dataclasses.dataclass
class SeasonalMetricConfig(MetricConfig):
    """seasonal.py:250-265.  ``variables``: seasonal means of these names only."""
    enabled: bool = False
    strict: bool = True
    name: Optional[str] = "seasonal"


@dataclasses.dataclass
class StepMeanMetricConfig(MetricConfig):
    """one_step/reduced.py:207-249: the ``mean`` metrics of one forward step, the snapshot at time index
    ``step + n_ic_steps - 1``.  ``target``: "denorm" (RMSE, bias, gradient-magnitude percent difference per name) or "norm" (RMSE
    per name and their ``channel_mean`` over ``channel_mean_names``, else the aggregator's, else every name); ``variables``: report
    the per-name entries of these names only (the channel mean still runs over all).  ``step`` has a default only because the
    fields of the base class have; ``name`` defaults to ``mean_step_{step}`` / ``mean_step_{step}_norm``."""
    step: int = 20
    target: str = "denorm"
    channel_mean_names: Optional[List[str]] = None

    def __post_init__(self):
        if self.target not in ("denorm", "norm"):
            raise ValueError(f"target must be 'denorm' or 'norm', got {self.target!r}")
        if self.name is None:
            self.name = f"mean_step_{self.step}" + ("_norm" if self.target == "norm" else "")


@dataclasses.dataclass
class EnsembleMetricConfig(MetricConfig):
    """one_step/ensemble.py:444-505: CRPS, spread-skill-ratio bias and ensemble-mean RMSE at the window step whose global time
    index equals ``step`` - with no ``n_ic_steps`` term, unlike the step means (ensemble.py:485-497 hands ``step`` to
    SelectStepEnsembleAggregator as the global index; reduced.py:231 adds ``n_ic_steps - 1``).  ``log_mean_maps``: also the
    per-pixel maps; ``target`` and ``channel_mean_names`` as in ``StepMeanMetricConfig``; ``name`` defaults to
    ``ensemble_step_{step}`` / ``ensemble_step_{step}_norm``."""
    step: int = 20
    log_mean_maps: bool = False
    target: str = "denorm"
    channel_mean_names: Optional[List[str]] = None

    def __post_init__(self):
        if self.target not in ("denorm", "norm"):
            raise ValueError(f"target must be 'denorm' or 'norm', got {self.target!r}")
        if self.name is None:
            self.name = f"ensemble_step_{self.step}" + ("_norm" if self.target == "norm" else "")


def _off() -> MetricConfig:
    return MetricConfig(enabled=False, strict=True)


@dataclasses.dataclass
class InferenceSummary:
    logs: Dict[str, Any]
    loss: Optional[float]


@dataclasses.dataclass
class InferenceEvaluatorAggregatorConfig:
    """main.py:186-361 (same field names and defaults; each metric carries ``enabled`` and ``strict``)."""
    mean_denorm: MetricConfig = dataclasses.field(default_factory=MetricConfig)
    mean_norm: MetricConfig = dataclasses.field(default_factory=MetricConfig)
    step_means: List[MetricConfig] = dataclasses.field(default_factory=lambda: [MetricConfig(), MetricConfig()])
    ensembles: List[MetricConfig] = dataclasses.field(default_factory=lambda: [MetricConfig()])
    power_spectrum: PowerSpectrumMetricConfig = dataclasses.field(default_factory=PowerSpectrumMetricConfig)
    zonal_mean: ZonalMeanMetricConfig = dataclasses.field(default_factory=ZonalMeanMetricConfig)
    time_mean_denorm: MetricConfig = dataclasses.field(default_factory=MetricConfig)
    time_mean_norm: MetricConfig = dataclasses.field(default_factory=MetricConfig)
    video: MetricConfig = dataclasses.field(default_factory=_off)
    histogram: MetricConfig = dataclasses.field(default_factory=HistogramMetricConfig)
    seasonal: MetricConfig = dataclasses.field(default_factory=SeasonalMetricConfig)
    annual: MetricConfig = dataclasses.field(default_factory=AnnualMetricConfig)
    enso_index: MetricConfig = dataclasses.field(default_factory=EnsoIndexMetricConfig)
    enso_coefficient: MetricConfig = dataclasses.field(default_factory=EnsoCoefficientMetricConfig)
    ipo_index: MetricConfig = dataclasses.field(default_factory=IpoIndexMetricConfig)
    trend: MetricConfig = dataclasses.field(default_factory=TrendMetricConfig)
    near_zero_fraction: MetricConfig = dataclasses.field(default_factory=NearZeroFractionMetricConfig)
    monthly_reference_data: Optional[str] = None
    time_mean_reference_data: Optional[str] = None
    step_diagnostics: Optional[Any] = None

    BUILT = {"mean_denorm": "mean", "mean_norm": "mean_norm", "time_mean_denorm": "time_mean", "time_mean_norm": "time_mean_norm",
             "power_spectrum": "power_spectrum", "zonal_mean": "zonal_mean"}
    NEVER_BUILT = ("video", "seasonal")
    TYPED = {"histogram": HistogramMetricConfig, "trend": TrendMetricConfig, "near_zero_fraction": NearZeroFractionMetricConfig}
    SKIPPED = ("step_means", "ensembles")                                 # main.py:143-153, the non-strict path
    # list fields: an entry of the typed class is built (_StepMeans, _Ensembles), a bare MetricConfig is what it always was
    STEPPED = {"step_means": StepMeanMetricConfig, "ensembles": EnsembleMetricConfig}
    # built by _Calendar from their typed configurations; a bare MetricConfig in one of these fields is what it always was: an
    # enabled annual / enso_index / ipo_index skipped (or raised when strict), an enabled seasonal "not built"
    CALENDAR = {"seasonal": SeasonalMetricConfig, "annual": AnnualMetricConfig, "enso_index": EnsoIndexMetricConfig,
                "ipo_index": IpoIndexMetricConfig}

    def _calendar_unsupported(self, field: str, dataset_info, n_timesteps: int) -> Optional[str]:
        """why the reference's ``build`` of this metric would raise MetricNotSupportedError here (annual.py:436-442,
        dynamic_index.py:367-381, ipo_index.py:383-394), or None"""
        if field == "seasonal":
            return None
        timestep = getattr(dataset_info, "timestep", None)
        if timestep is None:
            return "the dataset has no timestep"
        coords = getattr(dataset_info, "horizontal_coordinates", None)
        if field != "annual" and (getattr(coords, "lat", None) is None or getattr(coords, "lon", None) is None):
            return "requires lat-lon coordinates"
        total = n_timesteps * timestep
        if field == "ipo_index":
            if total <= datetime.timedelta(days=MIN_YEARS_FOR_FILTERED_TPI * 365):
                return f"requires > ~{MIN_YEARS_FOR_FILTERED_TPI} years of data, got {total.days} days"
            try:
                import scipy.signal  # noqa: F401  (the Chebyshev filter of the filtered scalars)
            except ImportError:
                return "requires scipy.signal"
        elif total <= datetime.timedelta(days=730):
            return f"requires > ~2 years of data, got {total.days} days"
        return None

    def build(self, dataset_info, n_ic_steps: int, n_forward_steps: int, normalize, output_dir: Optional[str] = None,
              channel_mean_names: Optional[Sequence[str]] = None, save_diagnostics: bool = False,
              sht_factory: Optional[Callable[[int, int], Callable]] = None,
              n_ensemble_per_ic: int = 1) -> "InferenceEvaluatorAggregator":
        """``normalize``: a ``StandardNormalizer``, its bound ``normalize``, or anything exposing per-name ``means`` and ``stds``
        (the fused path reads the statistics, the torch path calls it); a bare callable serves the torch path only.
        ``n_ensemble_per_ic``: the samples of a window are ``n_ic x n_ensemble_per_ic`` members, sample ``b = i * n_ensemble_per_ic +
        e`` (``inference.repeat_members``); with 1 the ensemble entries are accepted but neither recorded nor reported
        (main.py:560-562, 604-621)."""
        if int(n_ensemble_per_ic) < 1:
            raise ValueError(f"n_ensemble_per_ic must be >= 1, got {n_ensemble_per_ic}")
        if self.monthly_reference_data is not None or self.time_mean_reference_data is not None:
            raise NotImplementedError("monthly_reference_data / time_mean_reference_data are netCDF files and there is no netCDF "
                                      "reader here; compare the maps of get_dataset() offline")
        if self.step_diagnostics not in (None, {}):
            raise NotImplementedError("step_diagnostics: only the default configuration is supported (no step-diagnostics "
                                      "aggregator is built)")
        for field in self.NEVER_BUILT:
            if getattr(self, field).enabled and not isinstance(getattr(self, field), self.CALENDAR.get(field, ())):
                raise NotImplementedError(f"the {field} metric is not built")
        for field, typed in self.TYPED.items():
            if getattr(self, field).enabled and not isinstance(getattr(self, field), typed):
                if field == "histogram":
                    raise NotImplementedError("the histogram metric is built from its typed configuration only: pass a "
                                              "HistogramMetricConfig, not a bare MetricConfig")
                raise NotImplementedError(f"the {field} metric is not built")
        skipped = []
        trend = self.trend if self.trend.enabled else None
        if trend is not None and n_forward_steps < 2:                     # trend.py:300-308, through the skipped-metric path
            if trend.strict:
                raise NotImplementedError(f"trend metric requires at least 2 forward steps, got {n_forward_steps} (strict=True)")
            skipped.append("trend")
            trend = None
        enso = self.enso_coefficient
        if not (enso.enabled and isinstance(enso, EnsoCoefficientMetricConfig) and enso.index is not None):
            enso = None
        elif getattr(dataset_info, "timestep", None) is not None and \
                (n_ic_steps + n_forward_steps) * dataset_info.timestep <= datetime.timedelta(days=1800):
            enso = None                                                   # enso_coefficient.py:478-483; skipped or raised below
        annual = self.annual
        if annual.enabled and isinstance(annual, AnnualMetricConfig) and annual.reference_data is not None:
            raise NotImplementedError("annual.reference_data is a netCDF file and there is no netCDF reader here; compare the "
                                      "series of get_dataset() offline")
        calendar: Dict[str, MetricConfig] = {}
        why: Dict[str, Optional[str]] = {}
        unbuilt = list(self.SKIPPED)
        for field in ("seasonal", "annual", "enso_index", "enso_coefficient", "ipo_index"):      # their order in the reference's list
            m = getattr(self, field)
            if field == "enso_coefficient":
                if enso is None:
                    unbuilt.append(field)
            elif not (m.enabled and isinstance(m, self.CALENDAR[field])):
                if field != "seasonal":
                    unbuilt.append(field)
            else:
                why[field] = self._calendar_unsupported(field, dataset_info, n_ic_steps + n_forward_steps)
                if why[field] is None:
                    calendar[field] = m
                else:
                    unbuilt.append(field)
        stepped: Dict[str, List[MetricConfig]] = {field: [] for field in self.STEPPED}
        late: List[str] = []
        for field, typed in self.STEPPED.items():
            what = "step_mean step" if field == "step_means" else "ensemble step"
            for m in getattr(self, field):
                if not (m.enabled and isinstance(m, typed)):
                    continue
                if m.step > n_forward_steps:                              # reduced.py:226-230, ensemble.py:486-490
                    reason = f"{what} {m.step} exceeds n_forward_steps={n_forward_steps}"
                    if m.strict:
                        raise NotImplementedError(f"the {m.name} metric is not supported for this configuration: {reason} "
                                                  "(strict=True)")
                    late.append(m.name)
                else:
                    stepped[field].append(m)
        for field in unbuilt:
            v = getattr(self, field)
            for m in (v if isinstance(v, list) else [v]):
                if not m.enabled or isinstance(m, self.STEPPED.get(field, ())):
                    continue
                if m.strict and field in why:
                    raise NotImplementedError(f"the {field} metric is not supported for this configuration: {why[field]} "
                                              "(strict=True)")
                if m.strict:
                    raise NotImplementedError(f"the {field} metric is not built (strict=True)")
                if field not in skipped:
                    skipped.append(field)
        skipped += [n for n in late if n not in skipped]
        if skipped:
            logging.warning("metrics not supported for this configuration, omitting: " + ", ".join(skipped))
        labels = {}
        for field, default in self.BUILT.items():
            m = getattr(self, field)
            if m.variables is not None:
                raise NotImplementedError(f"{field}.variables: a per-metric variable filter is not built")
            if m.enabled:
                labels[default] = m.name or default
        taken = list(labels.values())                                     # every label that heads a block of the logs and the dataset
        taken += [m.name or field for field, m in (("histogram", self.histogram), ("trend", trend), ("enso_coefficient", enso),
                                                   ("near_zero_fraction", self.near_zero_fraction))
                  if m is not None and m.enabled]
        taken += [m.name or field for field, m in calendar.items()]
        for m in stepped["step_means"] + stepped["ensembles"]:
            if m.name in taken:
                raise ValueError(f"two metrics are named '{m.name}'; give one of them another name")
            taken.append(m.name)
        if _is_healpix(dataset_info):
            raise NotImplementedError("the inference evaluator aggregator is built for lat-lon grids only, not HEALPix")
        if getattr(dataset_info, "area_weights", None) is None:
            raise ValueError("the inference evaluator aggregator needs the dataset's area weights: build the DatasetInfo with lat "
                             "(and lon) or area_weights")
        return InferenceEvaluatorAggregator(
            dataset_info, int(n_ic_steps), int(n_forward_steps), normalize, labels=labels, skipped=skipped,
            zonal_mean_max_size=getattr(self.zonal_mean, "zonal_mean_max_size", 4096), channel_mean_names=channel_mean_names,
            report_directional_bias=getattr(self.power_spectrum, "report_directional_bias", True), output_dir=output_dir,
            save_diagnostics=save_diagnostics, sht_factory=sht_factory,
            histogram=self.histogram if self.histogram.enabled else None, trend=trend, enso_coefficient=enso,
            near_zero_fraction=self.near_zero_fraction if self.near_zero_fraction.enabled else None, calendar=calendar,
            step_means=stepped["step_means"], ensembles=stepped["ensembles"], n_ensemble_per_ic=int(n_ensemble_per_ic))


# ---- the reference's formulas in torch ops (the torch path) ---------------------------------------------------------------------
def _wmean(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """metrics.py:63-90 over the last two dimensions"""
    w = w.expand(x.shape)
    return (x.where(w != 0.0, 0.0) * w).sum(dim=(-2, -1)) / w.sum(dim=(-2, -1))


def _wstd(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """metrics.py:118-143"""
    return _wmean((x - _wmean(x, w)[..., None, None]) ** 2, w).sqrt()


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


HIST_BINS = 200                                                           # histogram.py:59
HIST_PERCENTILES = (99.9999,)


def trim_zero_bins(counts, edges):
    """fme/core/histogram.py:52-71: the empty bins at both ends removed"""
    import numpy as np
    mask = counts > 0
    first, last = int(np.argmax(mask)), len(mask) - int(np.argmax(mask[::-1]))
    return counts[first:last], edges[first:last + 1]


def histogram_quantile(edges, counts, probability: float) -> float:
    """fme/core/metrics.py:355-385: the inverse CDF, linear inside a bin"""
    import numpy as np
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
    fused path reads nothing back before ``dataset`` / ``logs``."""

    def __init__(self, config: HistogramMetricConfig):
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

    # ---- the torch path -----------------------------------------------------------------------------------------------
    def record_torch(self, gen, tgt):
        import numpy as np
        gen, tgt = self._select(gen, tgt)
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

    # ---- the fused path -----------------------------------------------------------------------------------------------
    def record_fused(self, gen, tgt) -> int:
        """one ``ace_diag_hist_window`` for both sides and all names of fields with contiguous planes; returns the launches made"""
        from . import _lib
        gen, tgt = self._select(gen, tgt)
        names = self._names
        n, first = len(names), gen[names[0]]
        dev, (B, T, H, W) = first.device, first.shape
        if self._range is None:
            self._range = torch.full((2, n, 2), math.nan, dtype=torch.float64, device=dev)
            self._counts = torch.zeros(2, n, HIST_BINS, dtype=torch.int64, device=dev)
            self._dropped = torch.zeros(2, n, dtype=torch.int32, device=dev)
            self._mask_planes = torch.stack([self._masks[nm].reshape(H * W) for nm in names]).to(torch.uint8).contiguous()
            self._rows = _upload(list(range(n)), torch.int32, dev)
        values, off = _plane_table(names, gen, tgt)
        values += [self._mask_planes.data_ptr() + i * H * W for i in range(n)]      # the mask pointers, from off["end"]
        table = _upload(values, torch.int64, dev)
        lib = _lib.lib()
        scratch = torch.empty(int(lib.ace_diag_hist_scratch_bytes(n, B, T, H * W)), dtype=torch.uint8, device=dev)
        at = {k: table.data_ptr() + o for k, o in off.items()}
        _check(lib.ace_diag_hist_window(at["gen"], at["gen_strides"], at["target"], at["target_strides"], self._rows.data_ptr(),
                                        at["end"], scratch.data_ptr(), self._range.data_ptr(), self._counts.data_ptr(),
                                        self._dropped.data_ptr(), n, HIST_BINS, n, B, T, H * W, _lib.current_stream()))
        return 1

    # ---- results ------------------------------------------------------------------------------------------------------
    def _state(self):
        """name -> ([target, prediction] int64 counts (2, n_bins), fp64 edges (2, n_bins + 1), dropped windows)"""
        import numpy as np
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

    def dataset(self) -> Dict[str, torch.Tensor]:
        """fme/core/histogram.py:480-509: ``<name>`` (2, n_bins) int64 and ``<name>_bin_edges`` (2, n_bins + 1) fp64, the leading
        axis source = [target, prediction]"""
        ds = {}
        for n, (counts, edges, _) in self._state().items():
            ds[n] = torch.from_numpy(counts.copy())
            ds[f"{n}_bin_edges"] = torch.from_numpy(edges.copy())
        return ds

    def logs(self) -> Dict[str, Any]:
        """fme/core/histogram.py:446-478 without the label: ``<source>/<p>th-percentile/<name>`` floats, ``<name>`` the trimmed
        densities and edges of both sources (the reference's figure), ``dropped_windows/<name>`` when any window was skipped.  A
        source without a recorded value has no percentile and an empty density."""
        import numpy as np
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
        return logs


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

    def labels(self) -> List[str]:
        return [m.name or d for m, d in ((self.trend, "trend"), (self.enso, "enso_coefficient"), (self.nzf, "near_zero_fraction"))
                if m is not None]

    def _eps_for(self, name: str) -> float:
        return self.nzf.per_variable_eps.get(name, self.nzf.eps)

    def _prepare(self, gen, tgt, i_time_start, time):
        """the host side of a window: the name lists of each metric, the years and the index values of its steps"""
        B, T = next(iter(gen.values())).shape[:2]
        begin = 1 if i_time_start == 0 else 0
        only = lambda d, v: [n for n in d if v is None or n in v]           # noqa: E731  (maybe_filter, build_context.py:19-46)
        years = None
        if self.trend is not None:
            if time is None:
                raise ValueError("the trend metric needs the window's time axis: record_batch(prediction, target, time=...)")
            if tuple(time.shape) != (B, T):
                raise ValueError(f"time must be (samples, steps) = {(B, T)}, got {tuple(time.shape)}")
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
        names = {"trend": [only(d, self.trend.variables) if self.trend is not None and T > begin else [] for d in (gen, tgt)],
                 "enso": [list(d) if self.enso is not None else [] for d in (gen, tgt)],
                 "nzf": [only(d, self.nzf.variables) if self.nzf is not None and T > begin else [] for d in (gen, tgt)]}
        for key, seen in (("trend", self._tnames), ("enso", self._enames), ("nzf", self._znames)):
            for side in (0, 1):
                seen[side] += [n for n in names[key][side] if n not in seen[side]]
        if self.nzf is not None:
            self._zcount += B * (T - begin)
        self._recorded = True
        return B, T, begin, years, index, names

    # ---- the torch path -----------------------------------------------------------------------------------------------
    def record_torch(self, gen, tgt, i_time_start, time=None):
        B, T, begin, years, index, names = self._prepare(gen, tgt, i_time_start, time)
        for side, d in enumerate((gen, tgt)):
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
                w = index[b].to(device=first.device, dtype=torch.float32)
                if side == 0:
                    self._t_ivar[b] = self._t_ivar.get(b, torch.tensor(0.0, dtype=torch.float32, device=first.device)) + (w ** 2).sum()
                cov = self._t_cov[side].setdefault(b, {})
                for n in names["enso"][side]:
                    c = (d[n][b] * w.view(T, 1, 1)).sum(dim=0)                # data_index_covariance, enso_coefficient.py:418-437
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

    # ---- the fused path -----------------------------------------------------------------------------------------------
    def record_fused(self, gen, tgt, i_time_start, time=None) -> int:
        """one ``ace_diag_regress_window`` for all the metrics that are on, both sides and all names (fields with contiguous
        planes); returns the launches made"""
        import numpy as np
        from . import _lib
        B, T, begin, years, index, names = self._prepare(gen, tgt, i_time_start, time)
        agg = self._agg
        first = next(iter(gen.values()))
        dev, (H, W) = first.device, first.shape[-2:]
        HW = H * W
        base_e = 2 if self.trend is not None else 0
        nmaps = base_e + (B if self.enso is not None else 0)
        if nmaps > MAX_REGRESS_MAPS:
            raise ValueError(f"the fused trend / enso_coefficient pass keeps 2 + samples maps per pixel in registers, at most "
                             f"{MAX_REGRESS_MAPS}: {B} samples with the ENSO coefficient on need {nmaps}; record fewer samples per "
                             "window or take the torch path (fused = False)")
        if self._maps is not None and nmaps != self._nmaps:
            raise ValueError("the number of samples changed between windows")
        planes = [n for n in gen if any(n in names[k][s] for k in names for s in (0, 1))]
        new = [n for n in planes if n not in self._rows]
        if new or self._maps is None:
            for n in new:
                self._rows[n] = len(self._rows)
            R = max(1, len(self._rows))
            self._nmaps = nmaps
            self._maps = _grow(self._maps, (2, R, max(1, nmaps), HW), torch.float64, dev)
            self._count = _grow(self._count, (2, R, HW), torch.int64, dev)
            self._frac = _grow(self._frac, (2, R), torch.float64, dev)
        if not planes:
            return 0
        n = len(planes)
        wrows = agg._weight_rows(planes, dev)
        values, off = _plane_table(planes, gen, tgt)
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
            # one pinned blob: the plane table, then from off["end"] the coefficients, the rows, the slots and the eps
            sections = [np.asarray(values, np.int64), np.asarray(coef, np.float64).reshape(-1),
                        np.asarray([self._rows[nm] for nm in planes], np.int32), np.asarray(slot, np.int32).reshape(-1),
                        np.asarray(eps, np.float32)]
            table = torch.from_numpy(np.concatenate([s.view(np.uint8) for s in sections])).pin_memory().to(dev, non_blocking=True)
            at = {k: table.data_ptr() + o for k, o in off.items()}
            p_coef, p_rows, p_slot, p_eps, _ = itertools.accumulate([s.nbytes for s in sections[1:]], initial=at["end"])
            partial = None
            if do_nzf:
                partial = torch.empty(int(lib.ace_diag_regress_partial_doubles(n, B, T, HW)), dtype=torch.float64, device=dev)
            with torch.cuda.device(dev):
                _check(lib.ace_diag_regress_window(
                    at["gen"], at["gen_strides"], at["target"], at["target_strides"], p_rows, p_coef if nterms else None,
                    p_slot if nterms else None, self._maps.data_ptr() if nterms else None, p_eps if do_nzf else None,
                    wrows.data_ptr(), agg._wplanes.data_ptr(), agg._wplanes.shape[0], partial.data_ptr() if do_nzf else None,
                    self._count.data_ptr(), self._frac.data_ptr(), self._maps.shape[1], nterms, nmaps if nterms else 0, t_begin, n,
                    B, T, HW, _lib.current_stream()))
            made += 1
        return made

    # ---- results ------------------------------------------------------------------------------------------------------
    def _fused(self) -> bool:
        return self._maps is not None

    def _trends(self) -> Dict[str, List[Optional[torch.Tensor]]]:
        """trend.py:163-194: name -> [target, prediction] fp64 (H, W) slopes (None for a side the name was not recorded on)"""
        n, st, stt = self._n, self._sum_t, self._sum_tt
        denom = n * stt - st * st
        out: Dict[str, List[Optional[torch.Tensor]]] = {}
        for side, slot in ((1, 0), (0, 1)):
            for name in sorted(self._tnames[side]):
                if self._fused():
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
                if self._fused():
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
                if self._fused():
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

    def logs(self) -> Dict[str, Any]:
        """trend.py:204-239, enso_coefficient.py:246-306 and near_zero_fraction.py:269-282 with tensors where the reference logs
        images: ``<label>/maps/<name>`` (2, H, W) [target, generated] and ``<label>/difference_map/<name>``,
        ``<label>/weighted_rmse/<name>`` from the fp32 casts; ``<label>/coefficient_maps/<name>``,
        ``<label>/coefficient_difference_map/<name>``, ``<label>/rmse/<name>``; ``<label>/gen/<name>``,
        ``<label>/gen_minus_target/<name>`` and with include_maps ``<label>/gen_target_map/<name>`` (2, H, W) [generated, target],
        ``<label>/error_map/<name>`` (``<label>/gen_map/<name>`` for a name without a target)."""
        logs: Dict[str, Any] = {}
        if not self._recorded:
            return logs
        if self.trend is not None and self._n > 0:
            label = self.trend.name or "trend"
            for n, (t, g) in self._trends().items():
                if t is None:
                    continue
                logs[f"{label}/maps/{n}"] = torch.stack([t, g]).cpu()
                logs[f"{label}/difference_map/{n}"] = (g - t).cpu()
                logs[f"{label}/weighted_rmse/{n}"] = self._rmse(n, g.to(torch.float32), t.to(torch.float32))
        if self.enso is not None:
            label = self.enso.name or "enso_coefficient"
            for n, (t, g) in self._coefficients().items():
                if t is None:
                    continue
                logs[f"{label}/coefficient_maps/{n}"] = torch.stack([t, g]).cpu()
                logs[f"{label}/coefficient_difference_map/{n}"] = (g - t).cpu()
                logs[f"{label}/rmse/{n}"] = self._rmse(n, g, t)
        if self.nzf is not None and self._zcount > 0:
            label = self.nzf.name or "near_zero_fraction"
            fr, maps = self._fractions()
            for n, (g, t) in fr.items():
                if g is None:
                    continue
                logs[f"{label}/gen/{n}"] = g
                if t is not None:
                    logs[f"{label}/gen_minus_target/{n}"] = g - t
            for n, (g, t) in maps.items():
                if g is None:
                    continue
                if t is None:
                    logs[f"{label}/gen_map/{n}"] = g.cpu()
                else:
                    logs[f"{label}/gen_target_map/{n}"] = torch.stack([g, t]).cpu()
                    logs[f"{label}/error_map/{n}"] = (g - t).cpu()
        return logs


SEA_SURFACE_TEMPERATURE_NAMES = ["sst", "surface_temperature", "TS"]      # enso/dynamic_index.py:33
NINO34_LAT, NINO34_LON = (-5, 5), (190, 240)                              # enso/dynamic_index.py:354-355
IPO_SST_NAMES = ["sst"]                                                   # ipo/ipo_index.py:32
MIN_YEARS_FOR_FILTERED_TPI = 80                                           # ipo/ipo_index.py:34
IPO_CUTOFF_YEARS = 13.0                                                   # ipo/ipo_index.py:226
TPI_REGIONS = {"T1": {"lat_bounds": (25.0, 45.0), "lon_bounds": (140.0, 215.0)},      # ipo/ipo_index.py:36-40
               "T2": {"lat_bounds": (-10.0, 10.0), "lon_bounds": (170.0, 270.0)},
               "T3": {"lat_bounds": (-50.0, -15.0), "lon_bounds": (150.0, 200.0)}}
SEASONS = ("DJF", "MAM", "JJA", "SON")                                    # seasonal.py:185, the order of the bins and of the maps
MIN_COMPLETE_YEAR_DAYS = 350                                              # annual.py:415
MAX_CALENDAR_BINS = 8                                                     # ACE_DIAG_CALENDAR_MAX_BINS (include/ace_sfno.h)


def latlon_region_weights(lat, lon, lat_bounds, lon_bounds) -> torch.Tensor:
    """LatLonRegion (utils.py:30-39): mask x cos(lat) as fp32 (H, W), computed in the dtype of ``lat`` as the reference does"""
    lat, lon = torch.as_tensor(lat), torch.as_tensor(lon)
    lat_mask = ((lat >= lat_bounds[0]) & (lat <= lat_bounds[1])).unsqueeze(-1)
    lon_mask = ((lon >= lon_bounds[0]) & (lon <= lon_bounds[1])).unsqueeze(-2)
    mask = torch.logical_and(lat_mask, lon_mask).float()
    return (mask * torch.cos(torch.deg2rad(lat)).unsqueeze(-1)).to(torch.float32)


def nan_aware_regional_mean(data: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """ipo/ipo_index.py:43-58"""
    valid = ~torch.isnan(data)
    filled = torch.where(valid, data, torch.zeros_like(data))
    w = weights.to(data.device).unsqueeze(0).unsqueeze(0)
    return (filled * w * valid).sum(dim=(-2, -1)) / (w * valid).sum(dim=(-2, -1))


def anomalies_from_monthly_climo(data: torch.Tensor, month) -> torch.Tensor:
    """utils.py:127-144: data (B, T) minus its per-sample mean over the steps of the same calendar month; month (B, T) ints"""
    import numpy as np
    nan = torch.tensor(float("nan"), dtype=data.dtype)
    anomalies = torch.full_like(data, float("nan"))
    for m in range(1, 13):
        mask = torch.from_numpy(np.asarray(month) == m)
        climo = (data.where(mask, nan).nansum(dim=1) / mask.sum(dim=1)).unsqueeze(dim=1)
        anomalies = torch.where(mask, data - climo, anomalies)
    return anomalies


def running_monthly_mean(data: torch.Tensor, year, month, n_months: int):
    """utils.py:184-220: the per-sample mean of every (year, month) of the record, then the mean of the last ``n_months`` of them;
    returns ((B, n unique months), the sorted (year, month) pairs)"""
    import numpy as np
    year, month = np.asarray(year), np.asarray(month)
    keys = sorted(set(zip(year.ravel().tolist(), month.ravel().tolist())))
    nan = torch.tensor(float("nan"), dtype=data.dtype)
    monthly = torch.full((data.shape[0], len(keys)), float("nan"), dtype=data.dtype)
    running = torch.full_like(monthly, float("nan"))
    for i, (y, m) in enumerate(keys):
        mask = torch.from_numpy((year == y) & (month == m))
        monthly[:, i] = data.where(mask, nan).nanmean(dim=1)
        if i >= n_months - 1:
            running[:, i] = monthly[:, i - n_months + 1:i + 1].nanmean(dim=1)
    return running, keys


def sample_mean_std(data, target=None) -> float:
    """utils.py:76-94: the standard deviation over time of every sample, optionally over the target's, averaged over samples"""
    import warnings
    import numpy as np
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        std = np.nanstd(data, axis=1)
        if target is not None:
            std = std / np.nanstd(target, axis=1)
    return std.mean().item()


def sample_average_power_spectrum(index):
    """utils.py:46-73, 97-124: (cycles per year, |rfft|^2 averaged over samples) of monthly (B, n) series, NaNs dropped and the
    samples truncated to the shortest; None when a sample has nothing left"""
    import numpy as np
    rows = [row[~np.isnan(row)] for row in np.asarray(index)]
    n = min(len(r) for r in rows)
    if n == 0:
        return None
    power = (np.abs(np.fft.rfft(np.array([r[:n] for r in rows]), axis=1)) ** 2).mean(axis=0)
    return np.fft.rfftfreq(n, d=1.0) * 12.0, power


def psd_band_power(freqs, power, period_bounds=(2.0, 5.0)) -> float:
    """utils.py:238-261"""
    import numpy as np
    mask = (freqs >= 1.0 / period_bounds[1]) & (freqs <= 1.0 / period_bounds[0])
    if mask.sum() < 2:
        return float("nan")
    trapezoid = np.trapezoid if hasattr(np, "trapezoid") else np.trapz
    return float(trapezoid(power[mask], freqs[mask]))


def fair_crps(gen: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """fme/core/ensemble.py:4-44 with alpha = 1: gen (n, members), target (n, 1)"""
    first = torch.mean(torch.abs(gen - target), dim=1)
    if gen.shape[1] == 1:
        return first
    i, j = torch.triu_indices(gen.shape[1], gen.shape[1], offset=1)
    return first - 0.5 * (gen[:, i] - gen[:, j]).abs().mean(dim=1)


def low_pass_filter(data, cutoff_period_yrs: float = IPO_CUTOFF_YEARS):
    """ipo/ipo_index.py:61-87: a fifth-order Chebyshev type I low pass (0.5 dB ripple) of monthly values, run forwards and back"""
    from scipy import signal
    b, a = signal.cheby1(N=5, rp=0.5, Wn=(1.0 / cutoff_period_yrs) / 6.0, btype="low", analog=False)
    return signal.filtfilt(b, a, data)


class _Calendar:
    """The four metrics that group a record by its calendar: ``seasonal`` (SeasonalAggregator, seasonal.py:22-175), ``annual``
    (PairedGlobalMeanAnnualAggregator, annual.py:24-275), ``enso_index`` (PairedRegionalIndexAggregator, enso/dynamic_index.py:36-351)
    and ``ipo_index`` (PairedIPOIndexAggregator, ipo/ipo_index.py:90-322).  Per window both paths form the same two things: the sum
    of the steps of each season per pixel, and per (sample, step) the regional means the other three start from - the area mean of
    every name (a region of ones), the Nino 3.4 box of the sea-surface-temperature names, the three tripole boxes of ``sst``.  The
    torch path states the reference's formulas in the reference's dtypes (fp32 sums and means); the fused path makes one
    ``ace_diag_calendar_window`` per window for everything that is on (csrc/calendar.hip; the header contract in
    include/ace_sfno.h) and keeps fp64 sums and series on the device until ``get_*``.  The (year, month) of every time level and the
    season counts stay on the host.  Every step handed to ``record_batch`` enters - none of the four drops a first step as the time
    mean does - and the initial condition never does (main.py:660-661 feeds it to the time series only).

    At ``get_*`` time the small series go through the reference's host formulas, restated on (year, month) arrays where the
    reference groups by xarray / cftime: yearly means of more than 350 days' worth of steps, monthly anomalies, the 5-month running
    mean, the sample-averaged power spectrum and its band powers, the tripole index and its 13-year Chebyshev low pass, the seasonal
    means with their bias, anomaly, R2 and area-mean RMSE.  Tensors stand where the reference logs figures.  Differences: no
    ``r2/<name>_target`` / ``_gen`` of the annual series (they need the monthly reference data); the seasonal R2, which the
    reference only shows in a caption, is logged as ``r2/<name>``; a generated name without a target is left out of the paired
    outputs; a sample without one complete year stays in the annual series as a row of NaN, where the reference's
    ``where(..., drop=True)`` (annual.py:227) drops it from the sample axis (the nan-means give the same scalars)."""

    def __init__(self, agg, configs: Mapping[str, MetricConfig], dataset_info):
        self._agg = agg
        self.seasonal, self.annual, self.enso, self.ipo = (configs.get(k) for k in ("seasonal", "annual", "enso_index", "ipo_index"))
        self._timestep = getattr(dataset_info, "timestep", None)
        coords = getattr(dataset_info, "horizontal_coordinates", None)
        H, W = agg._shape
        self._region_names: List[str] = []
        planes, self._modes = [], []
        if self.annual is not None:
            self._region_names.append("globe")                                # x 1 in fp32 leaves the area weights as they are
            planes.append(torch.ones(H, W))
            self._modes.append(0)
        if self.enso is not None:
            self._region_names.append("nino34")
            planes.append(latlon_region_weights(coords.lat, coords.lon, NINO34_LAT, NINO34_LON))
            self._modes.append(0)
        if self.ipo is not None:
            for name, spec in TPI_REGIONS.items():
                self._region_names.append(name)
                planes.append(latlon_region_weights(coords.lat, coords.lon, spec["lat_bounds"], spec["lon_bounds"]))
                self._modes.append(1)
        self._regions = torch.stack(planes) if planes else torch.zeros(0, H, W)
        self._year = self._month = None                                       # (B, n_time) int64, filled window by window
        self._seen = [False] * agg._n_time
        self._season_counts = [0.0] * len(SEASONS)
        self._have: List[set] = [set(), set()]                                # per side the (region, name) series recorded
        self._season_names: List[List[str]] = [[], []]
        self.calls = 0                                                        # ace_diag_calendar_window calls made
        # torch path
        self._t_series: List[Dict[Any, torch.Tensor]] = [{}, {}]
        self._t_bins: List[Dict[str, torch.Tensor]] = [{}, {}]
        # fused path: _bins (2, rows, 4, H W) fp64, _series (2, series rows, B, n_time) fp64 (NaN: not recorded)
        self._rows: Dict[str, int] = {}
        self._srows: Dict[Any, int] = {}
        self._bins = self._series = self._dev_regions = self._dev_modes = None

    def on(self) -> List[MetricConfig]:
        return [m for m in (self.seasonal, self.annual, self.enso, self.ipo) if m is not None]

    def _prepare(self, gen, tgt, i_time_start, time):
        """the host side of a window: its (year, month) levels, the season bin of every step, the names each output takes"""
        import numpy as np
        B, T = next(iter(gen.values())).shape[:2]
        if time is None:
            raise ValueError("the seasonal, annual, enso_index and ipo_index metrics need the window's time axis: "
                             "record_batch(prediction, target, time=...)")
        if tuple(time.shape) != (B, T):
            raise ValueError(f"time must be (samples, steps) = {(B, T)}, got {tuple(time.shape)}")
        year, month = time.year_month()
        if self._year is None:
            self._year, self._month = (np.zeros((B, self._agg._n_time), np.int64) for _ in range(2))
        elif self._year.shape[0] != B:
            raise ValueError("the number of samples changed between windows")
        self._year[:, i_time_start:i_time_start + T], self._month[:, i_time_start:i_time_start + T] = year, month
        for i in range(i_time_start, i_time_start + T):
            self._seen[i] = True
        season = ((month % 12) // 3).astype(np.int32)                        # DJF = 12, 1, 2 -> 0, MAM -> 1, JJA -> 2, SON -> 3
        only = lambda d, v: [n for n in d if v is None or n in v]           # noqa: E731  (maybe_filter, build_context.py:19-46)
        wanted = []
        for side, d in enumerate((gen, tgt)):
            w = {}
            for r in self._region_names:
                w[r] = only(d, self.annual.variables) if r == "globe" else \
                    [n for n in (SEA_SURFACE_TEMPERATURE_NAMES if r == "nino34" else IPO_SST_NAMES) if n in d]
                self._have[side].update((r, n) for n in w[r])
            w["seasonal"] = only(d, self.seasonal.variables) if self.seasonal is not None else []
            self._season_names[side] += [n for n in w["seasonal"] if n not in self._season_names[side]]
            wanted.append(w)
        if self.seasonal is not None:
            for m, c in enumerate(np.bincount(season.ravel(), minlength=len(SEASONS))):
                self._season_counts[m] += float(c)
        return B, T, season, wanted

    # ---- the torch path -----------------------------------------------------------------------------------------------
    def record_torch(self, gen, tgt, i_time_start, time):
        B, T, season, wanted = self._prepare(gen, tgt, i_time_start, time)
        sl = slice(i_time_start, i_time_start + T)
        dev = next(iter(gen.values())).device
        # the (sample, step) indices of the seasons this window has steps of, found on the host and uploaded once: indexing with
        # them gathers what a boolean mask would, in the same order, without the host synchronisation a mask's nonzero() costs
        import numpy as np
        steps = {m: tuple(torch.from_numpy(i).to(dev) for i in np.nonzero(season == m)) for m in range(len(SEASONS))
                 if (season == m).any()} if self.seasonal is not None else {}
        for side, d in enumerate((gen, tgt)):
            for ri, r in enumerate(self._region_names):
                for n in wanted[side][r]:
                    x = d[n]
                    if r == "globe":                                              # annual.py:185-188 on gridded_ops.py:350-359
                        v = _wmean(x, self._agg.weights_for(n, x.device).to(x.dtype))
                    elif self._modes[ri] == 0:                                    # dynamic_index.py:77-79 on gridded_ops.py:361-371
                        v = _wmean(x, self._regions[ri].to(x.device) * self._agg.weights_for(n, x.device).to(x.dtype))
                    else:                                                         # ipo_index.py:121-124
                        v = nan_aware_regional_mean(x, self._regions[ri])
                    buf = self._t_series[side].get((r, n))
                    if buf is None:
                        buf = self._t_series[side][(r, n)] = torch.full((B, self._agg._n_time), float("nan"), dtype=v.dtype,
                                                                        device=v.device)
                    buf[:, sl] = v
            for n in wanted[side]["seasonal"]:                                    # seasonal.py:40-69: groupby(season).sum(skipna=False)
                x = d[n]
                acc = self._t_bins[side].get(n)
                if acc is None:
                    acc = self._t_bins[side][n] = torch.zeros((len(SEASONS),) + tuple(x.shape[-2:]), dtype=x.dtype, device=x.device)
                for m, (bi, ti) in steps.items():
                    acc[m] += x[bi, ti].sum(dim=0)

    # ---- the fused path -----------------------------------------------------------------------------------------------
    def _layout(self, gen, wanted, B: int, HW: int, dev):
        """the planes of a window's call, their rows in ``_bins`` and the (plane, region) rows in ``_series``, both buffers grown
        to hold them: a plane takes part in the binned sums whenever they are on (the header contract ties the series of a plane
        to a valid row), and what the seasonal variable filter excludes is left out at get_* time"""
        planes = [n for n in gen if any(n in w[k] for w in wanted for k in w)]
        for n in planes:
            self._rows.setdefault(n, len(self._rows))
        for w in wanted:
            for r in self._region_names:
                for n in w[r]:
                    self._srows.setdefault((r, n), len(self._srows))
        if self.seasonal is not None and (self._bins is None or self._bins.shape[1] < len(self._rows)):
            self._bins = _grow(self._bins, (2, max(1, len(self._rows)), len(SEASONS), HW), torch.float64, dev)
        S = max(1, len(self._srows))
        if self._region_names and (self._series is None or self._series.shape[1] < S):
            fresh = torch.full((2, S, B, self._agg._n_time), float("nan"), dtype=torch.float64, device=dev)
            if self._series is not None:
                fresh[:, :self._series.shape[1]] = self._series
            self._series = fresh
        srow = [[self._srows[(r, nm)] if any(nm in w[r] for w in wanted) else -1 for r in self._region_names] for nm in planes]
        return planes, [self._rows[nm] for nm in planes], srow

    def record_fused(self, gen, tgt, i_time_start, time) -> int:
        """one ``ace_diag_calendar_window`` for all the metrics that are on, both sides and all names (fields with contiguous
        planes); returns the calls made"""
        import numpy as np
        from . import _lib
        B, T, season, wanted = self._prepare(gen, tgt, i_time_start, time)
        agg = self._agg
        first = next(iter(gen.values()))
        dev, (H, W) = first.device, first.shape[-2:]
        HW, nreg, n_time = H * W, len(self._region_names), agg._n_time
        planes, rows, srow = self._layout(gen, wanted, B, HW, dev)
        if not planes:
            return 0
        if nreg and self._dev_regions is None:
            self._dev_regions = self._regions.reshape(nreg, HW).to(dev, torch.float32).contiguous()
            self._dev_modes = _upload(self._modes, torch.int32, dev)
        n = len(planes)
        wrows = agg._weight_rows(planes, dev)
        values, off = _plane_table(planes, gen, tgt)
        # one pinned blob: the plane table, then from off["end"] the rows, the season bins and the series rows
        sections = [np.asarray(values, np.int64), np.asarray(rows, np.int32), np.ascontiguousarray(season, np.int32).reshape(-1),
                    np.asarray(srow, np.int32).reshape(-1)]
        table = torch.from_numpy(np.concatenate([s.view(np.uint8) for s in sections])).pin_memory().to(dev, non_blocking=True)
        at = {k: table.data_ptr() + o for k, o in off.items()}
        p_rows, p_bin, p_srow, _ = itertools.accumulate([s.nbytes for s in sections[1:]], initial=at["end"])
        lib = _lib.lib()
        do_bins = self.seasonal is not None
        partial = torch.empty(int(lib.ace_diag_calendar_partial_doubles(n, nreg, B, T, HW)), dtype=torch.float64, device=dev) \
            if nreg else None
        with torch.cuda.device(dev):
            _check(lib.ace_diag_calendar_window(
                at["gen"], at["gen_strides"], at["target"], at["target_strides"], p_rows, p_bin if do_bins else None,
                self._bins.data_ptr() if do_bins else None, self._dev_regions.data_ptr() if nreg else None, p_srow if nreg else None,
                self._dev_modes.data_ptr() if nreg else None, wrows.data_ptr() if nreg else None,
                agg._wplanes.data_ptr() if nreg else None, agg._wplanes.shape[0] if nreg else 0,
                partial.data_ptr() if nreg else None, self._series.data_ptr() if nreg else None, len(self._rows),
                len(SEASONS) if do_bins else 0, nreg, self._series.shape[1] if nreg else 0, n_time, i_time_start, 0, n, B, T, HW,
                _lib.current_stream()))
        self.calls += 1
        return 1

    # ---- results ------------------------------------------------------------------------------------------------------
    def _recorded(self):
        return [i for i, s in enumerate(self._seen) if s]

    def _raw(self, side: int, region: str, name: str) -> Optional[torch.Tensor]:
        """the (B, recorded steps) series of a region and name on the CPU: fp64 (fused) or the field's dtype (torch); None if the
        side never had the name"""
        if (region, name) not in self._have[side]:
            return None
        idx = self._recorded()
        if self._series is not None:
            return self._series[side, self._srows[(region, name)]].cpu()[:, idx]
        return self._t_series[side][(region, name)].cpu()[:, idx]

    def _names(self, region: str) -> List[str]:
        """the names both sides recorded for a region, sorted"""
        return sorted(n for r, n in self._have[0] if r == region and (r, n) in self._have[1])

    def _annual_means(self):
        """annual.py:210-235: (years int64 array, name -> [target, generated] (B, years) arrays); a year a sample holds no more
        than 350 days' worth of steps of is NaN, a year no sample holds that many of is dropped, gap years are NaN"""
        import numpy as np
        idx = self._recorded()
        year = np.ascontiguousarray(self._year[:, idx])
        labels = np.unique(year)
        counts = np.stack([(year == y).sum(axis=1) for y in labels], axis=1).astype(np.float32)      # (B, labels)
        min_samples = MIN_COMPLETE_YEAR_DAYS * (datetime.timedelta(days=1) / self._timestep)
        keep = counts > min_samples
        kept = labels[keep.any(axis=0)]
        years = np.arange(kept.min(), kept.max() + 1, dtype=np.int64) if kept.size else np.zeros(0, np.int64)
        out = {}
        for name in self._names("globe"):
            sides = []
            for side in (1, 0):
                x = self._raw(side, "globe", name).numpy()
                means = np.full((x.shape[0], len(years)), np.nan, dtype=x.dtype)
                for k, y in enumerate(labels):
                    if y in kept:
                        with np.errstate(all="ignore"):
                            total = np.stack([x[b, year[b] == y].sum(dtype=x.dtype) for b in range(x.shape[0])])
                            means[:, y - years[0]] = np.where(keep[:, k], total / counts[:, k], np.nan)
                sides.append(means)
            out[name] = sides
        return years, out

    def _index_series(self, side: int, kind: str):
        """enso_index (dynamic_index.py:94-113): name -> the 5-month running mean of the monthly anomalies of the Nino 3.4 mean;
        ipo_index (ipo_index.py:139-165): name -> T2 - (T1 + T3) / 2 of the monthly anomalies of the three boxes; (B, months)
        tensors, and the sorted (year, month) pairs"""
        import numpy as np
        idx = self._recorded()
        # C order: torch follows the layout of a mask in its sums, and the reference's masks are C-ordered
        year, month = np.ascontiguousarray(self._year[:, idx]), np.ascontiguousarray(self._month[:, idx])
        out, keys = {}, []
        if kind == "enso":
            for name in SEA_SURFACE_TEMPERATURE_NAMES:
                raw = self._raw(side, "nino34", name)
                if raw is not None:
                    out[name], keys = running_monthly_mean(anomalies_from_monthly_climo(raw, month), year, month, 5)
        else:
            for name in IPO_SST_NAMES:
                raws = {r: self._raw(side, r, name) for r in TPI_REGIONS}
                if all(v is not None for v in raws.values()):
                    an = {}
                    for r, raw in raws.items():
                        an[r], keys = running_monthly_mean(anomalies_from_monthly_climo(raw, month), year, month, 1)
                    out[name] = an["T2"] - 0.5 * (an["T1"] + an["T3"])
        return out, keys

    def _seasonal_means(self):
        """name -> [target, generated] fp64 (4, H, W) seasonal means (seasonal.py:90-91), in DJF, MAM, JJA, SON order, on the CPU
        as the reference's are: what follows them does not depend on the device the sums were taken on"""
        counts = torch.tensor(self._season_counts, dtype=torch.float64)
        out = {}
        for name in sorted(n for n in self._season_names[0] if n in self._season_names[1]):
            sides = []
            for side in (1, 0):
                if self._bins is not None:
                    sums = self._bins[side, self._rows[name]].reshape((len(SEASONS),) + tuple(self._agg._shape))
                else:
                    sums = self._t_bins[side][name]
                sides.append(sums.cpu().to(torch.float64) / counts[:, None, None])
            out[name] = sides
        return out

    def dataset(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """label -> variables.  annual (annual.py:155-166): ``<name>`` (2, samples, years), the leading axis source = [target,
        prediction], and ``year``; enso_index (dynamic_index.py:339-351) and ipo_index (ipo_index.py:287-298): ``<name>`` (2,
        samples, months) and the ``year`` and ``month`` of each column.  seasonal has none (seasonal.py:177-182)."""
        ds: Dict[str, Dict[str, torch.Tensor]] = {}
        if not any(self._seen):
            return ds
        if self.annual is not None:
            years, means = self._annual_means()
            d = ds[self.annual.name or "annual"] = {n: torch.stack([torch.from_numpy(t), torch.from_numpy(g)]) for n, (t, g) in means.items()}
            d["year"] = torch.from_numpy(years)
        for kind, m, default in (("enso", self.enso, "enso_index"), ("ipo", self.ipo, "ipo_index")):
            if m is None:
                continue
            (tgt, keys), (gen, _) = self._index_series(1, kind), self._index_series(0, kind)
            d = {n: torch.stack([tgt[n], gen[n]]) for n in gen if n in tgt}
            if d:
                d["year"] = torch.tensor([k[0] for k in keys], dtype=torch.int64)
                d["month"] = torch.tensor([k[1] for k in keys], dtype=torch.int64)
                ds[m.name or default] = d
        return ds

    def _annual_logs(self) -> Dict[str, Any]:
        """annual.py:86-153: ``<name>`` the (2, samples, years) series [target, generated] (the reference's figure), and with
        more than one year ``rmse/<name>`` and ``crps/<name>``"""
        import warnings
        import numpy as np
        logs: Dict[str, Any] = {}
        years, means = self._annual_means()
        for name, (tgt, gen) in means.items():
            logs[name] = torch.from_numpy(np.stack([tgt, gen]))
            if len(years) > 1:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")                                 # a gap year is an all-NaN slice
                    tmean, gmean = np.nanmean(tgt, axis=0), np.nanmean(gen, axis=0)
                    if self.annual.report_rmse:
                        logs[f"rmse/{name}"] = float(np.sqrt(np.nanmean((gmean - tmean) ** 2)))
                    if self.annual.report_crps:
                        crps = fair_crps(torch.as_tensor(gen.T.copy(), dtype=torch.float32),
                                         torch.as_tensor(tmean, dtype=torch.float32).unsqueeze(1))
                        logs[f"crps/{name}"] = float(np.nanmean(crps.numpy()))
        return logs

    @staticmethod
    def _spectrum_logs(prefix: str, pred, tgt, with_bands: bool) -> Dict[str, Any]:
        """``<prefix>_power_spectrum`` (2, frequencies): cycles per year and the prediction's power, ``..._target`` the target's;
        with bands ``<prefix>_power_2_5yr`` / ``_1_16yr`` and their ``_norm`` (dynamic_index.py:289-333)"""
        import numpy as np
        logs: Dict[str, Any] = {}
        ps, ts = sample_average_power_spectrum(pred), sample_average_power_spectrum(tgt)
        if ps is None:
            return logs
        logs[f"{prefix}_power_spectrum"] = torch.from_numpy(np.stack(ps))
        if ts is not None:
            logs[f"{prefix}_power_spectrum_target"] = torch.from_numpy(np.stack(ts))
        for tag, bounds in (("2_5yr", (2.0, 5.0)), ("1_16yr", (1.0, 16.0))) if with_bands else ():
            p = psd_band_power(*ps, period_bounds=bounds)
            t = psd_band_power(*ts, period_bounds=bounds) if ts is not None else float("nan")
            logs[f"{prefix}_power_{tag}"] = p
            if t != 0 and not np.isnan(t):
                logs[f"{prefix}_power_{tag}_norm"] = p / t
        return logs

    def _enso_logs(self) -> Dict[str, Any]:
        """dynamic_index.py:241-337: ``<sst>_nino34_index`` (2, samples, months) [target, generated], ``_std``, ``_std_norm``, the
        spectra and band powers"""
        import numpy as np
        logs: Dict[str, Any] = {}
        (tgt, _), (gen, _) = self._index_series(1, "enso"), self._index_series(0, "enso")
        for name in SEA_SURFACE_TEMPERATURE_NAMES:
            if name not in gen or name not in tgt:
                continue
            g, t = gen[name].numpy(), tgt[name].numpy()
            if g.shape[1] > 1:
                logs[f"{name}_nino34_index"] = torch.stack([tgt[name], gen[name]])
                logs[f"{name}_nino34_index_std"] = sample_mean_std(g)
                logs[f"{name}_nino34_index_std_norm"] = sample_mean_std(g, t)
            if bool((~np.isnan(g)).any()):
                logs.update(self._spectrum_logs(f"{name}_nino34_index", g, t, True))
        return logs

    def _ipo_logs(self) -> Dict[str, Any]:
        """ipo_index.py:253-322: with every sample at least 80 years of months long ``<sst>_ipo_tpi_filtered`` (2, samples, months
        - 2 x 156) [target, generated], ``_ipo_tpi_std``, ``_std_norm`` and the spectra of the unfiltered index"""
        import numpy as np
        logs: Dict[str, Any] = {}
        (tgt, _), (gen, _) = self._index_series(1, "ipo"), self._index_series(0, "ipo")
        trim = int(IPO_CUTOFF_YEARS * 12)

        def filtered(index):
            rows = []
            for row in index:
                row = row[~np.isnan(row)]
                if len(row) < MIN_YEARS_FOR_FILTERED_TPI * 12:
                    return None
                rows.append(low_pass_filter(row)[trim:-trim])
            return rows

        for name in IPO_SST_NAMES:
            if name not in gen or name not in tgt or gen[name].shape[1] < 2:
                continue
            g, t = gen[name].numpy(), tgt[name].numpy()
            fg, ft = filtered(g), filtered(t)
            if fg is not None and ft is not None:
                n = min(len(r) for r in fg + ft)                                 # samples of one record are equally long
                fg, ft = (np.stack([r[:n] for r in rows]) for rows in (fg, ft))
                logs[f"{name}_ipo_tpi_filtered"] = torch.from_numpy(np.stack([ft, fg]))
                logs[f"{name}_ipo_tpi_std"] = sample_mean_std(fg)
                logs[f"{name}_ipo_tpi_std_norm"] = sample_mean_std(fg, ft)
                logs.update(self._spectrum_logs(f"{name}_ipo_tpi", g, t, False))
        return logs

    def _seasonal_logs(self) -> Dict[str, Any]:
        """seasonal.py:72-175: nothing unless all four seasons were recorded; ``anomaly/<name>`` (2, 4, H, W) [target, generated]
        minus the target's mean over the seasons, ``bias/<name>`` (4, H, W), ``r2/<name>``, ``time-mean-rmse/<name>-<season>`` and
        ``time-mean-rmse/<name>`` (the area mean, then the mean over seasons, then the root)"""
        logs: Dict[str, Any] = {}
        if any(c == 0 for c in self._season_counts):
            return logs
        for name, (tgt, gen) in self._seasonal_means().items():
            bias = gen - tgt
            pattern = tgt.mean(dim=0)
            ganom, tanom = gen - pattern, tgt - pattern
            logs[f"anomaly/{name}"] = torch.stack([tanom, ganom])
            logs[f"bias/{name}"] = bias
            logs[f"r2/{name}"] = float(1 - ((ganom - tanom) ** 2).sum() / ((tanom - tanom.mean()) ** 2).sum())
            mse = _wmean(bias ** 2, self._agg.weights_for(name, bias.device))
            for i, season in enumerate(SEASONS):
                logs[f"time-mean-rmse/{name}-{season}"] = float(mse[i].sqrt())
            logs[f"time-mean-rmse/{name}"] = float(mse.mean().sqrt())
        return logs

    def logs(self) -> Dict[str, Any]:
        logs: Dict[str, Any] = {}
        if not any(self._seen):
            return logs
        for m, default, fn in ((self.seasonal, "seasonal", self._seasonal_logs), (self.annual, "annual", self._annual_logs),
                               (self.enso, "enso_index", self._enso_logs), (self.ipo, "ipo_index", self._ipo_logs)):
            if m is not None:
                logs.update({f"{m.name or default}/{k}": v for k, v in fn().items()})
        return logs


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


def _channel_mean(values: Mapping[str, float], own: Optional[Sequence[str]], fallback: Optional[Sequence[str]],
                  nan_targets) -> Optional[float]:
    """reduced_metrics.py:76-116 and ensemble.py:313-332: the mean of ``values`` over ``own`` names, else ``fallback``, else all,
    without the names whose target is all NaN; a name that is not present raises KeyError; None when no name is left"""
    names = own or fallback
    if names is None:
        names = list(values)
    missing = [n for n in names if n not in values]
    if missing:
        raise KeyError(f"channel_mean_names contains entries not present in the recorded data: {missing}. "
                       f"Available: {sorted(values)}.")
    names = [n for n in names if n not in nan_targets]
    return sum(values[n] for n in names) / len(names) if names else None


class _StepMeans:
    """``step_means`` (MeanAggregator behind StepMeanMetricConfig, one_step/reduced.py:24-249): the column of the ``mean`` series at
    time index ``step + n_ic_steps - 1`` - the sample-mean ``weighted_rmse``, ``weighted_bias`` and
    ``weighted_grad_mag_percent_diff`` of that step, averaged over the records that held it - so there is nothing to accumulate
    beyond what the paired pass (or the torch path's series) already holds; the norm form is the norm series' column.  Only
    ``record_batch`` feeds it, as in the reference (main.py:602-603, 660-661): an entry whose index lies inside the initial
    condition, or whose window has not come yet, reports nothing.  Which targets are entirely NaN (left out of the channel mean,
    reduced_metrics.py:101-110) is decided on the device at the first record of the selected step and read at ``get_*`` time."""

    def __init__(self, agg, configs: Sequence[StepMeanMetricConfig]):
        self._agg = agg
        self.configs = list(configs)
        self.kinds = {c.target for c in self.configs}
        self._nan: Dict[int, Any] = {}                                    # entry -> (names, device bool (names,))

    def index(self, c) -> int:
        return c.step + self._agg.n_ic_steps - 1

    def record(self, tgt, i_time_start: int):
        T = next(iter(tgt.values())).shape[1]
        for i, c in enumerate(self.configs):
            k = self.index(c) - i_time_start
            if c.target == "norm" and i not in self._nan and 0 <= k < T and self.index(c) >= self._agg.n_ic_steps:
                names = list(tgt)                                           # one stacked reduction over the names
                self._nan[i] = (names, torch.stack([tgt[n][:, k] for n in names]).isnan().flatten(1).all(dim=1))

    def _entries(self):
        agg = self._agg
        series: Dict[str, Any] = {}
        for i, c in enumerate(self.configs):
            ti = self.index(c)
            if ti < agg.n_ic_steps or agg._n_batches[ti] == 0:
                continue
            if c.target not in series:
                series[c.target] = agg._series_data(c.target)
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

    def logs(self) -> Dict[str, Any]:
        return {f"{label}/{k}": v for label, data in self._entries() for k, v in sorted(data.items())}

    def dataset(self) -> Dict[str, Dict[str, torch.Tensor]]:
        return {label: {k.replace("/", "-"): torch.tensor(v, dtype=torch.float64) for k, v in data.items()}
                for label, data in self._entries()}


class _Ensembles:
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
    window has not come yet reports nothing."""

    def __init__(self, agg, configs: Sequence[EnsembleMetricConfig], n_members: int):
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

    # ---- the torch path -----------------------------------------------------------------------------------------------
    def record_torch(self, kinds, i_time_start: int):
        """``kinds``: "denorm" (and "norm" when an entry needs it) -> (gen, target) windows"""
        E = self.n_members
        first = next(iter(kinds["denorm"][0].values()))
        B, T = first.shape[:2]
        eps = (1.0 - ENSEMBLE_CRPS_ALPHA) / 2.0
        for i, k in self._selected(i_time_start, T):
            gen, tgt = kinds[self.configs[i].target]
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

    # ---- the fused path -----------------------------------------------------------------------------------------------
    def record_fused(self, gen, tgt, i_time_start: int) -> int:
        """one ``ace_diag_ensemble_step`` per entry whose step lies in the window, for all paired names (fields with contiguous
        planes); returns the calls made"""
        from . import _lib
        first = next(iter(gen.values()))
        dev, (B, T, H, W) = first.device, first.shape
        todo = self._selected(i_time_start, T)
        if not todo:
            return 0
        E, HW = self.n_members, H * W
        if not 2 <= E <= MAX_ENSEMBLE_MEMBERS:
            raise ValueError(f"the fused ensemble pass keeps the members of a pixel in registers, at most {MAX_ENSEMBLE_MEMBERS}: "
                             f"{E} members per initial condition need the torch path (fused = False)")
        names = list(tgt)
        new = [n for n in names if n not in self._rows]
        if new or self._maps is None:
            for n in new:
                self._rows[n] = len(self._rows)
            R = max(1, len(self._rows))
            self._maps = _grow(self._maps, (len(self.configs), 4, R, HW), torch.float64, dev)
            self._seen = _grow(self._seen, (len(self.configs), R), torch.int32, dev)
        values, off = _plane_table(names, gen, tgt)
        table = _upload(values, torch.int64, dev)
        at = {k: table.data_ptr() + o for k, o in off.items()}
        rows32 = _upload([self._rows[n] for n in names], torch.int32, dev)
        lib = _lib.lib()
        pair_weight = 0.5 * (1.0 - (1.0 - ENSEMBLE_CRPS_ALPHA) / 2.0)
        for i, k in todo:
            with torch.cuda.device(dev):
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

    def logs(self) -> Dict[str, Any]:
        """ensemble.py:291-352 with tensors where the reference logs figures: ``<label>/<metric>/<name>`` the area-weighted mean of
        the map, with ``log_mean_maps`` ``<label>/<metric>/mean_map/<name>`` the (H, W) map, with ``target="norm"``
        ``<label>/<metric>/channel_mean``"""
        return {f"{label}/{k}": v for label, data in self._entries() for k, v in sorted(data.items())}

    def dataset(self) -> Dict[str, Dict[str, torch.Tensor]]:
        return {label: {k.replace("/", "-"): v if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=torch.float64)
                        for k, v in data.items()} for label, data in self._entries()}


class InferenceEvaluatorAggregator(InferenceAggregator):
    """main.py:526-732 for the sub-aggregators of the module docstring.  Weights, masks, routing and the SHT are the parent's."""

    def __init__(self, dataset_info, n_ic_steps: int, n_forward_steps: int, normalize, labels: Optional[Mapping[str, str]] = None,
                 skipped: Sequence[str] = (), zonal_mean_max_size: int = 4096, channel_mean_names: Optional[Sequence[str]] = None,
                 report_directional_bias: bool = True, output_dir: Optional[str] = None, save_diagnostics: bool = False,
                 sht_factory=None, spectrum_chunk_bytes: int = 256 << 20, histogram: Optional[HistogramMetricConfig] = None,
                 trend: Optional[TrendMetricConfig] = None, enso_coefficient: Optional[EnsoCoefficientMetricConfig] = None,
                 near_zero_fraction: Optional[NearZeroFractionMetricConfig] = None,
                 calendar: Optional[Mapping[str, MetricConfig]] = None, step_means: Sequence[StepMeanMetricConfig] = (),
                 ensembles: Sequence[EnsembleMetricConfig] = (), n_ensemble_per_ic: int = 1):
        super().__init__(dataset_info, n_ic_steps + n_forward_steps, True, output_dir, save_diagnostics, sht_factory,
                         spectrum_chunk_bytes)
        self.n_ensemble_per_ic = int(n_ensemble_per_ic)
        self._hist = None if histogram is None or not histogram.enabled else _Histograms(histogram)
        on = [None if m is None or not m.enabled else m for m in (trend, enso_coefficient, near_zero_fraction)]
        self._regress = _Regress(self, *on) if any(m is not None for m in on) else None
        self._calendar = _Calendar(self, calendar, dataset_info) if calendar else None
        self.n_ic_steps = int(n_ic_steps)
        self.skipped = list(skipped)
        default = InferenceEvaluatorAggregatorConfig.BUILT.values()
        self._labels = dict(labels) if labels is not None else {k: k for k in default}
        self._log_series = "mean" in self._labels or "mean_norm" in self._labels
        self._steps = _StepMeans(self, step_means) if step_means else None
        # main.py:560-562, 604-621: with one member per initial condition the ensemble entries are neither recorded nor reported
        self._ensembles = _Ensembles(self, ensembles, self.n_ensemble_per_ic) if ensembles and self.n_ensemble_per_ic > 1 else None
        self._record_series = self._log_series or self._steps is not None     # a step mean is a column of the series
        self._channel_mean_names = None if channel_mean_names is None else list(channel_mean_names)
        self._directional = bool(report_directional_bias)
        owner = getattr(normalize, "__self__", normalize)
        self._normalize_fn = normalize if callable(normalize) else getattr(normalize, "normalize", None)
        self._stats = None
        if hasattr(owner, "means") and hasattr(owner, "stds") and not getattr(owner, "fill_nans_on_normalize", False):
            self._stats = {n: (float(owner.means[n]), float(owner.stds[n])) for n in owner.means if n in owner.stds}
        self._factor, self._n_slots = zonal_coarsening(self._n_time, zonal_mean_max_size)
        self._zon_first: Optional[int] = None
        self._zon_steps = 0
        self._pair_names: List[str] = []
        self._present: Dict[str, Dict[str, List[int]]] = {"gen": {}, "target": {}}     # name -> records per time index
        self._spec_side_counts: List[Dict[str, int]] = [{}, {}]
        self._need_norm = "mean_norm" in self._labels or "time_mean_norm" in self._labels or \
            any(sub is not None and "norm" in sub.kinds for sub in (self._steps, self._ensembles))
        # torch path state
        self._t_series: Dict[str, Dict[str, Dict[str, torch.Tensor]]] = {"denorm": {}, "norm": {}}
        self._t_tsum: Dict[str, List[Dict[str, torch.Tensor]]] = {"denorm": [{}, {}], "norm": [{}, {}]}
        self._t_spec2: List[Dict[str, torch.Tensor]] = [{}, {}]
        self._t_zon: List[Dict[str, torch.Tensor]] = [{}, {}]
        # fused path state: _series (6, rows, n_time), _tsum (2, rows, H W), _spec (2, rows, lmax), _zon (2, rows, slots, H)
        self._zon = None

    # ---- routing ------------------------------------------------------------------------------------------------------
    def route(self, prediction: TensorMapping, target: Optional[TensorMapping] = None) -> str:
        """"fused" when recording this pair runs the HIP kernels, "torch" when it runs the torch ops."""
        if self._need_norm and self._stats is None:
            return "torch"
        return super().route({**{f"p:{k}": v for k, v in prediction.items()}, **{f"t:{k}": v for k, v in (target or {}).items()}})

    def launches(self) -> int:
        """Native launches made so far: one ``ace_diag_paired_window`` per window, one ``ace_diag_hist_window`` per window of
        ``record_batch`` when the histogram is on, one ``ace_diag_regress_window`` per window of ``record_batch`` when any of
        trend, enso_coefficient and near_zero_fraction is on (a second one for the ENSO term of a window at time index 0), and
        one ``ace_diag_ensemble_step`` per ensemble entry and window that holds its step, and per spectrum chunk of either side
        one forward SHT and one ``ace_diag_spectrum``."""
        return self._launches

    def calendar_launches(self) -> int:
        """``ace_diag_calendar_window`` calls made so far (C-ABI calls, not kernel launches): one per window of ``record_batch``
        when any of seasonal, annual, enso_index and ipo_index is on.  Counted apart from ``launches``, whose total the metrics
        above define."""
        return self._calendar.calls if self._calendar is not None else 0

    @property
    def needs_time(self) -> bool:
        """True when ``record_batch`` raises without the window's time axis: the trend metric regresses against it, and a strict
        calendar metric (a ``SeasonalMetricConfig`` is strict unless told otherwise) groups the steps by it."""
        return (self._regress is not None and self._regress.needs_time) or \
            (self._calendar is not None and any(m.strict for m in self._calendar.on()))

    @property
    def uses_time(self) -> bool:
        """True when ``record_batch`` takes the window's time axis if it is given one: ``needs_time``, or a non-strict calendar
        metric is on (annual, enso_index and ipo_index are by default), which a ``record_batch`` without ``time`` drops with a
        warning and lists in ``skipped``."""
        return self.needs_time or self._calendar is not None

    def _without_time(self):
        """``record_batch`` came without a time axis.  The trend metric was asked for by name and raises; the calendar metrics are
        on by default, so the non-strict ones are dropped with one warning and listed in ``skipped``, as an unsupported metric is
        at build time - unless a window already went into them."""
        if self._regress is not None and self._regress.needs_time:
            raise ValueError("the trend metric needs the window's time axis: record_batch(prediction, target, time=...)")
        names = [m.name for m in self._calendar.on()]
        if any(m.strict for m in self._calendar.on()) or any(self._calendar._seen):
            raise ValueError(f"the {', '.join(names)} metrics need the window's time axis: record_batch(prediction, target, time=...)")
        logging.warning("record_batch was given no time axis; metrics not supported without it, omitting: " + ", ".join(names))
        self.skipped += [n for n in names if n not in self.skipped]
        self._calendar = None

    def _pick_pair(self, prediction, target) -> str:
        path = self.route(prediction, target)
        if self._path is None:
            self._path = path
        elif path != self._path:
            raise ValueError(f"this aggregator reduces on the {self._path} path, but a window only the {path} path takes came in "
                             "(device, dtype or shape changed between windows)")
        return path

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
        if self._record_series:
            self._record_pair(gen, tgt, 0, with_maps=False)
        self._n_seen = n
        return []

    @torch.no_grad()
    def record_batch(self, prediction: TensorMapping, target: TensorMapping, time=None):
        """main.py:579-627: a paired window, each name -> (B, T, H, W), at time index ``i_time_start`` = the steps seen so far;
        ``time``: the ``TimeAxis`` (B, T) of the window's steps, needed when ``needs_time``.  Returns no per-step logs and does not
        synchronise."""
        if len(prediction) == 0:
            raise ValueError("No prediction values in data")
        if len(target) == 0:
            raise ValueError("No target values in data")
        B, n = next(iter(prediction.values())).shape[:2]
        if B % self.n_ensemble_per_ic != 0:
            raise ValueError(f"a window of {B} samples is not a multiple of n_ensemble_per_ic = {self.n_ensemble_per_ic}")
        if self.uses_time and time is None:
            self._without_time()
        if self.uses_time:
            from .timeaxis import as_time_axis
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
        path = self._pick_pair(gen, tgt)
        ignore_initial = i_time_start == 0
        if zonal and self._zon_first is None:
            self._zon_first = i_time_start
        if path == "fused":
            self._record_fused_pair(gen, tgt, i_time_start, with_maps, ignore_initial, time)
        else:
            self._record_torch_pair(gen, tgt, i_time_start, with_maps, ignore_initial, time)
        for n in gen:
            if n not in self._series_names:
                self._series_names.append(n)
        if self._record_series:
            for side, d in (("gen", gen), ("target", tgt)):
                for n in d:
                    seen = self._present[side].setdefault(n, [0] * self._n_time)
                    for i in range(i_time_start, i_time_start + T):
                        seen[i] += 1
            for i in range(i_time_start, i_time_start + T):
                self._n_batches[i] += 1
        if with_maps:
            if self._tm_samples is None:                                              # time_mean.py:127-146
                self._tm_samples = B
            self._tm_steps = T - 1 if ignore_initial else self._tm_steps + T
            for n in gen:
                if n not in self._tm_names:
                    self._tm_names.append(n)
            for n in tgt:                   # the maps' pairs: an initial condition that is its own target feeds the series only
                if n not in self._pair_names:
                    self._pair_names.append(n)
            if zonal:
                self._zon_steps += T
            for side, d in enumerate((gen, tgt)):
                for n in d:
                    if not self._omitted(n):
                        self._spec_side_counts[side][n] = self._spec_side_counts[side].get(n, 0) + B * T

    # ---- the torch path -------------------------------------------------------------------------------------------------------
    def _record_torch_pair(self, gen, tgt, i_time_start, with_maps, ignore_initial, time=None):
        T = next(iter(gen.values())).shape[1]
        sl = slice(i_time_start, i_time_start + T)
        if with_maps and self._hist is not None:
            self._hist.record_torch(gen, tgt)
        if with_maps and self._regress is not None:
            self._regress.record_torch(gen, tgt, i_time_start, time)
        if with_maps and self._calendar is not None:
            self._calendar.record_torch(gen, tgt, i_time_start, time)
        kinds = {"denorm": (gen, tgt)}
        if self._need_norm:
            kinds["norm"] = (self._normalize_fn(gen), self._normalize_fn(tgt))            # main.py:594-598
        if with_maps and self._steps is not None:
            self._steps.record(tgt, i_time_start)
        if with_maps and self._ensembles is not None:
            self._ensembles.record_torch(kinds, i_time_start)
        for kind, (g, t) in kinds.items():
            if ("mean" if kind == "denorm" else "mean_norm") in self._labels or \
                    (self._steps is not None and kind in self._steps.kinds):
                vals: Dict[str, Dict[str, torch.Tensor]] = {m: {} for m in (SERIES if kind == "denorm" else NORM_SERIES)}
                for n, x in g.items():
                    w = self.weights_for(n, x.device).to(x.dtype)
                    vals["weighted_mean_gen"][n] = _wmean(x, w)
                    vals["weighted_std_gen"][n] = _wstd(x, w)
                for n, y in t.items():
                    x, w = g[n], self.weights_for(n, y.device).to(y.dtype)
                    vals["weighted_mean_target"][n] = _wmean(y, w)
                    vals["weighted_bias"][n] = _wmean(x - y, w)                            # metrics.py:146-168
                    vals["weighted_rmse"][n] = _wmean(torch.square(x - y), w).sqrt()      # metrics.py:171-197
                    if kind == "denorm":                                                  # metrics.py:213-224
                        gt, gg = _grad_mag_mean(y, w), _grad_mag_mean(x, w)
                        vals["weighted_grad_mag_percent_diff"][n] = 100 * (gg - gt) / gt
                for metric, d in vals.items():
                    tot = self._t_series[kind].setdefault(metric, {})
                    for n, v in d.items():
                        if n not in tot:
                            tot[n] = torch.zeros(self._n_time, dtype=v.dtype, device=v.device)
                        tot[n][sl] += v.mean(dim=0)                                       # reduced.py:201-211
            if with_maps and ("time_mean" if kind == "denorm" else "time_mean_norm") in self._labels:
                part = slice(1, None) if ignore_initial else slice(0, None)
                for side, d in enumerate((g, t)):
                    acc = self._t_tsum[kind][side]
                    for n, x in d.items():
                        s = x[:, part].sum(dim=1).sum(dim=0)
                        acc[n] = s if n not in acc else acc[n] + s
        if not with_maps:
            return
        if "power_spectrum" in self._labels:
            for side, d in enumerate((gen, tgt)):
                for n, x in d.items():
                    if self._omitted(n):
                        continue
                    ps = torch.sum(abs(self._get_sht()(x)) ** 2, dim=-1)                  # metrics.py:388-408
                    mean_ps = torch.mean(ps, dim=(0, 1))
                    new, old = x.shape[0] * x.shape[1], self._spec_side_counts[side].get(n, 0)
                    acc = self._t_spec2[side]
                    acc[n] = mean_ps if n not in acc else (new * mean_ps + old * acc[n]) / (new + old)
        if "zonal_mean" in self._labels:
            z0 = i_time_start - self._zon_first
            slots = torch.arange(z0, z0 + T, device=next(iter(gen.values())).device) // self._factor
            keep = slots < self._n_slots
            for side, d in enumerate((gen, tgt)):
                for n, x in d.items():
                    zm = x.nanmean(dim=-1)                                                # non_distributed.py:136-137
                    acc = self._t_zon[side]
                    if n not in acc:
                        acc[n] = torch.zeros(x.shape[0], self._n_slots, x.shape[2], dtype=x.dtype, device=x.device)
                    acc[n].index_add_(1, slots[keep], zm[:, keep] / self._factor)

    # ---- the fused path -------------------------------------------------------------------------------------------------------
    def _ensure_rows(self, names: Sequence[str], dev):
        new = [n for n in names if n not in self._rows]
        if not new and self._series is not None:
            return
        for n in new:
            self._rows[n] = len(self._rows)
        R, (H, W) = len(self._rows), self._shape
        lmax = self._get_sht().lmax if "power_spectrum" in self._labels else 1
        self._series = _grow(self._series, (len(SERIES), R, self._n_time), torch.float64, dev)
        self._tsum = _grow(self._tsum, (2, R, H * W), torch.float64, dev)
        self._spec = _grow(self._spec, (2, R, lmax), torch.float64, dev)
        self._zon = _grow(self._zon, (2, R, self._n_slots if "zonal_mean" in self._labels else 1, H), torch.float64, dev)
        self._tables.clear()

    def _record_fused_pair(self, gen, tgt, i_time_start, with_maps, ignore_initial, time=None):
        from . import _lib
        first = next(iter(gen.values()))
        dev = first.device
        B, T, H, W = first.shape
        given = gen
        gen = {n: _flat(x, W) for n, x in given.items()}
        tgt = {n: (gen[n] if y is given[n] else _flat(y, W)) for n, y in tgt.items()}
        names = list(gen)
        n = len(names)
        self._ensure_rows(names, dev)
        wrows = self._weight_rows(names, dev)
        rows = self._row_table(names, dev)
        values, off = _plane_table(names, gen, tgt)
        table = _upload(values, torch.int64, dev)
        lib = _lib.lib()
        partial = torch.empty(int(lib.ace_diag_paired_partial_doubles(n, B, T, H, W)), dtype=torch.float64, device=dev)
        at = {k: table.data_ptr() + o for k, o in off.items()}
        series, n_time, t0 = self._series, self._n_time, i_time_start
        if not self._record_series:
            series, n_time, t0 = torch.empty(len(SERIES), len(self._rows), T, dtype=torch.float64, device=dev), T, 0
        zonal = with_maps and "zonal_mean" in self._labels
        zt0 = i_time_start - self._zon_first if zonal else 0
        with torch.cuda.device(dev):
            _check(lib.ace_diag_paired_window(
                at["gen"], at["gen_strides"], at["target"], at["target_strides"], rows.data_ptr(), wrows.data_ptr(),
                self._wplanes.data_ptr(), self._wplanes.shape[0], partial.data_ptr(), self._tsum.data_ptr(), self._zon.data_ptr(),
                series.data_ptr(),
                len(self._rows), n_time, t0, 1 if ignore_initial else 0, 1 if with_maps else 0, zt0,
                self._factor if zonal else 1, self._zon.shape[2], n, B, T, H, W, _lib.current_stream()))
            self._launches += 1
            if with_maps and self._hist is not None:
                self._launches += self._hist.record_fused(gen, tgt)
            if with_maps and self._regress is not None:
                self._launches += self._regress.record_fused(gen, tgt, i_time_start, time)
            if with_maps and self._calendar is not None:
                self._calendar.record_fused(gen, tgt, i_time_start, time)
            if with_maps and self._steps is not None:
                self._steps.record(tgt, i_time_start)
            if with_maps and self._ensembles is not None:
                self._launches += self._ensembles.record_fused(gen, tgt, i_time_start)
            if not with_maps or "power_spectrum" not in self._labels:
                return
            sht = self._get_sht()
            L, M = sht.lmax, sht.mmax
            k = max(1, self.spectrum_chunk_bytes // (B * T * (H * W * 4 + L * M * 8)))
            for side, d in enumerate((gen, tgt)):
                spec_names = [nm for nm in d if not self._omitted(nm)]
                acc = self._spec.data_ptr() + side * self._spec.shape[1] * L * 8
                for c0 in range(0, len(spec_names), k):
                    chunk = spec_names[c0:c0 + k]
                    coeffs = sht(torch.stack([d[nm] for nm in chunk]))            # (k, B, T, L, M) complex64
                    _check(lib.ace_diag_spectrum(coeffs.data_ptr(), self._row_table(chunk, dev).data_ptr(), acc,
                                                 self._spec.shape[1], len(chunk), B * T, L, M, _lib.current_stream()))
                    self._launches += 2

    # ---- results --------------------------------------------------------------------------------------------------------
    def _has_stats(self, name: str) -> bool:
        return self._stats is not None and name in self._stats

    def _series_data(self, kind: str = "denorm") -> Dict[str, Dict[str, torch.Tensor]]:
        """reduced.py:34-55, 213-218: metric -> name -> (n_timesteps,) series (sorted names), total / per-index count."""
        if not any(self._n_batches):
            raise ValueError("No batches have been recorded.")
        metrics = SERIES if kind == "denorm" else NORM_SERIES
        out: Dict[str, Dict[str, torch.Tensor]] = {m: {} for m in sorted(metrics)}
        if self._path != "fused":
            for metric in out:
                tot = self._t_series[kind].get(metric, {})
                for n in sorted(tot):
                    counts = torch.tensor(self._n_batches, dtype=torch.int32, device=tot[n].device)
                    out[metric][n] = self._reduce_mean(tot[n] / counts)
            return out
        dev = self._series.device
        counts = torch.tensor(self._n_batches, dtype=torch.float64, device=dev)
        for i, metric in enumerate(SERIES):
            if metric not in out:
                continue
            side = "gen" if metric in ("weighted_mean_gen", "weighted_std_gen") else "target"
            for n in sorted(self._present[side]):
                if kind == "norm" and not self._has_stats(n):
                    continue
                tot = self._series[i, self._rows[n]]
                if kind == "norm":
                    mu, sigma = self._stats[n]
                    if metric in _SHIFTED:                    # a record without the name adds 0 to the normalised total as well
                        tot = tot - mu * torch.tensor(self._present[side][n], dtype=torch.float64, device=dev)
                    tot = tot / sigma
                out[metric][n] = self._reduce_mean((tot / counts).float())
        return out

    def _time_means(self):
        """time_mean.py:151-162 for both sides: name -> (gen, target or None) fp64-or-input-dtype (H, W) maps, denormalised
        (fused) or per kind (torch)."""
        if self._tm_steps == 0 or not self._tm_names:
            raise ValueError("No data recorded.")
        div = self._tm_steps * self._tm_samples
        out: Dict[str, Dict[str, Any]] = {"denorm": {}, "norm": {}}
        for n in sorted(self._tm_names):
            if self._path == "fused":
                g = self._reduce_mean((self._tsum[0, self._rows[n]] / div).reshape(self._shape))
                t = self._reduce_mean((self._tsum[1, self._rows[n]] / div).reshape(self._shape)) if n in self._pair_names else None
                out["denorm"][n] = (g, t)
                if self._has_stats(n):
                    mu, sigma = self._stats[n]
                    out["norm"][n] = ((g - mu) / sigma, None if t is None else (t - mu) / sigma)
            else:
                for kind in out:
                    gs, ts = self._t_tsum[kind]
                    if n in gs:
                        out[kind][n] = (self._reduce_mean(gs[n] / self._tm_steps / self._tm_samples),
                                        self._reduce_mean(ts[n] / self._tm_steps / self._tm_samples) if n in ts else None)
        return out

    def _time_mean_logs(self, kind: str, maps) -> Dict[str, Any]:
        """time_mean.py:339-401 without the label"""
        logs: Dict[str, Any] = {}
        rmse_all, all_nan = {}, set()
        for n, (g, t) in maps.items():
            logs[f"gen_map/{n}"] = g.float().cpu()
            if t is None:
                continue
            w = self.weights_for(n, g.device).to(g.dtype)
            rmse_all[n] = float(_wmean(torch.square(g - t), w).sqrt())
            if bool(torch.isnan(t).all()):
                all_nan.add(n)
            logs[f"rmse/{n}"] = rmse_all[n]
            if kind == "denorm":
                logs[f"bias_map/{n}"] = (g - t).float().cpu()
                logs[f"bias/{n}"] = float(_wmean(g - t, w))
        if kind == "norm":
            if self._channel_mean_names is None:
                names = list(rmse_all)
            else:
                missing = [n for n in self._channel_mean_names if n not in rmse_all]
                if missing:
                    raise KeyError(f"channel_mean_names contains entries not present in the recorded data: {missing}. "
                                   f"Available: {sorted(rmse_all)}.")
                names = list(self._channel_mean_names)
            names = [n for n in names if n not in all_nan]
            if not names:
                raise ValueError("All target variables are NaN; cannot compute channel mean.")
            logs["rmse/channel_mean"] = sum(rmse_all[n] for n in names) / len(names)
        return logs

    def _spectra(self) -> Dict[str, torch.Tensor]:
        """spectrum.py:67-77, 207-215: name -> (2, lmax) [prediction, target] mean spectra; the target row of a name without a
        target is NaN."""
        out = {}
        for n in sorted(self._spec_side_counts[0]):
            sides = []
            for side in (0, 1):
                cnt = self._spec_side_counts[side].get(n)
                if cnt is None:
                    sides.append(None)
                elif self._path == "fused":
                    sides.append(self._reduce_mean((self._spec[side, self._rows[n]] / cnt).float()))
                else:
                    sides.append(self._reduce_mean(self._t_spec2[side][n].clone()))
            if sides[1] is None:
                sides[1] = torch.full_like(sides[0], float("nan"))
            out[n] = torch.stack(sides)
        return out

    def _zonal(self) -> Dict[str, torch.Tensor]:
        """zonal_mean.py:268-306: name -> (2, n_slots, H) [generated, target]; a slot that no window completed is NaN (the
        reference's 0 / 0)."""
        if self._zon_first is None:
            raise RuntimeError("No data recorded")
        done = self._zon_steps // self._factor
        out = {}
        for n in sorted(self._pair_names):
            if self._path == "fused":
                if n not in self._rows:
                    continue
                z = self._zon[:, self._rows[n]].float()
            elif n in self._t_zon[0] and n in self._t_zon[1]:
                z = torch.stack([self._t_zon[0][n].mean(dim=0), self._t_zon[1][n].mean(dim=0)])
            else:
                continue
            z = z.clone()
            z[:, done:] = float("nan")
            out[n] = torch.stack([self._reduce_mean(z[0]), self._reduce_mean(z[1])])
        return out

    @torch.no_grad()
    def get_dataset(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """get_reduced_diagnostics with the reference's variable keys (CPU tensors): ``mean`` / ``mean_norm``:
        ``<metric>-<name>`` (T,); ``time_mean`` / ``time_mean_norm``: ``bias_map-<name>``, ``gen_map-<name>`` (H, W);
        ``power_spectrum``: ``<name>`` (2, lmax) with the leading source axis [prediction, target]; ``zonal_mean``:
        ``gen-<name>``, ``error-<name>`` (n_slots, H)."""
        ds: Dict[str, Dict[str, torch.Tensor]] = {}
        L = self._labels
        for kind, key in (("denorm", "mean"), ("norm", "mean_norm")):
            if key in L:
                ds[L[key]] = {f"{m}-{n}": v.cpu() for m, d in self._series_data(kind).items() for n, v in d.items()}
        if "time_mean" in L or "time_mean_norm" in L:
            maps = self._time_means()
            for kind, key in (("denorm", "time_mean"), ("norm", "time_mean_norm")):
                if key in L:
                    d = ds[L[key]] = {}
                    for n, (g, t) in maps[kind].items():
                        if t is not None:
                            d[f"bias_map-{n}"] = (g - t).float().cpu() if self._path == "fused" else (g - t).cpu()
                            d[f"gen_map-{n}"] = g.float().cpu() if self._path == "fused" else g.cpu()
        if "power_spectrum" in L:
            ds[L["power_spectrum"]] = {n: v.cpu() for n, v in self._spectra().items()}
        if "zonal_mean" in L:
            d = ds[L["zonal_mean"]] = {}
            for n, z in self._zonal().items():
                d[f"gen-{n}"] = z[0].cpu()
                d[f"error-{n}"] = (z[0] - z[1]).cpu()
        if self._hist is not None and self._hist.recorded:
            ds[self._hist.label] = self._hist.dataset()
        if self._regress is not None:
            ds.update(self._regress.dataset())
        if self._calendar is not None:
            ds.update(self._calendar.dataset())
        for sub in (self._steps, self._ensembles):
            if sub is not None:
                ds.update(sub.dataset())
        return ds

    @torch.no_grad()
    def get_summary(self) -> InferenceSummary:
        """main.py:668-676: the logs of the sub-aggregators that are not time series, and ``loss`` =
        ``time_mean_norm/rmse/channel_mean``."""
        logs: Dict[str, Any] = {}
        L = self._labels
        if "time_mean" in L or "time_mean_norm" in L:
            maps = self._time_means()
            for kind, key in (("denorm", "time_mean"), ("norm", "time_mean_norm")):
                if key in L:
                    logs.update({f"{L[key]}/{k}": v for k, v in self._time_mean_logs(kind, maps[kind]).items()})
        if "power_spectrum" in L:
            label = L["power_spectrum"]
            for n, s in self._spectra().items():
                logs[f"{label}/{n}"] = s.cpu()
                if not bool(torch.isnan(s[1]).all()):
                    for k, v in spectrum_bias_scores(s[0].double().cpu(), s[1].double().cpu(), self._directional).items():
                        logs[f"{label}/{k}/{n}"] = v
        if "zonal_mean" in L:
            for n, z in self._zonal().items():
                logs[f"{L['zonal_mean']}/gen/{n}"] = z.cpu()
                logs[f"{L['zonal_mean']}/error/{n}"] = (z[0] - z[1]).cpu()
        if self._hist is not None and self._hist.recorded:
            logs.update({f"{self._hist.label}/{k}": v for k, v in self._hist.logs().items()})
        if self._regress is not None:
            logs.update(self._regress.logs())
        if self._calendar is not None:
            logs.update(self._calendar.logs())
        for sub in (self._steps, self._ensembles):
            if sub is not None:
                logs.update(sub.logs())
        key = L.get("time_mean_norm")
        return InferenceSummary(logs=logs, loss=logs.get(f"{key}/rmse/channel_mean") if key else None)

    def get_summary_logs(self) -> Dict[str, Any]:
        return self.get_summary().logs

    @torch.no_grad()
    def get_inference_logs(self) -> List[Dict[str, Any]]:
        """to_inference_logs (main.py:751-772): one dict per time index with ``<label>/forecast_step`` and
        ``<label>/<metric>/<name>`` floats for both ``mean`` labels; the summary logs go in the last dict."""
        rows: List[Dict[str, Any]] = [{} for _ in range(self._n_time if self._log_series else 1)]
        for kind, key in (("denorm", "mean"), ("norm", "mean_norm")):
            if key not in self._labels:
                continue
            label = self._labels[key]
            series = {f"{m}/{n}": v.cpu().tolist() for m, d in self._series_data(kind).items() for n, v in d.items()}
            for i, row in enumerate(rows):
                row[f"{label}/forecast_step"] = i
                for k in sorted(series):
                    row[f"{label}/{k}"] = series[k][i]
        rows[-1].update(self.get_summary_logs())
        return rows

    @torch.no_grad()
    def flush_diagnostics(self, subdir: Optional[str] = None):
        """main.py:713-731: one ``<sub-aggregator>_diagnostics.pt`` per non-empty sub-aggregator (root rank only)."""
        if not self._save:
            return
        if self._output_dir is None:
            raise ValueError("Output directory is not set.")
        from .distributed import Distributed
        out = self._output_dir if subdir is None else os.path.join(self._output_dir, subdir)
        ds = self.get_dataset()
        if Distributed.get_instance().is_root():
            os.makedirs(out, exist_ok=True)
            for name, d in ds.items():
                if d:
                    torch.save(d, os.path.join(out, f"{name}_diagnostics.pt"))
