"""The metric configurations of the inference evaluator aggregator and the build rules of its configuration."""
import dataclasses
import datetime
import logging
from typing import Any, Callable, Dict, List, Optional, Sequence

from ..aggregator import _is_healpix
from .calendar import MIN_YEARS_FOR_FILTERED_TPI


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
    """``fill_masked`` (not a field of the reference, which always fills): flood-fill the masked pixels of a masked name before the
    SHT (``SmoothFloodFill(num_steps=4)``, spectrum.py:331; ace_amd/fill.py) instead of omitting the name.  The reference's
    behaviour is ``True``; the default ``False`` keeps what the evaluator computed before the fill was built."""
    report_directional_bias: bool = True                                  # spectrum.py:317-322
    fill_masked: bool = False


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
class VideoMetricConfig(MetricConfig):
    """video.py:522-541.  ``variables``: videos of these names only (the accumulators hold every time index of every kept name:
    ace_amd/evaluator/video.py states the memory); ``enable_extended_videos``: also the bias, RMSE, error extrema and variance
    ratio videos."""
    enabled: bool = False
    strict: bool = True
    name: Optional[str] = "video"
    enable_extended_videos: bool = False


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


def _name_step(m, stem: str) -> None:
    if m.target not in ("denorm", "norm"):
        raise ValueError(f"target must be 'denorm' or 'norm', got {m.target!r}")
    if m.name is None:
        m.name = f"{stem}_{m.step}" + ("_norm" if m.target == "norm" else "")


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
        _name_step(self, "mean_step")


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
        _name_step(self, "ensemble_step")


@dataclasses.dataclass
class InferenceSummary:
    logs: Dict[str, Any]
    loss: Optional[float]


# Every metric field, in the order ``build`` decides them (the order of the labels and of ``skipped``): its typed class, what an
# enabled configuration that is not of that class means - "built" all the same, "skipped" as the reference's non-strict path skips
# an unsupported metric (main.py:143-153; a strict one raises), or "raises" - and the family that builds it.
_FIELDS = (
    ("mean_denorm", MetricConfig, "built", "paired"),
    ("mean_norm", MetricConfig, "built", "paired"),
    ("time_mean_denorm", MetricConfig, "built", "paired"),
    ("time_mean_norm", MetricConfig, "built", "paired"),
    ("power_spectrum", MetricConfig, "built", "paired"),
    ("zonal_mean", MetricConfig, "built", "paired"),
    ("step_means", StepMeanMetricConfig, "skipped", "stepped"),           # lists: an entry of the typed class is built
    ("ensembles", EnsembleMetricConfig, "skipped", "stepped"),
    ("video", VideoMetricConfig, "raises", "video"),
    ("seasonal", SeasonalMetricConfig, "raises", "calendar"),
    ("histogram", HistogramMetricConfig, "raises", "histogram"),
    ("annual", AnnualMetricConfig, "skipped", "calendar"),
    ("enso_index", EnsoIndexMetricConfig, "skipped", "calendar"),
    ("enso_coefficient", EnsoCoefficientMetricConfig, "skipped", "regress"),
    ("ipo_index", IpoIndexMetricConfig, "skipped", "calendar"),
    ("trend", TrendMetricConfig, "raises", "regress"),
    ("near_zero_fraction", NearZeroFractionMetricConfig, "raises", "regress"),
)


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
    video: MetricConfig = dataclasses.field(default_factory=lambda: MetricConfig(enabled=False, strict=True))
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
              n_ensemble_per_ic: int = 1, video_max_bytes: int = 32 << 30) -> "InferenceEvaluatorAggregator":
        """``normalize``: a ``StandardNormalizer``, its bound ``normalize``, or anything exposing per-name ``means`` and ``stds``
        (the fused path reads the statistics, the torch path calls it); a bare callable serves the torch path only.
        ``step_diagnostics`` (a field): a ``StepDiagnosticsMetricConfig`` (ace_amd/step_diagnostics.py) or its dict builds the
        correction aggregator; ``None`` / ``{}`` (the default) builds none - one deliberate difference from the reference, whose
        default ``StepDiagnosticsMetricConfig()`` is on; a dict with any other key raises ``NotImplementedError``.
        ``n_ensemble_per_ic``: the samples of a window are ``n_ic x n_ensemble_per_ic`` members, sample ``b = i * n_ensemble_per_ic +
        e`` (``inference.repeat_members``); with 1 the ensemble entries are accepted but neither recorded nor reported
        (main.py:560-562, 604-621).  ``video_max_bytes``: the most the video metric's accumulators may take (names x n_timesteps
        x H x W x 16 bytes, x 48 with extended videos); a window that would pass it raises ``ValueError``."""
        if int(n_ensemble_per_ic) < 1:
            raise ValueError(f"n_ensemble_per_ic must be >= 1, got {n_ensemble_per_ic}")
        if self.monthly_reference_data is not None or self.time_mean_reference_data is not None:
            raise NotImplementedError("monthly_reference_data / time_mean_reference_data are netCDF files and there is no netCDF "
                                      "reader here; compare the maps of get_dataset() offline")
        from ..step_diagnostics import StepDiagnosticsMetricConfig
        step_diagnostics = StepDiagnosticsMetricConfig.from_state(self.step_diagnostics)     # refuses what is not built
        for field, typed, bare, _ in _FIELDS:
            if bare == "raises" and getattr(self, field).enabled and not isinstance(getattr(self, field), typed):
                if field in ("histogram", "video"):
                    raise NotImplementedError(f"the {field} metric is built from its typed configuration only: pass a "
                                              f"{typed.__name__}, not a bare MetricConfig")
                raise NotImplementedError(f"the {field} metric is not built")
        skipped = []
        regress = {"trend": self.trend, "enso_coefficient": self.enso_coefficient, "near_zero_fraction": self.near_zero_fraction}
        regress = {field: m if m.enabled else None for field, m in regress.items()}
        if regress["trend"] is not None and n_forward_steps < 2:         # trend.py:300-308, through the skipped-metric path
            if self.trend.strict:
                raise NotImplementedError(f"trend metric requires at least 2 forward steps, got {n_forward_steps} (strict=True)")
            skipped.append("trend")
            regress["trend"] = None
        enso = regress["enso_coefficient"]
        if not (isinstance(enso, EnsoCoefficientMetricConfig) and enso.index is not None):
            regress["enso_coefficient"] = None
        elif getattr(dataset_info, "timestep", None) is not None and \
                (n_ic_steps + n_forward_steps) * dataset_info.timestep <= datetime.timedelta(days=1800):
            regress["enso_coefficient"] = None                            # enso_coefficient.py:478-483; skipped or raised below
        annual = self.annual
        if annual.enabled and isinstance(annual, AnnualMetricConfig) and annual.reference_data is not None:
            raise NotImplementedError("annual.reference_data is a netCDF file and there is no netCDF reader here; compare the "
                                      "series of get_dataset() offline")
        calendar: Dict[str, MetricConfig] = {}
        stepped: Dict[str, List[MetricConfig]] = {}
        why: Dict[str, Optional[str]] = {}
        unbuilt = []                                                      # (field, its typed class), in table order
        late: List[str] = []
        for field, typed, bare, by in _FIELDS:
            m = getattr(self, field)
            if by == "stepped":
                unbuilt.append((field, typed))                            # its bare entries, the defaults
                stepped[field] = []
                what = "step_mean step" if field == "step_means" else "ensemble step"
                for e in m:
                    if not (e.enabled and isinstance(e, typed)):
                        continue
                    if e.step > n_forward_steps:                          # reduced.py:226-230, ensemble.py:486-490
                        reason = f"{what} {e.step} exceeds n_forward_steps={n_forward_steps}"
                        if e.strict:
                            raise NotImplementedError(f"the {e.name} metric is not supported for this configuration: {reason} "
                                                      "(strict=True)")
                        late.append(e.name)
                    else:
                        stepped[field].append(e)
            elif by == "calendar" and m.enabled and isinstance(m, typed):
                why[field] = self._calendar_unsupported(field, dataset_info, n_ic_steps + n_forward_steps)
                if why[field] is None:
                    calendar[field] = m
                else:
                    unbuilt.append((field, typed))
            elif bare == "skipped" and regress.get(field) is None:
                unbuilt.append((field, typed))
        for field, typed in unbuilt:
            for m in (getattr(self, field) if field in stepped else [getattr(self, field)]):
                if not m.enabled or (field in stepped and isinstance(m, typed)):
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
        for field, _, _, by in _FIELDS:
            m = getattr(self, field)
            if by != "paired":
                continue
            if m.variables is not None:
                raise NotImplementedError(f"{field}.variables: a per-metric variable filter is not built")
            if m.enabled:
                labels[field.replace("_denorm", "")] = m.name or field.replace("_denorm", "")
        taken = list(labels.values())                                     # every label that heads a block of the logs and the dataset
        taken += [m.name or field for field, m in (("video", self.video), ("histogram", self.histogram), *regress.items())
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
        from .aggregator import InferenceEvaluatorAggregator
        agg = InferenceEvaluatorAggregator(
            dataset_info, int(n_ic_steps), int(n_forward_steps), normalize, labels=labels, skipped=skipped,
            zonal_mean_max_size=getattr(self.zonal_mean, "zonal_mean_max_size", 4096), channel_mean_names=channel_mean_names,
            report_directional_bias=getattr(self.power_spectrum, "report_directional_bias", True), output_dir=output_dir,
            save_diagnostics=save_diagnostics, sht_factory=sht_factory,
            histogram=self.histogram if self.histogram.enabled else None, video=self.video if self.video.enabled else None,
            video_max_bytes=int(video_max_bytes), calendar=calendar, **regress, **stepped,
            n_ensemble_per_ic=int(n_ensemble_per_ic), fill_masked=bool(getattr(self.power_spectrum, "fill_masked", False)))
        if step_diagnostics is not None:
            # step_diagnostics.py:115-165: the per-step series go with the evaluator's own (``mean`` / ``mean_norm`` enabled)
            agg._correction = step_diagnostics.build(agg, int(n_ic_steps) + int(n_forward_steps), agg._log_series, normalize)
        return agg
