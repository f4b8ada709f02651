"""Corrector step diagnostics: the record, its production on the rollout engine and its metrics.

  * ``StepDiagnostics`` (fme/core/step/step_diagnostics.py): ``delta[name]`` = corrected - network output, (B, T, H, W), for every
    variable the corrector wrote.  ``Stepper.predict(step_diagnostics=True)`` and ``RolloutEngine(step_diagnostics=True)`` attach
    it to the window they return (``WindowData.step_diagnostics``).  ``EnginePredict(step_diagnostics=True)`` clones it out with the outputs; the ocean and coupled engines refuse the flag.
    ``to_datasets`` is not built: there is no xarray here and no step-diagnostics writer.
  * ``CorrectionDeltaRecorder``: on the engine the corrector (``FusedPhysics``, csrc/physics.hip) edits the output planes in place,
    so the uncorrected planes of step s are copied into time slot s of a static (K, B, T, H, W) buffer between the unpack and the
    physics (``ace_stepdiag_snapshot``, one launch per step), and after the window one ``ace_stepdiag_delta_window`` turns the
    buffer into ``out - snapshot`` in place.  Stream ordered, no allocation, no host synchronisation, capturable.
  * ``CorrectionDeltaAggregator`` (fme/ace/aggregator/inference/step_diagnostics.py: ``CorrectionDeltaAggregator`` with its
    ``CorrectionDeltaTimeMeanAggregator`` and ``CorrectionDeltaMeanAggregator``): ``time_mean_norm/correction_magnitude/<name>``,
    ``time_mean_norm/correction_map/<name>`` and the per-step series ``mean_norm/weighted_correction_magnitude/<name>`` and
    ``mean_norm/weighted_correction_std/<name>`` of the normalised correction ``delta / std``.  Two paths compute the same thing:
    the torch path (any device) is the reference's ops in the reference's order; on the GPU one ``ace_diag_correction_window``
    (csrc/stepdiag.hip) reads every delta plane once, with no normalised or absolute copy, into fp64 accumulators.
  * ``StepDiagnosticsMetricConfig``: the reference's fields and defaults.  Both ``InferenceAggregatorConfig.step_diagnostics`` and
    ``InferenceEvaluatorAggregatorConfig.step_diagnostics`` take it (or its dict); ``run_inference`` / ``run_evaluator`` hand the
    window's record to an aggregator built with it.

ONE DELIBERATE DIFFERENCE FROM THE REFERENCE: there the record is always attached and the aggregators' default
``StepDiagnosticsMetricConfig()`` has ``correction_scalars=True``, so an evaluator run logs the correction metrics without being
asked.  Here both are opt-in - ``step_diagnostics=None`` (or ``{}``) in an aggregator configuration builds no correction aggregator
and the predict functions attach nothing unless ``step_diagnostics=True`` - so that nothing changes for a caller who does not ask.
Passing ``StepDiagnosticsMetricConfig()`` gives the reference's default."""
import dataclasses
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple

import torch

from .aggregator import _check

TensorMapping = Mapping[str, torch.Tensor]

TIME_MEAN_LABEL = "time_mean_norm"
TIME_SERIES_LABEL = "mean_norm"
SERIES_METRICS = ("weighted_correction_magnitude", "weighted_correction_std")


@dataclasses.dataclass
class StepDiagnostics:
    """step_diagnostics.py:27-65: per-sample diagnostic series aligned with the prediction data's forward steps.  ``delta`` may be
    empty; every operation is a no-op on an empty mapping."""
    delta: TensorMapping

    def to_device(self, device=None) -> "StepDiagnostics":
        dev = device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
        return StepDiagnostics(delta={k: v.to(dev) for k, v in self.delta.items()})

    def to_cpu(self) -> "StepDiagnostics":
        return StepDiagnostics(delta={k: v.cpu() for k, v in self.delta.items()})

    def sample_dim_size(self) -> Optional[int]:
        for tensor in self.delta.values():
            return tensor.shape[0]
        return None


class WindowData(dict):
    """name -> (B, T, H, W) outputs of a window plus the ``StepDiagnostics`` that rides with them (``None``: no corrector ran or
    it wrote nothing), in the manner of ``PrognosticState``."""
    step_diagnostics = None

    def __init__(self, data=(), step_diagnostics: Optional[StepDiagnostics] = None):
        super().__init__(data)
        self.step_diagnostics = step_diagnostics


def diagnosed_names(corrector, ocean, out_names: Sequence[str], prescribed: Sequence[str]) -> List[str]:
    """The names an engine reports a delta for, before any data exists: ``AtmosphereCorrector.modified_names`` without the
    prescribed prognostic names (single_module.py:717-728); the ocean's surface temperature among them raises
    (single_module.py:692-706).  No corrector: none."""
    if corrector is None:
        return []
    if not hasattr(corrector, "modified_names"):
        raise NotImplementedError(f"step_diagnostics: the deltas of {type(corrector).__name__} are not built (only the atmosphere "
                                  "corrector reports them)")
    names = list(corrector.modified_names(out_names))
    if ocean is not None and ocean.surface_temperature_name in names:
        raise ValueError("post-corrector adjustment names overlap the corrector's modified names: "
                         f"{[ocean.surface_temperature_name]}")
    return [n for n in names if n not in prescribed]


class CorrectionDeltaRecorder:
    """The engine's producer of ``StepDiagnostics.delta``: ``locate_gen(name, s)`` returns (data_ptr, per-sample stride in floats)
    of the plane holding output ``name`` of window step s, as for ``FusedPhysics``.  Owns the static (K, B, T, H, W) fp32 buffer;
    ``snapshot(s, stream)`` stores the planes of step s as they are (the uncorrected network output) into time slot s,
    ``finish_window(stream)`` replaces the buffer by ``out - snapshot`` in one launch, ``delta()`` returns its views per name."""

    def __init__(self, names: Sequence[str], batch: int, img_shape: Tuple[int, int], n_steps: int, locate_gen: Callable, device):
        self.names = list(names)
        self.batch, self.n_steps = int(batch), int(n_steps)
        H, W = img_shape
        self.hw = H * W
        K, B, T = len(self.names), self.batch, self.n_steps
        self.buffer = torch.zeros(K, B, T, H, W, dtype=torch.float32, device=device)
        where = [[locate_gen(n, s) for n in self.names] for s in range(T)]
        for s in range(T):
            for k, n in enumerate(self.names):
                if where[s][k] is None:
                    raise KeyError(n)
                # the window launch walks the steps by one stride: the planes of a name must lie at base + s * step stride, with
                # one sample stride, or finish_window would subtract from the wrong planes
                ptr, stride = where[s][k]
                step = where[1][k][0] - where[0][k][0] if T > 1 else 4 * self.hw
                if step % 4 or ptr != where[0][k][0] + s * step or stride != where[0][k][1]:
                    raise ValueError(f"CorrectionDeltaRecorder: the planes of '{n}' are not evenly strided over the window's steps")
        # per step: the sources, their sample strides, the time slot's planes, their sample strides
        rows = [[[int(p) for p, _ in where[s]], [int(st) for _, st in where[s]],
                 [self.buffer[k, :, s].data_ptr() for k in range(K)], [T * self.hw] * K] for s in range(T)]
        # the window: the output planes with (sample, step) strides, then the buffer's
        step_stride = [(where[1][k][0] - where[0][k][0]) // 4 if T > 1 else self.hw for k in range(K)]
        outs = [where[0][k][0] for k in range(K)]
        ostr = [v for k in range(K) for v in (where[0][k][1], step_stride[k])]
        snaps = [self.buffer[k].data_ptr() for k in range(K)]
        sstr = [v for k in range(K) for v in (T * self.hw, self.hw)]
        self._steps = torch.tensor(rows, dtype=torch.int64, device=device).reshape(T, 4, K) if K else None
        self._window = torch.tensor(outs + ostr + snaps + sstr, dtype=torch.int64, device=device) if K else None

    def snapshot(self, s: int, stream: int) -> None:
        K = len(self.names)
        if K == 0:
            return
        from . import _lib
        at = self._steps.data_ptr() + 8 * (4 * K) * s
        _check(_lib.lib().ace_stepdiag_snapshot(at, at + 8 * K, at + 16 * K, at + 24 * K, K, self.batch, self.hw, stream))

    def finish_window(self, stream: int) -> None:
        K = len(self.names)
        if K == 0:
            return
        from . import _lib
        at = self._window.data_ptr()
        _check(_lib.lib().ace_stepdiag_delta_window(at, at + 8 * K, at + 24 * K, at + 32 * K, K, self.batch, self.n_steps, self.hw,
                                                    stream))

    def delta(self) -> Dict[str, torch.Tensor]:
        return {n: self.buffer[k] for k, n in enumerate(self.names)}

    def step_diagnostics(self) -> Optional[StepDiagnostics]:
        return StepDiagnostics(delta=self.delta()) if self.names else None


# ---- the metrics ----------------------------------------------------------------------------------------------------------------
_CONFIG_FIELDS = ("correction_scalars", "correction_maps")


@dataclasses.dataclass
class StepDiagnosticsMetricConfig:
    """step_diagnostics.py:94-165 of the reference's aggregator (same fields and defaults): ``correction_scalars``: the time-mean
    ``correction_magnitude`` per variable and, where the aggregator logs time series, the per-step
    ``weighted_correction_magnitude`` / ``weighted_correction_std``; ``correction_maps``: the signed time-mean map per variable."""
    correction_scalars: bool = True
    correction_maps: bool = False

    @classmethod
    def from_state(cls, state) -> Optional["StepDiagnosticsMetricConfig"]:
        """``None`` / ``{}``: no correction aggregator (this project's default, see the module docstring); an instance or its dict.
        Any other key raises ``NotImplementedError``: nothing else of the step diagnostics is built."""
        if state is None or (isinstance(state, Mapping) and not state):
            return None
        if isinstance(state, cls):
            return state
        if isinstance(state, Mapping):
            unknown = sorted(set(state) - set(_CONFIG_FIELDS))
            if unknown:
                raise NotImplementedError(f"step_diagnostics: only {list(_CONFIG_FIELDS)} are built, got {unknown}")
            return cls(**state)
        raise NotImplementedError(f"step_diagnostics: a StepDiagnosticsMetricConfig or its dict, got {type(state).__name__}")

    def build(self, host, n_timesteps: int, enable_time_series: bool, normalize) -> Optional["CorrectionDeltaAggregator"]:
        """step_diagnostics.py:115-165: None when nothing is enabled or, with the default fields, no normaliser is given; a
        non-default configuration without a normaliser raises.  ``host``: the inference aggregator whose weights and masks the
        correction metrics share."""
        if not (self.correction_scalars or self.correction_maps):
            return None
        if normalize is None:
            if self != StepDiagnosticsMetricConfig():
                raise ValueError("step_diagnostics metrics were explicitly configured, but the aggregator was built without a "
                                 "normalizer, which the normalized-space correction metrics require. Supply a normalizer or leave "
                                 "the step_diagnostics configuration at its defaults.")
            return None
        return CorrectionDeltaAggregator(host, normalize, n_timesteps, record_scalars=self.correction_scalars,
                                         record_maps=self.correction_maps,
                                         time_series=self.correction_scalars and enable_time_series)


class CorrectionDeltaAggregator:
    """The correction metrics of the windows' ``StepDiagnostics`` (see the module docstring).  Silent until data arrives: no
    batches recorded, no logs, no datasets.  ``fused``: CUDA fp32 deltas take the HIP path; False: the torch ops on any device.
    ``normalize``: a ``StandardNormalizer``, its bound ``normalize``, or anything exposing per-name ``stds`` (the fused path reads
    them, the torch path calls ``normalize(delta, apply_mean=False)``); a bare callable serves the torch path only."""

    def __init__(self, host, normalize, n_timesteps: int, record_scalars: bool = True, record_maps: bool = False,
                 time_series: bool = True):
        self.fused = True
        self._host = host
        self._n_time = int(n_timesteps)
        self._scalars, self._maps, self._log_series = bool(record_scalars), bool(record_maps), bool(time_series)
        owner = getattr(normalize, "__self__", normalize)
        self._normalize_fn = normalize if callable(normalize) else getattr(normalize, "normalize", None)
        self._stds: Optional[Dict[str, float]] = None
        if hasattr(owner, "stds") and not getattr(owner, "fill_nans_on_normalize", False):
            self._stds = {n: float(v) for n, v in owner.stds.items()}
        self._path: Optional[str] = None
        self._launches = 0
        self._names: Optional[List[str]] = None
        self._n_samples = 0
        self._n_steps = 0
        self._n_batches = [0] * self._n_time
        # torch path state (the reference's own accumulators)
        self._t_signed: Dict[str, torch.Tensor] = {}
        self._t_magnitude: Dict[str, torch.Tensor] = {}
        self._t_total: Dict[str, Dict[str, torch.Tensor]] = {m: {} for m in SERIES_METRICS}
        # fused path state: one row per name in every fp64 accumulator
        self._rows: Dict[str, int] = {}
        self._sgn = None                  # (rows, H * W)
        self._mag = None                  # (rows, H * W)
        self._series = None               # (2, rows, n_time)
        self._wtab: Dict[str, int] = {}
        self._wplanes = None
        self._partial = None              # scratch of the window kernel
        self._scratch_series = None       # where the series go when they are not logged

    @property
    def log_time_series(self) -> bool:
        return self._log_series

    @property
    def has_data(self) -> bool:
        return self._n_steps > 0 and bool(self._names)

    def launches(self) -> int:
        """``ace_diag_correction_window`` calls made so far: one per recorded window on the fused path."""
        return self._launches

    def route(self, delta: TensorMapping) -> str:
        """"fused" when recording these deltas runs the HIP kernel, "torch" when it runs the torch ops."""
        if not self.fused or not delta or self._stds is None:
            return "torch"
        first = next(iter(delta.values()))
        for n, t in delta.items():
            if not (isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.device == first.device and t.dtype == torch.float32
                    and t.dim() == 4 and t.shape == first.shape and tuple(t.shape[-2:]) == tuple(self._host._shape)
                    and n in self._stds):
                return "torch"
        return "fused"

    # ---- recording --------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def record_batch(self, step_diagnostics: Optional[StepDiagnostics], i_time_start: int) -> None:
        """step_diagnostics.py:208-232, 288-323, 422-428: one window of deltas at time index ``i_time_start``.  ``None`` or an empty
        delta (no corrector ran) records nothing."""
        if step_diagnostics is None or not step_diagnostics.delta:
            return
        delta = dict(step_diagnostics.delta)
        first = next(iter(delta.values()))
        B, T = first.shape[:2]
        known = self._stds if self._stds is not None else None
        if known is not None:
            missing = sorted(set(delta) - set(known))
        else:
            probe = self._normalize_fn({k: v[:0] for k, v in delta.items()}, apply_mean=False)
            missing = sorted(set(delta) - set(probe))
        if missing:
            raise ValueError(f"The normalizer has no normalization constants for the correction delta variables {missing}; their "
                             "correction metrics cannot be computed.")
        if self._names is not None:
            if set(delta) != set(self._names):
                raise ValueError("The correction delta variable set must be constant across batches; previously recorded "
                                 f"{sorted(self._names)}, got {sorted(delta)}.")
            if B != self._n_samples:
                raise ValueError("The correction delta sample count must be constant across batches; previously recorded "
                                 f"{self._n_samples}, got {B}.")
        if self._log_series and (i_time_start < 0 or i_time_start + T > self._n_time):
            raise ValueError(f"steps {i_time_start}..{i_time_start + T - 1} are past the aggregator's n_timesteps {self._n_time}")
        if tuple(first.shape[-2:]) != tuple(self._host._shape):
            raise ValueError(f"deltas of shape {tuple(first.shape[-2:])} on an aggregator of {tuple(self._host._shape)}")
        path = self.route(delta)
        if self._path is None:
            self._path = path
        elif path != self._path:
            raise ValueError(f"this aggregator reduces on the {self._path} path, but a window only the {path} path takes came in "
                             "(device, dtype or shape changed between windows)")
        if path == "fused":
            self._record_fused(delta, i_time_start)
        else:
            self._record_torch(delta, i_time_start)
        self._names = sorted(delta)
        self._n_samples = B
        self._n_steps += T
        if self._log_series:
            for i in range(i_time_start, i_time_start + T):
                self._n_batches[i] += 1

    def _record_torch(self, delta, i_time_start):
        """The reference's ops in the reference's order: normalize(delta, apply_mean=False), the time-mean sums
        (step_diagnostics.py:313-321), the two area-weighted series (reduced.py:390-413; gridded_ops.py:75-154)."""
        norm = self._normalize_fn(delta, apply_mean=False)
        T = next(iter(norm.values())).shape[1]
        sl = slice(i_time_start, i_time_start + T)
        for n, x in norm.items():
            signed = x.sum(dim=1).sum(dim=0)
            magnitude = x.abs().sum(dim=1).sum(dim=0)
            if n in self._t_signed:
                self._t_signed[n] += signed
                self._t_magnitude[n] += magnitude
            else:
                self._t_signed[n], self._t_magnitude[n] = signed, magnitude
        if not self._log_series:
            return
        for n, x in norm.items():
            w = self._host.weights_for(n, x.device)
            values = {"weighted_correction_magnitude": _wmean(x.abs(), w),
                      "weighted_correction_std": _wmean((x - _wmean(x, w, keepdim=True)) ** 2, w).sqrt()}
            for metric, v in values.items():
                tot = self._t_total[metric]
                if n not in tot:
                    tot[n] = torch.zeros(self._n_time, dtype=v.dtype, device=x.device)
                tot[n][sl] += v.mean(dim=0)

    def _record_fused(self, delta, i_time_start):
        import numpy as np

        from . import _lib
        from .aggregator import _flat, _grow_rows, _upload_planes
        first = next(iter(delta.values()))
        dev = first.device
        B, T, H, W = first.shape
        HW = H * W
        delta = {n: _flat(x, W) for n, x in delta.items()}
        names = list(delta)
        _grow_rows(self, names, dev, _sgn=lambda R: (R, HW), _mag=lambda R: (R, HW), _series=lambda R: (2, R, self._n_time))
        wrows = []
        for n in names:
            k = self._host._mask_key(n) or ""
            if k not in self._wtab:
                self._wtab[k] = len(self._wtab)
                w = self._host.weights_for(n, dev).reshape(1, -1)
                self._wplanes = w.clone() if self._wplanes is None else torch.cat([self._wplanes, w])
            wrows.append(self._wtab[k])
        sections = [np.asarray([self._stds[n] for n in names], np.float32), np.asarray([self._rows[n] for n in names], np.int32),
                    np.asarray(wrows, np.int32)]
        at, (stds_at, rows_at, wrows_at) = _upload_planes(names, delta, None, dev, sections=sections)
        lib = _lib.lib()
        K = len(names)
        # the partial moments, and without the time series a zeroed stand-in the window's series are added to (the kernel computes
        # them with the same loads): kept from window to window, regrown only when a window needs more
        need = int(lib.ace_diag_correction_partial_doubles(K, B, T, HW))
        if self._partial is None or self._partial.numel() < need or self._partial.device != dev:
            self._partial = torch.empty(need, dtype=torch.float64, device=dev)
        partial = self._partial
        series, n_time, t0 = self._series, self._n_time, i_time_start
        if not self._log_series:
            shape = (2, len(self._rows), T)
            if self._scratch_series is None or tuple(self._scratch_series.shape) != shape or self._scratch_series.device != dev:
                self._scratch_series = torch.zeros(shape, dtype=torch.float64, device=dev)
            series, n_time, t0 = self._scratch_series, T, 0
        with torch.cuda.device(dev):
            _check(lib.ace_diag_correction_window(at["gen"], at["gen_strides"], stds_at, rows_at, wrows_at, self._wplanes.data_ptr(),
                                                  self._wplanes.shape[0], partial.data_ptr(), self._sgn.data_ptr(),
                                                  self._mag.data_ptr(), series.data_ptr(), len(self._rows), n_time, t0, K, B, T, HW,
                                                  _lib.current_stream()))
        self._launches += 1

    # ---- results ----------------------------------------------------------------------------------------------------------------
    def _time_means(self) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
        """step_diagnostics.py:329-336: (signed, magnitude) time-mean maps, sum / (steps * samples), sorted names."""
        denom = self._n_steps * self._n_samples
        shape = tuple(self._host._shape)
        signed, magnitude = {}, {}
        for n in self._names:
            if self._path == "fused":
                s = (self._sgn[self._rows[n]] / denom).float().reshape(shape)
                m = (self._mag[self._rows[n]] / denom).float().reshape(shape)
            else:
                s, m = self._t_signed[n] / denom, self._t_magnitude[n] / denom
            signed[n], magnitude[n] = self._host._reduce_mean(s), self._host._reduce_mean(m)
        return signed, magnitude

    @torch.no_grad()
    def summary_logs(self) -> Dict[str, Any]:
        """step_diagnostics.py:338-361 under the ``time_mean_norm`` label: ``correction_magnitude/<name>`` (a float: the
        area-weighted mean of the time-mean magnitude map under the name's mask weights) and, with ``correction_maps``,
        ``correction_map/<name>`` (the signed time-mean map, an (H, W) tensor in place of the reference's image)."""
        if not self.has_data:
            return {}
        signed, magnitude = self._time_means()
        logs: Dict[str, Any] = {}
        for n in signed:
            if self._scalars:
                w = self._host.weights_for(n, magnitude[n].device)
                logs[f"{TIME_MEAN_LABEL}/correction_magnitude/{n}"] = float(_wmean(magnitude[n], w))
            if self._maps:
                logs[f"{TIME_MEAN_LABEL}/correction_map/{n}"] = signed[n].cpu()
        return logs

    @torch.no_grad()
    def series_data(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """step_diagnostics.py:430-431: metric -> name -> (n_timesteps,) series, total / per-index record count (NaN at an index
        never recorded), sorted names."""
        if not (self._log_series and self.has_data):
            return {}
        out: Dict[str, Dict[str, torch.Tensor]] = {m: {} for m in SERIES_METRICS}
        for i, metric in enumerate(SERIES_METRICS):
            for n in self._names:
                if self._path == "fused":
                    counts = torch.tensor(self._n_batches, dtype=torch.float64, device=self._series.device)
                    v = (self._series[i, self._rows[n]] / counts).float()
                else:
                    tot = self._t_total[metric][n]
                    v = tot / torch.tensor(self._n_batches, dtype=torch.int32, device=tot.device)
                out[metric][n] = self._host._reduce_mean(v)
        return out

    @torch.no_grad()
    def series_rows(self) -> List[Dict[str, float]]:
        """One dict per time index: ``mean_norm/<metric>/<name>`` floats (what the reference's ``mean_norm/correction_series``
        table resolves to in ``to_inference_logs``); empty without the series."""
        data = {f"{TIME_SERIES_LABEL}/{m}/{n}": v.cpu().tolist() for m, d in self.series_data().items() for n, v in d.items()}
        if not data:
            return []
        return [{k: v[i] for k, v in sorted(data.items())} for i in range(self._n_time)]

    @torch.no_grad()
    def datasets(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """step_diagnostics.py:246-255, 86-91: ``time_mean_norm_correction``: ``correction_map-<name>`` (H, W) with
        ``correction_maps``; ``mean_norm_correction``: ``<metric>-<name>`` (n_timesteps,) (CPU tensors; empty blocks left out)."""
        out: Dict[str, Dict[str, torch.Tensor]] = {}
        if not self.has_data:
            return out
        if self._maps:
            out[f"{TIME_MEAN_LABEL}_correction"] = {f"correction_map-{n}": v.cpu() for n, v in self._time_means()[0].items()}
        series = {f"{m}-{n}": v.cpu() for m, d in self.series_data().items() for n, v in d.items()}
        if series:
            out[f"{TIME_SERIES_LABEL}_correction"] = series
        return out


def _wmean(x: torch.Tensor, w: torch.Tensor, keepdim: bool = False) -> torch.Tensor:
    """metrics.py:63-90 under gridded_ops.py:271-281: the weighted mean over the last two dimensions; a pixel of weight 0 does not
    count, NaN included."""
    w = w.expand(x.shape)
    return (x.where(w != 0.0, 0.0) * w).sum(dim=(-2, -1), keepdim=keepdim) / w.sum(dim=(-2, -1), keepdim=keepdim)
