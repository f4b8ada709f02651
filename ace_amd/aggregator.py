"""The no-target inference aggregator on a lat-lon grid (fme/ace/aggregator/inference/main.py:785-985): the global-mean time
series (``mean``, reduced.py:370-497), the time-mean maps (``time_mean``, time_mean.py:103-163) and the spherical power spectra
(``power_spectrum``, spectrum.py:25-78) of an inference run, for ``ace_amd.inference.run_inference``.

xarray, netCDF, wandb and torch_harmonics are not on this stack: logs hold tensors and floats where the reference logs images and
figures, ``get_dataset`` returns plain dicts of tensors, ``flush_diagnostics`` writes ``torch.save`` archives with the reference's
stems (``<sub-aggregator>_diagnostics.pt`` for its ``.nc``, as ``TensorFileWriter`` writes ``restart.pt``), and the spectrum's SHT
is the project's own forward transform.  Not built: the ``annual`` and ``enso_index`` sub-aggregators, reference time means and
HEALPix grids.  The correction metrics of the corrector's step diagnostics (ace_amd/step_diagnostics.py) are opt-in:
``InferenceAggregatorConfig(step_diagnostics=StepDiagnosticsMetricConfig())`` with ``build(..., normalize=...)``.  The evaluator that compares a rollout with a target record (``InferenceEvaluatorAggregator``) is
ace_amd/evaluator/.

The reference flood-fills the NaNs of a masked field before the spectrum (``SmoothFloodFill(num_steps=4)``, spectrum.py:331).  Here
that is the option ``fill_masked_spectrum`` (ace_amd/fill.py), off by default: a name whose mask has a zero is then left out of the
spectrum and listed in ``omitted``.  The reference's behaviour is "on": a masked name with a valid pixel is filled, takes part and is
listed in ``filled``; a name without a valid pixel stays in ``omitted``.

Two paths compute the same thing.  The torch path (``fused = False``, any device) is the reference's formulas in fp32 torch ops.
On the GPU (fp32 (B, T, H, W) fields with contiguous rows) a window is reduced by the HIP kernels of csrc/diag.hip, reading every
``data[name]`` in place through a pointer table:

  * ``ace_diag_window``: one read of every plane gives the per-(sample, step, name) weighted mean and std (fp64 two-pass moments per
    wave, combined with Chan's update in a fixed order) and the per-pixel time sums, added to a persistent fp64 accumulator;
  * per chunk of names: the planes stacked into one buffer, one forward SHT (``RealSHT(nlat, nlon, grid="legendre-gauss")``, fp32)
    and one ``ace_diag_spectrum`` adding sum over m of |c_lm|^2 to a fp64 per-(name, l) accumulator.  With ``fill_masked_spectrum``
    the buffer is built by one ``ace_diag_fill_planes`` (csrc/fill.hip) in place of the ``torch.stack``: the planes of masked names
    filled, the others copied.

No float atomics and no host synchronisation in ``record_batch``: results are read back by the ``get_*`` calls only, and two
identical runs give bitwise identical diagnostics.  Peak extra device memory of a fused window: the fp64 partial moments
(B * T * names * ceil(H * W / 1024) * 4 * 24 bytes, 9.8 MB at 1 degree with 40 names and 40 steps) plus one spectrum chunk of at
most ``spectrum_chunk_bytes`` (default 256 MiB: stacked planes and their coefficients)."""
import dataclasses
import functools
import itertools
import os
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple

import torch

from ._lib import check

TensorMapping = Mapping[str, torch.Tensor]


def _is_healpix(dataset_info) -> bool:
    hc = getattr(dataset_info, "horizontal_coordinates", None)
    aw = getattr(dataset_info, "area_weights", None)
    return (getattr(dataset_info, "grid", None) == "healpix" or (hc is not None and hasattr(hc, "face"))
            or (aw is not None and torch.as_tensor(aw).dim() != 2))


@dataclasses.dataclass
class InferenceAggregatorConfig:
    """main.py:785-890 (same fields).  ``time_mean_reference_data`` (a netCDF path) is refused at build time: there is no netCDF
    reader here.  ``step_diagnostics``: a ``StepDiagnosticsMetricConfig`` (ace_amd/step_diagnostics.py) or its dict builds the
    correction aggregator; ``None`` / ``{}`` (the default) builds none - one deliberate difference from the reference, whose
    default ``StepDiagnosticsMetricConfig()`` is on; pass that for the reference's behaviour.  A dict with any other key is
    refused (``NotImplementedError``): nothing else of the step diagnostics is built.  ``fill_masked_spectrum`` (not a
    field of the reference, which always fills): flood-fill masked names before the spectrum instead of omitting them; the
    reference's behaviour is ``True``, the default ``False`` keeps what this aggregator computed before the fill was built."""
    log_global_mean_time_series: bool = True
    time_mean_reference_data: Optional[str] = None
    step_diagnostics: Optional[Any] = None
    fill_masked_spectrum: bool = False

    def build(self, dataset_info, n_timesteps: int, output_dir: Optional[str] = None, save_diagnostics: bool = False,
              sht_factory: Optional[Callable[[int, int], Callable]] = None, normalize=None) -> "InferenceAggregator":
        """``sht_factory(nlat, nlon)``: the forward SHT of the spectrum (default: the native
        ``ace_amd.sht.RealSHT(nlat, nlon, grid="legendre-gauss", precision="fp32")``, device tensors only).  ``normalize``: the
        stepper's normaliser (or its bound ``normalize``), which the correction metrics of ``step_diagnostics`` need."""
        from .step_diagnostics import StepDiagnosticsMetricConfig
        step_diagnostics = StepDiagnosticsMetricConfig.from_state(self.step_diagnostics)
        if self.time_mean_reference_data is not None:
            raise NotImplementedError("time_mean_reference_data is a netCDF file and there is no netCDF reader here; "
                                      "compare the time-mean maps of get_dataset() offline")
        if _is_healpix(dataset_info):
            raise NotImplementedError("the inference aggregator is built for lat-lon grids only, not HEALPix")
        if getattr(dataset_info, "area_weights", None) is None:
            raise ValueError("the inference aggregator needs the dataset's area weights: build the DatasetInfo with lat (and "
                             "lon) or area_weights")
        agg = InferenceAggregator(dataset_info, int(n_timesteps), log_global_mean_time_series=self.log_global_mean_time_series,
                                  output_dir=output_dir, save_diagnostics=save_diagnostics, sht_factory=sht_factory,
                                  fill_masked_spectrum=self.fill_masked_spectrum)
        if step_diagnostics is not None:
            agg._correction = step_diagnostics.build(agg, int(n_timesteps), self.log_global_mean_time_series, normalize)
        return agg


def _default_sht(nlat: int, nlon: int):
    from .sht import RealSHT
    # the reference's spectrum always uses a legendre-gauss SHT, whatever the data grid: LatLonCoordinates builds its
    # LatLonOperations without a grid (coordinates.py:687-690) and LatLonOperations defaults to "legendre-gauss"
    # (gridded_ops.py:291)
    return RealSHT(nlat, nlon, grid="legendre-gauss", precision="fp32")


class InferenceAggregator:
    """main.py:893-1005 for the ``mean``, ``time_mean`` and ``power_spectrum`` sub-aggregators."""

    def __init__(self, dataset_info, n_timesteps: int, log_global_mean_time_series: bool = True,
                 output_dir: Optional[str] = None, save_diagnostics: bool = False,
                 sht_factory: Optional[Callable[[int, int], Callable]] = None, spectrum_chunk_bytes: int = 256 << 20,
                 fill_masked_spectrum: bool = False):
        if save_diagnostics and output_dir is None:
            raise ValueError("Output directory must be set to save diagnostics")
        self.fused = True                 # CUDA fp32 windows take the HIP path; False: the torch ops on any device
        self.spectrum_chunk_bytes = int(spectrum_chunk_bytes)
        self.fill_masked_spectrum = bool(fill_masked_spectrum)
        self._log_series = bool(log_global_mean_time_series)
        self._n_time = int(n_timesteps)
        self._output_dir = output_dir
        self._save = save_diagnostics
        self._sht_factory = sht_factory or _default_sht
        self._sht = None
        self._area = torch.as_tensor(dataset_info.area_weights).detach().to("cpu", torch.float32)
        self._shape = tuple(self._area.shape)
        self._masks = getattr(dataset_info, "mask_provider", None)
        self._weights: Dict[Tuple[str, str], torch.Tensor] = {}
        self._omit: Dict[str, bool] = {}
        self._fill_names: Dict[str, bool] = {}
        from .fill import FillTables
        self._fill = FillTables()
        self._n_seen = 0
        self._correction = None           # the CorrectionDeltaAggregator of a configured ``step_diagnostics`` (step_diagnostics.py)
        self._path: Optional[str] = None
        self._launches = 0
        # per-time-index record count (reduced.py: _n_batches), host side
        self._n_batches = [0] * self._n_time
        self._series_names: List[str] = []
        self._tm_names: List[str] = []
        self._tm_steps = 0
        self._tm_samples: Optional[int] = None
        self._spec_names: List[str] = []
        self._spec_counts: Dict[str, int] = {}
        # torch path state (the reference's own accumulators)
        self._t_total: Dict[str, Dict[str, torch.Tensor]] = {"weighted_mean_gen": {}, "weighted_std_gen": {}}
        self._t_tm: Optional[Dict[str, torch.Tensor]] = None
        self._t_spec: Dict[str, torch.Tensor] = {}
        # fused path state: one row per name in every fp64 accumulator
        self._rows: Dict[str, int] = {}
        self._series = None               # (2, rows, n_time)
        self._tsum = None                 # (rows, H * W)
        self._spec = None                 # (rows, lmax)
        self._wtab: Dict[str, int] = {}
        self._wplanes = None
        self._tables: Dict[Any, torch.Tensor] = {}

    # ---- weights ------------------------------------------------------------------------------------------------------
    def _mask_key(self, name: str) -> Optional[str]:
        if not self._masks:
            return None
        if hasattr(self._masks, "mask_key_for"):
            return self._masks.mask_key_for(name)
        return name if self._masks.get_mask_tensor_for(name) is not None else None

    def weights_for(self, name: str, device) -> torch.Tensor:
        """gridded_ops.py:271-281: area weights x the name's mask, when the dataset has one for it."""
        key = self._mask_key(name) or ""
        cached = self._weights.get((key, str(device)))
        if cached is None:
            w = self._area
            if key:
                w = w * self._masks.get_mask_tensor_for(name).detach().to("cpu", torch.float32)
            cached = self._weights[(key, str(device))] = w.to(device)
        return cached

    @property
    def omitted(self) -> List[str]:
        """Names left out of the power spectrum: their mask has zeros and ``fill_masked_spectrum`` is off (the reference
        flood-fills the NaNs there first), or it is on and their mask has no valid pixel to fill from."""
        return [n for n, o in self._omit.items() if o]

    @property
    def filled(self) -> List[str]:
        """Names whose masked pixels are flood-filled before the spectrum (``fill_masked_spectrum``)."""
        return [n for n, f in self._fill_names.items() if f]

    def _omitted(self, name: str) -> bool:
        o = self._omit.get(name)
        if o is None:
            key = self._mask_key(name)
            o = bool(key) and bool((self._masks.get_mask_tensor_for(name) == 0).any())
            if o and self.fill_masked_spectrum and self._fill.has_valid(key, self._masks.get_mask_tensor_for(name)):
                self._fill_names[name], o = True, False
            self._omit[name] = o
        return o

    def _filled(self, name: str) -> bool:
        return not self._omitted(name) and self._fill_names.get(name, False)

    def _fill_torch(self, name: str, x: torch.Tensor) -> torch.Tensor:
        """the torch path's input of the SHT: ``x`` flood-filled when ``name`` is a filled name"""
        if not self._filled(name):
            return x
        from .fill import smooth_flood_fill
        mask = self._masks.get_mask_tensor_for(name)
        return smooth_flood_fill(x, mask, tables=self._fill.on(self._mask_key(name), mask, x.device))

    def _spectrum_input(self, names: Sequence[str], fields: Sequence[torch.Tensor], dev):
        """The fused path's (len(names), B, T, H, W) input of the SHT and the native launches it took: the ``torch.stack`` of the
        fields (0: a copy, not a native launch), or with ``fill_masked_spectrum`` one ``ace_diag_fill_planes`` (1) that fills the
        planes of the filled names and copies the others."""
        if not self.fill_masked_spectrum:
            return torch.stack(list(fields)), 0
        import numpy as np

        from . import _lib
        B, T, H, W = fields[0].shape
        tab = []
        for n in names:
            mask = self._masks.get_mask_tensor_for(n) if self._filled(n) else None
            tab.append(-1 if mask is None else self._fill.row(self._mask_key(n), mask, dev))
        at, (tab_at,) = _upload_planes(names, dict(zip(names, fields)), None, dev, sections=[np.asarray(tab, np.int32)])
        layers, blurred, nmasks = self._fill.stacks(dev)
        lib = _lib.lib()
        planes = torch.empty((len(names), B, T, H, W), dtype=torch.float32, device=dev)
        scratch = torch.empty(max(1, int(lib.ace_diag_fill_scratch_doubles(len(names), B, T, H, W))), dtype=torch.float64, device=dev)
        _check(lib.ace_diag_fill_planes(at["gen"], at["gen_strides"], tab_at, layers.data_ptr() if nmasks else None,
                                        blurred.data_ptr() if nmasks else None, nmasks, scratch.data_ptr(), planes.data_ptr(),
                                        len(names), B, T, H, W, _lib.current_stream()))
        return planes, 1

    @property
    def records_step_diagnostics(self) -> bool:
        """True when ``record_batch`` takes the window's ``StepDiagnostics`` (a correction aggregator was built): the drivers then
        pass ``step_diagnostics=`` and otherwise call ``record_batch`` as ever."""
        return self._correction is not None

    def _record_step_diagnostics(self, step_diagnostics) -> None:
        """main.py:588-592: the window's corrector deltas at ``i_time_start`` = the steps seen so far, before the other metrics"""
        if self._correction is not None:
            self._correction.fused = self._correction.fused and self.fused
            self._correction.record_batch(step_diagnostics, self._n_seen)
        elif step_diagnostics is not None:
            raise ValueError("record_batch was given step_diagnostics, but this aggregator was built without a correction "
                             "aggregator: configure step_diagnostics=StepDiagnosticsMetricConfig() and a normalizer")

    # ---- routing ------------------------------------------------------------------------------------------------------
    def route(self, data: TensorMapping) -> str:
        """"fused" when ``record_batch`` on this window runs the HIP kernels, "torch" when it runs the torch ops."""
        if not self.fused or not data:
            return "torch"
        first = next(iter(data.values()))
        for t in data.values():
            if not (isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.device == first.device
                    and t.dtype == torch.float32 and t.dim() == 4 and t.shape == first.shape
                    and tuple(t.shape[-2:]) == self._shape):
                return "torch"
        return "fused"

    def launches(self) -> int:
        """Native launches made by ``record_batch`` so far: one ``ace_diag_window`` per window, and per spectrum chunk one
        forward SHT and one ``ace_diag_spectrum`` - with ``fill_masked_spectrum`` three per chunk: one ``ace_diag_fill_planes``
        ahead of them."""
        return self._launches

    def _pick(self, *data: TensorMapping) -> str:
        path = self.route(*data)
        if self._path is None:
            self._path = path
        elif path != self._path:
            raise ValueError(f"this aggregator reduces on the {self._path} path, but a window only the {path} path takes came in "
                             "(device, dtype or shape changed between windows)")
        return path

    # ---- recording ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def record_initial_condition(self, initial_condition: TensorMapping):
        """main.py:962-985: the initial condition (name -> (B, H, W) or (B, 1, H, W)) feeds the time series only.  Returns no
        per-step logs (reading them back would synchronise); ``get_inference_logs`` has them."""
        if self._n_seen != 0:
            raise RuntimeError("record_initial_condition may only be called once, before recording any batches")
        data = {k: (v if v.dim() == 4 else v.unsqueeze(1)) for k, v in initial_condition.items()}
        if not data:
            raise ValueError("data is empty")
        n = next(iter(data.values())).shape[1]
        if self._log_series:
            self._record(data, i_time_start=0, with_maps=False)
        self._n_seen = n
        return []

    @torch.no_grad()
    def record_batch(self, data: TensorMapping, step_diagnostics=None):
        """main.py:937-960: name -> (B, T, H, W), derived variables included, at time index ``i_time_start`` = the steps seen
        so far; ``step_diagnostics``: the window's ``StepDiagnostics`` for the correction metrics.  Returns no per-step logs (see
        ``record_initial_condition``)."""
        if len(data) == 0:
            raise ValueError("data is empty")
        self._record_step_diagnostics(step_diagnostics)
        data = dict(data)
        n = next(iter(data.values())).shape[1]
        self._record(data, i_time_start=self._n_seen, with_maps=True)
        self._n_seen += n
        return []

    def _record(self, data: Dict[str, torch.Tensor], i_time_start: int, with_maps: bool):
        B, T = next(iter(data.values())).shape[:2]
        if self._log_series and i_time_start + T > self._n_time:
            raise ValueError(f"steps {i_time_start}..{i_time_start + T - 1} are past the aggregator's n_timesteps {self._n_time}")
        if tuple(next(iter(data.values())).shape[-2:]) != self._shape:
            raise ValueError(f"fields of shape {tuple(next(iter(data.values())).shape[-2:])} on an aggregator of {self._shape}")
        for n in data:
            if n not in self._series_names and (self._log_series or with_maps):
                self._series_names.append(n)
        ignore_initial = i_time_start == 0
        if with_maps:
            # time_mean.py:127-146
            if self._tm_samples is None:
                self._tm_samples = B
            self._tm_steps = T - 1 if ignore_initial else self._tm_steps + T
            for n in data:
                if n not in self._tm_names:
                    self._tm_names.append(n)
                    self._omitted(n)
        if self._pick(data) == "fused":
            self._record_fused(data, i_time_start, with_maps, ignore_initial)
        else:
            self._record_torch(data, i_time_start, with_maps, ignore_initial)
        if self._log_series:
            for i in range(i_time_start, i_time_start + T):
                self._n_batches[i] += 1
        if with_maps:
            for n in data:
                if not self._omitted(n):
                    self._spec_counts[n] = self._spec_counts.get(n, 0) + B * T
                    if n not in self._spec_names:
                        self._spec_names.append(n)

    def _get_sht(self):
        if self._sht is None:
            self._sht = self._sht_factory(*self._shape)
        return self._sht

    # ---- the torch path: the reference's formulas -------------------------------------------------------------------------
    def _record_torch(self, data, i_time_start, with_maps, ignore_initial):
        T = next(iter(data.values())).shape[1]
        sl = slice(i_time_start, i_time_start + T)
        if self._log_series:
            for n, x in data.items():
                w = self.weights_for(n, x.device).expand(x.shape)
                x0 = x.where(w != 0.0, 0.0)
                wsum = w.sum(dim=(-2, -1))
                mean = (x0 * w).sum(dim=(-2, -1)) / wsum                                   # metrics.py:63-90
                var = (((x - mean[..., None, None]) ** 2).where(w != 0.0, 0.0) * w).sum(dim=(-2, -1)) / wsum
                for metric, v in (("weighted_mean_gen", mean), ("weighted_std_gen", var.sqrt())):
                    tot = self._t_total[metric]
                    if n not in tot:
                        tot[n] = torch.zeros(self._n_time, dtype=v.dtype, device=x.device)
                    tot[n][sl] += v.mean(dim=0)
        if not with_maps:
            return
        part = slice(1, None) if ignore_initial else slice(0, None)
        sums = {n: x[:, part].sum(dim=1).sum(dim=0) for n, x in data.items()}
        if self._t_tm is None:
            self._t_tm = sums
        else:
            for n, s in sums.items():
                self._t_tm[n] = self._t_tm[n] + s
        for n, x in data.items():
            if self._omitted(n):
                continue
            ps = torch.sum(abs(self._get_sht()(self._fill_torch(n, x))) ** 2, dim=-1)    # metrics.py:388-408
            mean_ps = torch.mean(ps, dim=(0, 1))
            new = x.shape[0] * x.shape[1]
            old = self._spec_counts.get(n, 0)
            self._t_spec[n] = mean_ps if n not in self._t_spec else (new * mean_ps + old * self._t_spec[n]) / (new + old)

    # ---- the fused path ---------------------------------------------------------------------------------------------------
    def _ensure_rows(self, names: Sequence[str], dev):
        HW = self._shape[0] * self._shape[1]
        if _grow_rows(self, names, dev, _series=lambda R: (2, R, self._n_time), _tsum=lambda R: (R, HW),
                      _spec=lambda R: (R, self._get_sht().lmax)):
            self._tables.clear()

    def _weight_rows(self, names, dev) -> torch.Tensor:
        key = ("w", tuple(names))
        t = self._tables.get(key)
        if t is None:
            rows = []
            for n in names:
                k = self._mask_key(n) or ""
                if k not in self._wtab:
                    self._wtab[k] = len(self._wtab)
                    w = self.weights_for(n, dev).reshape(1, -1)
                    self._wplanes = w.clone() if self._wplanes is None else torch.cat([self._wplanes, w])
                rows.append(self._wtab[k])
            t = self._tables[key] = _upload(rows, torch.int32, dev)
        return t

    def _row_table(self, names, dev) -> torch.Tensor:
        key = ("r", tuple(names))
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = _upload([self._rows[n] for n in names], torch.int32, dev)
        return t

    def _record_fused(self, data, i_time_start, with_maps, ignore_initial):
        from . import _lib
        first = next(iter(data.values()))
        dev = first.device
        B, T, H, W = first.shape
        HW = H * W
        data = {n: _flat(x, W) for n, x in data.items()}
        names = list(data)
        self._ensure_rows(names, dev)
        wrows = self._weight_rows(names, dev)
        rows = self._row_table(names, dev)
        at, _ = _upload_planes(names, data, None, dev)
        n = len(names)
        lib = _lib.lib()
        partial = torch.empty(int(lib.ace_diag_partial_doubles(n, B, T, HW)), dtype=torch.float64, device=dev)
        # without the time series the window's series go to scratch (the kernel computes them with the same loads)
        series, n_time, t0 = self._series, self._n_time, i_time_start
        if not self._log_series:
            series, n_time, t0 = torch.empty(2, len(self._rows), T, dtype=torch.float64, device=dev), T, 0
        with torch.cuda.device(dev):
            stream = _lib.current_stream()
            _check(lib.ace_diag_window(at["gen"], at["gen_strides"], rows.data_ptr(), wrows.data_ptr(), self._wplanes.data_ptr(),
                                       self._wplanes.shape[0], partial.data_ptr(), self._tsum.data_ptr(), series.data_ptr(),
                                       len(self._rows), n_time, t0, 1 if ignore_initial else 0, 1 if with_maps else 0, n, B, T,
                                       HW, stream))
            self._launches += 1
            if not with_maps:
                return
            spec_names = [nm for nm in names if not self._omitted(nm)]
            if not spec_names:
                return
            sht = self._get_sht()
            L, M = sht.lmax, sht.mmax
            per_name = B * T * (HW * 4 + L * M * 8)
            k = max(1, self.spectrum_chunk_bytes // per_name)
            for c0 in range(0, len(spec_names), k):
                chunk = spec_names[c0:c0 + k]
                planes, made = self._spectrum_input(chunk, [data[nm] for nm in chunk], dev)      # (k, B, T, H, W), one launch
                coeffs = sht(planes)                                          # (k, B, T, L, M) complex64
                crow = self._row_table(chunk, dev)
                _check(lib.ace_diag_spectrum(coeffs.data_ptr(), crow.data_ptr(), self._spec.data_ptr(), self._spec.shape[0],
                                             len(chunk), B * T, L, M, _lib.current_stream()))
                self._launches += 2 + made

    # ---- results --------------------------------------------------------------------------------------------------------
    def _reduce_mean(self, t: torch.Tensor) -> torch.Tensor:
        from .distributed import Distributed
        return Distributed.get_instance().reduce_mean(t)

    def _series_data(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """reduced.py:34-55, 390-430: metric -> name -> (n_timesteps,) series (sorted names), total / per-index count."""
        if not self._log_series:
            return {}
        if not any(self._n_batches):
            raise ValueError("No batches have been recorded.")
        out: Dict[str, Dict[str, torch.Tensor]] = {"weighted_mean_gen": {}, "weighted_std_gen": {}}
        if self._path == "fused":
            counts = torch.tensor(self._n_batches, dtype=torch.float64, device=self._series.device)
            for i, metric in enumerate(out):
                for n in sorted(self._series_names):
                    out[metric][n] = self._reduce_mean((self._series[i, self._rows[n]] / counts).float())
        else:
            for metric, tot in self._t_total.items():
                for n in sorted(tot):
                    counts = torch.tensor(self._n_batches, dtype=torch.int32, device=tot[n].device)
                    out[metric][n] = self._reduce_mean(tot[n] / counts)
        return out

    def _time_mean_data(self) -> Dict[str, torch.Tensor]:
        """time_mean.py:148-163: sum / n_timesteps / n_samples."""
        if self._tm_steps == 0 or not self._tm_names:
            raise ValueError("No data recorded.")
        out = {}
        for n in sorted(self._tm_names):
            if self._path == "fused":
                m = (self._tsum[self._rows[n]] / self._tm_steps / self._tm_samples).float().reshape(self._shape)
            else:
                m = self._t_tm[n] / self._tm_steps / self._tm_samples
            out[n] = self._reduce_mean(m)
        return out

    def _spectrum_data(self) -> Dict[str, torch.Tensor]:
        """spectrum.py:61-70: the mean power spectrum over samples and steps (sorted names)."""
        out = {}
        for n in sorted(self._spec_names):
            if self._path == "fused":
                s = (self._spec[self._rows[n]] / self._spec_counts[n]).float()
            else:
                s = self._t_spec[n].clone()
            out[n] = self._reduce_mean(s)
        return out

    @torch.no_grad()
    def get_dataset(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """main.py get_reduced_diagnostics with the reference's variable keys: {"mean": {"weighted_mean_gen-<name>": (T,)},
        "time_mean": {"gen_map-<name>": (H, W)}, "power_spectrum": {"<name>": (lmax,)}} (CPU tensors)."""
        ds: Dict[str, Dict[str, torch.Tensor]] = {}
        if self._log_series:
            ds["mean"] = {f"{metric}-{n}": v.cpu() for metric, d in self._series_data().items() for n, v in d.items()}
        ds["time_mean"] = {f"gen_map-{n}": v.cpu() for n, v in self._time_mean_data().items()}
        ds["power_spectrum"] = {n: v.cpu() for n, v in self._spectrum_data().items()}
        if self._correction is not None:
            ds.update(self._correction.datasets())
        return ds

    @torch.no_grad()
    def get_summary_logs(self) -> Dict[str, Any]:
        """main.py:987-995: the summary sub-aggregators' logs: ``time_mean/gen_map/<name>`` (H, W) and
        ``power_spectrum/<name>`` (lmax,) tensors in place of the reference's images and figures."""
        logs: Dict[str, Any] = {}
        for n, v in self._time_mean_data().items():
            logs[f"time_mean/gen_map/{n}"] = v.cpu()
        for n, v in self._spectrum_data().items():
            logs[f"power_spectrum/{n}"] = v.cpu()
        if self._correction is not None:
            logs.update(self._correction.summary_logs())
        return logs

    @torch.no_grad()
    def get_inference_logs(self) -> List[Dict[str, Any]]:
        """main.py:1015-1023 / to_inference_logs: one dict per time index with ``mean/forecast_step`` and
        ``mean/<metric>/<name>`` floats; the summary logs go in the last dict."""
        rows: List[Dict[str, Any]] = []
        if self._log_series:
            series = {f"{metric}/{n}": v.cpu().tolist() for metric, d in self._series_data().items() for n, v in d.items()}
            keys = sorted(series)
            for i in range(self._n_time):
                row: Dict[str, Any] = {"mean/forecast_step": i}
                for k in keys:
                    row[f"mean/{k}"] = series[k][i]
                rows.append(row)
            if self._correction is not None:
                for row, extra in zip(rows, self._correction.series_rows()):
                    row.update(extra)
        if not rows:
            rows.append({})
        rows[-1].update(self.get_summary_logs())
        return rows

    @torch.no_grad()
    def flush_diagnostics(self, subdir: Optional[str] = None):
        """diagnostics.py:39-60: one ``<sub-aggregator>_diagnostics.pt`` per non-empty sub-aggregator (root rank only)."""
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


def _upload(values: List[int], dtype, dev) -> torch.Tensor:
    """A small host table to ``dev`` from pinned memory without synchronising the host."""
    host = torch.tensor(values, dtype=dtype).pin_memory()
    return host.to(dev, non_blocking=True)


def _flat(x: torch.Tensor, W: int) -> torch.Tensor:
    """The planes of a field must be contiguous for the pointer table; anything else is made so."""
    return x if x.stride(-1) == 1 and x.stride(-2) == W else x.contiguous()


def _grow(buf: Optional[torch.Tensor], shape, dtype, dev) -> torch.Tensor:
    """A zeroed accumulator of ``shape`` with the old one (``None``: none yet) in its leading corner."""
    fresh = torch.zeros(shape, dtype=dtype, device=dev)
    if buf is not None:
        fresh[tuple(slice(0, s) for s in buf.shape)] = buf
    return fresh


def _grow_rows(owner, names: Sequence[str], dev, **buffers) -> bool:
    """Give every new name of ``names`` the next row of ``owner._rows`` and, when there was one or a buffer is still ``None``, grow
    the fp64 accumulators ``owner.<attribute>`` to ``shape(number of rows)``; True when it grew them."""
    new = [n for n in names if n not in owner._rows]
    if not new and all(getattr(owner, a) is not None for a in buffers):
        return False
    for n in new:
        owner._rows[n] = len(owner._rows)
    for a, shape in buffers.items():
        setattr(owner, a, _grow(getattr(owner, a), shape(max(1, len(owner._rows))), torch.float64, dev))
    return True


def _plane_table(names: Sequence[str], gen: TensorMapping, target: Optional[TensorMapping] = None):
    """The int64 table through which the diag kernels read a window's (B, T, H, W) fields in place, and the byte offsets of its
    sections.  Per side (``gen``, then ``target`` when given) one pointer per name, then one (stride(0), stride(1)) pair per name; a
    name ``target`` lacks has pointer 0 and strides 0, 0.  Offsets: ``gen``, ``gen_strides``, with a target ``target`` and
    ``target_strides``, and ``end``, where a caller appends sections of its own.  Uploading is ``_upload_planes``."""
    values: List[int] = []
    off: Dict[str, int] = {}
    for side, d in (("gen", gen),) if target is None else (("gen", gen), ("target", target)):
        fields = [d[n] if side == "gen" else d.get(n) for n in names]
        off[side] = 8 * len(values)
        values += [0 if x is None else x.data_ptr() for x in fields]
        off[side + "_strides"] = 8 * len(values)
        for x in fields:
            values += (0, 0) if x is None else x.stride()[:2]
    off["end"] = 8 * len(values)
    return values, off


def _upload_planes(names: Sequence[str], gen: TensorMapping, target: Optional[TensorMapping], dev, sections=()):
    """A window's plane table and the caller's trailing ``sections`` (numpy arrays) to ``dev`` as one pinned blob, without
    synchronising the host: (the device address of every offset of ``_plane_table``, the device address of every section)."""
    import numpy as np
    values, off = _plane_table(names, gen, target)
    parts = [np.asarray(values, np.int64), *sections]
    table = torch.from_numpy(np.concatenate([p.reshape(-1).view(np.uint8) for p in parts])).pin_memory().to(dev, non_blocking=True)
    at = {k: table.data_ptr() + o for k, o in off.items()}
    at["table"] = table                                                   # the caller keeps the blob alive through its call
    return at, list(itertools.accumulate([p.nbytes for p in sections[:-1]], initial=at["end"])) if sections else []


_check = functools.partial(check, family="diag")
