"""The inference data writers that reduce in time (fme/ace/inference/data_writer/: main.py, time_coarsen.py, monthly.py, utils.py):
``TimeCoarsen`` hands block means of ``coarsen_factor`` steps to the writer it wraps, ``MonthlyDataWriter`` keeps per-sample monthly
means, ``DataWriterConfig`` builds the fan-out of both that a reference inference run writes by default.  On plain
``name -> (B, T, H, W)`` tensor dicts and a ``TimeAxis``, as the rest of ace_amd/inference.py; netCDF / xarray are not on the path, so
files are ``torch.save`` archives with the reference's stems (``monthly_mean_predictions.pt`` for its ``.nc``).

Both writers are one operation: per-pixel sums over runs of consecutive steps of a window.  ``segment_sums`` is that primitive, with
two paths that compute the same thing, the split of ace_amd/aggregator.py:

  * fused (``SegmentReducer.fused``, CUDA fp32 fields with contiguous rows): one ``ace_diag_time_segments`` (csrc/timeseg.hip) reads
    every ``data[name]`` in place through a pointer table and writes the reduced record to a staging buffer, which one copy takes to
    pinned host memory.  The device-to-host traffic and the host footprint shrink by the length of the segments: 4 for 6-hourly
    steps coarsened to days, about 20 per 40-step window for monthly means.
  * torch (anything else): per segment a sequential fp64 sum over its steps, in the same step order.

The stated numerical difference: the reference means in fp32 - torch's fp32 ``mean`` for the blocks, and for the months the running
update ``(old_mean * old_count + new_sum) / (old_count + n)`` once per window on fp32 arrays.  Here every sum is fp64, in step order,
and is rounded to fp32 once, the stance of csrc/coupler.hip.  With u = 2^-24 and m = max |x| over the steps that enter one output
pixel: |ours - reference| <= (f + 2) u m for a block of f steps, |ours - reference| <= (N + 3 k + 1) u m for a month of N steps
delivered in k windows, and |ours - the exact mean| <= u |mean|.  The monthly totals are fp64 sums of the windows' fp64 segment sums:
how a record is cut into windows changes them only where a fp64 add of fp32 data rounds (a spread of more than 2^29 / N within one
pixel's month), and never by more than one fp64 rounding per window.

Not built: netCDF / zarr output and ``FileWriterConfig`` (``files``), the step-diagnostics writer (``save_step_diagnostics``), the
histogram and video writers, and the coupled loop's writer."""
import dataclasses
import os
import warnings
from typing import Any, Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from .inference import TensorFileWriter
from .timeaxis import TimeAxis, days_since_base

TensorMapping = Mapping[str, torch.Tensor]
TIME_DIM = 1            # sample, time, lat, lon


# ---- configs ----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class TimeCoarsenConfig:
    """time_coarsen.py:42-90.  ``coarsen_factor``: an integer 1 or greater; the time labels are coarsened to the mean of the
    original labels.  ``method``: only "block_mean"."""
    coarsen_factor: int
    method: str = "block_mean"

    def __post_init__(self):
        if self.coarsen_factor < 1:
            raise ValueError(f"coarsen_factor must be 1 or greater, got {self.coarsen_factor}")
        if self.method != "block_mean":
            raise ValueError(f"method must be 'block_mean', got {self.method!r}")

    def build(self, data_writer) -> "TimeCoarsen":
        return TimeCoarsen(data_writer, coarsen_factor=self.coarsen_factor)

    def build_paired(self, data_writer) -> "PairedTimeCoarsen":
        return PairedTimeCoarsen(data_writer, coarsen_factor=self.coarsen_factor)

    def n_coarsened_timesteps(self, n_timesteps: int) -> int:
        """Assumes the initial condition is NOT in n_timesteps."""
        return n_timesteps // self.coarsen_factor

    def validate(self, forward_steps_in_memory: int, n_forward_steps: int):
        if forward_steps_in_memory % self.coarsen_factor != 0:
            raise ValueError("forward_steps_in_memory must be divisible by time_coarsen.coarsen_factor. "
                             f"Got {forward_steps_in_memory} and {self.coarsen_factor}.")
        if n_forward_steps % self.coarsen_factor != 0:
            raise ValueError("n_forward_steps must be divisible by time_coarsen.coarsen_factor. "
                             f"Got {n_forward_steps} and {self.coarsen_factor}.")


@dataclasses.dataclass
class MonthlyCoarsenConfig:
    """time_coarsen.py:93-107: monthly coarsening works with any combination of steps."""
    method: str = "monthly_mean"

    def __post_init__(self):
        if self.method != "monthly_mean":
            raise ValueError(f"method must be 'monthly_mean', got {self.method!r}")

    def validate(self, forward_steps_in_memory: int, n_forward_steps: int):
        pass


def get_all_names(*data_varnames: Iterable[str], allowlist: Optional[Iterable[str]] = None) -> set:
    """utils.py:9-27: the union of the names, cut to ``allowlist`` when there is one; a warning for requested names that are absent."""
    variables: set = set()
    for varnames in data_varnames:
        variables = variables.union(set(varnames))
    if allowlist is None:
        return variables
    allowlist = set(allowlist)
    missing = allowlist - variables
    if missing:
        warnings.warn(f"Requested variable(s) not present in data: {list(missing)}")
    return variables.intersection(allowlist)


# ---- the shared primitive ---------------------------------------------------------------------------------------------------
class SegmentReducer:
    """Per-pixel sums and means over runs of consecutive steps of a window: the statement of ``ace_diag_time_segments``
    (include/ace_sfno.h), on either path.  Keeps the fused path's tables and staging buffers between windows."""

    def __init__(self):
        self.fused = True                 # CUDA fp32 windows take the HIP path; False: the torch ops on any device
        self.last_path: Optional[str] = None
        self.launches = 0                 # native launches so far
        self.bytes_to_host = 0            # bytes the results took from the device to the host so far
        self._table_key: Optional[bytes] = None
        self._table: Optional[torch.Tensor] = None
        self._dev: Dict[str, torch.Tensor] = {}
        self._host: Dict[str, torch.Tensor] = {}

    def route(self, fields: Sequence[torch.Tensor]) -> str:
        """"fused" when these fields are reduced by the HIP kernel, "torch" when by the torch ops."""
        if not self.fused or not fields:
            return "torch"
        first = fields[0]
        for t in fields:
            if not (isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.device == first.device
                    and t.dtype == torch.float32 and t.dim() == 4 and t.shape == first.shape):
                return "torch"
        if len(fields) > 65535 or first.shape[0] > 65535 or first.shape[1] < 1 or first.shape[2] * first.shape[3] < 1:
            return "torch"
        return "fused"

    def _pick(self, fields: Sequence[torch.Tensor]) -> str:
        # the results live on the host and the two paths agree bit for bit, so a writer may change path between windows
        self.last_path = self.route(fields)
        return self.last_path

    def __call__(self, data: TensorMapping, names: Sequence[str], edges, want: Sequence[str] = ("sums", "means")
                 ) -> Dict[str, Optional[torch.Tensor]]:
        """``edges``: int (B, nseg + 1); segment s of sample b is the steps [edges[b, s], edges[b, s + 1]), every edge clamped to
        [0, T].  Returns {"sums": fp64 (len(names), B, nseg, H, W) or None, "means": fp32, the same shape, or None}, CPU tensors;
        on the fused path they are views of the pinned staging buffers, valid until the next call: copy what is to be kept."""
        want = tuple(want)
        if not want or any(w not in ("sums", "means") for w in want):
            raise ValueError(f"want must name 'sums' and / or 'means', got {want}")
        names = list(names)
        fields = [data[n] for n in names]
        for x in fields:
            if x.dim() != 4 or x.shape != fields[0].shape:
                raise ValueError(f"fields must share one (B, T, H, W) shape, got {[tuple(f.shape) for f in fields]}")
        edges = np.ascontiguousarray(np.asarray(edges), dtype=np.int64)
        if names and (edges.ndim != 2 or edges.shape[0] != fields[0].shape[0] or edges.shape[1] < 1):
            raise ValueError(f"edges must be (B, nseg + 1) with B = {fields[0].shape[0]}, got {edges.shape}")
        if not names or edges.shape[1] == 1:
            B, H, W = (fields[0].shape[0], *fields[0].shape[2:]) if names else (0, 0, 0)
            shape = (len(names), B, 0, H, W)
            return {"sums": torch.zeros(shape, dtype=torch.float64) if "sums" in want else None,
                    "means": torch.zeros(shape, dtype=torch.float32) if "means" in want else None}
        if self._pick(fields) == "fused":
            return self._fused(fields, edges, want)
        return self._torch(fields, edges, want)

    # ---- the torch path -----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _torch(self, fields, edges, want):
        B, T, H, W = fields[0].shape
        nseg = edges.shape[1] - 1
        e = np.clip(edges, 0, T)
        sums = torch.zeros((len(fields), B, nseg, H, W), dtype=torch.float64, device=fields[0].device)
        for i, x in enumerate(fields):
            for b in range(B):
                for s in range(nseg):
                    acc = sums[i, b, s]
                    for t in range(int(e[b, s]), int(e[b, s + 1])):      # one fp64 add per step, in step order
                        acc.add_(x[b, t])
        out: Dict[str, Optional[torch.Tensor]] = {"sums": None, "means": None}
        if "means" in want:
            n = torch.from_numpy(np.maximum(e[:, 1:] - e[:, :-1], 0).astype(np.float64)).to(sums.device)
            out["means"] = (sums / n[None, :, :, None, None]).to(torch.float32).cpu()          # 0.0 / 0.0: NaN
        if "sums" in want:
            out["sums"] = sums.cpu()
        if sums.device.type != "cpu":
            self.bytes_to_host += sum(v.numel() * v.element_size() for v in out.values() if v is not None)
        return out

    # ---- the fused path -----------------------------------------------------------------------------------------------------
    def _staging(self, kind: str, dtype, numel: int, dev) -> Tuple[torch.Tensor, torch.Tensor]:
        d = self._dev.get(kind)
        if d is None or d.numel() < numel or d.device != dev:
            self._dev[kind] = torch.empty(numel, dtype=dtype, device=dev)
            self._host[kind] = torch.empty(numel, dtype=dtype).pin_memory()
        return self._dev[kind], self._host[kind]

    @torch.no_grad()
    def _fused(self, fields, edges, want):
        from . import _lib
        from .aggregator import _check, _flat, _plane_table
        dev = fields[0].device
        B, T, H, W = fields[0].shape
        HW, N, nseg = H * W, len(fields), edges.shape[1] - 1
        fields = [_flat(x, W) for x in fields]
        names = [str(i) for i in range(N)]
        values, off = _plane_table(names, dict(zip(names, fields)))
        parts = [np.asarray(values, np.int64), np.arange(N, dtype=np.int32), np.clip(edges, -2**31, 2**31 - 1).astype(np.int32)]
        blob = np.concatenate([p.reshape(-1).view(np.uint8) for p in parts])
        key = blob.tobytes()
        if key != self._table_key or self._table is None or self._table.device != dev:      # built once per window shape
            self._table = torch.from_numpy(blob).pin_memory().to(dev, non_blocking=True)
            self._table_key = key
        base = self._table.data_ptr()
        rows_at = base + off["end"]
        edges_at = rows_at + parts[1].nbytes
        numel = N * B * nseg * HW
        sums = self._staging("sums", torch.float64, numel, dev) if "sums" in want else None
        means = self._staging("means", torch.float32, numel, dev) if "means" in want else None
        lib = _lib.lib()
        with torch.cuda.device(dev):
            _check(lib.ace_diag_time_segments(base + off["gen"], base + off["gen_strides"], rows_at, edges_at,
                                              sums[0].data_ptr() if sums else None, means[0].data_ptr() if means else None,
                                              N, nseg, N, B, T, HW, _lib.current_stream()))
            self.launches += 1
            out: Dict[str, Optional[torch.Tensor]] = {"sums": None, "means": None}
            for kind, pair in (("sums", sums), ("means", means)):
                if pair is not None:
                    d, h = pair
                    h[:numel].copy_(d[:numel], non_blocking=True)
                    self.bytes_to_host += numel * d.element_size()
                    out[kind] = h[:numel].view(N, B, nseg, H, W)
            torch.cuda.current_stream().synchronize()            # the host reads the record next
        return out


_DEFAULT_REDUCER = SegmentReducer()


def segment_sums(data: TensorMapping, names: Sequence[str], edges, want: Sequence[str] = ("sums", "means"),
                 reducer: Optional[SegmentReducer] = None) -> Dict[str, Optional[torch.Tensor]]:
    """``SegmentReducer.__call__`` on ``reducer`` (default: a module-wide one)."""
    return (reducer or _DEFAULT_REDUCER)(data, names, edges, want)


# ---- time coarsening --------------------------------------------------------------------------------------------------------
def coarsen_time(time: Optional[TimeAxis], factor: int) -> Optional[TimeAxis]:
    """``batch_time.coarsen(time=factor).mean()`` (time_coarsen.py:183) on integer microseconds: per block the floor of the mean."""
    if time is None:
        return None
    us = time.us
    if us.ndim != 2 or us.shape[1] % factor != 0:
        raise ValueError(f"time must be (samples, a multiple of {factor} steps), got {us.shape}")
    blocks = us.reshape(us.shape[0], us.shape[1] // factor, factor)
    first = blocks[:, :, :1]
    return TimeAxis(time.calendar, first[:, :, 0] + (blocks - first).sum(axis=-1) // factor)


def _coarsen(reducer: SegmentReducer, data: TensorMapping, factor: int) -> Dict[str, torch.Tensor]:
    names = list(data)
    if not names:
        return {}
    B, T = data[names[0]].shape[:2]
    if T % factor != 0:
        raise ValueError(f"a window of {T} steps is not a multiple of coarsen_factor {factor} "
                         "(TimeCoarsenConfig.validate checks the schedule up front)")
    edges = np.broadcast_to(np.arange(0, T + 1, factor, dtype=np.int64), (B, T // factor + 1))
    means = reducer(data, names, edges, want=("means",))["means"]
    return {n: means[i].clone() for i, n in enumerate(names)}            # the inner writer owns what it is handed


def _hand_down(writer, time: Optional[TimeAxis], **batches):
    if time is not None and (getattr(writer, "uses_time", False) or getattr(writer, "needs_time", False)):
        writer.append_batch(time=time, **batches)
    else:
        writer.append_batch(**batches)


class _Wrapper:
    uses_time = True                      # takes the window's TimeAxis when there is one

    def __init__(self, data_writer, coarsen_factor: int):
        if coarsen_factor < 1:
            raise ValueError(f"coarsen_factor must be 1 or greater, got {coarsen_factor}")
        self._data_writer = data_writer
        self._coarsen_factor = int(coarsen_factor)
        self.reducer = SegmentReducer()

    @property
    def needs_time(self) -> bool:
        return bool(getattr(self._data_writer, "needs_time", False))

    def write(self, data: TensorMapping, filename: str):
        self._data_writer.write(data, filename)

    def flush(self):
        if hasattr(self._data_writer, "flush"):
            self._data_writer.flush()

    def finalize(self):
        if hasattr(self._data_writer, "finalize"):
            self._data_writer.finalize()
        else:
            self.flush()


class TimeCoarsen(_Wrapper):
    """time_coarsen.py:146-174: wraps any writer with ``append_batch`` and hands it the block means of ``coarsen_factor`` steps,
    (B, T / f, H, W) fp32 CPU tensors it may keep, and the coarsened ``TimeAxis`` when the writer takes one."""

    def append_batch(self, batch: TensorMapping, time: Optional[TimeAxis] = None):
        coarse = _coarsen(self.reducer, batch, self._coarsen_factor)
        _hand_down(self._data_writer, coarsen_time(time, self._coarsen_factor), batch=coarse)


class PairedTimeCoarsen(_Wrapper):
    """time_coarsen.py:110-143: the same for a writer of (prediction, target) pairs."""
    paired = True

    def append_batch(self, batch: TensorMapping, target: TensorMapping, time: Optional[TimeAxis] = None):
        tgt = _coarsen(self.reducer, target, self._coarsen_factor)
        gen = _coarsen(self.reducer, batch, self._coarsen_factor)
        _hand_down(self._data_writer, coarsen_time(time, self._coarsen_factor), batch=gen, target=tgt)


# ---- monthly means ----------------------------------------------------------------------------------------------------------
class MonthlyDataWriter:
    """monthly.py:89-336: per-sample monthly means of every saved name, months counted from each sample's first appended step.
    Keeps fp64 totals (B, months, H, W) per name and int64 counts (B, months) on the host; ``flush`` writes
    ``<directory>/<label>.pt``: every name as fp32 (B, months, H, W) = (float)(total / count) (0.0 where the count is 0, as the
    reference leaves such a month), ``counts``, ``time`` = arange(months), ``valid_time`` int64 (B, months), days since 1970-01-01
    of the 15th of each month in the axis' calendar, and ``calendar``."""
    uses_time = True
    needs_time = True

    def __init__(self, directory: str, label: str, names: Optional[Sequence[str]] = None):
        self._dir = directory
        self._label = label
        self._save_names = None if names is None else list(names)
        self._init_years: Optional[np.ndarray] = None
        self._init_months: Optional[np.ndarray] = None
        self._calendar: Optional[str] = None
        self._totals: Dict[str, torch.Tensor] = {}
        self._counts: Optional[np.ndarray] = None
        self.reducer = SegmentReducer()
        os.makedirs(directory, exist_ok=True)

    @property
    def path(self) -> str:
        return os.path.join(self._dir, self._label + ".pt")

    def _month_indices(self, time: TimeAxis) -> np.ndarray:
        """monthly.py:169-190"""
        years, months = time.year_month()
        months = months - 1
        if self._init_years is None:
            self._init_years, self._init_months, self._calendar = years[:, 0].copy(), months[:, 0].copy(), time.calendar
        elif time.calendar != self._calendar:
            raise ValueError(f"the calendar changed between windows: {self._calendar} then {time.calendar}")
        return 12 * (years - self._init_years[:, None]) + (months - self._init_months[:, None])

    def write(self, data: TensorMapping, filename: str):
        pass

    def append_batch(self, batch: TensorMapping, time: Optional[TimeAxis] = None):
        if time is None:
            raise ValueError("the monthly writer needs the windows' time axis: build the ForcingWindows with time=")
        if not batch:
            raise ValueError("data is empty")
        first = next(iter(batch.values()))
        B, T, H, W = first.shape
        if time.ndim != 2:
            raise ValueError(f"time must be (samples, steps), got {tuple(time.shape)}")
        if B != time.shape[0]:
            raise ValueError(f"Batch size mismatch, data has {B} samples and batch_time has {time.shape[0]} samples.")
        if T != time.shape[1]:
            raise ValueError(f"Batch time dimension mismatch, data has {T} times and batch_time has {time.shape[1]} times.")
        if self._counts is not None and self._counts.shape[0] != B:
            raise ValueError(f"Batch size mismatch, data has {B} samples and the record has {self._counts.shape[0]} samples.")
        names = sorted(get_all_names(batch.keys(), allowlist=self._save_names))
        months = self._month_indices(time)
        if np.any(months[:, 1:] < months[:, :-1]) or months.min() < 0:
            raise ValueError("the times of a sample must not go back to an earlier month")
        month_min, new_size = int(months.min()), int(months.max()) + 1
        nseg = new_size - month_min
        # edges[b][s]: the first step of sample b in month month_min + s or later
        edges = np.stack([np.searchsorted(months[b], month_min + np.arange(nseg + 1), side="left") for b in range(B)])
        old_size = 0 if self._counts is None else self._counts.shape[1]
        if new_size > old_size:
            grown = np.zeros((B, new_size), np.int64)
            if self._counts is not None:
                grown[:, :old_size] = self._counts
            self._counts = grown
        if names:
            sums = self.reducer(batch, names, edges, want=("sums",))["sums"]
            for i, n in enumerate(names):
                tot = self._totals.get(n)
                if tot is None or tot.shape[1] < new_size:
                    fresh = torch.zeros((B, new_size, H, W), dtype=torch.float64)
                    if tot is not None:
                        fresh[:, :tot.shape[1]] = tot
                    tot = self._totals[n] = fresh
                tot[:, month_min:new_size] += sums[i]
        self._counts[:, month_min:new_size] += np.diff(edges, axis=1)

    def _valid_time(self, n_months: int) -> np.ndarray:
        """monthly.py:201-216, 393-432"""
        k = self._init_months[:, None] + np.arange(n_months)[None, :]
        first = days_since_base(self._calendar, self._init_years[:, None] + k // 12, k % 12 + 1, 1)
        return first - days_since_base(self._calendar, 1970, 1, 1) + 14          # the 15th is 14 days into the month

    def get_dataset(self) -> Dict[str, Any]:
        if self._counts is None:
            return {}
        counts = torch.from_numpy(self._counts.copy())
        n_months = counts.shape[1]
        out: Dict[str, Any] = {}
        for n, tot in self._totals.items():
            full = tot
            if tot.shape[1] < n_months:                                   # a name that stopped coming in
                full = torch.zeros((tot.shape[0], n_months, *tot.shape[2:]), dtype=torch.float64)
                full[:, :tot.shape[1]] = tot
            c = counts[:, :, None, None].to(torch.float64)
            out[n] = torch.where(c > 0, full / c, torch.zeros((), dtype=torch.float64)).to(torch.float32)
        out["counts"] = counts
        out["time"] = torch.arange(n_months)
        out["valid_time"] = torch.from_numpy(self._valid_time(n_months).astype(np.int64))
        out["calendar"] = self._calendar
        return out

    def flush(self):
        ds = self.get_dataset()
        if not ds:
            return
        tmp = self.path + ".tmp"
        torch.save(ds, tmp)
        os.replace(tmp, self.path)

    def finalize(self):
        self.flush()


class PairedMonthlyDataWriter:
    """monthly.py:33-86: ``monthly_mean_target`` and ``monthly_mean_predictions`` side by side."""
    uses_time = True
    needs_time = True
    paired = True

    def __init__(self, directory: str, names: Optional[Sequence[str]] = None):
        self._target_writer = MonthlyDataWriter(directory, "monthly_mean_target", names)
        self._prediction_writer = MonthlyDataWriter(directory, "monthly_mean_predictions", names)

    def write(self, data: TensorMapping, filename: str):
        pass

    def append_batch(self, batch: TensorMapping, target: TensorMapping, time: Optional[TimeAxis] = None):
        if target:
            self._target_writer.append_batch(target, time=time)
        self._prediction_writer.append_batch(batch, time=time)

    def flush(self):
        self._target_writer.flush()
        self._prediction_writer.flush()

    def finalize(self):
        self._target_writer.finalize()
        self._prediction_writer.finalize()


# ---- the fan-out ------------------------------------------------------------------------------------------------------------
class PairedTensorFileWriter:
    """The paired raw writer (raw.py: PairedRawDataWriter): ``autoregressive_predictions.pt`` and ``autoregressive_target.pt``."""
    paired = True

    def __init__(self, directory: str, names: Optional[Sequence[str]] = None):
        self._names = None if names is None else list(names)
        self._prediction_writer = TensorFileWriter(directory, label="autoregressive_predictions")
        self._target_writer = TensorFileWriter(directory, label="autoregressive_target")

    def write(self, data: TensorMapping, filename: str):
        self._prediction_writer.write(data, filename)

    def append_batch(self, batch: TensorMapping, target: TensorMapping):
        names = get_all_names(batch.keys(), target.keys(), allowlist=self._names)
        self._prediction_writer.append_batch({k: v for k, v in batch.items() if k in names})
        self._target_writer.append_batch({k: v for k, v in target.items() if k in names})

    def flush(self):
        self._prediction_writer.flush()
        self._target_writer.flush()

    def finalize(self):
        self.flush()


class _RawSubset(TensorFileWriter):
    """``TensorFileWriter`` with the ``names`` rule of ``get_all_names``: the intersection, and a warning for absent names."""

    def append_batch(self, batch: TensorMapping):
        names = get_all_names(batch.keys(), allowlist=self._names)
        self._windows.append({k: v.detach().cpu() for k, v in batch.items() if k in names})


@dataclasses.dataclass
class DataWriterConfig:
    """main.py:36-100 (same fields and defaults).  ``save_step_diagnostics=True`` and ``files`` other than ``None`` are refused at
    build time: there are no step-diagnostics records and no netCDF / zarr file writers here."""
    save_prediction_files: bool = True
    save_monthly_files: bool = True
    save_step_diagnostics: bool = False
    names: Optional[Sequence[str]] = None
    time_coarsen: Optional[TimeCoarsenConfig] = None
    files: Optional[List[Any]] = None

    def __post_init__(self):
        if (not any([self.save_prediction_files, self.save_monthly_files, self.save_step_diagnostics])
                and self.names is not None):
            warnings.warn("names provided but all options to save subsettable output files are False.")

    def validate_time_coarsen(self, forward_steps_in_memory: int, n_forward_steps: int):
        if self.time_coarsen is not None:
            self.time_coarsen.validate(forward_steps_in_memory, n_forward_steps)

    def _refuse(self):
        if self.save_step_diagnostics:
            raise NotImplementedError("save_step_diagnostics: no step-diagnostics records are produced here, so there is no "
                                      "step-diagnostics writer")
        if self.files is not None:
            raise NotImplementedError("files: FileWriterConfig (netCDF / zarr files with lat / lon extents and time selections) is "
                                      "not built; only the default prediction and monthly files are written")

    def build(self, directory: str) -> "DataWriter":
        self._refuse()
        writers: List[Any] = []
        if self.save_prediction_files:
            raw: Any = _RawSubset(directory, names=self.names)
            if self.time_coarsen is not None:
                raw = self.time_coarsen.build(raw)
            writers.append(raw)
        if self.save_monthly_files:
            writers.append(MonthlyDataWriter(directory, "monthly_mean_predictions", names=self.names))
        return DataWriter(writers, directory)

    def build_paired(self, directory: str) -> "PairedDataWriter":
        self._refuse()
        writers: List[Any] = []
        if self.save_prediction_files:
            raw: Any = PairedTensorFileWriter(directory, names=self.names)
            if self.time_coarsen is not None:
                raw = self.time_coarsen.build_paired(raw)
            writers.append(raw)
        if self.save_monthly_files:
            writers.append(PairedMonthlyDataWriter(directory, names=self.names))
        return PairedDataWriter(writers, directory)


class DataWriter:
    """main.py:386-471: every batch goes to every sub-writer; ``write`` stores a snapshot (``restart.pt``) whichever are on."""
    uses_time = True

    def __init__(self, writers: Sequence[Any], directory: str):
        self._writers = list(writers)
        self._snapshots = TensorFileWriter(directory)

    @property
    def needs_time(self) -> bool:
        return any(getattr(w, "needs_time", False) for w in self._writers)

    def write(self, data: TensorMapping, filename: str):
        self._snapshots.write(data, filename)

    def append_batch(self, batch: TensorMapping, time: Optional[TimeAxis] = None):
        for w in self._writers:
            _hand_down(w, time, batch=dict(batch))

    def flush(self):
        for w in self._writers:
            w.flush()

    def finalize(self):
        for w in self._writers:
            w.finalize()


class PairedDataWriter(DataWriter):
    """main.py:261-344: the same for (prediction, target) pairs."""
    paired = True

    def append_batch(self, batch: TensorMapping, target: TensorMapping, time: Optional[TimeAxis] = None):
        for w in self._writers:
            _hand_down(w, time, batch=dict(batch), target=dict(target))
