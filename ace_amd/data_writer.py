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

The region- and time-selected files (file_writer.py: ``FileWriterConfig``, the entries of ``DataWriterConfig.files``) are the same
operation on a box: ``FileWriter`` turns the names, the lat / lon extents, the time selection (a ``Slice`` of step indices or a
``MonthSelector``, applied after coarsening as in the reference) and the block mean of a ``TimeCoarsenConfig`` into one ``bounds``
table - one segment of ``coarsen_factor`` source steps per kept output step - and one ``SegmentReducer`` call per window and side:
on CUDA windows one ``ace_diag_region_segments`` (csrc/region.hip), after which only the kept record crosses to the host,
names * B * n_kept * nlat_r * nlon_r * 4 bytes.  With a ``MonthlyCoarsenConfig`` it is a ``MonthlyDataWriter`` on the box.  A segment
of one step is the step itself, except that a -0.0 comes back as +0.0 (0.0 + -0.0).  Three stated differences from the reference:
the files are ``torch.save`` archives ``<label>.pt``; a ``TimeSlice`` selection (xarray's partial-datetime-string indexing of a
``CFTimeIndex``), a zarr ``format`` and ``separate_ensemble_members`` raise ``NotImplementedError``; a box that holds no grid point
raises ``ValueError`` at build time where the reference would write empty arrays.

Not built: netCDF / zarr output, the step-diagnostics writer (``save_step_diagnostics``; the records themselves are, step_diagnostics.py), the histogram and video writers, and the
coupled loop's writer."""
import dataclasses
import logging
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
def _check_region(region, H: int, W: int) -> Tuple[int, int, int, int]:
    lat0, nlat_r, lon0, nlon_r = (int(v) for v in region)
    if not (0 <= lat0 and 1 <= nlat_r and lat0 + nlat_r <= H and 0 <= lon0 and 1 <= nlon_r and lon0 + nlon_r <= W):
        raise ValueError(f"region (lat0, nlat_r, lon0, nlon_r) = {(lat0, nlat_r, lon0, nlon_r)} does not lie in a {H} x {W} plane")
    return lat0, nlat_r, lon0, nlon_r


class SegmentReducer:
    """Per-pixel sums and means over runs of consecutive steps of a window: the statement of ``ace_diag_time_segments``
    (include/ace_sfno.h), on either path.  Keeps the fused path's tables and staging buffers between windows.

    With ``region=(lat0, nlat_r, lon0, nlon_r)``, or when a call gives ``bounds`` in place of ``edges``, the statement is that of
    ``ace_diag_region_segments``: only the rows [lat0, lat0 + nlat_r) and columns [lon0, lon0 + nlon_r) enter, the results are
    compact (names, B, nseg, nlat_r, nlon_r), and segments given as ``bounds`` need not touch.  ``region=None`` with ``bounds``
    is the whole plane.  With ``region=None`` and ``edges`` nothing changes: the path and the results are ``time_segments``'."""

    def __init__(self, region: Optional[Sequence[int]] = None):
        self.region = None if region is None else tuple(int(v) for v in region)
        if self.region is not None and len(self.region) != 4:
            raise ValueError(f"region must be (lat0, nlat_r, lon0, nlon_r), got {region}")
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

    def __call__(self, data: TensorMapping, names: Sequence[str], edges=None, want: Sequence[str] = ("sums", "means"), bounds=None
                 ) -> Dict[str, Optional[torch.Tensor]]:
        """``edges``: int (B, nseg + 1); segment s of sample b is the steps [edges[b, s], edges[b, s + 1]), every edge clamped to
        [0, T].  ``bounds``, in place of ``edges``: int (B, nseg, 2); segment s of sample b is the steps [bounds[b, s, 0],
        bounds[b, s, 1]), both clamped to [0, T]; segments need not touch and may overlap.  Returns {"sums": fp64 (len(names), B,
        nseg, H, W) or None, "means": fp32, the same shape, or None} - H, W those of the region when there is one - CPU tensors; on
        the fused path they are views of the pinned staging buffers, valid until the next call: copy what is to be kept."""
        want = tuple(want)
        if not want or any(w not in ("sums", "means") for w in want):
            raise ValueError(f"want must name 'sums' and / or 'means', got {want}")
        if (edges is None) == (bounds is None):
            raise ValueError("exactly one of edges and bounds must be given")
        names = list(names)
        fields = [data[n] for n in names]
        for x in fields:
            if x.dim() != 4 or x.shape != fields[0].shape:
                raise ValueError(f"fields must share one (B, T, H, W) shape, got {[tuple(f.shape) for f in fields]}")
        if self.region is not None or bounds is not None:
            return self._region_call(fields, edges, bounds, want)
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

    # ---- the region: the statement of ace_diag_region_segments, on either path ------------------------------------------------
    def _region_call(self, fields, edges, bounds, want):
        if bounds is None:                                       # touching segments: the bounds are consecutive edges
            edges = np.asarray(edges, dtype=np.int64)
            if fields and (edges.ndim != 2 or edges.shape[0] != fields[0].shape[0] or edges.shape[1] < 1):
                raise ValueError(f"edges must be (B, nseg + 1) with B = {fields[0].shape[0]}, got {edges.shape}")
            bounds = np.stack([edges[:, :-1], edges[:, 1:]], axis=-1) if edges.ndim == 2 else np.zeros((0, 0, 2), np.int64)
        bounds = np.ascontiguousarray(np.asarray(bounds), dtype=np.int64)
        if fields and (bounds.ndim != 3 or bounds.shape[0] != fields[0].shape[0] or bounds.shape[2] != 2):
            raise ValueError(f"bounds must be (B, nseg, 2) with B = {fields[0].shape[0]}, got {bounds.shape}")
        if not fields or bounds.shape[1] == 0:
            B = fields[0].shape[0] if fields else 0
            h, w = (self.region[1], self.region[3]) if self.region is not None else (fields[0].shape[2:] if fields else (0, 0))
            shape = (len(fields), B, 0, h, w)
            return {"sums": torch.zeros(shape, dtype=torch.float64) if "sums" in want else None,
                    "means": torch.zeros(shape, dtype=torch.float32) if "means" in want else None}
        H, W = fields[0].shape[2:]
        region = _check_region(self.region if self.region is not None else (0, H, 0, W), H, W)
        if self._pick(fields) == "fused":
            return self._fused_region(fields, bounds, region, want)
        return self._torch_region(fields, bounds, region, want)

    @torch.no_grad()
    def _torch_region(self, fields, bounds, region, want):
        B, T = fields[0].shape[:2]
        lat0, h, lon0, w = region
        nseg = bounds.shape[1]
        e = np.clip(bounds, 0, T)
        sums = torch.zeros((len(fields), B, nseg, h, w), dtype=torch.float64, device=fields[0].device)
        for i, x in enumerate(fields):
            box = x[:, :, lat0:lat0 + h, lon0:lon0 + w]
            for b in range(B):
                for s in range(nseg):
                    acc = sums[i, b, s]
                    for t in range(int(e[b, s, 0]), int(e[b, s, 1])):    # one fp64 add per step, in step order
                        acc.add_(box[b, t])
        out: Dict[str, Optional[torch.Tensor]] = {"sums": None, "means": None}
        if "means" in want:
            n = torch.from_numpy(np.maximum(e[:, :, 1] - e[:, :, 0], 0).astype(np.float64)).to(sums.device)
            out["means"] = (sums / n[None, :, :, None, None]).to(torch.float32).cpu()          # 0.0 / 0.0: NaN
        if "sums" in want:
            out["sums"] = sums.cpu()
        if sums.device.type != "cpu":
            self.bytes_to_host += sum(v.numel() * v.element_size() for v in out.values() if v is not None)
        return out

    @torch.no_grad()
    def _fused_region(self, fields, bounds, region, want):
        from . import _lib
        from .aggregator import _check, _flat, _plane_table
        dev = fields[0].device
        B, T, H, W = fields[0].shape
        lat0, h, lon0, w = region
        N, nseg = len(fields), bounds.shape[1]
        fields = [_flat(x, W) for x in fields]
        names = [str(i) for i in range(N)]
        values, off = _plane_table(names, dict(zip(names, fields)))
        parts = [np.asarray(values, np.int64), np.arange(N, dtype=np.int32), np.clip(bounds, -2**31, 2**31 - 1).astype(np.int32)]
        blob = np.concatenate([p.reshape(-1).view(np.uint8) for p in parts])
        key = b"region" + blob.tobytes()
        if key != self._table_key or self._table is None or self._table.device != dev:      # built once per window shape
            self._table = torch.from_numpy(blob).pin_memory().to(dev, non_blocking=True)
            self._table_key = key
        base = self._table.data_ptr()
        rows_at = base + off["end"]
        bounds_at = rows_at + parts[1].nbytes
        numel = N * B * nseg * h * w
        sums = self._staging("sums", torch.float64, numel, dev) if "sums" in want else None
        means = self._staging("means", torch.float32, numel, dev) if "means" in want else None
        lib = _lib.lib()
        with torch.cuda.device(dev):
            _check(lib.ace_diag_region_segments(base + off["gen"], base + off["gen_strides"], rows_at, bounds_at,
                                                sums[0].data_ptr() if sums else None, means[0].data_ptr() if means else None,
                                                N, nseg, N, B, T, H, W, lat0, h, lon0, w, _lib.current_stream()))
            self.launches += 1
            out: Dict[str, Optional[torch.Tensor]] = {"sums": None, "means": None}
            for kind, pair in (("sums", sums), ("means", means)):
                if pair is not None:
                    d, hst = pair
                    hst[:numel].copy_(d[:numel], non_blocking=True)
                    self.bytes_to_host += numel * d.element_size()
                    out[kind] = hst[:numel].view(N, B, nseg, h, w)
            torch.cuda.current_stream().synchronize()            # the host reads the record next
        return out


_DEFAULT_REDUCER = SegmentReducer()


def segment_sums(data: TensorMapping, names: Sequence[str], edges=None, want: Sequence[str] = ("sums", "means"),
                 reducer: Optional[SegmentReducer] = None, bounds=None) -> Dict[str, Optional[torch.Tensor]]:
    """``SegmentReducer.__call__`` on ``reducer`` (default: a module-wide one)."""
    return (reducer or _DEFAULT_REDUCER)(data, names, edges, want, bounds=bounds)


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

    def __init__(self, directory: str, label: str, names: Optional[Sequence[str]] = None,
                 region: Optional[Sequence[int]] = None, coords: Optional[Mapping[str, Any]] = None):
        """``region=(lat0, nlat_r, lon0, nlon_r)``: the monthly means of that box only, cut out on the device (the regional file
        writers); ``coords``: what ``flush`` stores beside the names, as they are (the ``lat`` / ``lon`` of the box)."""
        self._dir = directory
        self._label = label
        self._save_names = None if names is None else list(names)
        self._init_years: Optional[np.ndarray] = None
        self._init_months: Optional[np.ndarray] = None
        self._calendar: Optional[str] = None
        self._totals: Dict[str, torch.Tensor] = {}
        self._counts: Optional[np.ndarray] = None
        self._coords = {} if coords is None else {k: torch.as_tensor(np.asarray(v)) for k, v in coords.items()}
        self.reducer = SegmentReducer(region=region)
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
            H, W = sums.shape[3:]                                        # the region's, when there is one
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
        out.update(self._coords)
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


# ---- region- and time-selected files ----------------------------------------------------------------------------------------
def _shift_bound(value: Optional[int], shift: int, out_of_bounds_value: Optional[int]) -> Optional[int]:
    """fme/core/typing_.py:19-40: a slice bound moved ``shift`` steps to the left; ``None`` stays ``None``, a bound that would
    fall below 0 becomes ``out_of_bounds_value``, a negative bound to start from is refused."""
    if value is None:
        return None
    if value < 0:
        raise ValueError("Negative slice bounds as an initial value are not supported")
    shifted = value - shift
    return out_of_bounds_value if shifted < 0 else shifted


@dataclasses.dataclass
class Slice:
    """fme/core/typing_.py:43-85: a python ``slice`` as a config.  As a ``time_selection`` it indexes the steps of the whole
    inference, counted after coarsening, the initial condition not among them."""
    start: Optional[int] = None
    stop: Optional[int] = None
    step: Optional[int] = None

    @property
    def slice(self) -> slice:
        return slice(self.start, self.stop, self.step)

    def contains(self, value: int) -> bool:
        start = self.start if self.start is not None else 0
        stop = self.stop if self.stop is not None else float("inf")
        step = self.step if self.step is not None else 1
        return start <= value < stop and (value - start) % step == 0

    @classmethod
    def shift_left(cls, original: "Slice", start_index: int) -> "Slice":
        """The slice as seen from a window whose first step is step ``start_index`` of the whole: a start that lies before the
        window becomes ``None``, a stop that does becomes 0 (nothing), the step is kept as it is.  So with ``step > 1`` the
        stride starts anew at the first step of every window whose start lies past ``start``, as the reference's does: the kept
        steps are those of ``range(n)[slice]`` only when the windows' lengths are multiples of the step."""
        return cls(start=_shift_bound(original.start, start_index, None), stop=_shift_bound(original.stop, start_index, 0),
                   step=original.step)


_MONTHS = ("january", "february", "march", "april", "may", "june", "july", "august", "september", "october", "november", "december")
_SEASONS = {"DJF": (12, 1, 2), "MAM": (3, 4, 5), "JJA": (6, 7, 8), "SON": (9, 10, 11)}


def _month_string_to_int(month_str: str) -> int:
    """file_writer.py:50-66: a full or three-letter English month name, in any letter case as ``strptime`` reads them."""
    key = str(month_str).lower()
    for number, name in enumerate(_MONTHS, start=1):
        if key == name or key == name[:3]:
            return number
    raise ValueError(f"Invalid month string: {month_str}. Use full month name (e.g., 'January') or abbreviated name (e.g., 'Jan').")


@dataclasses.dataclass
class MonthSelector:
    """file_writer.py:97-120: the steps whose month is one of ``months`` - full names, three-letter names, or the seasons "DJF",
    "MAM", "JJA", "SON".  An empty list selects every step."""
    months: List[str]

    def mask(self, month: np.ndarray) -> np.ndarray:
        """file_writer.py:69-94 on an int array of months (1 .. 12): the boolean mask of the selected ones."""
        month = np.asarray(month)
        if not self.months:
            return np.ones(month.shape, dtype=bool)
        mask = np.zeros(month.shape, dtype=bool)
        for selection in self.months:
            wanted = _SEASONS[selection] if selection in _SEASONS else (_month_string_to_int(selection),)
            mask |= np.isin(month, wanted)
        return mask


@dataclasses.dataclass
class TimeSlice:
    """fme/core/dataset/time.py:10-41, the fields only: as a ``time_selection`` it is refused, its meaning being xarray's
    partial-datetime-string indexing of a ``CFTimeIndex``."""
    start_time: Optional[str] = None
    stop_time: Optional[str] = None
    step: Optional[int] = None


@dataclasses.dataclass
class NetCDFWriterConfig:
    """raw.py:32-34.  Here the netCDF-shaped file is a ``torch.save`` archive: the stem is the reference's, the suffix ``pt``."""
    name: str = "netcdf"
    suffix: str = "nc"


@dataclasses.dataclass
class ZarrWriterConfig:
    """zarr.py:88-94, the fields only: zarr output is refused."""
    name: str = "zarr"
    chunks: Optional[Dict[str, int]] = dataclasses.field(default_factory=lambda: {"time": 1, "sample": 1})
    overwrite_check: bool = False
    suffix: str = "zarr"


def extent_indices(coord, lo, hi) -> Tuple[int, int]:
    """The index range [start, stop) that xarray's ``.sel(x=slice(lo, hi))`` keeps of a monotonic coordinate, i.e.
    ``pandas.Index(coord).slice_indexer(lo, hi)``, on ``numpy.searchsorted``.  On an increasing coordinate both ends are inclusive
    and ``lo > hi`` is empty; on a decreasing one the bounds are given in the coordinate's order (``lo >= hi``); ``None`` leaves an
    end open.  ``stop <= start`` is an empty range."""
    c = np.asarray(coord, dtype=np.float64).reshape(-1)
    n = c.size
    if n > 1 and not (np.all(np.diff(c) >= 0) or np.all(np.diff(c) <= 0)):
        raise ValueError("a coordinate must be monotonic to be cut by an extent")
    if n > 1 and c[0] > c[-1]:                                           # decreasing: search the reversed array, mirror the result
        rev = c[::-1]
        start = 0 if lo is None else n - int(np.searchsorted(rev, lo, side="right"))
        stop = n if hi is None else n - int(np.searchsorted(rev, hi, side="left"))
    else:
        start = 0 if lo is None else int(np.searchsorted(c, lo, side="left"))
        stop = n if hi is None else int(np.searchsorted(c, hi, side="right"))
    return start, stop


_log = logging.getLogger(__name__)


@dataclasses.dataclass
class FileWriterConfig:
    """file_writer.py:205-312 (same fields and defaults): one extra output file of ``names`` (``None``: every name), cut to the
    box ``lat_extent`` x ``lon_extent`` (each (lo, hi) in degrees, ``None``: everything; no wrap across the date line), coarsened
    in time by ``time_coarsen`` and then cut to the steps of ``time_selection`` (a ``Slice`` of step indices or a ``MonthSelector``).
    With ``save_reference`` the paired build writes ``<label>_predictions`` and ``<label>_target``, else ``<label>`` alone.

    Differences from the reference, all stated: the files are ``torch.save`` archives ``<label>.pt``; a ``TimeSlice`` selection, a
    zarr ``format`` and ``separate_ensemble_members`` raise ``NotImplementedError`` at build time; a box that holds no grid point
    raises ``ValueError`` at build time (the reference would write empty arrays)."""
    label: str
    names: Optional[List[str]] = None
    lat_extent: Optional[Sequence[float]] = None
    lon_extent: Optional[Sequence[float]] = None
    time_selection: Any = None
    save_reference: bool = True
    time_coarsen: Any = None
    format: Any = dataclasses.field(default_factory=NetCDFWriterConfig)
    separate_ensemble_members: bool = False

    def __post_init__(self):
        if self.lat_extent and len(self.lat_extent) != 2:
            raise ValueError("lat_extent must be a tuple of (min_lat, max_lat)")
        if self.lon_extent and len(self.lon_extent) != 2:
            raise ValueError("lon_extent must be a tuple of (min_lon, max_lon)")
        if self.time_selection is not None and self.time_coarsen is not None:
            _log.warning("Time coarsening is enabled. Time subselection is applied *after* time coarsening.")
        if isinstance(self.format, ZarrWriterConfig):
            if self.time_selection is not None:
                raise NotImplementedError("Time selection is not currently supported when writing to zarr.")
            if isinstance(self.time_coarsen, MonthlyCoarsenConfig):
                raise NotImplementedError("Monthly coarsening is not currently supported for the zarr format.")
        if isinstance(self.time_coarsen, MonthlyCoarsenConfig) and self.time_selection is not None:
            raise NotImplementedError("Time selection is not currently supported when using monthly coarsening.")

    @property
    def filenames(self) -> List[str]:
        """The files an entry may write (file_writer.py:287-297), with the suffix they have here."""
        return [f"{stem}.pt" for stem in (self.label, f"{self.label}_target", f"{self.label}_predictions")]

    def validate_time_coarsen(self, forward_steps_in_memory: int, n_forward_steps: int):
        if self.time_coarsen is not None:
            self.time_coarsen.validate(forward_steps_in_memory, n_forward_steps)

    def _region(self, coords: Mapping[str, Any]):
        """(region or ``None`` for the whole plane, the coordinates of what is written)"""
        if (self.lat_extent and "lat" not in coords) or (self.lon_extent and "lon" not in coords):
            raise ValueError(f"Coordinates must include 'lat' and 'lon' if using lat/lon extents. Got {list(coords.keys())}.")
        subset = {k: np.asarray(coords[k]) for k in ("lat", "lon") if k in coords}
        if not (self.lat_extent or self.lon_extent):
            return None, subset
        if "lat" not in coords or "lon" not in coords:
            raise ValueError(f"Coordinates must include 'lat' and 'lon' if using lat/lon extents. Got {list(coords.keys())}.")
        a, b = extent_indices(coords["lat"], *self.lat_extent) if self.lat_extent else (0, len(subset["lat"]))
        c, d = extent_indices(coords["lon"], *self.lon_extent) if self.lon_extent else (0, len(subset["lon"]))
        if b <= a or d <= c:
            raise ValueError(f"the region of '{self.label}' is empty: lat_extent {self.lat_extent} keeps {max(b - a, 0)} rows and "
                             f"lon_extent {self.lon_extent} keeps {max(d - c, 0)} columns (an extent is given in the coordinate's "
                             "own order, and there is no wrap across the date line)")
        return (a, b - a, c, d - c), {"lat": subset["lat"][a:b], "lon": subset["lon"][c:d]}

    def build(self, directory: str, coords: Optional[Mapping[str, Any]] = None) -> "FileWriter":
        """file_writer.py:354-478.  ``coords``: the coordinates of the whole domain, ``lat`` and ``lon`` arrays; needed only with an
        extent, stored (their subset) in the file when given."""
        if isinstance(self.time_selection, TimeSlice):
            raise NotImplementedError("TimeSlice selection is not built: its meaning is xarray's partial-datetime-string indexing "
                                      "of a CFTimeIndex; use a Slice of step indices or a MonthSelector")
        if self.time_selection is not None and not isinstance(self.time_selection, (Slice, MonthSelector)):
            raise ValueError(f"Unsupported time selection type: {type(self.time_selection)}")
        if isinstance(self.format, ZarrWriterConfig) or not isinstance(self.format, NetCDFWriterConfig):
            raise NotImplementedError("only the default (netCDF-shaped) format is written, as a torch.save archive; zarr is not built")
        if self.separate_ensemble_members:
            raise NotImplementedError("Writing separate ensemble members is not currently supported for netcdf output.")
        if self.time_coarsen is not None and not isinstance(self.time_coarsen, (TimeCoarsenConfig, MonthlyCoarsenConfig)):
            raise ValueError(f"time_coarsen must be a TimeCoarsenConfig or a MonthlyCoarsenConfig, got {type(self.time_coarsen)}")
        coords = {} if coords is None else coords
        region, subset = self._region(coords)
        plane = (len(np.asarray(coords["lat"])), len(np.asarray(coords["lon"]))) if region is not None else None
        return FileWriter(directory, self.label, names=self.names, region=region, plane=plane, coords=subset,
                          time_selection=self.time_selection, time_coarsen=self.time_coarsen)

    def build_paired(self, directory: str, coords: Optional[Mapping[str, Any]] = None, prediction_suffix: str = "predictions",
                     reference_suffix: str = "target") -> "PairedFileWriter":
        """file_writer.py:314-352"""
        reference = None
        prediction_label = self.label
        if self.save_reference:
            reference = dataclasses.replace(self, label=f"{self.label}_{reference_suffix}").build(directory, coords)
            prediction_label = f"{self.label}_{prediction_suffix}"
        return PairedFileWriter(dataclasses.replace(self, label=prediction_label).build(directory, coords), reference)


class FileWriter:
    """file_writer.py:481-591: cuts each window to the names, the box and the steps of its config and keeps what is left.  Region,
    selection and block mean are one ``SegmentReducer`` call per window - one segment of ``coarsen_factor`` source steps per kept
    output step - so on CUDA windows one ``ace_diag_region_segments`` launch, and only the kept record crosses to the host.

    ``flush`` writes ``<directory>/<label>.pt`` atomically: every kept name as fp32 (B, n_kept, nlat_r, nlon_r); ``time`` (int64
    microseconds of the ``TimeAxis``, (B, n_kept); the coarsened labels under time coarsening) and ``calendar`` when the windows
    came with a time axis; ``lat`` and ``lon`` (the box's) when coordinates were given.  Windows with nothing kept add nothing.
    With a ``MonthlyCoarsenConfig`` the record is a ``MonthlyDataWriter``'s on the box, and the file is its file."""
    uses_time = True

    def __init__(self, directory: str, label: str, names: Optional[Sequence[str]] = None, region: Optional[Sequence[int]] = None,
                 plane: Optional[Tuple[int, int]] = None, coords: Optional[Mapping[str, Any]] = None, time_selection=None,
                 time_coarsen=None):
        """``region``: (lat0, nlat_r, lon0, nlon_r), ``None`` for the whole plane; ``plane``: the (nlat, nlon) the region was cut
        from, checked against every window when given; ``coords``: stored in the file as they are."""
        self._dir = directory
        self._label = label
        self._names = None if names is None else list(names)
        self._region = None if region is None else tuple(int(v) for v in region)
        self._plane = None if plane is None else (int(plane[0]), int(plane[1]))
        self._coords = {} if coords is None else {k: torch.as_tensor(np.asarray(v)) for k, v in coords.items()}
        self._time_selection = time_selection
        self._factor = time_coarsen.coarsen_factor if isinstance(time_coarsen, TimeCoarsenConfig) else 1
        self._monthly: Optional[MonthlyDataWriter] = None
        if isinstance(time_coarsen, MonthlyCoarsenConfig):
            if time_selection is not None:
                raise NotImplementedError("Time selection is not currently supported when using monthly coarsening.")
            self._monthly = MonthlyDataWriter(directory, label, names=None, region=self._region, coords=self._coords)
        self.reducer = self._monthly.reducer if self._monthly is not None else SegmentReducer(region=self._region)
        self._no_write_count = 0
        self._n_timesteps_seen = 0                  # steps handed to the selection so far: coarsened ones under time coarsening
        self._records: List[Dict[str, torch.Tensor]] = []
        self._times: List[np.ndarray] = []
        self._calendar: Optional[str] = None
        os.makedirs(directory, exist_ok=True)

    @property
    def needs_time(self) -> bool:
        return self._monthly is not None or isinstance(self._time_selection, MonthSelector)

    @property
    def path(self) -> str:
        return os.path.join(self._dir, self._label + ".pt")

    def write(self, data: TensorMapping, filename: str):
        pass

    def _kept(self, n: int, time: Optional[TimeAxis], B: int) -> List[int]:
        """the steps of a window of ``n`` (coarsened) steps that the selection keeps, the window starting at ``_n_timesteps_seen``"""
        sel = self._time_selection
        if sel is None:
            return list(range(n))
        if isinstance(sel, Slice):
            return list(range(n)[Slice.shift_left(sel, self._n_timesteps_seen).slice])
        if time is None:
            raise ValueError("a MonthSelector needs the windows' time axis: build the ForcingWindows with time=")
        if B > 1:
            raise NotImplementedError("MonthSelector selection is not currently supported for multiple initial conditions.")
        return [int(i) for i in np.nonzero(sel.mask(time.year_month()[1][0]))[0]]

    def _nothing(self, start: int):
        # file_writer.py:567-578: it might be expected, so no more than ten lines about it
        self._no_write_count += 1
        if self._no_write_count < 10:
            _log.warning(f"No data to write for region {self._label} at timestep {start}.")
        elif self._no_write_count == 10:
            _log.warning("Further warnings about empty data will be suppressed.")

    def append_batch(self, batch: TensorMapping, time: Optional[TimeAxis] = None):
        names = [k for k in batch if self._names is None or k in self._names]
        if not batch:                               # a target side without fields: nothing to count the steps on either
            return self._nothing(self._n_timesteps_seen)
        first = next(iter(batch.values()))
        B, T, H, W = first.shape
        if self._plane is not None and (H, W) != self._plane:
            raise ValueError(f"the coordinates the region of '{self._label}' was cut from are {self._plane[0]} x {self._plane[1]}, "
                             f"the fields are {H} x {W}")
        if time is not None and tuple(time.shape) != (B, T):
            raise ValueError(f"time must be (samples, steps) = {(B, T)}, got {tuple(time.shape)}")
        f = self._factor
        if T % f != 0:
            raise ValueError(f"a window of {T} steps is not a multiple of coarsen_factor {f} "
                             "(FileWriterConfig.validate_time_coarsen checks the schedule up front)")
        start = self._n_timesteps_seen
        if self._monthly is not None:
            self._n_timesteps_seen += T
            if not names:
                return self._nothing(start)
            return self._monthly.append_batch({k: batch[k] for k in names}, time=time)
        coarse = coarsen_time(time, f)
        kept = self._kept(T // f, coarse, B)
        self._n_timesteps_seen += T // f
        if not names or not kept:
            return self._nothing(start)
        bounds = np.array([[k * f, (k + 1) * f] for k in kept], dtype=np.int64)
        means = self.reducer(batch, names, want=("means",), bounds=np.broadcast_to(bounds, (B,) + bounds.shape))["means"]
        self._records.append({n: means[i].clone() for i, n in enumerate(names)})
        if coarse is not None:
            if self._calendar is not None and coarse.calendar != self._calendar:
                raise ValueError(f"the calendar changed between windows: {self._calendar} then {coarse.calendar}")
            self._calendar = coarse.calendar
            self._times.append(coarse.us[:, kept].copy())

    def get_dataset(self) -> Dict[str, Any]:
        if self._monthly is not None:
            return self._monthly.get_dataset()
        if not self._records:
            return {}
        out: Dict[str, Any] = {k: torch.cat([r[k] for r in self._records if k in r], dim=1) for k in self._records[0]}
        if self._times and len(self._times) == len(self._records):
            out["time"] = torch.from_numpy(np.concatenate(self._times, axis=1).astype(np.int64))
            out["calendar"] = self._calendar
        out.update(self._coords)
        return out

    def flush(self):
        if self._monthly is not None:
            return self._monthly.flush()
        ds = self.get_dataset()
        if not ds:
            return
        tmp = self.path + ".tmp"
        torch.save(ds, tmp)
        os.replace(tmp, self.path)

    def finalize(self):
        self.flush()


class PairedFileWriter:
    """file_writer.py:594-627: the prediction's writer and, with ``save_reference``, the target's."""
    uses_time = True
    paired = True

    def __init__(self, prediction_writer: FileWriter, reference_writer: Optional[FileWriter]):
        self.prediction_writer = prediction_writer
        self.reference_writer = reference_writer

    @property
    def needs_time(self) -> bool:
        return self.prediction_writer.needs_time

    def write(self, data: TensorMapping, filename: str):
        pass

    def append_batch(self, batch: TensorMapping, target: TensorMapping, time: Optional[TimeAxis] = None):
        self.prediction_writer.append_batch(batch, time=time)
        if self.reference_writer is not None:
            self.reference_writer.append_batch(target, time=time)

    def flush(self):
        self.prediction_writer.flush()
        if self.reference_writer is not None:
            self.reference_writer.flush()

    def finalize(self):
        self.prediction_writer.finalize()
        if self.reference_writer is not None:
            self.reference_writer.finalize()


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
    """main.py:36-100 (same fields and defaults).  ``files``: a list of ``FileWriterConfig``, one extra region- / time-selected file
    (or pair of files) each; their file names must differ.  ``save_step_diagnostics=True`` is refused at build time: the records
    exist (ace_amd/step_diagnostics.py) but their file writer is not built.  So are an empty ``files`` list and an entry that is not a ``FileWriterConfig``."""
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
        all_filenames = [name for f in self._file_configs() for name in f.filenames]
        if len(set(all_filenames)) != len(all_filenames):
            raise ValueError(f"Duplicate filenames found in file writer configurations. Filenames: {all_filenames}")

    def _file_configs(self) -> List["FileWriterConfig"]:
        return [f for f in self.files or [] if isinstance(f, FileWriterConfig)]

    def validate_time_coarsen(self, forward_steps_in_memory: int, n_forward_steps: int):
        if self.time_coarsen is not None:
            self.time_coarsen.validate(forward_steps_in_memory, n_forward_steps)
        for f in self._file_configs():
            f.validate_time_coarsen(forward_steps_in_memory, n_forward_steps)

    def _refuse(self):
        if self.save_step_diagnostics:
            raise NotImplementedError("save_step_diagnostics: the step-diagnostics records are produced (predict(..., "
                                      "step_diagnostics=True)), but the step-diagnostics file writer is not built")
        if self.files is not None and (not self.files or len(self._file_configs()) != len(self.files)):
            raise NotImplementedError("files: a non-empty list of FileWriterConfig entries is what is built; got "
                                      f"{[type(f).__name__ for f in self.files]}")

    def build(self, directory: str, coords: Optional[Mapping[str, Any]] = None) -> "DataWriter":
        """``coords``: the ``lat`` and ``lon`` arrays of the whole domain (``DatasetInfo.horizontal_coordinates``); needed only by a
        ``files`` entry with an extent."""
        self._refuse()
        writers: List[Any] = []
        if self.save_prediction_files:
            raw: Any = _RawSubset(directory, names=self.names)
            if self.time_coarsen is not None:
                raw = self.time_coarsen.build(raw)
            writers.append(raw)
        if self.save_monthly_files:
            writers.append(MonthlyDataWriter(directory, "monthly_mean_predictions", names=self.names))
        writers += [f.build(directory, coords) for f in self._file_configs()]
        return DataWriter(writers, directory)

    def build_paired(self, directory: str, coords: Optional[Mapping[str, Any]] = None) -> "PairedDataWriter":
        self._refuse()
        writers: List[Any] = []
        if self.save_prediction_files:
            raw: Any = PairedTensorFileWriter(directory, names=self.names)
            if self.time_coarsen is not None:
                raw = self.time_coarsen.build_paired(raw)
            writers.append(raw)
        if self.save_monthly_files:
            writers.append(PairedMonthlyDataWriter(directory, names=self.names))
        writers += [f.build_paired(directory, coords) for f in self._file_configs()]
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
