"""Global-mean removal of the single-module step (fme/core/step/global_mean_removal.py; applied by ``step_with_adjustments``,
fme/core/step/single_module.py:650-668): listed fields are shifted so that a sample's cellwise (unweighted) spatial mean sits on
the climatological mean before the normaliser, and shifted back after the de-normaliser; optionally the removed mean is appended
to the network input as broadcast channels in normalised space.

The transforms here are the reference's torch ops verbatim and run on any device.  On the device, with ``fused=True`` (the
default), the per-sample means of fp32 fields come from ``ace_gmr_sample_means`` (csrc/gmr.hip) instead of ``t.mean``: the fp64
sum of the plane in the kernel's fixed order, divided and rounded to fp32 once - the reduction the rollout engine's fused pack
uses, so that ``Stepper.predict`` and ``RolloutEngine`` see the same shifts.  That mean is the one numerical difference to the
reference (an fp32 sum in torch's order); everything downstream of it is the same torch ops on both paths.  ``fused=False`` keeps
``t.mean`` on the device (the A/B of tools/bench_gmr.py and of the tests)."""
import abc
import dataclasses
import logging
from collections.abc import Mapping
from typing import Dict, List, Optional, Tuple

import torch

TensorMapping = Mapping[str, torch.Tensor]
TensorDict = Dict[str, torch.Tensor]

DEFAULT_TEMPERATURE_FIELD_NAMES: List[str] = [
    "surface_temperature",
    "TMP2m",
    "TMP850",
    "air_temperature_0",
    "air_temperature_1",
    "air_temperature_2",
    "air_temperature_3",
    "air_temperature_4",
    "air_temperature_5",
    "air_temperature_6",
    "air_temperature_7",
]

logger = logging.getLogger(__name__)

_EXTRA_CHANNEL_PREFIX = "__gmr_extra__"


def _extra_channel_name(field: str) -> str:
    return f"{_EXTRA_CHANNEL_PREFIX}{field}"


def extra_channel_source_field(name: str) -> Optional[str]:
    """The source field of a synthetic input channel ``__gmr_extra__<field>``, None for any other name."""
    if name.startswith(_EXTRA_CHANNEL_PREFIX):
        return name[len(_EXTRA_CHANNEL_PREFIX):]
    return None


@dataclasses.dataclass
class GlobalMeanRemovalState:
    """What ``forward_transform`` hands to ``inverse_transform`` and ``extras_normalized`` of the same transform: the per-sample
    shift of every name to un-shift, and the synthetic input channels (normalised space)."""

    shifts: Dict[str, torch.Tensor]
    extras: TensorDict


def _refuse_mask(data_mask) -> None:
    if data_mask is not None:
        raise NotImplementedError("data masks are outside the accelerated hot path")


def _broadcast_to_spatial(scalar_per_sample: torch.Tensor, spatial_shape: Tuple[int, ...]) -> torch.Tensor:
    return scalar_per_sample.view(-1, *(1,) * len(spatial_shape)).expand(-1, *spatial_shape)


def _plane_rows(t: torch.Tensor) -> torch.Tensor:
    """t as (batch, pixels) with unit pixel stride (a view where the layout allows it)"""
    return t.reshape(t.shape[0], -1)


_TABLES: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}     # sample_means' device tables, by (device, pointers, strides)


def sample_means(fields: List[torch.Tensor], fused: bool = True) -> List[torch.Tensor]:
    """Per-sample cellwise means ``t.mean(dim=(1, ...))`` of every field, each of shape [batch].  fp32 fields on the device with
    ``fused``: one ``ace_gmr_sample_means`` launch pair over all of them (the fp64 sum in the fixed order of include/ace_sfno.h,
    rounded to fp32 once)."""
    if not fields:
        return []
    first = fields[0]
    native = fused and all(t.is_cuda and t.dtype == torch.float32 and t.ndim >= 2 and t.shape == first.shape and t.numel() > 0
                           for t in fields)
    if not native:
        return [t.mean(dim=tuple(range(1, t.ndim))) for t in fields]
    from . import _lib
    L = _lib.lib()
    rows = []
    for t in fields:
        r = _plane_rows(t)
        rows.append(r if r.stride(1) == 1 else r.contiguous())
    B, hw, K, dev = first.shape[0], rows[0].shape[1], len(rows), first.device
    with torch.cuda.device(dev):
        # the pointer table is a blocking upload: a rollout's fields come back at the addresses the allocator handed out the
        # step before, so the last few tables are kept by their contents
        key = (dev, tuple(r.data_ptr() for r in rows), tuple(r.stride(0) for r in rows))
        cached = _TABLES.get(key)
        if cached is None:
            if len(_TABLES) >= 16:
                _TABLES.clear()
            cached = _TABLES[key] = (torch.tensor([key[1], key[2]], dtype=torch.int64, device=dev),
                                     torch.arange(K, dtype=torch.int32, device=dev))
        table, index = cached
        partials = torch.empty(B * K * int(L.ace_gmr_chunks(hw)), dtype=torch.float64, device=dev)
        means = torch.empty(B, K, dtype=torch.float32, device=dev)
        _lib.check(L.ace_gmr_sample_means(table.data_ptr(), table.data_ptr() + 8 * K, index.data_ptr(), K, partials.data_ptr(),
                                          means.data_ptr(), B, K, hw, _lib.current_stream()))
    return [means[:, k] for k in range(K)]


class GlobalMeanRemoval(abc.ABC):
    """global_mean_removal.py:63-148.  Fields of ``field_names`` that are outputs only are not shifted by ``forward_transform``
    (they are not inputs) but are un-shifted by ``inverse_transform``; "global mean" is the cellwise mean of a sample, not the
    area-weighted one."""

    fused = True        # device fp32 fields: the means from the native reduction (False: t.mean)

    @property
    @abc.abstractmethod
    def extra_channel_names(self) -> List[str]:
        """The synthetic input channels this transform appends to the packed input (after the in_names), [] without any."""

    @property
    def n_extra_input_channels(self) -> int:
        return len(self.extra_channel_names)

    @abc.abstractmethod
    def forward_transform(self, input: TensorMapping, data_mask=None) -> Tuple[TensorDict, GlobalMeanRemovalState]:
        """Shift the de-normalised input fields; returns (shifted input, the state for the other two methods)."""

    def inverse_transform(self, output: TensorDict, state: GlobalMeanRemovalState) -> TensorDict:
        result = dict(output)
        for name, shift in state.shifts.items():
            if name not in result:
                continue
            t = result[name]
            broadcast = shift.view(shift.shape[0], *(1,) * (t.ndim - 1))
            result[name] = t - broadcast
        return result

    def extras_normalized(self, state: GlobalMeanRemovalState) -> TensorDict:
        """The synthetic input channels in NORMALISED space, keyed by ``extra_channel_names``, each [batch, *spatial]."""
        return dict(state.extras)


class SharedGlobalMeanRemoval(GlobalMeanRemoval):
    """global_mean_removal.py:182-266: one offset, from the reference field's mean, for every listed field."""

    def __init__(self, reference_field: str, field_names: frozenset, append_as_input: bool, reference_mean: torch.Tensor,
                 reference_std: torch.Tensor, fused: bool = True):
        self._reference_field = reference_field
        self._field_names = field_names
        self._append_as_input = append_as_input
        self._reference_mean = reference_mean
        self._reference_std = reference_std
        self.fused = fused

    @property
    def reference_field(self) -> str:
        return self._reference_field

    @property
    def field_names(self) -> frozenset:
        return self._field_names

    @property
    def extra_channel_names(self) -> List[str]:
        if not self._append_as_input:
            return []
        return [_extra_channel_name(self._reference_field)]

    def forward_transform(self, input: TensorMapping, data_mask=None) -> Tuple[TensorDict, GlobalMeanRemovalState]:
        _refuse_mask(data_mask)
        ref_name = self._reference_field
        if ref_name not in input:
            raise ValueError(f"Reference field '{ref_name}' is not present in the input.")
        ref = input[ref_name]
        sample_mean = sample_means([ref], self.fused)[0]
        offset = self._reference_mean.to(ref.device) - sample_mean
        spatial_shape = tuple(ref.shape[1:])

        extras: TensorDict = {}
        if self._append_as_input:
            normalized_mean = -offset / self._reference_std.to(ref.device)
            extras[_extra_channel_name(ref_name)] = _broadcast_to_spatial(normalized_mean, spatial_shape)

        result = dict(input)
        for name in self._field_names:
            if name not in result:
                continue
            t = result[name]
            broadcast = offset.view(offset.shape[0], *(1,) * (t.ndim - 1))
            result[name] = t + broadcast

        # every listed field shares the offset; the inverse un-shifts those that are outputs (output-only ones too)
        shifts = {name: offset for name in self._field_names}
        return result, GlobalMeanRemovalState(shifts=shifts, extras=extras)


class PerChannelGlobalMeanRemoval(GlobalMeanRemoval):
    """global_mean_removal.py:269-348: each listed input field's own mean is moved onto its climatological mean."""

    def __init__(self, field_names: List[str], append_as_input: bool, means: TensorDict, stds: TensorDict, fused: bool = True):
        self._field_names = field_names
        self._append_as_input = append_as_input
        self._means = means
        self._stds = stds
        self.fused = fused

    @property
    def field_names(self) -> List[str]:
        return self._field_names

    @property
    def extra_channel_names(self) -> List[str]:
        if not self._append_as_input:
            return []
        return [_extra_channel_name(name) for name in self._field_names]

    def forward_transform(self, input: TensorMapping, data_mask=None) -> Tuple[TensorDict, GlobalMeanRemovalState]:
        _refuse_mask(data_mask)
        result = dict(input)
        shifts: Dict[str, torch.Tensor] = {}
        spatial_shape: Optional[Tuple[int, ...]] = None

        present = [name for name in self._field_names if name in result]
        means = dict(zip(present, sample_means([result[name] for name in present], self.fused)))
        for name in present:
            t = result[name]
            if spatial_shape is None:
                spatial_shape = tuple(t.shape[1:])
            shift = self._means[name].to(t.device) - means[name]
            shifts[name] = shift
            broadcast = shift.view(shift.shape[0], *(1,) * (t.ndim - 1))
            result[name] = t + broadcast

        extras: TensorDict = {}
        if self._append_as_input and spatial_shape is not None:
            for name in self._field_names:
                if name not in shifts:
                    continue
                normalized = -shifts[name] / self._stds[name].to(shifts[name].device)
                extras[_extra_channel_name(name)] = _broadcast_to_spatial(normalized, spatial_shape)

        return result, GlobalMeanRemovalState(shifts=shifts, extras=extras)


def _warn_unused(name: str) -> None:
    logger.warning("global_mean_removal field_name '%s' is not in in_names or out_names and will have no effect", name)


@dataclasses.dataclass
class SharedGlobalMeanRemovalConfig:
    """global_mean_removal.py:351-410.  ``reference_field``: the input whose per-sample cellwise mean sets the offset applied to
    all ``field_names`` (inputs, outputs or both); ``append_as_input``: the removed mean, normalised, is one more input channel."""

    kind: str = "shared"
    reference_field: str = "surface_temperature"
    field_names: List[str] = dataclasses.field(default_factory=lambda: list(DEFAULT_TEMPERATURE_FIELD_NAMES))
    append_as_input: bool = False

    def __post_init__(self):
        if self.kind != "shared":
            raise ValueError(f"SharedGlobalMeanRemovalConfig.kind must be 'shared', got {self.kind!r}")
        self.field_names = list(self.field_names)

    def validate_names(self, in_names: List[str], out_names: List[str]) -> None:
        if self.reference_field not in in_names:
            raise ValueError(f"reference_field '{self.reference_field}' not in in_names: {in_names}")
        all_names = set(in_names) | set(out_names)
        for name in self.field_names:
            if name not in all_names:
                _warn_unused(name)

    def build(self, normalizer, in_names: List[str], fused: bool = True) -> SharedGlobalMeanRemoval:
        return SharedGlobalMeanRemoval(reference_field=self.reference_field, field_names=frozenset(self.field_names),
                                       append_as_input=self.append_as_input,
                                       reference_mean=normalizer.means[self.reference_field],
                                       reference_std=normalizer.stds[self.reference_field], fused=fused)


@dataclasses.dataclass
class PerChannelGlobalMeanRemovalConfig:
    """global_mean_removal.py:413-467.  ``field_names``: the input fields to process, None for all of them; an explicit name has
    to be an input.  ``append_as_input``: one more input channel per processed field."""

    kind: str = "per_channel"
    field_names: Optional[List[str]] = None
    append_as_input: bool = False

    def __post_init__(self):
        if self.kind != "per_channel":
            raise ValueError(f"PerChannelGlobalMeanRemovalConfig.kind must be 'per_channel', got {self.kind!r}")
        if self.field_names is not None:
            self.field_names = list(self.field_names)

    def _resolve_names(self, in_names: List[str]) -> List[str]:
        return self.field_names if self.field_names is not None else list(in_names)

    def validate_names(self, in_names: List[str], out_names: List[str]) -> None:
        if self.field_names is not None:
            all_names = set(in_names) | set(out_names)
            for name in self.field_names:
                if name not in all_names:
                    _warn_unused(name)
                elif name not in in_names:
                    raise ValueError(f"field_name '{name}' not in in_names: {in_names}")

    def build(self, normalizer, in_names: List[str], fused: bool = True) -> PerChannelGlobalMeanRemoval:
        # a listed name in neither in_names nor out_names (the warning above) has no statistics and no effect
        names = [n for n in self._resolve_names(in_names) if n in normalizer.means]
        return PerChannelGlobalMeanRemoval(field_names=names, append_as_input=self.append_as_input,
                                           means={n: normalizer.means[n] for n in names},
                                           stds={n: normalizer.stds[n] for n in names}, fused=fused)


_KINDS = {"shared": SharedGlobalMeanRemovalConfig, "per_channel": PerChannelGlobalMeanRemovalConfig}


def config_from_state(state):
    """A configuration instance, or its state mapping with ``kind`` "shared" / "per_channel" (as a checkpoint's step configuration
    carries it), or None.  Anything else - another or no kind, keys the configuration does not have - is refused."""
    if state is None or isinstance(state, tuple(_KINDS.values())):
        return state
    if not isinstance(state, Mapping) or state.get("kind") not in _KINDS:
        raise NotImplementedError("SingleModuleStepConfig.global_mean_removal must be a SharedGlobalMeanRemovalConfig, a "
                                  "PerChannelGlobalMeanRemovalConfig or its state with kind 'shared' / 'per_channel'")
    cls = _KINDS[state["kind"]]
    extra = set(state) - {f.name for f in dataclasses.fields(cls)}
    if extra:
        raise NotImplementedError(f"global_mean_removal ({state['kind']}): unknown options {sorted(extra)}")
    return cls(**state)
