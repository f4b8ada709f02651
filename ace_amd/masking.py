"""Static spatial masking around the step (fme/core/spatial_masking.py:11-167, fme/core/spatial_mask_provider.py:70-170,
fme/core/name_and_prefix_matcher.py): a dataset's time-invariant masks ("mask_<variable>", "mask_<level>", "mask_2d"), the
replacement of masked regions of the step INPUTS by a fill value (StepperConfig.input_masking, single_module.py:615-632) and of the
step OUTPUTS by NaN where the data has no valid points (the provider's output masker).  Outside the network - used by
``Stepper.step``; the static-buffer ``RolloutEngine`` refuses a stepper that masks, ``OceanRolloutEngine`` runs it.

Two paths compute the same thing.  The torch path is the reference's elementwise ops per name.  On the GPU (fp32 fields of one
(B, H, W) or (B, 1, H, W) shape with contiguous rows, 2-D masks; ``StaticSpatialMasking.fused``) the whole dict is one
``ace_mask_planes`` launch (csrc/masking.hip): a host plan resolves each name once to (mask, fp32 fill), and one uint8 hit plane
per distinct mask is computed on the device with the reference's own torch expression and cached, so the kernel only selects
and its output is bitwise the torch path's."""
import dataclasses
import functools
import re
from typing import Any, Dict, List, Mapping, Optional, Tuple, Union

import torch

from ._lib import check

TensorMapping = Mapping[str, torch.Tensor]
_LEVEL = re.compile(r"_(\d+)$")


class NameMatcher:
    """name_and_prefix_matcher.py: 'thetao' matches thetao and thetao_<level>; 'thetao_' matches thetao_<level>; 'thetao_3' itself."""

    def __init__(self, names_and_prefixes: Optional[List[str]] = None):
        self._patterns = []
        for name in names_and_prefixes or []:
            if name.endswith("_"):
                self._patterns.append(re.compile(rf"^{name}\d+$"))
            elif re.match(r".+_\d+$", name):
                self._patterns.append(re.compile(rf"^{name}$"))
            else:
                self._patterns += [re.compile(rf"^{name}$"), re.compile(rf"^{name}_\d+$")]

    def match(self, name: str) -> bool:
        return any(p.match(name) for p in self._patterns)


class SpatialMaskProvider:
    """spatial_mask_provider.py:70-170: 2-D masks by name; lookup order variable-specific, level-specific, "mask_2d"."""

    def __init__(self, masks: Optional[TensorMapping] = None):
        self._masks: Dict[str, torch.Tensor] = dict(masks) if masks is not None else {}
        for key in self._masks:
            if not key.startswith("mask_"):
                raise ValueError("The 'mask' TensorDict passed to SpatialMaskProvider init has non-mask tensors, including "
                                 f"{key}. Expected all keys to start with the string 'mask_'.")

    @property
    def masks(self) -> TensorMapping:
        return self._masks

    def get_mask_tensor_for(self, name: str) -> Optional[torch.Tensor]:
        key = self.mask_key_for(name)
        return self._masks[key] if key is not None else None

    def mask_key_for(self, name: str) -> Optional[str]:
        """The key of the mask ``get_mask_tensor_for`` returns (None: no mask)."""
        if f"mask_{name}" in self._masks:
            return f"mask_{name}"
        level = _LEVEL.search(name)
        if level:
            key = f"mask_{int(level.group(1))}"
            return key if key in self._masks else None
        return "mask_2d" if "mask_2d" in self._masks else None

    def to(self, device) -> "SpatialMaskProvider":
        return SpatialMaskProvider({k: v.to(device) for k, v in self._masks.items()})

    def build_output_spatial_masker(self) -> "StaticSpatialMasking":
        """NaN where the mask is 0 (no valid data)."""
        return StaticSpatialMasking(mask_value=0, fill_value=float("nan"), mask=self)

    def get_state(self) -> Dict[str, Any]:
        return {"masks": dict(self._masks)}

    @classmethod
    def from_state(cls, state: Optional[Mapping[str, Any]]) -> "SpatialMaskProvider":
        return cls(dict(state["masks"]) if state and state.get("masks") else None)

    def __bool__(self) -> bool:
        return bool(self._masks)


class StaticSpatialMasking:
    """spatial_masking.py:98-150: data[name] = fill where round(mask) == mask_value, per variable with a mask, unless excluded."""

    def __init__(self, mask_value: int, fill_value: Union[float, TensorMapping], mask: SpatialMaskProvider,
                 exclude: Optional[NameMatcher] = None):
        self._value = mask_value
        self._fill = fill_value
        self._mask = mask
        self._exclude = exclude or NameMatcher()
        self._on: Dict[str, SpatialMaskProvider] = {}
        self.fused = True                 # CUDA fp32 fields take the HIP path; False: the torch ops on any device
        self._plans: Dict[Tuple[str, ...], List[Tuple[Optional[str], float]]] = {}
        self._hits: Dict[str, Tuple[Dict[str, int], torch.Tensor]] = {}
        self._tables: Dict[Tuple[str, Tuple[str, ...]], Tuple[torch.Tensor, torch.Tensor]] = {}
        self._launches = 0

    @property
    def mask_value(self) -> int:
        return self._value

    def _provider(self, device) -> SpatialMaskProvider:
        key = str(device)
        if key not in self._on:
            self._on[key] = self._mask.to(device)
        return self._on[key]

    def _fill_for(self, name: str):
        if isinstance(self._fill, Mapping):
            if name not in self._fill:
                raise KeyError(f"StaticSpatialMasking was initialized with a fill_value mapping but the mapping is missing key '{name}'.")
            return self._fill[name]
        return self._fill

    # ---- the host plan: which names are masked, with which mask and fp32 fill ----------------------------------------------
    def resolve(self, name: str) -> Tuple[Optional[str], Optional[float]]:
        """(key of the provider's mask this name is filled by, the fill as the fp32 value the torch path writes); (None, None)
        for a name that is excluded or has no mask - the rules of ``__call__``."""
        if self._exclude.match(name):
            return None, None
        key = self._mask.mask_key_for(name)
        if key is None:
            return None, None
        fill = self._fill_for(name)
        fill = fill.detach().to("cpu", torch.float32) if isinstance(fill, torch.Tensor) else torch.tensor(fill, dtype=torch.float32)
        return key, float(fill)

    def plan(self, names) -> List[Tuple[Optional[str], Optional[float]]]:
        """``resolve`` of every name, cached per name tuple."""
        names = tuple(names)
        p = self._plans.get(names)
        if p is None:
            p = self._plans[names] = [self.resolve(n) for n in names]
        return p

    def hit_planes(self, device, shape: Tuple[int, int]) -> Tuple[Dict[str, int], torch.Tensor]:
        """One uint8 plane per 2-D (H, W) mask of the provider, (nmask, H * W) on ``device``: the reference's
        ``torch.round(mask).to(torch.int64) == mask_value`` evaluated once with those very ops on the device (cached, as
        ``_provider`` caches the masks); masks of another shape have no plane."""
        key = f"{device}:{shape[0]}x{shape[1]}"
        cached = self._hits.get(key)
        if cached is None:
            index, rows = {}, []
            for k, m in self._provider(device).masks.items():
                if tuple(m.shape) == tuple(shape):
                    index[k] = len(rows)
                    rows.append((torch.round(m).to(torch.int64) == self._value).to(torch.uint8).reshape(-1))
            hits = torch.stack(rows).contiguous() if rows else torch.zeros(1, shape[0] * shape[1], dtype=torch.uint8, device=device)
            cached = self._hits[key] = (index, hits)
        return cached

    def device_tables(self, names, device, shape: Tuple[int, int]) -> Tuple[torch.Tensor, torch.Tensor]:
        """(mask_idx int32, fill fp32) device arrays of ``names`` for the masking kernels: the row of the name's hit plane (-1:
        unmasked) and its fill.  Raises NotImplementedError when a name's mask is not a 2-D (H, W) plane."""
        names = tuple(names)
        key = (f"{device}:{shape[0]}x{shape[1]}", names)
        cached = self._tables.get(key)
        if cached is None:
            index, _ = self.hit_planes(device, shape)
            idx, fills = [], []
            for n, (k, f) in zip(names, self.plan(names)):
                if k is not None and k not in index:
                    raise NotImplementedError(f"the mask '{k}' of '{n}' is not a 2-D {tuple(shape)} plane: the masking kernels "
                                              "broadcast 2-D masks over the batch only")
                idx.append(index[k] if k is not None else -1)
                fills.append(f if f is not None else 0.0)
            cached = self._tables[key] = (torch.tensor(idx, dtype=torch.int32, device=device),
                                          torch.tensor(fills, dtype=torch.float32, device=device))
        return cached

    # ---- the call -------------------------------------------------------------------------------------------------------
    def route(self, data: TensorMapping) -> str:
        """"fused" when ``__call__`` on this dict makes one ``ace_mask_planes`` launch, "torch" when it runs the torch ops."""
        return "fused" if self._fusable(data) is not None else "torch"

    def launches(self) -> int:
        """``ace_mask_planes`` launches made by ``__call__`` so far (the route query of the tests and benchmarks)."""
        return self._launches

    def _fusable(self, data: TensorMapping):
        """The masked names and their (B, H, W) views when the HIP path applies, else None."""
        if not self.fused or not data:
            return None
        first = next(iter(data.values()))
        if not isinstance(first, torch.Tensor) or first.device.type != "cuda" or first.dim() not in (3, 4):
            return None
        B, H, W = first.shape[0], first.shape[-2], first.shape[-1]
        dev = first.device
        names, planes = [], []
        for (name, t), (k, _) in zip(data.items(), self.plan(tuple(data))):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev:
                return None
            if not ((t.dim() == 3 or (t.dim() == 4 and t.shape[1] == 1)) and t.shape[0] == B and tuple(t.shape[-2:]) == (H, W)
                    and t.stride(-1) == 1 and t.stride(-2) == W):
                return None
            if k is None:
                continue
            if tuple(self._mask.masks[k].shape) != (H, W):
                return None
            names.append(name)
            planes.append(t.reshape(B, H, W) if t.dim() == 3 else t[:, 0])
        return names, planes, (B, H, W), dev

    def __call__(self, data: TensorMapping) -> Dict[str, torch.Tensor]:
        fusable = self._fusable(data)
        if fusable is not None:
            return self._fused(data, *fusable)
        out = dict(data)
        for name, tensor in out.items():
            if self._exclude.match(name):
                continue
            mask = self._provider(tensor.device).get_mask_tensor_for(name)
            if mask is None:
                continue
            fill = self._fill_for(name)
            fill = fill.to(tensor.device, tensor.dtype) if isinstance(fill, torch.Tensor) else torch.tensor(fill, dtype=tensor.dtype, device=tensor.device)
            where = torch.round(mask).to(torch.int64).expand(tensor.shape) == self._value
            out[name] = torch.where(where, fill, tensor)
        return out

    def _fused(self, data: TensorMapping, names, planes, bhw, dev) -> Dict[str, torch.Tensor]:
        from . import _lib
        out = dict(data)
        if not names:
            return out
        B, H, W = bhw
        HW = H * W
        mask_idx, fill = self.device_tables(names, dev, (H, W))
        _, hits = self.hit_planes(dev, (H, W))
        # one allocation holds every masked output (each a contiguous tensor of its input's shape, aliasing no input)
        block = torch.empty(len(names), B * HW, dtype=torch.float32, device=dev)
        results = [block[i].view(data[n].shape) for i, n in enumerate(names)]
        # one table upload per call: source pointers, source strides, destination pointers, destination strides
        table = [p.data_ptr() for p in planes] + [p.stride(0) if B > 1 else HW for p in planes]
        table += [r.data_ptr() for r in results] + [HW] * len(names)
        table = torch.tensor(table, dtype=torch.int64).to(dev)
        n = len(names)
        base = table.data_ptr()
        with torch.cuda.device(dev):
            rc = _lib.lib().ace_mask_planes(base, base + 8 * n, base + 16 * n, base + 24 * n, mask_idx.data_ptr(), hits.data_ptr(),
                                            hits.shape[0], fill.data_ptr(), n, B, HW, _lib.current_stream())
        _check(rc)
        self._launches += 1
        for name, r in zip(names, results):
            out[name] = r
        return out


_check = functools.partial(check, family="mask")


class NullSpatialMasking:
    def __call__(self, data: TensorMapping) -> Dict[str, torch.Tensor]:
        return dict(data)


@dataclasses.dataclass
class StaticSpatialMaskingConfig:
    """spatial_masking.py:44-95 (same fields)."""
    mask_value: int
    fill_value: Union[str, float] = 0.0
    exclude_names_and_prefixes: Optional[List[str]] = None

    def __post_init__(self):
        if self.mask_value not in (0, 1):
            raise ValueError(f"mask_value must be either 0 or 1, but got {self.mask_value}")
        if isinstance(self.fill_value, str) and self.fill_value != "mean":
            raise ValueError(f"fill_value must be a float or 'mean', got {self.fill_value!r}")

    @classmethod
    def from_state(cls, state) -> Optional["StaticSpatialMaskingConfig"]:
        if state is None or isinstance(state, cls):
            return state
        extra = set(state) - {"mask_value", "fill_value", "exclude_names_and_prefixes"}
        if extra:
            raise ValueError(f'can not match {sorted(extra)} to any data class field of "StaticSpatialMaskingConfig"')
        return cls(**state)

    def build(self, mask: SpatialMaskProvider, means: Optional[TensorMapping] = None) -> StaticSpatialMasking:
        exclude = NameMatcher(self.exclude_names_and_prefixes)
        if isinstance(self.fill_value, (int, float)) and not isinstance(self.fill_value, bool):
            return StaticSpatialMasking(self.mask_value, float(self.fill_value), mask, exclude)
        if means is None:
            raise ValueError("fill_values mapping required by build unless configured fill_value is a float.")
        return StaticSpatialMasking(self.mask_value, means, mask, exclude)
