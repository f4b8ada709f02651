"""Derived variables of an ocean rollout (fme/core/ocean_derived_variables.py; the ``OceanData`` properties of
fme/core/ocean_data.py they read; ``OceanDeriveFn`` of fme/core/coordinates.py:75-109): same registry names, order, metadata
and ``exists_ok`` flags, same skip and error rules.

Two paths compute the same thing.  The torch path (``OceanDeriveFn(fused=False)``, and every CPU tensor) is the reference's op
sequence on the name resolution of ace_amd/ocean_corrector.py.  With the window on the GPU the seven variables are one HIP launch
(ace_amd/csrc/ocean_derive.hip, ``ace_ocean_derive_window``): every input plane read once, every output written once, the heat
content summed in fp64; ``OceanDeriveFn.window`` hands the initial condition to the kernel where it lies, so nothing is
concatenated.  The fused heat content differs from the torch path by the fp32 roundings of the latter (include/ace_sfno.h states
the contract, tests/_ocean_derive_ref.py restates it in numpy); the surface variables are bitwise equal."""
import ctypes
import dataclasses
import datetime
import math
import os
import types
from typing import Any, Callable, Dict, List, Mapping, MutableMapping, Optional, Tuple

import torch

from . import ocean_corrector as oc
from .ocean_corrector import DepthCoordinate, _get, level_names

TensorMapping = Mapping[str, torch.Tensor]
TensorDict = Dict[str, torch.Tensor]


@dataclasses.dataclass
class VariableMetadata:
    """fme/core/dataset/data_typing.py"""
    units: str
    long_name: str


class _OceanData:
    """What a registered function reads: the merged fields, the depth coordinate and the cell-area provider."""

    def __init__(self, data: TensorMapping, depth_coordinate: Optional[DepthCoordinate], cell_area_provider=None):
        self.data = data
        self.depth = depth_coordinate
        self._area = cell_area_provider

    @property
    def ocean_heat_content(self) -> torch.Tensor:
        if self.depth is None:
            raise ValueError("Depth coordinate must be provided to compute column-integrated ocean heat content.")
        return oc.ocean_heat_content(self.data, self.depth)

    @property
    def net_energy_flux_into_ocean(self) -> torch.Tensor:
        return ((oc.net_downward_surface_heat_flux(self.data) + oc.geothermal_heat_flux(self.data))
                * oc.sea_surface_fraction(self.data))

    @property
    def area_weights_m2(self) -> torch.Tensor:
        if self._area is None:
            raise ValueError("A cell area provider must be provided to access cell area information.")
        return self._area.area_weights_m2

    @property
    def sea_ice_thickness(self) -> torch.Tensor:
        """ocean_data.py:233-260"""
        try:
            return _get(self.data, "sea_ice_thickness")
        except KeyError:
            sfrac = oc.sea_surface_fraction(self.data)
            sea_ice_vol = _get(self.data, "sea_ice_volume")
            try:
                sea_ice_frac = _get(self.data, "ocean_sea_ice_fraction") * sfrac
            except KeyError:
                lfrac = _get(self.data, "land_fraction")
                sea_ice_frac = oc.sea_ice_fraction(self.data) * sfrac / (1 - lfrac)
            cell_area = self.area_weights_m2.to(sea_ice_vol.device)
            return torch.where(torch.isnan(sea_ice_vol), float("nan"),
                               torch.nan_to_num(torch.exp(9 * math.log(10) + torch.log(sea_ice_vol) - torch.log(cell_area)
                                                          - torch.log(sea_ice_frac))))


OceanDerivedVariableFunc = Callable[[_OceanData, datetime.timedelta], torch.Tensor]


def _ohc_tendency(d: _OceanData, dt: datetime.timedelta) -> torch.Tensor:
    ohc = d.ocean_heat_content
    out = torch.zeros_like(ohc)
    out[:, 1:] = torch.diff(ohc, n=1, dim=1) / dt.total_seconds()
    return out


# name -> (function, metadata, exists_ok) in the reference's registration order (ocean_derived_variables.py:128-210); the order is
# bit i of the kernel's `want` and slot i of its `out` (ace_amd/_lib.py: OCEAN_DERIVE_OUTPUTS)
_OCEAN_DERIVED_VARIABLE_REGISTRY: MutableMapping[str, Tuple[OceanDerivedVariableFunc, VariableMetadata, bool]] = {
    "ocean_heat_content": (lambda d, dt: d.ocean_heat_content,
                           VariableMetadata("J/m**2", "Column-integrated ocean heat content"), False),
    "ocean_heat_content_tendency": (_ohc_tendency,
                                    VariableMetadata("W/m**2", "Tendency of column-integrated ocean heat content"), False),
    "implied_tendency_of_ocean_heat_content_due_to_advection": (
        lambda d, dt: _ohc_tendency(d, dt) - d.net_energy_flux_into_ocean,       # residual of the column's energy budget
        VariableMetadata("W/m**2", "Implied advective tendency of ocean heat content assuming closed budget"), False),
    "net_energy_flux_into_ocean_column": (lambda d, dt: d.net_energy_flux_into_ocean,
                                          VariableMetadata("W/m**2", "Net energy flux through surface and sea floor into ocean"), False),
    "sea_ice_fraction": (lambda d, dt: oc.sea_ice_fraction(d.data), VariableMetadata("[0-1]", "sea ice concentration"), True),
    "HI": (lambda d, dt: d.sea_ice_thickness, VariableMetadata("m", "Sea ice thickness"), True),
    "hfds": (lambda d, dt: oc.net_downward_surface_heat_flux(d.data), VariableMetadata("W/m**2", "Surface ocean heat flux"), True),
}


def get_ocean_derived_variable_metadata() -> Dict[str, VariableMetadata]:
    return {label: metadata for label, (_, metadata, _) in _OCEAN_DERIVED_VARIABLE_REGISTRY.items()}


def _exists_error(label: str) -> ValueError:
    return ValueError(f"Variable {label} already exists. It is not permitted to have derived variables with same name as "
                      "existing variables unless the derived variable is registered with exists_ok=True.")


def _compute_ocean_derived_variable(data: TensorDict, depth_coordinate, timestep: datetime.timedelta, label: str,
                                    func: OceanDerivedVariableFunc, forcing_data: Optional[TensorMapping] = None,
                                    exists_ok: bool = False, cell_area_provider=None) -> TensorDict:
    """ocean_derived_variables.py:40-101"""
    new_data = data.copy()
    if label in new_data:
        if exists_ok:
            return new_data
        raise _exists_error(label)
    if forcing_data is not None:
        for key, value in forcing_data.items():
            if key not in data:
                data[key] = value
    try:
        output = func(_OceanData(data, depth_coordinate, cell_area_provider), timestep)
    except KeyError:
        return new_data
    new_data[label] = output
    return new_data


def compute_ocean_derived_quantities(data: TensorDict, depth_coordinate, timestep: datetime.timedelta,
                                     forcing_data: Optional[TensorMapping] = None, cell_area_provider=None) -> TensorDict:
    """ocean_derived_variables.py:104-125: every registered variable, in registration order.  A forcing name takes part in the
    computation but is not in the result, except as the value of an ``exists_ok`` variable that it is."""
    for label, (func, _, exists_ok) in _OCEAN_DERIVED_VARIABLE_REGISTRY.items():
        data = _compute_ocean_derived_variable(data, depth_coordinate, timestep, label, func, forcing_data=forcing_data,
                                               exists_ok=exists_ok, cell_area_provider=cell_area_provider)
    return data


# ---------------------------------------------------------------------------------------------------------------------
# the fused path: the same rules decided from the names alone, then one launch
# descriptor slot -> the standard name ``OceanData`` resolves it by (ocean_corrector.OCEAN_FIELD_NAME_PREFIXES)
_FIELDS = {"hfds": "net_downward_surface_heat_flux", "hfds_total_area": "net_downward_surface_heat_flux_total_area",
           "hfgeou": "geothermal_heat_flux", "sea_surface_fraction": "sea_surface_fraction", "land_fraction": "land_fraction",
           "ocean_sea_ice_fraction": "ocean_sea_ice_fraction", "sea_ice_fraction": "sea_ice_fraction",
           "sea_ice_volume": "sea_ice_volume"}
# ``exists_ok`` variable -> the standard name of the field it is when that field exists
_EXISTING = {"sea_ice_fraction": "sea_ice_fraction", "HI": "sea_ice_thickness", "hfds": "net_downward_surface_heat_flux"}


@dataclasses.dataclass
class _Plan:
    want: List[str]              # computed by the kernel, in registry order
    alias: Dict[str, str]        # ``exists_ok`` variables that are a forcing field: variable -> the field returned as it
    thetao: List[str]            # level names, where a heat-content variable is wanted
    fields: Dict[str, str]       # descriptor slot -> the name of the surface field present among data and forcing


def _plan(data_names, forcing_names, have_depth: bool, have_area: bool) -> _Plan:
    """What ``compute_ocean_derived_quantities`` would compute, skip or refuse on fields of these names, in registry order; the
    names resolved as ``OceanData`` resolves them (``ocean_corrector._name`` / ``level_names``)."""
    merged = set(data_names) | set(forcing_names)
    name = lambda standard: oc._name(merged, standard)                                        # noqa: E731
    has = lambda standard: name(standard) is not None                                         # noqa: E731
    ssf = has("sea_surface_fraction") or has("land_fraction")
    hfds = has("net_downward_surface_heat_flux") or (has("net_downward_surface_heat_flux_total_area") and ssf)
    net = hfds and ssf

    def thetao() -> Optional[List[str]]:
        if not have_depth:
            raise ValueError("Depth coordinate must be provided to compute column-integrated ocean heat content.")
        try:
            return level_names(merged, "sea_water_potential_temperature")
        except KeyError:
            return None

    plan = _Plan([], {}, [], {slot: name(std) for slot, std in _FIELDS.items() if has(std)})
    for label, (_, _, exists_ok) in _OCEAN_DERIVED_VARIABLE_REGISTRY.items():
        if label in data_names:
            if exists_ok:
                continue
            raise _exists_error(label)
        existing = name(_EXISTING[label]) if exists_ok else None
        if existing is not None:
            plan.alias[label] = existing
            continue
        if label == "ocean_heat_content" or label == "ocean_heat_content_tendency":
            ok = thetao() is not None
        elif label == "implied_tendency_of_ocean_heat_content_due_to_advection":
            ok = thetao() is not None and net
        elif label == "net_energy_flux_into_ocean_column":
            ok = net
        elif label == "sea_ice_fraction":
            ok = has("ocean_sea_ice_fraction") and has("land_fraction")
        elif label == "HI":
            ok = ssf and has("sea_ice_volume") and (has("ocean_sea_ice_fraction")
                                                    or (has("land_fraction") and has("sea_ice_fraction")))
            if ok and not have_area:
                raise ValueError("A cell area provider must be provided to access cell area information.")
        else:
            ok = hfds
        if ok:
            plan.want.append(label)
    if any(n.startswith("ocean_heat_content") or n.startswith("implied_") for n in plan.want):
        plan.thetao = thetao()
    return plan


class OceanDeriveFn:
    """coordinates.py:75-109, with the choice of path: ``fused=False`` the torch ops, ``fused=True`` the HIP launch (needs the built
    library and float32 CUDA tensors), ``None`` the launch whenever both hold - every field of the call float32 on one CUDA device
    - and the torch path otherwise.

    The fused path writes each derived variable to a tensor of its own, so keeping one keeps only that one alive.  ``window``
    equals the concatenation path (``stepper.derive_by_concatenation``) in every corner: a thetao level that comes from the forcing
    takes its head from the forcing's time level ``n_ic - 1``, and a derived name that the forcing holds is left out of the result."""

    def __init__(self, depth_coordinate: Optional[DepthCoordinate], timestep: datetime.timedelta, horizontal_coordinates=None,
                 fused: Optional[bool] = None):
        self.depth_coordinate = depth_coordinate
        self.timestep = timestep
        self.horizontal_coordinates = horizontal_coordinates
        self.fused = fused
        self.t_chunk = 0                                   # 0: chosen by the library (the result does not depend on it)
        self.launches = 0                                  # launches made by the fused path (the route query)
        # the cell areas, evaluated once (``LatLonGrid.area_weights_m2`` recomputes them on every access) and kept per device
        area = getattr(horizontal_coordinates, "area_weights_m2", None) if horizontal_coordinates is not None else None
        self._area: Dict[str, Any] = {} if area is None else {"cpu": types.SimpleNamespace(area_weights_m2=torch.as_tensor(area).detach().cpu())}
        self._static: Dict[str, Tuple[Optional[torch.Tensor], ...]] = {}
        self._depth_on: Dict[str, DepthCoordinate] = {}
        self._plans: Dict[Tuple, Tuple[_Plan, "ctypes.Structure"]] = {}

    # ---- which path --------------------------------------------------------------------------------------------------
    def _use_fused(self, data: TensorMapping, *others: Optional[TensorMapping]) -> bool:
        from . import _lib
        if self.fused is False:
            return False
        cuda = all(v.is_cuda for v in data.values()) and len(data) > 0
        built = os.path.exists(_lib.LIB_PATH)
        if self.fused is None and cuda:                    # what the launch takes: everything float32 on the data's device
            device = next(iter(data.values())).device
            cuda = all(v.dtype == torch.float32 and v.device == device for d in (data,) + others if d for v in d.values())
        if self.fused:
            if not cuda:
                raise RuntimeError("OceanDeriveFn(fused=True) needs the window on an MI355X (got a CPU tensor); use fused=False "
                                   "for the torch path")
            _lib.lib()                                     # raises AceLibraryMissing when the library has not been built
            return True
        return cuda and built

    def _area_provider(self, device="cpu"):
        """the cell areas on ``device`` as a cell-area provider, or None"""
        if not self._area:
            return None
        key = str(device)
        if key not in self._area:
            self._area[key] = types.SimpleNamespace(area_weights_m2=self._area["cpu"].area_weights_m2.to(device))
        return self._area[key]

    # ---- the torch path ------------------------------------------------------------------------------------------------
    def _torch(self, data: TensorMapping, forcing_data: TensorMapping) -> TensorDict:
        depth = self.depth_coordinate
        if depth is not None:
            dev = str(next(iter(data.values())).device)
            if dev not in self._depth_on:
                self._depth_on[dev] = depth.to(dev)
            depth = self._depth_on[dev]
        return compute_ocean_derived_quantities(dict(data), depth, self.timestep, forcing_data=dict(forcing_data),
                                                cell_area_provider=self._area_provider(next(iter(data.values())).device))

    # ---- the HIP path --------------------------------------------------------------------------------------------------
    def _static_planes(self, device, shape):
        """dz (L, H, W), mask0 (H, W) and area_m2 (H, W) as contiguous fp32 on ``device``, uploaded once"""
        key = f"{device}:{shape}"
        if key not in self._static:
            H, W = shape
            dz = mask0 = area = None
            depth = self.depth_coordinate
            if depth is not None:
                L = depth.nlev
                dz = depth.dz.detach().to(torch.float32).expand(H, W, L).permute(2, 0, 1).contiguous().to(device)
                mask0 = depth.mask.detach().to(torch.float32).select(-1, 0).expand(H, W).contiguous().to(device)
            provider = self._area_provider(device)
            if provider is not None:
                area = provider.area_weights_m2.to(torch.float32).expand(H, W).contiguous()
            self._static[key] = (dz, mask0, area)
        return self._static[key]

    @staticmethod
    def _plane(t: torch.Tensor, name: str, device, shape, steps: int, first: int = 0):
        """(tensor kept alive, address of step ``first``, sample stride, step stride) of a (B, >= first + steps, H, W) field"""
        B, H, W = shape
        if t.dtype != torch.float32 or t.device != device:
            raise TypeError(f"fused ocean derive: '{name}' must be float32 on {device}, got {t.dtype} on {t.device}")
        if t.dim() != 4 or t.shape[0] != B or tuple(t.shape[-2:]) != (H, W) or t.shape[1] < first + steps:
            raise ValueError(f"fused ocean derive: '{name}' must be ({B}, >= {first + steps}, {H}, {W}), got {tuple(t.shape)}")
        if t.stride(-1) != 1 or t.stride(-2) != W:
            t = t.contiguous()
        return t, t.data_ptr() + 4 * first * t.stride(1), t.stride(0), t.stride(1)

    def _fused(self, data: TensorMapping, forcing: TensorMapping, head: Optional[TensorMapping], first: int, steps: int,
               keep_alias: bool) -> TensorDict:
        from . import _lib
        from ._lib import OCEAN_DERIVE_OUTPUTS, OCEAN_MAX_LEVELS, OceanDeriveDesc
        depth = self.depth_coordinate
        any_t = next(iter(data.values()))
        device, B, (H, W) = any_t.device, any_t.shape[0], tuple(any_t.shape[-2:])
        key = (str(device), tuple(data), tuple(forcing), None if head is None else tuple(head))
        cached = self._plans.get(key)
        if cached is None:
            cached = self._plans[key] = (_plan(list(data), list(forcing), depth is not None, bool(self._area)), OceanDeriveDesc())
        plan, d = cached
        out = dict(data)
        if keep_alias:
            for label, field in plan.alias.items():
                out[label] = forcing[field]
        # the concatenation path leaves a derived name that the forcing holds out of its result
        want = [label for label in plan.want if keep_alias or label not in forcing]
        if not want:
            return out
        if plan.thetao:
            if len(plan.thetao) != depth.nlev:
                raise ValueError("The last dimension of integrand must match the number of vertical layers in the depth vertical "
                                 f"coordinate. Got {len(plan.thetao)} thetao levels and idepth.shape: {tuple(depth.idepth.shape)}.")
            if depth.nlev > OCEAN_MAX_LEVELS:
                raise NotImplementedError(f"the fused ocean derive supports up to {OCEAN_MAX_LEVELS} depth levels, got {depth.nlev}")
        dz, mask0, area = self._static_planes(device, (H, W))
        keep = []

        def resolve(name):
            if name in data:
                return self._plane(data[name], name, device, (B, H, W), steps)
            return self._plane(forcing[name], name, device, (B, H, W), steps, first)

        d.nlev = len(plan.thetao)
        for k, name in enumerate(plan.thetao):
            t, p, sb, st = resolve(name)
            keep.append(t)
            lev = d.thetao[k]
            lev.f.base, lev.f.bstride, lev.f.tstride = p, sb, st
            lev.head, lev.head_bstride = None, 0
            # the time level before step 0: the last initial time level of a generated field, the forcing's own of a forcing field
            h = None if head is None else (head.get(name) if name in data else forcing[name][:, :first])
            if h is not None:
                ht, hp, hsb, _ = self._plane(h, name, device, (B, H, W), 1, h.shape[1] - 1)
                keep.append(ht)
                lev.head, lev.head_bstride = hp, hsb
        d.dz = dz.data_ptr() if dz is not None else None
        d.mask0 = mask0.data_ptr() if mask0 is not None else None
        d.area_m2 = area.data_ptr() if area is not None else None
        for slot in _FIELDS:
            f = getattr(d, slot)
            f.base, f.bstride, f.tstride = None, 0, 0
            if slot in plan.fields:
                t, p, sb, st = resolve(plan.fields[slot])
                keep.append(t)
                f.base, f.bstride, f.tstride = p, sb, st
        d.want = 0
        for i in range(len(OCEAN_DERIVE_OUTPUTS)):
            d.out[i] = None
        for label in want:                                 # a tensor of its own per variable: keeping one keeps only that one
            i = OCEAN_DERIVE_OUTPUTS.index(label)
            out[label] = torch.empty((B, steps, H, W), dtype=torch.float32, device=device)
            d.want |= 1 << i
            d.out[i] = out[label].data_ptr()
        d.out_bstride, d.out_tstride = steps * H * W, H * W
        d.has_head = int(head is not None)
        d.dt_seconds = self.timestep.total_seconds()
        d.batch, d.steps, d.hw, d.t_chunk = B, steps, H * W, int(self.t_chunk)
        with torch.cuda.device(device):
            rc = _lib.lib().ace_ocean_derive_window(ctypes.byref(d), torch.cuda.current_stream(device).cuda_stream)
        _lib.check(rc, "ocean_derive")
        self.launches += 1
        del keep                                          # the launch is enqueued on the tensors' own stream: a copy made above may go
        return out

    # ---- the interface -------------------------------------------------------------------------------------------------
    def __call__(self, data: TensorMapping, forcing_data: TensorMapping) -> TensorDict:
        """The reference's signature: every time level of ``data`` against the same time levels of ``forcing_data``; the tendency
        of the first time level is zero."""
        if not self._use_fused(data, forcing_data):
            return self._torch(data, forcing_data)
        steps = next(iter(data.values())).shape[1]
        return self._fused(data, forcing_data, None, 0, steps, keep_alias=True)

    def window(self, data: TensorDict, initial_condition: TensorMapping, forcing: TensorMapping, n_ic: int,
               n_forward_steps: int) -> TensorDict:
        """``stepper.derive_over_window`` without the concatenation: the generated steps of ``data`` against the forcing's time
        levels ``n_ic ..``, the tendency of the first step taken against the initial condition (a level it does not hold is NaN
        there, that is nothing in the column sum; a level that is a forcing field is taken at the forcing's time level
        ``n_ic - 1``)."""
        if not self._use_fused(data, forcing, {k: v for k, v in initial_condition.items() if k in data}):
            from .stepper import derive_by_concatenation
            return derive_by_concatenation(self, data, initial_condition, forcing, n_ic, n_forward_steps)
        f = {k: v[:, : n_ic + n_forward_steps] for k, v in forcing.items()}
        return self._fused(data, f, initial_condition, n_ic, n_forward_steps, keep_alias=False)
