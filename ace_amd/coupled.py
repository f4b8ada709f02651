"""The coupled atmosphere-ocean stepper (fme/coupled/stepper.py): the SFNO atmosphere stepper and the Samudra ocean stepper run
together, the atmosphere ``n_inner = ocean_timestep // atmosphere_timestep`` steps per ocean step.

One coupled step (``CoupledStepper.predict_generator``, stepper.py:1150-1292):
  1. ocean -> atmosphere (``Coupler.atmosphere_forcings``; _get_atmosphere_forcings, 1020-1101): the ocean's current state as the
     atmosphere's forcings, constant over the n_inner + 1 time levels of the window; the ocean fraction either carried over from
     the atmosphere forcing or computed from the ocean's sea-ice fraction and the land fraction; every ocean-supplied field 0
     where the ocean's mask of its name is 0;
  2. the atmosphere's initial surface temperature overwritten by the atmosphere ``ocean`` config's prescriber (986-1018);
  3. n_inner atmosphere steps, each yielded;
  4. atmosphere -> ocean (``Coupler.ocean_forcings``; _get_ocean_forcings, 1103-1148): time means of generated fields and of
     shared exogenous forcings in a two-level ocean forcing window, ``[NaN, mean]`` for a next-step forcing, else ``[mean, NaN]``;
  5. one ocean step, yielded; both states are the next coupled step's initial conditions.

``Coupler`` has two paths computing the same thing, as the evaluator has: ``fused=False`` is the reference's formulas in torch ops
on any device; on CUDA fp32 (the default there) the exchange is two native calls per coupled step (csrc/coupler.hip).  The
ocean -> atmosphere products are bitwise the torch path's.  The means differ by rounding only: the kernel accumulates in fp64 and
rounds once, the reference's fp32 ``mean`` rounds at every addition.

The coupled rollout on static windows with graph capture is ``CoupledRolloutEngine`` (coupled_rollout.py).  Not here
(follow-ups): a coupled inference loop, aggregators, training, ensembles."""
import dataclasses
import datetime
import functools
import pathlib
import re
from collections.abc import Generator, Iterable, Mapping
from typing import Any, Dict, List, Optional, Tuple, Union

import torch
from torch import nn

from ._lib import check
from .ocean import Prescriber
from .ocean_corrector import OCEAN_FIELD_NAME_PREFIXES
from .ocean_derived_variables import OceanDeriveFn
from .stepper import PrognosticState, Stepper, derive_over_window

TensorMapping = Mapping[str, torch.Tensor]
TensorDict = Dict[str, torch.Tensor]

MAX_NAMES = 64          # ACE_COUPLE_MAX_NAMES (include/ace_sfno.h)
OFRAC_CARRIED, OFRAC_FROM_SIF, OFRAC_FROM_OCEAN_SIF = 0, 1, 2


# ---- durations ------------------------------------------------------------------------------------------------------------
_ISO = re.compile(r"^P(?:(?P<W>\d+(?:\.\d+)?)W)?(?:(?P<D>\d+(?:\.\d+)?)D)?"
                  r"(?:T(?:(?P<H>\d+(?:\.\d+)?)H)?(?:(?P<M>\d+(?:\.\d+)?)M)?(?:(?P<S>\d+(?:\.\d+)?)S)?)?$")
_UNIT_SECONDS = {"w": 604800.0, "d": 86400.0, "day": 86400.0, "days": 86400.0, "h": 3600.0, "hr": 3600.0, "hour": 3600.0,
                 "hours": 3600.0, "min": 60.0, "minute": 60.0, "minutes": 60.0, "t": 60.0, "m": 60.0, "s": 1.0, "sec": 1.0,
                 "second": 1.0, "seconds": 1.0, "ms": 1e-3, "us": 1e-6}
_TERM = re.compile(r"\s*(\d+(?:\.\d+)?)\s*([A-Za-z]+)")


def _parse_timedelta_plain(text: str) -> datetime.timedelta:
    """ISO-8601 durations (``P5D``, ``PT6H``) and pandas-style ones (``5D``, ``6h``, ``1D12h``) without pandas."""
    s = text.strip()
    m = _ISO.match(s.upper()) if s[:1] in "Pp" else None
    if m is not None and any(m.groupdict().values()):
        g = {k: float(v) if v else 0.0 for k, v in m.groupdict().items()}
        return datetime.timedelta(weeks=g["W"], days=g["D"], hours=g["H"], minutes=g["M"], seconds=g["S"])
    seconds, pos = 0.0, 0
    while pos < len(s):
        t = _TERM.match(s, pos)
        if t is None or t.group(2).lower() not in _UNIT_SECONDS:
            raise ValueError(f"unit abbreviation w/o a number or unknown duration: {text!r}")
        seconds += float(t.group(1)) * _UNIT_SECONDS[t.group(2).lower()]
        pos = t.end()
    if pos == 0:
        raise ValueError(f"unknown duration: {text!r}")
    return datetime.timedelta(seconds=seconds)


def parse_timedelta(value: Union[str, datetime.timedelta]) -> datetime.timedelta:
    """``pd.Timedelta(value).to_pytimedelta()`` (stepper.py:291-294); the plain parser when pandas is not importable."""
    if isinstance(value, datetime.timedelta):
        return value
    try:
        import pandas as pd
    except ImportError:
        return _parse_timedelta_plain(value)
    return pd.Timedelta(value).to_pytimedelta()


# ---- configuration --------------------------------------------------------------------------------------------------------
def step_config_from_stepper_state(cfg: Mapping[str, Any]):
    """The ``SingleModuleStepConfig`` of a serialized ``StepperConfig`` (new format ``{"step": {"type", "config"}, ...}``,
    possibly ``multi_call``-wrapped, or the legacy flat one) - for its names; the normalisation statistics are not read."""
    from .registry import ModuleSelector
    from .step import NormalizationConfig, SingleModuleStepConfig
    if "step" in cfg:
        sel = cfg["step"]
        step_type, c = sel["type"], dict(sel["config"])
        if step_type == "multi_call":
            inner = c["wrapped_step"]
            step_type, c = inner["type"], dict(inner["config"])
        if step_type not in ("single_module", "default"):
            raise NotImplementedError(f"step type '{step_type}' is outside the accelerated hot path")
    else:
        c = dict(cfg)
    builder = c["builder"]
    known = {f.name for f in dataclasses.fields(SingleModuleStepConfig)}
    drop = ("normalization", "builder", "global_mean_removal", "input_dropout", "include_channel_mask_inputs")   # no name set reads them
    c = {k: v for k, v in c.items() if k in known and k not in drop}
    return SingleModuleStepConfig(builder=ModuleSelector(type=builder["type"], config=dict(builder.get("config", {}))),
                                  normalization=NormalizationConfig(means={}, stds={}), **c)


@dataclasses.dataclass
class ComponentConfig:
    """stepper.py:69-82.  ``stepper``: the component's ``SingleModuleStepConfig`` (``Stepper.config``) or a serialized
    ``StepperConfig`` state, kept as given for ``get_state``."""
    timedelta: str
    stepper: Any

    def __post_init__(self):
        self._state = None
        if isinstance(self.stepper, Mapping):
            self._state = self.stepper
            self.stepper = step_config_from_stepper_state(self.stepper)

    def get_state(self) -> Dict[str, Any]:
        stepper = self._state if self._state is not None else dataclasses.asdict(self.stepper)
        return {"timedelta": self.timedelta, "stepper": stepper}


@dataclasses.dataclass
class CoupledOceanFractionConfig:
    """stepper.py:85-186: the ocean fraction computed from the ocean-predicted sea-ice fraction and the land fraction."""
    sea_ice_fraction_name: str
    land_fraction_name: str
    sea_ice_fraction_name_in_atmosphere: Optional[str] = None

    def __post_init__(self):
        self.canonical_sea_ice_fraction_name()

    def canonical_sea_ice_fraction_name(self) -> str:
        name = self.sea_ice_fraction_name
        if name in OCEAN_FIELD_NAME_PREFIXES["sea_ice_fraction"]:
            return "sea_ice_fraction"
        if name in OCEAN_FIELD_NAME_PREFIXES["ocean_sea_ice_fraction"]:
            return "ocean_sea_ice_fraction"
        raise ValueError(f"CoupledOceanFractionConfig expected {name} to be "
                         "registered in OCEAN_FIELD_NAME_PREFIXES as a sea ice fraction.")

    @property
    def atmosphere_sea_ice_fraction_name(self) -> str:
        return self.sea_ice_fraction_name_in_atmosphere or self.sea_ice_fraction_name

    def validate_ocean_prognostic_names(self, prognostic_names: Iterable[str]):
        if self.sea_ice_fraction_name not in prognostic_names:
            raise ValueError(f"CoupledOceanFractionConfig expected {self.sea_ice_fraction_name} "
                             "to be a prognostic variable of the ocean model, but it is not.")

    def validate_atmosphere_forcing_names(self, forcing_names: Iterable[str]):
        if self.land_fraction_name not in forcing_names:
            raise ValueError(f"CoupledOceanFractionConfig expected {self.land_fraction_name} "
                             "to be an ML forcing of the atmosphere model, but it is not.")

    def filter_atmosphere_forcing_names(self, unfiltered_names: Iterable[str], ocean_fraction_name: str) -> List[str]:
        drop = {ocean_fraction_name, self.atmosphere_sea_ice_fraction_name}
        return [n for n in unfiltered_names if n not in drop]


def _input_only(step_config) -> set:
    return set(step_config.input_names) - set(step_config.output_names)


def _all_names(step_config) -> set:
    return set(step_config.input_names).union(step_config.output_names)


@dataclasses.dataclass
class CoupledStepperConfig:
    """stepper.py:238-739: the name sets of the exchange and the validation of the two component configurations."""
    ocean: ComponentConfig
    atmosphere: ComponentConfig
    sst_name: str = "sst"
    ocean_fraction_prediction: Optional[CoupledOceanFractionConfig] = None

    def __post_init__(self):
        if isinstance(self.ocean, Mapping):
            self.ocean = ComponentConfig(**self.ocean)
        if isinstance(self.atmosphere, Mapping):
            self.atmosphere = ComponentConfig(**self.atmosphere)
        if isinstance(self.ocean_fraction_prediction, Mapping):
            self.ocean_fraction_prediction = CoupledOceanFractionConfig(**self.ocean_fraction_prediction)
        self._validate_component_configs()
        self._ocean_timestep = parse_timedelta(self.ocean.timedelta)
        self._atmosphere_timestep = parse_timedelta(self.atmosphere.timedelta)
        self.validate_prescribed_prognostic_names()

    # -- the exchange's name sets, computed from the current component configs (an inference-time override shows at once)
    @property
    def atmosphere_ocean_config(self):
        """The OceanConfig defined in the atmosphere's step config."""
        return self.atmosphere.stepper.ocean

    @property
    def ocean_fraction_name(self) -> str:
        return self.atmosphere_ocean_config.ocean_fraction_name

    @property
    def surface_temperature_name(self) -> str:
        return self.atmosphere_ocean_config.surface_temperature_name

    @property
    def timestep(self) -> datetime.timedelta:
        return self._ocean_timestep

    @property
    def ocean_timestep(self) -> datetime.timedelta:
        return self._ocean_timestep

    @property
    def atmosphere_timestep(self) -> datetime.timedelta:
        return self._atmosphere_timestep

    @property
    def n_inner_steps(self) -> int:
        return self.ocean_timestep // self.atmosphere_timestep

    @property
    def ocean_next_step_forcing_names(self) -> List[str]:
        return list(self.ocean.stepper.next_step_forcing_names)

    @property
    def ocean_forcing_exogenous_names(self) -> List[str]:
        """Ocean forcing variables that are not outputs of the atmosphere."""
        return list(_input_only(self.ocean.stepper).difference(self.atmosphere.stepper.output_names))

    @property
    def atmosphere_forcing_exogenous_names(self) -> List[str]:
        """Atmosphere forcing variables that are not outputs of the ocean (nor computed from them)."""
        names = list(_input_only(self.atmosphere.stepper).difference(self.ocean.stepper.output_names))
        if self.ocean_fraction_prediction is not None:
            names = self.ocean_fraction_prediction.filter_atmosphere_forcing_names(names, self.ocean_fraction_name)
        return names

    @property
    def shared_forcing_exogenous_names(self) -> List[str]:
        return list(set(self.ocean_forcing_exogenous_names).intersection(self.atmosphere_forcing_exogenous_names))

    @property
    def atmosphere_to_ocean_forcing_names(self) -> List[str]:
        return list(_input_only(self.ocean.stepper).intersection(self.atmosphere.stepper.output_names))

    @property
    def ocean_to_atmosphere_forcing_names(self) -> List[str]:
        extra = [self.sst_name]
        if self.ocean_fraction_prediction is not None:
            extra.append(self.ocean_fraction_prediction.sea_ice_fraction_name)
        return list(_input_only(self.atmosphere.stepper).intersection(self.ocean.stepper.output_names).union(extra))

    @property
    def atmosphere_forcing_window_names(self) -> List[str]:
        prescribed = self.atmosphere.stepper.prescribed_prognostic_names
        return list(set(self.atmosphere_forcing_exogenous_names).union(prescribed))

    @property
    def ocean_forcing_window_names(self) -> List[str]:
        prescribed = self.ocean.stepper.prescribed_prognostic_names
        return list(set(self.ocean_forcing_exogenous_names).difference(self.shared_forcing_exogenous_names).union(prescribed))

    def _ocean_supplied_atmosphere_names(self) -> set:
        names = set(self.ocean_to_atmosphere_forcing_names)
        names.discard(self.sst_name)
        names.add(self.surface_temperature_name)
        names.add(self.ocean_fraction_name)
        if self.ocean_fraction_prediction is not None:
            names.add(self.ocean_fraction_prediction.atmosphere_sea_ice_fraction_name)
        return names

    def validate_prescribed_prognostic_names(self) -> None:
        """stepper.py:388-405; called again after an inference-time override of ``prescribed_prognostic_names``."""
        prescribed = self.atmosphere.stepper.prescribed_prognostic_names
        clobbered = sorted(set(prescribed) & self._ocean_supplied_atmosphere_names())
        if clobbered:
            raise ValueError("Atmosphere prescribed_prognostic_names overlap ocean-supplied "
                             f"forcings and would be overwritten: {clobbered}.")

    def _validate_component_configs(self):
        """stepper.py:524-602."""
        ocean, atmosphere = self.ocean.stepper, self.atmosphere.stepper
        if atmosphere.ocean is None:
            raise ValueError("The atmosphere stepper 'ocean' config is missing but must be set for coupled emulation.")
        if atmosphere.ocean.is_slab:
            raise ValueError("The atmosphere stepper 'ocean' config cannot use 'slab' for coupled emulation.")
        ocean_timestep = parse_timedelta(self.ocean.timedelta)
        atmosphere_timestep = parse_timedelta(self.atmosphere.timedelta)
        if atmosphere_timestep > ocean_timestep:
            raise ValueError("Atmosphere timedelta must not be larger than ocean's.")
        n_inner_steps = ocean_timestep / atmosphere_timestep
        if n_inner_steps != int(n_inner_steps):
            raise ValueError("Ocean timedelta must be a multiple of the atmosphere's.")
        duplicate_outputs = set(ocean.output_names).intersection(atmosphere.output_names)
        if len(duplicate_outputs) > 0:
            raise ValueError("Output variable names of CoupledStepper components cannot "
                             f"overlap. Found the following duplicated names: {duplicate_outputs}")
        ocean_diags_as_atmos_forcings = list(
            _input_only(atmosphere).intersection(ocean.output_names).difference(ocean.input_names))
        if len(ocean_diags_as_atmos_forcings) > 0:
            raise ValueError("CoupledStepper only supports ocean prognostic variables as atmosphere "
                             "forcings, but the following ocean diagnostic variables are inputs to "
                             f"the atmosphere: {ocean_diags_as_atmos_forcings}.")
        atmosphere_to_ocean = _input_only(ocean).intersection(atmosphere.output_names)
        missing_next_step_forcings = list(atmosphere_to_ocean.difference(ocean.next_step_forcing_names))
        if len(missing_next_step_forcings) > 0:
            raise ValueError("The following variables which are atmosphere component outputs "
                             "and ocean component inputs were not found among the ocean's "
                             f"next_step_forcing_names: {missing_next_step_forcings}.")
        if self.sst_name not in ocean.output_names:
            raise ValueError(f"The variable {self.sst_name} is not in the ocean's output "
                             "names but is required for coupling with the atmosphere.")
        if self.ocean_fraction_prediction is not None:
            self.ocean_fraction_prediction.validate_ocean_prognostic_names(ocean.prognostic_names)
            self.ocean_fraction_prediction.validate_atmosphere_forcing_names(_input_only(atmosphere))

    def get_state(self) -> Dict[str, Any]:
        ofp = self.ocean_fraction_prediction
        return {"ocean": self.ocean.get_state(), "atmosphere": self.atmosphere.get_state(), "sst_name": self.sst_name,
                "ocean_fraction_prediction": dataclasses.asdict(ofp) if ofp is not None else None}

    @classmethod
    def from_state(cls, state: Mapping[str, Any]) -> "CoupledStepperConfig":
        state = cls.remove_deprecated_keys(state)
        unknown = set(state) - {f.name for f in dataclasses.fields(cls)}
        if unknown:
            raise ValueError(f'can not match {sorted(unknown)} to any data class field of "CoupledStepperConfig"')
        for key in ("ocean", "atmosphere"):
            extra = set(state[key]) - {"timedelta", "stepper"}
            if extra:
                raise ValueError(f'can not match {sorted(extra)} to any data class field of "ComponentConfig"')
        return cls(**state)

    @classmethod
    def remove_deprecated_keys(cls, state: Mapping[str, Any]) -> Dict[str, Any]:
        """stepper.py:729-739."""
        state_copy = dict(state)
        state_copy.pop("sst_mask_name", None)
        state_copy.pop("parameter_init", None)
        for component_key in ("ocean", "atmosphere"):
            if "loss_contributions" in state_copy[component_key]:
                state_copy[component_key] = {k: v for k, v in state_copy[component_key].items() if k != "loss_contributions"}
        return state_copy


class MissingCoupledDatasetInfo(ValueError):
    def __init__(self, info: str):
        super().__init__(f"Dataset used for initialization is missing required information: {info}")


class CoupledDatasetInfo:
    """fme/coupled/dataset_info.py: the two components' ``DatasetInfo``."""

    def __init__(self, ocean, atmosphere):
        self.ocean = ocean
        self.atmosphere = atmosphere

    @property
    def ocean_spatial_mask_provider(self):
        provider = getattr(self.ocean, "mask_provider", None)
        if provider is None:
            raise MissingCoupledDatasetInfo("ocean_spatial_mask_provider")
        return provider

    def get_state(self) -> Dict[str, Dict[str, Any]]:
        return {"ocean": _dataset_info_state(self.ocean), "atmosphere": _dataset_info_state(self.atmosphere)}

    @classmethod
    def from_state(cls, state: Mapping[str, Mapping[str, Any]]) -> "CoupledDatasetInfo":
        from .checkpoint import dataset_info_from_state
        return cls(ocean=dataset_info_from_state(state["ocean"]), atmosphere=dataset_info_from_state(state["atmosphere"]))


def _dataset_info_state(info) -> Dict[str, Any]:
    """What ``checkpoint.dataset_info_from_state`` reads, in the reference's ``DatasetInfo.get_state`` layout."""
    state: Dict[str, Any] = {"img_shape": list(info.img_shape),
                             "timestep": info.timestep // datetime.timedelta(microseconds=1)}
    hc = info.horizontal_coordinates
    if hc is not None:
        state["horizontal_coordinates"] = {"lat": hc.lat, "lon": hc.lon}
    elif info.area_weights is not None:
        state["gridded_operations"] = {"type": "LatLonOperations", "state": {"area_weights": info.area_weights}}
    vc, depth = info.vertical_coordinate, info.ocean_vertical_coordinate
    if depth is not None:
        state["vertical_coordinate"] = {"idepth": depth.idepth, "mask": depth.mask,
                                        **({"deptho": depth.deptho} if depth.deptho is not None else {})}
    elif vc is not None:
        state["vertical_coordinate"] = {"ak": vc.ak, "bk": vc.bk}
    if info.mask_provider is not None:
        state["mask_provider"] = info.mask_provider.get_state()
    if info.all_labels:
        state["all_labels"] = sorted(info.all_labels)
    return state


# ---- the exchange ---------------------------------------------------------------------------------------------------------
class Coupler:
    """The exchange of one coupled step.  ``fused``: on CUDA the two native calls (fp32 fields, 2-D masks); ``False``: the
    reference's torch ops.  CPU tensors always take the torch ops (there is no CPU kernel)."""

    def __init__(self, config: CoupledStepperConfig, mask_provider, prescriber: Prescriber, img_shape: Tuple[int, int],
                 fused: bool = True):
        self._config = config
        self._mask_provider = mask_provider
        self._prescriber = prescriber
        self._img_shape = (int(img_shape[0]), int(img_shape[1]))
        self.fused = fused
        self._providers: Dict[str, Any] = {}
        self._mask_planes: Dict[Tuple[str, str], Optional[torch.Tensor]] = {}
        self._launches = 0

    def launches(self) -> int:
        """Native calls (``ace_couple_*``) made so far: the route query of the tests and benchmarks."""
        return self._launches

    def route(self, example: torch.Tensor) -> str:
        return "fused" if self.fused and example.device.type == "cuda" else "torch"

    def _provider(self, device):
        key = str(device)
        if key not in self._providers:
            self._providers[key] = self._mask_provider.to(device)
        return self._providers[key]

    # -- ocean -> atmosphere
    def atmosphere_forcings(self, atmos_window: TensorMapping, ocean_state: TensorMapping,
                            atmos_ic: TensorMapping) -> Tuple[TensorDict, PrognosticState]:
        """(the atmosphere's forcing window over the n_inner + 1 time levels with the ocean's fields written over it, the
        atmosphere's initial condition with the prescribed surface temperature).  ``atmos_window``: name -> (B, n_inner + 1, H,
        W); ``ocean_state`` / ``atmos_ic``: name -> (B, 1, H, W)."""
        cfg = self._config
        example = ocean_state[cfg.sst_name]
        if example.shape[1] != 1:
            raise ValueError(f"Ocean initial condition must have 1 timesteps, got {example.shape[1]}.")
        forcing = {k: atmos_window[k] for k in cfg.atmosphere_forcing_window_names}
        if self.route(example) == "fused":
            from_ocean, ts = self._atmosphere_forcings_fused(atmos_window, ocean_state, atmos_ic)
        else:
            from_ocean = self._atmosphere_forcings_torch(atmos_window, ocean_state)
            level0 = {k: v[:, :1] for k, v in from_ocean.items()}
            ts = self._prescriber(level0, atmos_ic, level0)[cfg.surface_temperature_name]
        forcing.update(from_ocean)
        new_ic = PrognosticState({**atmos_ic, cfg.surface_temperature_name: ts})
        new_ic.stepper_state = getattr(atmos_ic, "stepper_state", None)
        return forcing, new_ic

    def _atmosphere_forcings_torch(self, atmos_window: TensorMapping, ocean_state: TensorMapping) -> TensorDict:
        """stepper.py:1020-1094 in its own ops and order."""
        cfg = self._config
        T = cfg.n_inner_steps + 1
        out = {k: ocean_state[k].expand(-1, T, -1, -1) for k in cfg.ocean_to_atmosphere_forcing_names}
        out[cfg.surface_temperature_name] = out.pop(cfg.sst_name)
        ofp = cfg.ocean_fraction_prediction
        if ofp is None:
            out[cfg.ocean_fraction_name] = atmos_window[cfg.ocean_fraction_name]
        else:
            sea_ice = torch.nan_to_num(out[ofp.sea_ice_fraction_name])
            land = atmos_window[ofp.land_fraction_name]
            if ofp.canonical_sea_ice_fraction_name() == "ocean_sea_ice_fraction":
                sea_ice = sea_ice * (1 - land)                       # ocean_data.py:194-201
            out[ofp.atmosphere_sea_ice_fraction_name] = sea_ice
            out[cfg.ocean_fraction_name] = torch.clip(1 - land - sea_ice, min=0)      # ocean_data.py:214-218
        provider = self._provider(next(iter(out.values())).device)
        for name, tensor in out.items():
            mask = provider.get_mask_tensor_for(name)
            if mask is not None:
                out[name] = tensor.where(mask.expand(tensor.shape) != 0, 0)
        return out

    def _mask_plane(self, name: str, device) -> Optional[torch.Tensor]:
        key = (str(device), name)
        if key not in self._mask_planes:
            mask = self._provider(device).get_mask_tensor_for(name)
            if mask is not None:
                if tuple(mask.shape) != self._img_shape:
                    raise NotImplementedError(f"the mask of '{name}' is not a 2-D {self._img_shape} plane: the coupler kernel "
                                              "broadcasts 2-D masks over batch and time only")
                mask = mask.to(torch.float32).contiguous()
            self._mask_planes[key] = mask
        return self._mask_planes[key]

    def _atmosphere_forcings_fused(self, atmos_window, ocean_state, atmos_ic) -> Tuple[TensorDict, torch.Tensor]:
        from . import _lib
        from .aggregator import _flat, _plane_table, _upload
        cfg = self._config
        ofp = cfg.ocean_fraction_prediction
        ts_name, of_name = cfg.surface_temperature_name, cfg.ocean_fraction_name
        sst = ocean_state[cfg.sst_name]
        dev = sst.device
        B, _, H, W = sst.shape
        T = cfg.n_inner_steps + 1
        if (H, W) != self._img_shape:
            raise ValueError(f"fields of {(H, W)} pixels for a coupler of {self._img_shape}")
        # slot -> (source, name of the destination in the atmosphere (None: no destination), its time levels)
        slots: List[Tuple[torch.Tensor, Optional[str], int]] = [(sst, ts_name, 1), (atmos_ic[ts_name], "", 1)]
        if ofp is None:
            mode = OFRAC_CARRIED
            carried = atmos_window[of_name]
            slots.append((carried, of_name if self._mask_plane(of_name, dev) is not None else None, T))
            passed = [n for n in cfg.ocean_to_atmosphere_forcing_names if n != cfg.sst_name]
        else:
            ocean_sif = ofp.canonical_sea_ice_fraction_name() == "ocean_sea_ice_fraction"
            mode = OFRAC_FROM_OCEAN_SIF if ocean_sif else OFRAC_FROM_SIF
            sif, si_name = ocean_state[ofp.sea_ice_fraction_name], ofp.atmosphere_sea_ice_fraction_name
            slots.append((atmos_window[ofp.land_fraction_name], of_name, T))
            slots.append((sif, si_name, T if ocean_sif else 1))
            slots.append((sif, ofp.sea_ice_fraction_name if si_name != ofp.sea_ice_fraction_name else None, 1))
            passed = [n for n in cfg.ocean_to_atmosphere_forcing_names if n not in (cfg.sst_name, ofp.sea_ice_fraction_name)]
        if len(passed) > MAX_NAMES:
            raise ValueError(f"{len(passed)} pass-through fields, the coupler kernel takes {MAX_NAMES}")
        slots += [(ocean_state[n], n, 1) for n in passed]
        for src, _, _ in slots:
            if src.dtype != torch.float32 or src.device != dev:
                raise TypeError("the fused coupler needs fp32 fields on one device (Coupler.fused = False runs the torch ops)")
        levels = [0 if name is None else nt for _, name, nt in slots]
        block = torch.empty(B, sum(levels), H, W, dtype=torch.float32, device=dev)     # one allocation holds every product
        keys = [str(j) for j in range(len(slots))]
        srcs, dsts, masks, at = {}, {}, [], 0
        for key, (src, name, _), nt in zip(keys, slots, levels):
            srcs[key] = _flat(src, W)
            dsts[key] = block[:, at:at + nt] if nt else None
            at += nt
            plane = self._mask_plane(name, dev) if name else None
            masks.append(0 if plane is None else plane.data_ptr())
        values, off = _plane_table(keys, srcs, dsts)
        table = _upload(values + masks, torch.int64, dev)
        base = table.data_ptr()
        with torch.cuda.device(dev):
            rc = _lib.lib().ace_couple_ocean_to_atmosphere(
                base + off["gen"], base + off["gen_strides"], base + off["target"], base + off["target_strides"],
                base + off["end"], len(passed), mode, int(self._prescriber.interpolate), T - 1, B, H * W, _lib.current_stream())
        _check(rc)
        self._launches += 1
        out: TensorDict = {}
        for key, (_, name, _), nt in zip(keys, slots, levels):
            if name:
                out[name] = dsts[key] if nt == T else dsts[key].expand(-1, T, -1, -1)
        if ofp is None and of_name not in out:
            out[of_name] = atmos_window[of_name]
        return out, dsts["1"]

    # -- atmosphere -> ocean
    def ocean_forcings(self, ocean_window: TensorMapping, atmos_steps: List[TensorMapping],
                       atmos_window: TensorMapping) -> TensorDict:
        """The ocean's two-level forcing window.  ``ocean_window``: name -> (B, 2, H, W), the ocean forcing record at this
        coupled step's two time levels; ``atmos_steps``: the n_inner generated atmosphere steps, name -> (B, H, W) each;
        ``atmos_window``: name -> (B, n_inner + 1, H, W), the atmosphere forcing record (shared exogenous forcings are averaged
        over its levels 1 .. n_inner)."""
        cfg = self._config
        n_inner = cfg.n_inner_steps
        if len(atmos_steps) != n_inner:
            raise ValueError(f"{len(atmos_steps)} atmosphere steps for n_inner = {n_inner}")
        forcing = {k: ocean_window[k] for k in cfg.ocean_forcing_window_names}
        generated, shared = cfg.atmosphere_to_ocean_forcing_names, cfg.shared_forcing_exogenous_names
        next_step = set(cfg.ocean_next_step_forcing_names)
        names = list(generated) + [n for n in shared if n not in generated]
        if not names:
            return forcing
        planes = {k: [s[k] for s in atmos_steps] for k in generated}
        planes.update({k: [atmos_window[k][:, 1 + t] for t in range(n_inner)] for k in shared})
        example = planes[names[0]][0]
        if self.route(example) == "fused":
            forcing.update(self._ocean_forcings_fused(names, planes, next_step))
            return forcing
        for k in names:                                              # stepper.py:1127-1146
            v = torch.stack(planes[k], dim=1).mean(1, keepdim=True)
            nan = torch.full_like(v, float("nan"))
            forcing[k] = torch.cat([nan, v], dim=1) if k in next_step else torch.cat([v, nan], dim=1)
        return forcing

    def _ocean_forcings_fused(self, names: List[str], planes: Dict[str, List[torch.Tensor]], next_step: set) -> TensorDict:
        from . import _lib
        from .aggregator import _flat, _plane_table, _upload
        if len(names) > MAX_NAMES:
            raise ValueError(f"{len(names)} averaged fields, the coupler kernel takes {MAX_NAMES}")
        first = planes[names[0]][0]
        dev = first.device
        B, H, W = first.shape
        n_inner = len(planes[names[0]])
        ptrs, strides = [], []
        for k in names:
            for p in planes[k]:
                if p.dtype != torch.float32 or p.device != dev or tuple(p.shape) != (B, H, W):
                    raise TypeError("the fused coupler needs fp32 (B, H, W) fields on one device (Coupler.fused = False runs "
                                    "the torch ops)")
                p = _flat(p, W)
                ptrs.append(p)                                       # a contiguous copy stays alive until the call is enqueued
                strides.append(p.stride(0))
        block = torch.empty(len(names), B, 2, H, W, dtype=torch.float32, device=dev)
        windows = {k: block[i] for i, k in enumerate(names)}
        values, off = _plane_table(names, windows)
        slot_at = off["end"]
        values += [p.data_ptr() for p in ptrs] + strides
        table = _upload(values, torch.int64, dev)
        slot = _upload([1 if k in next_step else 0 for k in names], torch.int32, dev)
        base = table.data_ptr()
        n = len(ptrs)
        with torch.cuda.device(dev):
            rc = _lib.lib().ace_couple_atmosphere_to_ocean(base + slot_at, base + slot_at + 8 * n, base + off["gen"],
                                                           base + off["gen_strides"], slot.data_ptr(), len(names), n_inner, B,
                                                           H * W, _lib.current_stream())
        _check(rc)
        self._launches += 1
        return windows


_check = functools.partial(check, family="couple")


# ---- the coupled stepper --------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class ComponentStepPrediction:
    """stepper.py:842-869: one step of one component."""
    realm: str                  # "atmosphere" or "ocean"
    data: TensorDict            # name -> (B, H, W)
    step: int
    stepper_state: Any = None


class CoupledStepper:
    """stepper.py:872-1439 on plain dicts, built on the two components' ``Stepper.predict_generator``.

    As in the reference (its coupled path calls the components' ``get_prediction_generator``), forcings derived from the time
    axis - the insolation - are NOT computed inside: a caller applies ``stepper.atmosphere.forcing_deriver(forcing, time)`` to
    the atmosphere record beforehand."""
    TIME_DIM = 1

    def __init__(self, config: CoupledStepperConfig, ocean: Stepper, atmosphere: Stepper, dataset_info: CoupledDatasetInfo,
                 fused: bool = True):
        if ocean.n_ic_timesteps != 1 or atmosphere.n_ic_timesteps != 1:
            raise ValueError("Only n_ic_timesteps = 1 is currently supported.")
        self.ocean = ocean
        self.atmosphere = atmosphere
        self._config = config
        # the component configs are the loaded steppers' own, so an inference-time override shows in the name sets (stepper.py:895-899)
        config.ocean.stepper = ocean.config
        config.atmosphere.stepper = atmosphere.config
        config._validate_component_configs()
        config.validate_prescribed_prognostic_names()
        self._dataset_info = dataset_info
        for realm, stepper, want in (("Ocean", ocean, config.ocean_timestep), ("Atmosphere", atmosphere, config.atmosphere_timestep)):
            have = getattr(stepper._dataset_info, "timestep", None)          # stepper.py:664-693
            if have is not None and have != want:
                raise ValueError(f"{realm} timestep must match the dataset timestep. Got {want} and {have}, respectively.")
        shapes =[tuple(getattr(s._dataset_info, "img_shape", ())) for s in (ocean, atmosphere)]
        if shapes[0] and shapes[1] and shapes[0] != shapes[1]:
            raise ValueError(f"the component steppers are on different grids (ocean {shapes[0]}, atmosphere {shapes[1]}): the "
                             "coupled stepper exchanges fields pixel by pixel")
        provider = dataset_info.ocean_spatial_mask_provider           # raises MissingCoupledDatasetInfo without one
        ocean_hook = atmosphere._step_obj._ocean
        self.coupler = Coupler(config, provider, ocean_hook.prescriber, shapes[1] or shapes[0], fused=fused)

    @property
    def config(self) -> CoupledStepperConfig:
        return self._config

    @property
    def modules(self) -> nn.ModuleList:
        return nn.ModuleList([*self.atmosphere.modules, *self.ocean.modules])

    def set_eval(self):
        self.atmosphere.set_eval()
        self.ocean.set_eval()

    @property
    def training_dataset_info(self) -> CoupledDatasetInfo:
        return self._dataset_info

    @property
    def n_ic_timesteps(self) -> int:
        return 1

    @property
    def n_inner_steps(self) -> int:
        """Number of atmosphere steps per ocean step."""
        return self._config.n_inner_steps

    def get_state(self) -> Dict[str, Any]:
        return {"config": self._config.get_state(), "atmosphere_state": self.atmosphere.get_state(),
                "ocean_state": self.ocean.get_state(), "dataset_info": self._dataset_info.get_state()}

    def load_state(self, state: Mapping[str, Any]):
        self.atmosphere.load_state(state["atmosphere_state"])
        self.ocean.load_state(state["ocean_state"])

    @classmethod
    def from_state(cls, state: Mapping[str, Any], device=None, ignore_unsupported: bool = False) -> "CoupledStepper":
        """stepper.py:1421-1439; each component state goes through ``checkpoint.load_stepper``."""
        from .checkpoint import load_stepper
        ocean = load_stepper(state["ocean_state"], device=device, ignore_unsupported=ignore_unsupported)
        atmosphere = load_stepper(state["atmosphere_state"], device=device, ignore_unsupported=ignore_unsupported)
        for realm, loaded in (("ocean", ocean), ("atmosphere", atmosphere)):
            if loaded.stepper.config.global_mean_removal is not None:
                raise NotImplementedError(f"coupled stepper: the {realm} component's step carries global_mean_removal, which the "
                                          "coupled exchange has not been built for; load the component on its own with load_stepper")
        config = CoupledStepperConfig.from_state(state["config"])
        if "dataset_info" in state:
            dataset_info = CoupledDatasetInfo.from_state(state["dataset_info"])
        else:       # backwards compatibility (stepper.py:1426-1433)
            dataset_info = CoupledDatasetInfo(ocean=ocean.dataset_info, atmosphere=atmosphere.dataset_info)
        return cls(config=config, ocean=ocean.stepper, atmosphere=atmosphere.stepper, dataset_info=dataset_info)

    def predict_generator(self, initial_condition: Mapping[str, TensorMapping],
                          forcing: Mapping[str, TensorMapping]) -> Generator[ComponentStepPrediction, None, None]:
        """stepper.py:1150-1292.  ``initial_condition``: {"atmosphere": name -> (B, 1, H, W), "ocean": ...};
        ``forcing``: {"atmosphere": name -> (B, n_outer * n_inner + 1, H, W), "ocean": name -> (B, n_outer + 1, H, W)}.
        Yields the n_inner atmosphere steps of a coupled step, then its ocean step."""
        n_inner = self.n_inner_steps
        atmos_ic, ocean_ic = initial_condition["atmosphere"], initial_condition["ocean"]
        for realm, ic in (("Atmosphere", atmos_ic), ("Ocean", ocean_ic)):
            nt = next(iter(ic.values())).shape[self.TIME_DIM]
            if nt != 1:
                raise ValueError(f"{realm} initial condition must have 1 timesteps, got {nt}.")
        atmos_record, ocean_record = forcing["atmosphere"], forcing["ocean"]
        if ocean_record:
            n_outer = next(iter(ocean_record.values())).shape[self.TIME_DIM] - 1
        else:
            n_outer = (next(iter(atmos_record.values())).shape[self.TIME_DIM] - 1) // n_inner
        for i_outer in range(n_outer):
            atmos_window = {k: v[:, i_outer * n_inner:(i_outer + 1) * n_inner + 1] for k, v in atmos_record.items()}
            atmos_forcings, atmos_ic = self.coupler.atmosphere_forcings(atmos_window, ocean_ic, atmos_ic)
            atmos_steps: List[TensorDict] = []
            atmos_state = getattr(atmos_ic, "stepper_state", None)
            for i_inner, result in enumerate(self.atmosphere.predict_generator(atmos_ic, atmos_forcings, n_inner,
                                                                               stepper_state=atmos_state)):
                atmos_state = result.stepper_state
                yield ComponentStepPrediction("atmosphere", result.output, i_outer * n_inner + i_inner, atmos_state)
                atmos_steps.append(result.output)
            ocean_window = {k: v[:, i_outer:i_outer + 2] for k, v in ocean_record.items()}
            ocean_forcings = self.coupler.ocean_forcings(ocean_window, atmos_steps, atmos_window)
            ocean_result = next(iter(self.ocean.predict_generator(ocean_ic, ocean_forcings, 1,
                                                                  stepper_state=getattr(ocean_ic, "stepper_state", None))))
            yield ComponentStepPrediction("ocean", ocean_result.output, i_outer, ocean_result.stepper_state)
            atmos_ic = _prognostic_state(atmos_steps[-1], self.atmosphere.prognostic_names, atmos_state)
            ocean_ic = _prognostic_state(ocean_result.output, self.ocean.prognostic_names, ocean_result.stepper_state)

    def predict(self, initial_condition: Mapping[str, TensorMapping], forcing: Mapping[str, TensorMapping],
                compute_derived_variables: bool = False) -> Tuple[Dict[str, TensorDict], Dict[str, PrognosticState]]:
        """stepper.py:1388-1409: ({"atmosphere": name -> (B, n_outer * n_inner, H, W), "ocean": name -> (B, n_outer, H, W)},
        the final state).  The state - a ``PrognosticState`` per realm carrying the component's ``stepper_state`` - can be fed
        back as the next window's ``initial_condition``.  ``compute_derived_variables``: each realm's, as ``Stepper.predict``
        computes them with the component's ``derive_func``: the atmosphere's on its hybrid sigma-pressure coordinate, the ocean's
        (ocean heat content and its budget, sea-ice thickness, ...) on its depth coordinate, the first step's tendencies taken
        against the initial condition."""
        with torch.no_grad():
            outs = list(self.predict_generator(initial_condition, forcing))
        data: Dict[str, TensorDict] = {}
        state: Dict[str, PrognosticState] = {}
        for realm, stepper in (("atmosphere", self.atmosphere), ("ocean", self.ocean)):
            steps = [o for o in outs if o.realm == realm]
            if not steps:
                raise ValueError("the forcing records hold no coupled step")
            data[realm] = {k: torch.stack([o.data[k] for o in steps], dim=self.TIME_DIM) for k in steps[0].data}
            # an ocean without a depth coordinate derives nothing (the reference's NullDeriveFn)
            if compute_derived_variables and (realm == "atmosphere" or isinstance(stepper.derive_func, OceanDeriveFn)):
                data[realm] = derive_over_window(stepper.derive_func, data[realm], initial_condition[realm], forcing[realm],
                                                 1, len(steps))
            state[realm] = _prognostic_state(steps[-1].data, stepper.prognostic_names, steps[-1].stepper_state)
        return data, state


def _prognostic_state(step: TensorMapping, names: Iterable[str], stepper_state) -> PrognosticState:
    state = PrognosticState({k: step[k].unsqueeze(1) for k in names})
    state.stepper_state = stepper_state
    return state


def load_coupled_stepper(checkpoint: Union[str, pathlib.Path, Mapping[str, Any]], device=None,
                         ignore_unsupported: bool = False) -> CoupledStepper:
    """``fme.coupled.stepper.load_coupled_stepper`` (stepper.py:2280-2283): a path (torch.load) or the loaded dict, the whole
    checkpoint ``{"stepper": {"config", "atmosphere_state", "ocean_state", "dataset_info"}}`` or the stepper state itself."""
    if not isinstance(checkpoint, Mapping):
        checkpoint = torch.load(checkpoint, map_location="cpu", weights_only=False)
    state = checkpoint["stepper"] if "stepper" in checkpoint else checkpoint
    stepper = CoupledStepper.from_state(state, device=device, ignore_unsupported=ignore_unsupported)
    stepper.set_eval()
    return stepper
