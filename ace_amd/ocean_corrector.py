"""Post-step ocean corrector: fme/core/corrector/ocean.py (``OceanCorrectorConfig``, registered as "ocean_corrector").

Mirror of the reference's configuration (same fields, defaults and deprecated-key handling, so a checkpoint's step config
round-trips) and of the ``CorrectionSequence`` it builds, applied in the reference's order:
force positive -> sea-ice fraction (clamp, rebalance, zero where ice free) -> surface energy flux (hfds) -> ocean heat
content (one uniform scaling of every thetao level and of the SST in Celsius).
The geometry it needs lives here too: ``DepthCoordinate`` (fme/core/coordinates.py:287-440) and the mask-aware area mean
(``LatLonOperations.area_weighted_mean`` with ``name=``, fme/core/gridded_ops.py:271-359).

Two paths compute the same thing.  On the CPU (and whenever ``OceanCorrector.fused`` is False) the corrections run as the
readable torch restatement below, pinned to the reference by tests/golden/gen_ocean_corrector_*.pt.  With the fields on the
GPU the whole sequence is two HIP launches (ace_amd/csrc/ocean_phys.hip, ``ace_ocean_phys_*``): one pass over the columns
that does every column-local correction and the per-workgroup fp64 partial sums of the heat-content means, one pass that
forms the ratio per sample and scales the temperatures.  The fused path corrects the output tensors in place (the step's
output is fresh every step, and a strided view of a larger tensor is used as it is); inputs and forcings are only read.  The
torch path, like the reference, returns new tensors for the fields it changes."""
import dataclasses
from typing import Any, Dict, List, Mapping, Optional, Tuple

import torch

from .atmosphere import AreaWeightedMean, AtmosphereData
from .corrector import force_positive

TensorMapping = Mapping[str, torch.Tensor]
TensorDict = Dict[str, torch.Tensor]

# fme/core/constants.py
SPECIFIC_HEAT_OF_SEA_WATER_CM4 = 3992.0
DENSITY_OF_SEA_WATER_CM4 = 1035.0
FREEZING_TEMPERATURE_KELVIN = 273.15
LATENT_HEAT_OF_VAPORIZATION = 2.5e6

# fme/core/ocean_data.py:10-30
OCEAN_FIELD_NAME_PREFIXES = {
    "sea_water_potential_temperature": ["thetao_"],
    "sea_water_salinity": ["so_"],
    "sea_water_x_velocity": ["uo_"],
    "sea_water_y_velocity": ["vo_"],
    "sea_surface_height_above_geoid": ["zos"],
    "sea_surface_temperature": ["sst"],
    "sea_ice_fraction": ["sea_ice_fraction"],
    "sea_ice_thickness": ["HI"],
    "sea_ice_volume": ["sea_ice_volume"],
    "ocean_sea_ice_fraction": ["ocean_sea_ice_fraction"],
    "land_fraction": ["land_fraction"],
    "net_downward_surface_heat_flux": ["hfds"],
    "net_downward_surface_heat_flux_total_area": ["hfds_total_area"],
    "geothermal_heat_flux": ["hfgeou"],
    "sea_surface_fraction": ["sea_surface_fraction"],
}


# ---------------------------------------------------------------------------------------------------------------------
# geometry
def dz_from_idepth(idepth: torch.Tensor, mask: torch.Tensor, deptho: Optional[torch.Tensor] = None) -> torch.Tensor:
    """coordinates.py:287-299: layer thickness per column, partial bottom cells from ``deptho``, zero where masked."""
    z_top, z_bot = idepth[..., :-1], idepth[..., 1:]
    if deptho is None:
        deptho_expanded = (mask * z_bot).max(dim=-1, keepdim=True).values
    else:
        deptho_expanded = deptho.unsqueeze(-1)
    dz = torch.clamp(deptho_expanded, min=z_top, max=z_bot) - z_top
    return dz.nan_to_num() * mask


class DepthCoordinate:
    """coordinates.py:302-440: interface depths (L + 1,), a (..., L) ocean mask (1 valid, 0 land) and an optional sea-floor
    depth (...)."""

    def __init__(self, idepth: torch.Tensor, mask: torch.Tensor, deptho: Optional[torch.Tensor] = None):
        idepth, mask = torch.as_tensor(idepth), torch.as_tensor(mask)
        if idepth.dim() != 1:
            raise ValueError(f"idepth must be a 1-dimensional tensor. Got shape: {idepth.shape}")
        if len(idepth) < 2:
            raise ValueError(f"idepth must have at least two elements. Got {idepth}.")
        if idepth.shape[0] != mask.shape[-1] + 1:
            raise ValueError("The last dimension of mask must be one shorter than length of idepth."
                             f"Got idepth.shape: {idepth.shape} and mask.shape: {mask.shape}.")
        self.idepth, self.mask = idepth, mask
        self.deptho = torch.as_tensor(deptho) if deptho is not None else None
        self._dz = dz_from_idepth(self.idepth, self.mask, self.deptho)

    @classmethod
    def from_state(cls, state: Mapping[str, Any]) -> "DepthCoordinate":
        unknown = set(state) - {"idepth", "mask", "deptho"}
        if unknown:
            raise ValueError(f"unknown depth coordinate fields: {sorted(unknown)}")
        return cls(state["idepth"], state["mask"], state.get("deptho"))

    @property
    def dz(self) -> torch.Tensor:
        return self._dz

    @property
    def nlev(self) -> int:
        return len(self.idepth) - 1

    def __len__(self):
        return len(self.idepth)

    def to(self, device) -> "DepthCoordinate":
        return DepthCoordinate(self.idepth.to(device), self.mask.to(device),
                               self.deptho.to(device) if self.deptho is not None else None)

    def as_dict(self) -> TensorDict:
        out = {"idepth": self.idepth, "mask": self.mask}
        if self.deptho is not None:
            out["deptho"] = self.deptho
        return out

    def build_derive_function(self, timestep, horizontal_coordinates=None):
        """coordinates.py:349-354: the ocean's derived variables on this coordinate (``horizontal_coordinates``: the cell areas the
        sea-ice thickness needs)."""
        from .ocean_derived_variables import OceanDeriveFn
        return OceanDeriveFn(self, timestep, horizontal_coordinates)

    def depth_integral(self, integrand: torch.Tensor) -> torch.Tensor:
        """sum_k x_k dz_k with NaNs counted as zero; NaN where the top level is masked."""
        if len(self.idepth) != integrand.shape[-1] + 1:
            raise ValueError("The last dimension of integrand must match the number of vertical layers in the depth vertical "
                             f"coordinate. Got integrand.shape: {integrand.shape} and idepth.shape: {self.idepth.shape}.")
        dz = self._dz.to(integrand.device)
        integral = (integrand * dz).nansum(dim=-1)
        mask_0 = self.mask.to(integrand.device).select(dim=-1, index=0).expand(integral.shape)
        return integral.where(mask_0 > 0, float("nan"))


class MaskedAreaWeightedMean(AreaWeightedMean):
    """``area_weighted_mean(data, keepdim, name)`` of LatLonOperations with a mask provider: the weights are the area weights
    times ``mask_provider.get_mask_tensor_for(name)`` (no mask for that name, or no name: the plain area weights); values
    with weight 0 are dropped, NaNs included (metrics.py:63-90)."""

    def __init__(self, area_weights: torch.Tensor, mask_provider=None):
        super().__init__(area_weights)
        self._provider = mask_provider
        self._masked: Dict[Tuple[str, str], torch.Tensor] = {}

    def weights_for(self, name: Optional[str], device) -> torch.Tensor:
        w = self._w(device)
        if name is None or self._provider is None:
            return w
        key = (name, str(device))
        if key not in self._masked:
            mask = self._provider.get_mask_tensor_for(name)
            self._masked[key] = w if mask is None else w * mask.to(device)
        return self._masked[key]

    def __call__(self, data: torch.Tensor, keepdim: bool = False, name: Optional[str] = None) -> torch.Tensor:
        w = self.weights_for(name, data.device).expand(data.shape)
        data = data.where(w != 0.0, 0.0)
        return (data * w).sum(dim=(-2, -1), keepdim=keepdim) / w.sum(dim=(-2, -1), keepdim=keepdim)


# ---------------------------------------------------------------------------------------------------------------------
# name resolution (OceanData, fme/core/ocean_data.py:48-330, and the Stacker's level rules)
def _get(data: TensorMapping, standard: str) -> torch.Tensor:
    for prefix in OCEAN_FIELD_NAME_PREFIXES[standard]:
        if prefix in data:
            return data[prefix]
    raise KeyError(standard)


def _name(data, standard: str) -> Optional[str]:
    for prefix in OCEAN_FIELD_NAME_PREFIXES[standard]:
        if prefix in data:
            return prefix
    return None


def level_names(data, standard: str) -> List[str]:
    """stacker.py:111-160: the prefix itself (one level) or prefix_0 .. prefix_{n-1} in natural order."""
    data = AtmosphereData(dict.fromkeys(data))
    for prefix in OCEAN_FIELD_NAME_PREFIXES[standard]:
        if prefix in data.data:
            return [prefix]
        try:
            return data._level_names(prefix)
        except KeyError:
            pass
    raise KeyError(f"Found no matches for any of {OCEAN_FIELD_NAME_PREFIXES[standard]} among the data names {list(data.data)}.")


def sea_surface_fraction(data: TensorMapping) -> torch.Tensor:
    try:
        return _get(data, "sea_surface_fraction")
    except KeyError:
        return 1 - _get(data, "land_fraction")


def sea_ice_fraction(data: TensorMapping) -> torch.Tensor:
    try:
        return _get(data, "sea_ice_fraction")
    except KeyError:
        return _get(data, "ocean_sea_ice_fraction") * (1 - _get(data, "land_fraction"))


def ocean_fraction(data: TensorMapping) -> torch.Tensor:
    return 1 - _get(data, "land_fraction") - sea_ice_fraction(data)


def geothermal_heat_flux(data: TensorMapping) -> torch.Tensor:
    try:
        return _get(data, "geothermal_heat_flux")
    except KeyError:
        return torch.zeros_like(sea_surface_fraction(data))


def net_downward_surface_heat_flux(data: TensorMapping) -> torch.Tensor:
    try:
        return _get(data, "net_downward_surface_heat_flux")
    except KeyError:
        return _get(data, "net_downward_surface_heat_flux_total_area") / sea_surface_fraction(data)


def ocean_heat_content(data: TensorMapping, depth: DepthCoordinate) -> torch.Tensor:
    thetao = torch.stack([data[n] for n in level_names(data, "sea_water_potential_temperature")], dim=-1)
    return depth.depth_integral(thetao * SPECIFIC_HEAT_OF_SEA_WATER_CM4 * DENSITY_OF_SEA_WATER_CM4)


# ---------------------------------------------------------------------------------------------------------------------
# the corrections (ocean.py:55-108, 310-486)
def correct_sea_ice_fraction(cfg: "SeaIceFractionConfig", gen: TensorMapping, inp: TensorMapping) -> TensorDict:
    out: TensorDict = {}
    sif = torch.clamp(gen[cfg.sea_ice_fraction_name], min=0.0, max=1.0)
    if cfg.remove_negative_ocean_fraction:
        negative_ocean_fraction = (1 - sif - inp[cfg.land_fraction_name]).clip(max=0)
        sif = sif + negative_ocean_fraction
    out[cfg.sea_ice_fraction_name] = sif
    for name in cfg.zero_where_ice_free_names:
        out[name] = gen[name] * (sif > 0.0)
    return out


def ocean_net_surface_energy_flux(forcing: TensorMapping, sst: torch.Tensor) -> torch.Tensor:
    """ocean.py:369-390: the atmosphere's net surface energy flux plus the heat carried by precipitation and evaporation."""
    atmos = AtmosphereData(forcing)
    mass_heat_flux = (SPECIFIC_HEAT_OF_SEA_WATER_CM4
                      * (atmos.precipitation_rate + atmos.frozen_precipitation_rate
                         - (atmos._get("latent_heat_flux") / LATENT_HEAT_OF_VAPORIZATION))
                      * (sst - FREEZING_TEMPERATURE_KELVIN))
    return atmos.net_surface_energy_flux + mass_heat_flux


def correct_hfds(inp: TensorMapping, gen: TensorMapping, forcing: TensorMapping, method: str) -> TensorDict:
    """ocean.py:393-428."""
    ofrac = ocean_fraction(inp)
    net_flux = ocean_net_surface_energy_flux(forcing, _get(inp, "sea_surface_temperature"))
    if "hfds" in gen:
        hfds_name = "hfds"
    else:
        hfds_name = "hfds_total_area"
        net_flux = net_flux * sea_surface_fraction(forcing)
    g = gen[hfds_name]
    if method == "residual_prediction":
        return {hfds_name: net_flux * ofrac + g}
    if method == "prescribed":
        return {hfds_name: net_flux * ofrac + g * (1 - ofrac)}
    raise NotImplementedError(f"Method {method!r} not implemented for surface energy flux correction")


def ohc_flux_source(gen: TensorMapping, forcing: TensorMapping) -> str:
    """which net flux into the ocean the heat budget uses (ocean.py:459-476, in priority order)"""
    for src, probe in (("gen_total_area", lambda: (gen["hfds_total_area"], sea_surface_fraction(forcing))),
                       ("gen", lambda: (gen["hfds"], sea_surface_fraction(forcing)))):
        try:
            probe()
            return src
        except KeyError:
            pass
    return "input"


def net_energy_flux_into_ocean(inp: TensorMapping, gen: TensorMapping, forcing: TensorMapping) -> torch.Tensor:
    src = ohc_flux_source(gen, forcing)
    if src == "gen_total_area":
        return gen["hfds_total_area"] + geothermal_heat_flux(forcing) * sea_surface_fraction(forcing)
    if src == "gen":
        return (gen["hfds"] + geothermal_heat_flux(forcing)) * sea_surface_fraction(forcing)
    return (net_downward_surface_heat_flux(inp) + geothermal_heat_flux(forcing)) * sea_surface_fraction(forcing)


def ohc_ratio(inp, gen, forcing, mean, depth: DepthCoordinate, dt: float, heating: float) -> torch.Tensor:
    """(mean_in + (flux_mean + heating) dt) / mean_gen per sample, (B, 1, 1) (ocean.py:431-486)."""
    if "hfds" in gen and "hfds" in forcing:
        raise ValueError("Net downward surface heat flux cannot be present in both gen_data and forcing_data.")
    gen_ohc = mean(ocean_heat_content(gen, depth), keepdim=True, name="ocean_heat_content")
    in_ohc = mean(ocean_heat_content(inp, depth), keepdim=True, name="ocean_heat_content")
    flux = mean(net_energy_flux_into_ocean(inp, gen, forcing), keepdim=True, name="ocean_heat_content")
    return (in_ohc + (flux + heating) * dt) / gen_ohc


def conserve_ocean_heat_content(inp, gen, forcing, mean, depth, dt, method="scaled_temperature", heating=0.0) -> TensorDict:
    if method != "scaled_temperature":
        raise NotImplementedError(f"Method {method!r} not implemented for ocean heat content conservation")
    ratio = ohc_ratio(inp, gen, forcing, mean, depth, dt, heating)
    out = {n: gen[n] * ratio for n in level_names(gen, "sea_water_potential_temperature")}
    if "sst" in gen:
        out["sst"] = (gen["sst"] - FREEZING_TEMPERATURE_KELVIN) * ratio + FREEZING_TEMPERATURE_KELVIN
    return out


# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class SeaIceFractionConfig:
    sea_ice_fraction_name: str
    land_fraction_name: str
    zero_where_ice_free_names: List[str] = dataclasses.field(default_factory=list)
    remove_negative_ocean_fraction: bool = True


@dataclasses.dataclass
class OceanHeatContentBudgetConfig:
    method: str
    constant_unaccounted_heating: float = 0.0


@dataclasses.dataclass
class SurfaceEnergyFluxCorrectionConfig:
    method: str


def _sub(cls, value):
    if value is None or isinstance(value, cls):
        return value
    if isinstance(value, Mapping):
        unknown = set(value) - {f.name for f in dataclasses.fields(cls)}
        if unknown:
            raise ValueError(f"unknown {cls.__name__} fields: {sorted(unknown)}")
        return cls(**value)
    raise TypeError(f"expected a {cls.__name__} or its state, got {type(value).__name__}")


@dataclasses.dataclass
class OceanCorrectorConfig:
    force_positive_names: List[str] = dataclasses.field(default_factory=list)
    sea_ice_fraction_correction: Optional[SeaIceFractionConfig] = None
    surface_energy_flux_correction: Optional[SurfaceEnergyFluxCorrectionConfig] = None
    ocean_heat_content_correction: Optional[OceanHeatContentBudgetConfig] = None
    # straight-through gradients through the clamps: forward values are unchanged, so inference ignores it
    keep_gradient_through_clamps: bool = False
    # CorrectorConfigABC (registry.py:14-62): a training-epoch schedule; inference always applies the corrector
    corrector_disabled_epochs: int = 0

    def __post_init__(self):
        if self.corrector_disabled_epochs < 0:
            raise ValueError(f"corrector_disabled_epochs must be non-negative, got {self.corrector_disabled_epochs}")
        self.sea_ice_fraction_correction = _sub(SeaIceFractionConfig, self.sea_ice_fraction_correction)
        self.surface_energy_flux_correction = _sub(SurfaceEnergyFluxCorrectionConfig, self.surface_energy_flux_correction)
        self.ocean_heat_content_correction = _sub(OceanHeatContentBudgetConfig, self.ocean_heat_content_correction)
        sef = self.surface_energy_flux_correction
        if sef is not None and sef.method not in ("residual_prediction", "prescribed"):
            raise NotImplementedError(f"Method {sef.method!r} not implemented for surface energy flux correction")
        ohc = self.ocean_heat_content_correction
        if ohc is not None and ohc.method != "scaled_temperature":
            raise NotImplementedError(f"Method {ohc.method!r} not implemented for ocean heat content conservation")

    @classmethod
    def remove_deprecated_keys(cls, state: Mapping[str, Any]) -> Dict[str, Any]:
        """ocean.py:272-294: drop ``masking``; a boolean heat-content option; the sea-ice thickness name."""
        state = dict(state)
        state.pop("masking", None)
        if isinstance(state.get("ocean_heat_content_correction"), bool):
            state["ocean_heat_content_correction"] = (
                OceanHeatContentBudgetConfig(method="scaled_temperature") if state["ocean_heat_content_correction"] else None)
        sif = state.get("sea_ice_fraction_correction")
        if isinstance(sif, Mapping) and "sea_ice_thickness_name" in sif:
            sif = dict(sif)
            thickness_name = sif.pop("sea_ice_thickness_name")
            if thickness_name is not None:
                sif["zero_where_ice_free_names"] = list(sif.get("zero_where_ice_free_names", [])) + [thickness_name]
            state["sea_ice_fraction_correction"] = sif
        return state

    @classmethod
    def from_state(cls, state: Mapping[str, Any]) -> "OceanCorrectorConfig":
        state = dict(state)
        if "type" in state and "config" in state:      # CorrectorSelector form (fme/core/registry/corrector.py)
            if set(state) - {"type", "config", "corrector_disabled_epochs"}:
                raise ValueError(f"unknown corrector selector fields: {sorted(state)}")
            if state.get("corrector_disabled_epochs", 0) != 0:
                raise ValueError("corrector_disabled_epochs must be set on the wrapped corrector config (inside "
                                 "`config:`), not on the CorrectorSelector.")
            if state["type"] != "ocean_corrector":
                raise ValueError(f"not an ocean corrector: {state['type']!r}")
            state = dict(state["config"] or {})
        state = cls.remove_deprecated_keys(state)
        unknown = set(state) - {f.name for f in dataclasses.fields(cls)}
        if unknown:
            raise ValueError(f"unknown ocean corrector fields: {sorted(unknown)}")
        return cls(**state)

    def unsupported(self, dataset_info=None) -> List[str]:
        """options that cannot be honoured with this dataset_info: the heat-content means need the grid's area weights"""
        if self.ocean_heat_content_correction is not None and getattr(dataset_info, "area_weights", None) is None:
            return ["ocean_heat_content_correction"]
        return []

    def get_corrector(self, dataset_info=None, ignore_unsupported: bool = False) -> Optional["OceanCorrector"]:
        missing = self.unsupported(dataset_info)
        if missing and not ignore_unsupported:
            raise NotImplementedError("ocean_corrector options that need the grid's area weights, which this dataset_info does not "
                                      "carry: " + ", ".join(missing))
        corrector = OceanCorrector(self, dataset_info, skip=set(missing))
        return corrector if corrector.corrections else None


def corrector_config_from_state(state):
    """the step config's ``corrector``: an AtmosphereCorrectorConfig / OceanCorrectorConfig / IceCorrectorConfig, a
    CorrectorSelector state ({"type", "config"}) or a bare atmosphere corrector state (what every checkpoint without a selector
    carries)."""
    from .corrector import AtmosphereCorrectorConfig
    if isinstance(state, Mapping) and state.get("type") == "ocean_corrector" and "config" in state:
        return OceanCorrectorConfig.from_state(state)
    if isinstance(state, Mapping) and state.get("type") == "ice_corrector" and "config" in state:
        from .ice_corrector import IceCorrectorConfig
        return IceCorrectorConfig.from_state(state)
    return AtmosphereCorrectorConfig.from_state(state)


class OceanCorrector:
    """CorrectionSequence built as in ocean.py:296-345; the same call signature and return as ``AtmosphereCorrector``:
    ``(input, gen, forcing, state) -> (corrected gen dict, state)`` (the ocean corrector carries no state)."""

    def __init__(self, config: OceanCorrectorConfig, dataset_info=None, skip=frozenset()):
        self._cfg = config
        self.force_positive_names = list(config.force_positive_names)
        area = getattr(dataset_info, "area_weights", None)
        self._mean = MaskedAreaWeightedMean(area, getattr(dataset_info, "mask_provider", None)) if area is not None else None
        self._depth: Optional[DepthCoordinate] = getattr(dataset_info, "ocean_vertical_coordinate", None)
        ts = getattr(dataset_info, "timestep", None)
        self._dt = ts.total_seconds() if ts is not None else None
        self.corrections: List[str] = []
        if self.force_positive_names:
            self.corrections.append("force_positive")
        if config.sea_ice_fraction_correction is not None:
            self.corrections.append("sea_ice_fraction_correction")
        if config.surface_energy_flux_correction is not None:
            self.corrections.append("surface_energy_flux_correction")
        if config.ocean_heat_content_correction is not None and "ocean_heat_content_correction" not in skip:
            self.corrections.append("ocean_heat_content_correction")
        self.fused = True              # GPU tensors take the HIP path; False: the torch ops on any device
        self._handles: Dict[Any, Any] = {}

    @property
    def config(self) -> OceanCorrectorConfig:
        return self._cfg

    def _depth_on(self, device) -> DepthCoordinate:
        if self._depth is None:
            raise ValueError("Ocean heat content correction is turned on, but no vertical coordinate is available.")
        return self._depth.to(device)

    def __call__(self, input_data: TensorMapping, gen_data: TensorMapping, forcing_data: TensorMapping,
                 corrector_state=None) -> Tuple[TensorDict, Any]:
        gen = dict(gen_data)
        if not self.corrections:
            return gen, corrector_state
        dev = next(iter(gen.values())).device
        if self.fused and dev.type == "cuda":
            return self._fused(input_data, gen, forcing_data), corrector_state
        return self.torch_apply(input_data, gen, forcing_data), corrector_state

    def torch_apply(self, input_data: TensorMapping, gen_data: TensorMapping, forcing_data: TensorMapping) -> TensorDict:
        gen = dict(gen_data)
        for name in self.corrections:
            if name == "force_positive":
                changed = force_positive(gen, self.force_positive_names)
            elif name == "sea_ice_fraction_correction":
                changed = correct_sea_ice_fraction(self._cfg.sea_ice_fraction_correction, gen, input_data)
            elif name == "surface_energy_flux_correction":
                changed = correct_hfds(input_data, gen, forcing_data, self._cfg.surface_energy_flux_correction.method)
            else:
                ohc = self._cfg.ocean_heat_content_correction
                dev = next(iter(gen.values())).device
                changed = conserve_ocean_heat_content(input_data, gen, forcing_data, self._mean, self._depth_on(dev), self._dt,
                                                      ohc.method, ohc.constant_unaccounted_heating)
            gen.update(changed)
        return gen

    # ---- the HIP path ------------------------------------------------------------------------------------------------
    def _fused(self, input_data: TensorMapping, gen: TensorDict, forcing_data: TensorMapping) -> TensorDict:
        from .ocean_phys import FusedOceanCorrector
        any_t = next(iter(gen.values()))
        B, H, W = any_t.shape[0], any_t.shape[-2], any_t.shape[-1]
        key = (str(any_t.device), B, H, W)
        h = self._handles.get(key)
        if h is None:
            h = self._handles[key] = FusedOceanCorrector(self, B, (H, W), any_t.device)
        return h(input_data, gen, forcing_data)

    def launches(self) -> Tuple[int, int]:
        """(O1, O2) launches made by the HIP path of this corrector so far, over all its handles (the route query)."""
        o1 = o2 = 0
        for h in self._handles.values():
            a, b = h.launches()
            o1, o2 = o1 + a, o2 + b
        return o1, o2
