"""Host side of the fused ocean corrector (include/ace_sfno.h: ace_ocean_phys_*; ace_amd/csrc/ocean_phys.hip).

``FusedOceanCorrector`` is one HIP handle per (device, batch, grid) of an ``OceanCorrector``: the static geometry (area weights
per row, the depth coordinate's dz table, the masks the heat-content mean and the depth integral read) is uploaded once; each
call resolves the reference's names (OceanData / AtmosphereData rules, ace_amd/ocean_corrector.py) to ``{pointer, per-sample
stride}`` planes of the caller's tensors and makes two launches on the current stream.  Output planes are corrected in
place; a field the step produced as a strided view of a larger tensor is used as it is."""
import ctypes
from ctypes import c_long, c_void_p
from typing import Tuple

import torch

from . import _lib
from ._lib import OCEAN_MAX_LEVELS, OCEAN_MAX_POSITIVE, OCEAN_MAX_ZERO, OceanConfig, OceanFields
from .atmosphere import ATMOSPHERE_FIELD_NAME_PREFIXES
from .ocean_corrector import _name, level_names, ohc_flux_source

_HFDS = {"residual_prediction": 1, "prescribed": 2}


def _atm(data, standard: str):
    for prefix in ATMOSPHERE_FIELD_NAME_PREFIXES[standard]:
        if prefix in data:
            return data[prefix]
    raise KeyError(standard)


class FusedOceanCorrector:
    def __init__(self, corrector, batch: int, img_shape: Tuple[int, int], device):
        cfg = corrector.config
        active = set(corrector.corrections)
        H, W = img_shape
        self.batch, self.shape, self.device = batch, (H, W), torch.device(device)
        self._corrector = corrector
        c = OceanConfig()
        c.nlat, c.nlon, c.max_batch = H, W, batch
        sic = cfg.sea_ice_fraction_correction
        c.sea_ice = int("sea_ice_fraction_correction" in active)
        c.remove_negative_ocean_fraction = int(bool(sic.remove_negative_ocean_fraction)) if c.sea_ice else 0
        c.hfds = _HFDS[cfg.surface_energy_flux_correction.method] if "surface_energy_flux_correction" in active else 0
        c.ohc = int("ocean_heat_content_correction" in active)
        wl = dz = mask_ohc = mask0 = None
        if c.ohc:
            ohc = cfg.ocean_heat_content_correction
            depth = corrector._depth_on("cpu")
            c.nlev = depth.nlev
            if c.nlev > OCEAN_MAX_LEVELS:
                raise NotImplementedError(f"the fused ocean corrector supports up to {OCEAN_MAX_LEVELS} depth levels, got {c.nlev}")
            c.timestep_seconds, c.unaccounted_heating = float(corrector._dt), float(ohc.constant_unaccounted_heating)
            mean = corrector._mean
            wl = mean._cpu.to(torch.float32).reshape(H, W)[:, 0].contiguous()
            # the weights of the masked mean: area weights times the provider's mask for "ocean_heat_content"
            masked = mean.weights_for("ocean_heat_content", "cpu")
            full = mean._w("cpu")
            mask_ohc = None
            if masked is not full:
                m = mean._provider.get_mask_tensor_for("ocean_heat_content")
                mask_ohc = m.detach().to("cpu", torch.float32).expand(H, W).contiguous()
            dz = depth.dz.detach().to("cpu", torch.float32).expand(H, W, c.nlev).permute(2, 0, 1).contiguous()
            mask0 = depth.mask.detach().to("cpu", torch.float32).select(-1, 0).expand(H, W).contiguous()
        self.config = c
        self._keep = (wl, dz, mask_ohc, mask0)
        self.handle = c_void_p()
        p = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ace_ocean_phys_create(ctypes.byref(c), p(wl), p(dz), p(mask_ohc), p(mask0), ctypes.byref(self.handle)), "ocean_phys")

    def fields(self, inp, gen, forcing) -> OceanFields:
        cfg, c = self._corrector.config, self.config
        f = OceanFields()
        plane = lambda dst, t, name: _lib.bind_plane(dst, t, self.batch, self.shape, self.device, "fused ocean corrector", name)
        active = set(self._corrector.corrections)
        positive = self._corrector.force_positive_names if "force_positive" in active else []
        if len(positive) > OCEAN_MAX_POSITIVE:
            raise NotImplementedError(f"the fused ocean corrector clamps up to {OCEAN_MAX_POSITIVE} fields, got {len(positive)}")
        for k, n in enumerate(positive):
            plane(f.positive[k], gen[n], n)
        f.npositive = len(positive)
        if c.sea_ice:
            sic = cfg.sea_ice_fraction_correction
            plane(f.sif, gen[sic.sea_ice_fraction_name], sic.sea_ice_fraction_name)
            if len(sic.zero_where_ice_free_names) > OCEAN_MAX_ZERO:
                raise NotImplementedError(f"the fused ocean corrector zeroes up to {OCEAN_MAX_ZERO} fields where ice free")
            for k, n in enumerate(sic.zero_where_ice_free_names):
                plane(f.zero[k], gen[n], n)
            f.nzero = len(sic.zero_where_ice_free_names)
            if c.remove_negative_ocean_fraction:
                plane(f.reb_land, inp[sic.land_fraction_name], sic.land_fraction_name)
        ssf_forcing = False
        if c.hfds:
            hname = "hfds" if "hfds" in gen else "hfds_total_area"
            plane(f.hfds, gen[hname], hname)
            f.hfds_total_area = int(hname == "hfds_total_area")
            plane(f.in_land, inp["land_fraction"], "land_fraction")
            sname = _name(inp, "sea_ice_fraction") or "ocean_sea_ice_fraction"
            plane(f.in_sif, inp[sname], sname)
            f.in_sif_is_ocean_sif = int(sname == "ocean_sea_ice_fraction")
            plane(f.in_sst, inp["sst"], "sst")
            for attr, std in (("dlw", "sfc_down_lw_radiative_flux"), ("ulw", "sfc_up_lw_radiative_flux"),
                              ("dsw", "sfc_down_sw_radiative_flux"), ("usw", "sfc_up_sw_radiative_flux"),
                              ("lhf", "latent_heat_flux"), ("shf", "sensible_heat_flux"), ("precip", "precipitation_rate")):
                plane(getattr(f, attr), _atm(forcing, std), std)
            if "total_frozen_precipitation_rate" in forcing:
                plane(f.frozen, forcing["total_frozen_precipitation_rate"], "total_frozen_precipitation_rate")
            elif all(n in forcing for n in ("ICEsfc", "GRAUPELsfc", "SNOWsfc")):
                for k, n in enumerate(("ICEsfc", "GRAUPELsfc", "SNOWsfc")):
                    plane(f.frozen_parts[k], forcing[n], n)
            else:
                _atm(forcing, "surface_pressure")      # AtmosphereData's zero fallback is zeros_like(surface_pressure)
            ssf_forcing = bool(f.hfds_total_area)
        if c.ohc:
            if "hfds" in gen and "hfds" in forcing:
                raise ValueError("Net downward surface heat flux cannot be present in both gen_data and forcing_data.")
            thetao = level_names(gen, "sea_water_potential_temperature")
            thetao_in = level_names(inp, "sea_water_potential_temperature")
            if len(thetao) != c.nlev or len(thetao_in) != c.nlev:
                raise ValueError(f"The last dimension of integrand must match the number of vertical layers in the depth vertical "
                                 f"coordinate: {len(thetao)} / {len(thetao_in)} thetao levels, {c.nlev} layers.")
            for k in range(c.nlev):
                plane(f.thetao[k], gen[thetao[k]], thetao[k])
                plane(f.thetao_in[k], inp[thetao_in[k]], thetao_in[k])
            if "sst" in gen:
                plane(f.sst, gen["sst"], "sst")
            src = ohc_flux_source(gen, forcing)
            if src in ("gen_total_area", "gen"):
                hname = "hfds_total_area" if src == "gen_total_area" else "hfds"
                if c.hfds and f.hfds.p and f.hfds.p != gen[hname].data_ptr():
                    raise NotImplementedError("fused ocean corrector: output with both hfds and hfds_total_area and both flux "
                                              "corrections on; use the torch path (OceanCorrector.fused = False)")
                plane(f.hfds, gen[hname], hname)
                f.flux_source = 0 if src == "gen_total_area" else 1
            elif "hfds" in inp:
                plane(f.in_flux, inp["hfds"], "hfds")
                f.flux_source = 2
            else:
                plane(f.in_flux, inp["hfds_total_area"], "hfds_total_area")
                iname = "sea_surface_fraction" if "sea_surface_fraction" in inp else "land_fraction"
                plane(f.in_ssf, inp[iname], iname)
                f.in_ssf_is_land = int(iname == "land_fraction")
                f.flux_source = 3
            if "hfgeou" in forcing:
                plane(f.hfgeou, forcing["hfgeou"], "hfgeou")
            ssf_forcing = True
        if ssf_forcing:
            fname = "sea_surface_fraction" if "sea_surface_fraction" in forcing else "land_fraction"
            plane(f.f_ssf, forcing[fname], fname)
            f.f_ssf_is_land = int(fname == "land_fraction")
        return f

    def __call__(self, inp, gen, forcing):
        f = self.fields(inp, gen, forcing)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ace_ocean_phys_apply(self.handle, ctypes.byref(f), self.batch,
                                                       torch.cuda.current_stream(self.device).cuda_stream), "ocean_phys")
        return gen

    def apply(self, fields: OceanFields, stream: int) -> None:
        """One step on planes resolved once by ``fields`` (static buffers: ``OceanRolloutEngine`` keeps a struct per step)."""
        _lib.check(_lib.lib().ace_ocean_phys_apply(self.handle, ctypes.byref(fields), self.batch, stream), "ocean_phys")

    def launches(self) -> Tuple[int, int]:
        o1, o2 = c_long(0), c_long(0)
        _lib.check(_lib.lib().ace_ocean_phys_launches(self.handle, ctypes.byref(o1), ctypes.byref(o2)), "ocean_phys")
        return o1.value, o2.value

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.lib().ace_ocean_phys_destroy(self.handle)
                self.handle = None
        except Exception:
            pass
