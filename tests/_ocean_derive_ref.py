"""ace_ocean_derive_window (include/ace_sfno.h) restated in numpy: the contract the kernel is held to bit for bit
(tests/test_gpu_ocean_derive_kernels.py) and that tests/test_ocean_derive_ref_cpu.py holds to the reference's outputs.

The column sum is a sequential fp64 loop over the levels; the fp32 arithmetic is numpy's float32, one IEEE operation at a time."""
import numpy as np

OUTPUTS = ("ocean_heat_content", "ocean_heat_content_tendency", "implied_tendency_of_ocean_heat_content_due_to_advection",
           "net_energy_flux_into_ocean_column", "sea_ice_fraction", "HI", "hfds")
CP_RHO = 3992.0 * 1035.0
FLT_MAX = np.finfo(np.float32).max
F32 = np.float32


def column_sum(levels, dz):
    """CP_RHO * sum_k (double) thetao_k * (double) dz_k, k ascending, a NaN thetao_k (or a level that is None) adding nothing.
    levels: per level a (..., hw) fp32 array or None; dz: (nlev, hw) fp32."""
    shape = next(x.shape for x in levels if x is not None)
    acc = np.zeros(shape, np.float64)
    for k, th in enumerate(levels):
        if th is None:
            continue
        th = th.astype(np.float64)
        with np.errstate(invalid="ignore"):
            acc = np.where(np.isnan(th), acc, acc + th * dz[k].astype(np.float64))
    return acc * CP_RHO


def sea_ice_thickness(vol, area, frac):
    """the table of the header, first matching row; fp32 in, fp32 out"""
    vol, area, frac = (np.asarray(x, np.float64) for x in np.broadcast_arrays(vol, area, frac))
    with np.errstate(all="ignore"):
        q = ((vol * 1e9) / (area * frac)).astype(F32)
        q = np.where(q > FLT_MAX, FLT_MAX, q)
        conds = [np.isnan(vol), np.isnan(frac) | np.isnan(area), (vol < 0) | (frac < 0) | (area < 0), vol == 0,
                 np.isinf(frac) | np.isinf(area), np.isinf(vol), area * frac == 0]
    return np.select(conds, [F32(np.nan), F32(0), F32(0), F32(0), F32(0), FLT_MAX, FLT_MAX], q).astype(F32)


def derive_window(want, dt_seconds, thetao=None, head=None, dz=None, mask0=None, area_m2=None, **fields):
    """want: names of OUTPUTS.  thetao: list of (B, T, hw) fp32; head: None (has_head = 0) or a list of (B, hw) fp32 / None per level;
    dz (nlev, hw), mask0 (hw), area_m2 (hw) fp32; fields: hfds, hfds_total_area, hfgeou, sea_surface_fraction, land_fraction,
    ocean_sea_ice_fraction, sea_ice_fraction, sea_ice_volume as (B, T, hw) fp32 or absent.  -> {name: (B, T, hw) fp32}."""
    f = {k: v for k, v in fields.items() if v is not None}
    out = {}
    one = F32(1)
    with np.errstate(all="ignore"):
        if any(n in want for n in OUTPUTS[:3]):
            S = column_sum(thetao, dz)                                           # (B, T, hw)
            ocean = mask0 > 0
            if "ocean_heat_content" in want:
                out["ocean_heat_content"] = np.where(ocean, S.astype(F32), F32(np.nan))
            tend = np.zeros(S.shape, F32)
            tend[:, 1:] = np.where(ocean, ((S[:, 1:] - S[:, :-1]) / dt_seconds).astype(F32), F32(np.nan))
            if head is not None:
                S_head = column_sum(head, dz) if any(h is not None for h in head) else np.zeros(S[:, 0].shape)
                tend[:, 0] = np.where(ocean, ((S[:, 0] - S_head) / dt_seconds).astype(F32), F32(np.nan))
            if "ocean_heat_content_tendency" in want:
                out["ocean_heat_content_tendency"] = tend
        land = f.get("land_fraction")
        ssf = f.get("sea_surface_fraction")
        if ssf is None and land is not None:
            ssf = one - land
        hfds = f.get("hfds")
        if hfds is None and "hfds_total_area" in f and ssf is not None:
            hfds = f["hfds_total_area"] / ssf
            if "hfds" in want:
                out["hfds"] = hfds
        if "net_energy_flux_into_ocean_column" in want or OUTPUTS[2] in want:
            geo = f.get("hfgeou", np.zeros_like(ssf))
            net = (hfds + geo) * ssf
            if "net_energy_flux_into_ocean_column" in want:
                out["net_energy_flux_into_ocean_column"] = net
            if OUTPUTS[2] in want:
                out[OUTPUTS[2]] = tend - net
        if "sea_ice_fraction" in want:
            out["sea_ice_fraction"] = f["ocean_sea_ice_fraction"] * (one - land)
        if "HI" in want:
            if "ocean_sea_ice_fraction" in f:
                frac = f["ocean_sea_ice_fraction"] * ssf
            else:
                frac = (f["sea_ice_fraction"] * ssf) / (one - land)
            out["HI"] = sea_ice_thickness(f["sea_ice_volume"], area_m2, frac)
    assert all(v.dtype == F32 for v in out.values()) and set(out) == set(want), (set(out), set(want))
    return out
