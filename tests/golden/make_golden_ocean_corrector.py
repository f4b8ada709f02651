"""Golden vectors for the ocean corrector, emitted by the REAL reference (fme/core/corrector/ocean.py, fme/core/coordinates.py
DepthCoordinate, fme/core/gridded_ops.py LatLonOperations, fme/core/spatial_mask_provider.py) imported under the stubs of
oracle/ref_loader.load_corrector - build container only.  One small file per case, tests/golden/gen_ocean_corrector_<case>.pt:
the grid (lat / lon), the depth coordinate (idepth, mask, deptho or None), the provider's masks, the corrector config as a
checkpoint would carry it, the step's input / output / forcing in fp32, the reference's corrected output on those fp32
tensors, and the same correction run on float64 copies of everything, stored as its (fp16) difference from the fp32 output.
Only the fields a case's corrections read are stored, the 0 / 1 masks as bool, so each file stays small."""
import copy
import datetime
import importlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader  # noqa: E402

NLEV = 7
IDEPTH = [0.0, 10.0, 30.0, 60.0, 110.0, 220.0, 450.0, 900.0]
FLUXES = ["DLWRFsfc", "ULWRFsfc", "DSWRFsfc", "USWRFsfc", "LHTFLsfc", "SHTFLsfc", "PRATEsfc"]
SIF = {"sea_ice_fraction_name": "ocean_sea_ice_fraction", "land_fraction_name": "land_fraction"}


def geometry(seed, H, W, land: bool):
    g = torch.Generator().manual_seed(seed)
    deptho = torch.rand(H, W, generator=g) * 1000.0
    if land:
        deptho[torch.rand(H, W, generator=g) < 0.25] = 0.0          # land columns
    else:
        deptho = deptho.clamp(min=12.0)
    idepth = torch.tensor(IDEPTH)
    mask = (deptho.unsqueeze(-1) > idepth[:-1]).float()              # a level exists where the floor is below its top
    return idepth, mask, deptho


def fields(seed, B, H, W, mask, *, names, nan_below_floor=False, thetao=True, so=3):
    g = torch.Generator().manual_seed(seed)
    r = lambda scale=1.0, shift=0.0: torch.randn(B, H, W, generator=g) * scale + shift
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(B, H, W, generator=g)
    d = {}
    for k in range(NLEV):
        t = r(2.0, 14.0 - 1.5 * k)
        if nan_below_floor:
            t = t.where(mask[..., k] > 0, float("nan"))
        if thetao:
            d[f"thetao_{k}"] = t
    for k in range(3):
        s = r(0.3, 0.2 * k)                       # some negative values: force positive has work
        if k < so:
            d[f"so_{k}"] = s
    gen = {"sst": r(3.0, 290.0), "HI": r(0.5, 0.2), "ocean_sea_ice_fraction": u(-0.2, 1.2), "sea_ice_fraction": u(-0.2, 1.2),
           "hfds": r(40.0, 5.0), "hfds_total_area": r(40.0, 3.0), "zos": r(0.2)}
    for n in names:
        if n in gen:
            d[n] = gen[n]
    return d


def forcing_fields(seed, B, H, W, *, names):
    g = torch.Generator().manual_seed(seed)
    r = lambda scale=1.0, shift=0.0: torch.randn(B, H, W, generator=g) * scale + shift
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(B, H, W, generator=g)
    all_f = {"DLWRFsfc": r(30.0, 330.0), "ULWRFsfc": r(30.0, 390.0), "DSWRFsfc": r(40.0, 180.0).abs(), "USWRFsfc": r(10.0, 30.0).abs(),
             "LHTFLsfc": r(40.0, 80.0), "SHTFLsfc": r(15.0, 20.0), "PRATEsfc": r(2e-5, 3e-5).abs(),
             "total_frozen_precipitation_rate": r(1e-5, 1e-5).abs(), "PRESsfc": r(1500.0, 98000.0),
             "sea_surface_fraction": u(0.0, 1.0), "land_fraction": u(0.0, 1.0), "hfgeou": r(0.02, 0.08), "hfds": r(30.0)}
    return {n: all_f[n] for n in names}


CASES = {
    # the CM4 piControl uncoupled ocean's options (force positive so_* and HI; sea-ice fraction without rebalance)
    "cm4_shipped": dict(shape=(46, 92), land=True, gen=["HI", "ocean_sea_ice_fraction"],
                        inp=["ocean_sea_ice_fraction", "land_fraction"], forcing=["land_fraction"],
                        config={"force_positive_names": ["so_0", "so_1", "HI"],
                                "sea_ice_fraction_correction": {**SIF, "remove_negative_ocean_fraction": False}}),
    "rebalance_zero_thickness": dict(shape=(23, 46), land=True, gen=["HI", "ocean_sea_ice_fraction"],
                                     inp=["HI", "ocean_sea_ice_fraction", "land_fraction"], forcing=["land_fraction"],
                                     config={"sea_ice_fraction_correction": {**SIF, "zero_where_ice_free_names": ["HI"]}}),
    "hfds_residual": dict(shape=(23, 46), land=True, gen=["sst", "hfds"], inp=["sst", "sea_ice_fraction", "land_fraction"],
                          forcing=FLUXES + ["total_frozen_precipitation_rate", "land_fraction"],
                          config={"surface_energy_flux_correction": {"method": "residual_prediction"}}),
    "hfds_prescribed_total_area": dict(shape=(23, 46), land=True, gen=["sst", "hfds_total_area"],
                                       inp=["sst", "ocean_sea_ice_fraction", "land_fraction"],
                                       forcing=FLUXES + ["PRESsfc", "sea_surface_fraction"],
                                       config={"surface_energy_flux_correction": {"method": "prescribed"}}),
    "ohc_gen_total_area_deptho_mask2d": dict(shape=(23, 46), land=True, deptho=True, mask_2d=True, gen=["sst", "hfds_total_area"],
                                             inp=["sst"], forcing=["sea_surface_fraction", "hfgeou"],
                                             config={"ocean_heat_content_correction": {"method": "scaled_temperature",
                                                                                       "constant_unaccounted_heating": 0.4}}),
    "ohc_gen_hfds_no_deptho": dict(shape=(23, 46), land=False, deptho=False, mask_2d=False, gen=["sst", "hfds"], inp=["sst"],
                                   forcing=["land_fraction", "hfgeou"],
                                   config={"ocean_heat_content_correction": {"method": "scaled_temperature"}}),
    "ohc_input_hfds_mask2d": dict(shape=(23, 46), land=True, deptho=False, mask_2d=True, gen=["zos"], inp=["sst", "hfds"],
                                  forcing=["land_fraction"], config={"ocean_heat_content_correction": {"method": "scaled_temperature"}}),
    "ohc_input_total_area": dict(shape=(23, 46), land=False, deptho=True, mask_2d=False, gen=["sst"],
                                 inp=["sst", "hfds_total_area", "land_fraction"], forcing=["sea_surface_fraction", "hfgeou"],
                                 config={"ocean_heat_content_correction": {"method": "scaled_temperature"}}),
    # a legacy checkpoint's config: ``masking``, the boolean heat-content option, ``sea_ice_thickness_name``; every correction
    "legacy_bool_all": dict(shape=(17, 34), land=True, deptho=True, mask_2d=True, gen=["sst", "HI", "ocean_sea_ice_fraction", "hfds"],
                            inp=["sst", "HI", "ocean_sea_ice_fraction", "land_fraction"],
                            forcing=FLUXES + ["total_frozen_precipitation_rate", "land_fraction", "sea_surface_fraction", "hfgeou"],
                            config={"masking": {"mask_value": 0}, "force_positive_names": ["so_0", "so_1"],
                                    "sea_ice_fraction_correction": {**SIF, "sea_ice_thickness_name": "HI"},
                                    "surface_energy_flux_correction": {"method": "residual_prediction"},
                                    "ocean_heat_content_correction": True}),
}


def build_config(oc, state):
    state = oc.OceanCorrectorConfig.remove_deprecated_keys(copy.deepcopy(state))
    sub = {"sea_ice_fraction_correction": oc.SeaIceFractionConfig,
           "surface_energy_flux_correction": oc.SurfaceEnergyFluxCorrectionConfig,
           "ocean_heat_content_correction": oc.OceanHeatContentBudgetConfig}
    for k, cls in sub.items():
        if isinstance(state.get(k), dict):
            state[k] = cls(**state[k])
    return oc.OceanCorrectorConfig(**state)


def run(ref, oc, coords, smp, case, dtype, idepth, mask, deptho, masks, lat, lon, inp, gen, forcing):
    c = lambda d: {k: v.to(dtype) for k, v in d.items()}
    provider = smp.SpatialMaskProvider(c(masks))
    ops = ref.LatLonCoordinates(lat=lat.to(dtype), lon=lon.to(dtype)).get_gridded_operations(provider)
    depth = coords.DepthCoordinate(idepth.to(dtype), mask.to(dtype), deptho.to(dtype) if deptho is not None else None)
    corrector = build_config(oc, case["config"])._build(ops, depth, datetime.timedelta(days=5))
    return corrector(c(inp), c(gen), c(forcing), None).corrected


def main():
    ref = ref_loader.load_corrector()
    oc = importlib.import_module("fme.core.corrector.ocean")
    coords = importlib.import_module("fme.core.coordinates")
    smp = importlib.import_module("fme.core.spatial_mask_provider")
    B = 2
    for i, (name, case) in enumerate(CASES.items()):
        H, W = case["shape"]
        lat = torch.linspace(-89.0 + 90.0 / H, 89.0 - 90.0 / H, H)
        lon = torch.arange(W) * (360.0 / W)
        idepth, mask, deptho = geometry(100 + i, H, W, case["land"])
        masks = {"mask_2d": mask[..., 0].clone()} if case.get("mask_2d") else {}
        for k in range(NLEV):
            masks[f"mask_{k}"] = mask[..., k].clone()                 # level masks: not used by the heat-content mean
        n_so = sum(n.startswith("so_") for n in case["config"].get("force_positive_names", []))
        kw = dict(thetao="ocean_heat_content_correction" in case["config"], so=n_so)
        inp = fields(200 + i, B, H, W, mask, names=case["inp"], nan_below_floor=True, **{**kw, "so": 0})   # input salinity: unused
        gen = fields(300 + i, B, H, W, mask, names=case["gen"], **kw)
        forcing = forcing_fields(400 + i, B, H, W, names=case["forcing"])
        if "land_fraction" in case["inp"]:      # static: the forcing's own field where it has one
            inp["land_fraction"] = forcing.get("land_fraction", 0.5 * torch.rand(B, H, W, generator=torch.Generator().manual_seed(i)))
        dep = deptho if case.get("deptho") else None
        args = (idepth, mask, dep, masks, lat, lon, inp, gen, forcing)
        out32 = run(ref, oc, coords, smp, case, torch.float32, *args)
        out64 = run(ref, oc, coords, smp, case, torch.float64, *args)
        changed = sorted(k for k in out32 if not torch.equal(out32[k], gen[k]))
        depth64 = coords.DepthCoordinate(idepth.double(), mask.double(), dep.double() if dep is not None else None)
        # the masks are 0 / 1: stored as bool (the tests read them back as float32)
        record = {"config": case["config"], "lat": lat, "lon": lon, "idepth": idepth, "mask": mask.bool(), "deptho": dep,
                  "masks": {k: v.bool() for k, v in masks.items()},
                  "timestep_seconds": datetime.timedelta(days=5).total_seconds(), "input": inp, "gen": gen, "forcing": forcing,
                  "expected": {k: out32[k].clone() for k in changed},
                  "expected64_minus_32": {k: (out64[k] - out32[k].double()).half() for k in changed},
                  "dz": depth64.dz.float() if kw["thetao"] else None}
        path = os.path.join(HERE, f"gen_ocean_corrector_{name}.pt")
        torch.save(record, path)
        print(f"{name}: modified {changed}; wrote {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
