"""Golden vectors for the ocean's derived variables, emitted by the REAL reference (fme/core/ocean_derived_variables.py,
fme/core/ocean_data.py, ``DepthCoordinate.build_derive_function`` and ``LatLonCoordinates`` of fme/core/coordinates.py) imported
under the stubs of oracle/ref_loader.load_corrector - build container only.  One file, tests/golden/gen_ocean_derived.pt: per case
of tests/_ocean_derive_cases.py the geometry (idepth, mask, deptho or None, the reference's fp32 dz and cell areas), the fields,
the variables the reference adds on the fp32 fields and the same on float64 copies of everything.

The cases with special values of the cell area cannot come from a grid: they call the reference's
``compute_ocean_derived_quantities`` with a cell-area provider that holds the grid's areas times the case's factor.

Asserted here, for the reference itself (fp32 against its own fp64 run): its share of each bar that
tests/test_ocean_derive_ref_cpu.py gives the contract, so a bar that the reference's rounding alone would exhaust is seen at
generation.  u = 2^-24, L levels, A = CP RHO sum_k |thetao_k| dz_k:
  ocean_heat_content                 |f32 - f64| <= (L + 2) u A
  ocean_heat_content_tendency        |f32 - f64| <= (L + 2) u (A_t + A_{t-1}) / dt + u |f64|
  implied advective tendency         the same + u |f64| + the net flux's own difference
  HI at finite positive inputs       |f32 - f64| <= (2 u M + u) |f64|,  M = 9 ln 10 + |ln vol| + |ln area| + |ln frac|"""
import datetime
import importlib
import math
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_loader  # noqa: E402
import _ocean_derive_cases as C  # noqa: E402

U = 2.0 ** -24
CP_RHO = 3992.0 * 1035.0


def run(ref, coords, odv, case, dtype, idepth, mask, deptho, data, forcing):
    c = lambda d: {k: v.to(dtype) for k, v in d.items()}                                            # noqa: E731
    lat, lon = C.latlon()
    hc = ref.LatLonCoordinates(lat=lat.to(dtype), lon=lon.to(dtype))
    depth = coords.DepthCoordinate(idepth.to(dtype), mask.to(dtype), deptho.to(dtype) if deptho is not None else None)
    timestep = datetime.timedelta(seconds=C.TIMESTEP_SECONDS)
    if case.get("special"):
        provider = types.SimpleNamespace(area_weights_m2=hc.area_weights_m2 * C.area_factor(case).to(dtype))
        out = odv.compute_ocean_derived_quantities(c(data), depth, timestep, forcing_data=c(forcing), cell_area_provider=provider)
        area = provider.area_weights_m2
    else:
        out = depth.build_derive_function(timestep, hc)(c(data), c(forcing))
        area = hc.area_weights_m2
    return {k: v for k, v in out.items() if k not in data}, depth.dz, area


def check_reference_share(name, case, d32, d64, dz, area, data, forcing):
    L = C.NLEV
    dt = C.TIMESTEP_SECONDS
    if "ocean_heat_content" in d32:
        th = torch.stack([data[n] for n in C.THETAO], dim=-1).double()
        A = CP_RHO * (th.abs() * dz.double()).nansum(dim=-1)
        ok = ~torch.isnan(d64["ocean_heat_content"])
        err = (d32["ocean_heat_content"].double() - d64["ocean_heat_content"]).abs()
        assert bool((err[ok] <= ((L + 2) * U * A)[ok]).all()), name
        bar = (L + 2) * U * (A[:, 1:] + A[:, :-1]) / dt + U * d64["ocean_heat_content_tendency"][:, 1:].abs()
        err = (d32["ocean_heat_content_tendency"].double() - d64["ocean_heat_content_tendency"])[:, 1:].abs()
        assert bool((err[ok[:, 1:]] <= bar[ok[:, 1:]]).all()), name
        key = "implied_tendency_of_ocean_heat_content_due_to_advection"
        if key in d32:
            net = (d32["net_energy_flux_into_ocean_column"].double() - d64["net_energy_flux_into_ocean_column"]).abs()[:, 1:]
            err = (d32[key].double() - d64[key])[:, 1:].abs()
            assert bool((err[ok[:, 1:]] <= (bar + U * d64[key][:, 1:].abs() + net)[ok[:, 1:]]).all()), name
    if "HI" in d32 and not case.get("special"):
        merged = {**forcing, **data}
        ssf = merged["sea_surface_fraction"] if "sea_surface_fraction" in merged else 1 - merged["land_fraction"]
        if "ocean_sea_ice_fraction" in merged:
            frac = merged["ocean_sea_ice_fraction"] * ssf
        else:
            frac = merged["sea_ice_fraction"] * ssf / (1 - merged["land_fraction"])
        M = 9 * math.log(10) + merged["sea_ice_volume"].double().log().abs() + area.double().log().abs() + frac.double().log().abs()
        rel = (d32["HI"].double() - d64["HI"]).abs() / d64["HI"].abs()
        assert bool((rel <= 2 * U * M + U).all()), (name, float((rel / (U * M)).max()))


def main():
    ref = ref_loader.load_corrector()
    coords = importlib.import_module("fme.core.coordinates")
    odv = importlib.import_module("fme.core.ocean_derived_variables")
    record = {"timestep_seconds": C.TIMESTEP_SECONDS, "cases": {}}
    for i, name in enumerate(C.CASES):
        case, idepth, mask, deptho, data, forcing = C.case_inputs(i, name)
        d32, dz, area = run(ref, coords, odv, case, torch.float32, idepth, mask, deptho, data, forcing)
        d64, _, _ = run(ref, coords, odv, case, torch.float64, idepth, mask, deptho, data, forcing)
        assert tuple(d32) == tuple(n for n in C.OUTPUTS if n in case["derived"]), (name, list(d32))
        assert all(v.dtype == torch.float32 for v in d32.values()) and all(v.dtype == torch.float64 for v in d64.values())
        for k in d32:
            assert torch.equal(torch.isnan(d32[k]), torch.isnan(d64[k])), (name, k)
        check_reference_share(name, case, d32, d64, dz, area, data, forcing)
        if case.get("special"):
            got = d32["HI"].reshape(C.B, C.T, C.HW)[0, 0, :len(C.SPECIAL_ROWS)]
            want = torch.tensor(C.SPECIAL_EXPECTED)
            assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(-1.0), want.nan_to_num(-1.0)), \
                (name, got.tolist())
        record["cases"][name] = {"idepth": idepth, "mask": mask.bool(), "deptho": deptho, "dz": dz.clone(), "area_m2": area.clone(),
                                 "data": data, "forcing": forcing, "expected": d32, "expected64": d64}
        print(f"{name}: derived {list(d32)}")
    path = os.path.join(HERE, "gen_ocean_derived.pt")
    torch.save(record, path)
    print(f"wrote {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
