"""The cases of tests/golden/gen_ocean_derived.pt, shared by its generator (tests/golden/make_golden_ocean_derived.py, which runs the
reference on them) and the tests that read it: B = 2, 5 time levels, 4 x 8 pixels, 7 levels on the interface depths of
tests/golden/make_golden_ocean_corrector.py, a 5-day timestep.  Every case is a seeded set of ``data`` and ``forcing`` fields
(B, T, H, W) and a geometry; what is derived follows from the names present, as in the reference."""
import numpy as np
import torch

B, T, H, W, NLEV = 2, 5, 4, 8, 7
HW = H * W
IDEPTH = [0.0, 10.0, 30.0, 60.0, 110.0, 220.0, 450.0, 900.0]
TIMESTEP_SECONDS = 5 * 86400.0
FLT_MAX = float(np.finfo(np.float32).max)
OUTPUTS = ("ocean_heat_content", "ocean_heat_content_tendency", "implied_tendency_of_ocean_heat_content_due_to_advection",
           "net_energy_flux_into_ocean_column", "sea_ice_fraction", "HI", "hfds")
THETAO = [f"thetao_{k}" for k in range(NLEV)]

# name -> what the case holds; ``derived``: the variables the reference adds (asserted by the generator)
CASES = {
    # hfds present, sea_surface_fraction present, hfgeou present; partial bottom cells from deptho; land; NaN below the floor
    "budget_hfds_ssf_geo": dict(deptho=True, land=True, nan_below_floor=True, data=THETAO + ["hfds"],
                                forcing=["sea_surface_fraction", "hfgeou"],
                                derived=OUTPUTS[:4]),
    # hfds from hfds_total_area, sea-surface fraction from land_fraction, no hfgeou; no deptho
    "budget_total_area_land": dict(deptho=False, land=True, nan_below_floor=False, data=THETAO + ["hfds_total_area"],
                                   forcing=["land_fraction"], derived=OUTPUTS[:4] + ("hfds",)),
    # sea_ice_fraction derived; HI from ocean_sea_ice_fraction (sea-surface fraction from land_fraction); no thetao: heat content skipped
    "ice_from_ocean_fraction": dict(deptho=True, land=True, data=["ocean_sea_ice_fraction", "sea_ice_volume"],
                                    forcing=["land_fraction"], derived=("sea_ice_fraction", "HI")),
    # sea_ice_fraction present (left as it is); HI from sea_ice_fraction * ssf / (1 - land)
    "ice_from_total_fraction": dict(deptho=True, land=True, data=["sea_ice_fraction", "sea_ice_volume"],
                                    forcing=["land_fraction", "sea_surface_fraction"], derived=("HI",)),
    # the special rows of HI's table, both routes (the cell areas of this case carry special values too)
    "hi_special_ocean_fraction": dict(deptho=True, land=True, data=["ocean_sea_ice_fraction", "sea_ice_volume"],
                                      forcing=["sea_surface_fraction"], derived=("HI",), special="ocean_fraction"),
    "hi_special_total_fraction": dict(deptho=True, land=True, data=["sea_ice_fraction", "sea_ice_volume"],
                                      forcing=["land_fraction", "sea_surface_fraction"], derived=("HI",), special="total_fraction"),
    # inputs missing: only the heat content and its tendency can be computed
    "thetao_only": dict(deptho=False, land=True, nan_below_floor=True, data=THETAO + ["zos"], forcing=["hfgeou"],
                        derived=OUTPUTS[:2]),
    # all seven
    "all_seven": dict(deptho=True, land=True, nan_below_floor=True,
                      data=THETAO + ["hfds_total_area", "ocean_sea_ice_fraction", "sea_ice_volume"],
                      forcing=["land_fraction", "hfgeou"], derived=OUTPUTS),
}

# (vol, fraction, area factor) of the special pixels: the area is the grid's own times the factor (nan: NaN)
_INF, _NAN = float("inf"), float("nan")
SPECIAL_ROWS = [(_NAN, 0.5, 1.0), (-1.0, 0.5, 1.0), (1.0, -0.5, 1.0), (1.0, _NAN, 1.0), (1.0, 0.5, _NAN), (1.0, 0.5, -1.0),
                (0.0, 0.5, 1.0), (0.0, 0.0, 1.0), (0.0, _INF, 1.0), (1.0, _INF, 1.0), (1.0, 0.0, 1.0), (_INF, 0.5, 1.0),
                (1e30, 1e-30, 1.0), (_NAN, _NAN, 1.0), (_INF, 0.0, 1.0), (-0.0, 0.5, 1.0)]
SPECIAL_EXPECTED = [_NAN, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, FLT_MAX, FLT_MAX, FLT_MAX, _NAN, FLT_MAX, 0.0]


def latlon():
    lat = torch.linspace(-89.0 + 90.0 / H, 89.0 - 90.0 / H, H)
    lon = torch.arange(W) * (360.0 / W)
    return lat, lon


def geometry(seed: int, deptho: bool, land: bool):
    """(idepth, mask (H, W, L), deptho or None)"""
    g = torch.Generator().manual_seed(seed)
    floor = torch.rand(H, W, generator=g) * 1000.0
    if land:
        floor[torch.rand(H, W, generator=g) < 0.25] = 0.0
    else:
        floor = floor.clamp(min=12.0)
    idepth = torch.tensor(IDEPTH)
    mask = (floor.unsqueeze(-1) > idepth[:-1]).float()
    return idepth, mask, (floor if deptho else None)


def fields(seed: int, case, mask):
    """(data, forcing): name -> (B, T, H, W) fp32"""
    g = torch.Generator().manual_seed(seed)
    r = lambda scale=1.0, shift=0.0: torch.randn(B, T, H, W, generator=g) * scale + shift          # noqa: E731
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(B, T, H, W, generator=g)                         # noqa: E731
    every = {}
    for k in range(NLEV):
        t = r(2.0, 14.0 - 1.5 * k)
        if case.get("nan_below_floor"):
            t = t.where(mask[..., k] > 0, float("nan"))
        every[f"thetao_{k}"] = t
    every.update({"hfds": r(40.0, 5.0), "hfds_total_area": r(40.0, 3.0), "hfgeou": r(0.02, 0.08), "zos": r(0.2),
                  "sea_surface_fraction": u(0.1, 1.0), "land_fraction": u(0.0, 0.9), "ocean_sea_ice_fraction": u(0.05, 1.0),
                  "sea_ice_fraction": u(0.05, 0.9), "sea_ice_volume": u(0.01, 5.0)})
    data = {n: every[n] for n in case["data"]}
    forcing = {n: every[n] for n in case["forcing"]}
    special = case.get("special")
    if special:                                             # sample 0, step 0: pixel j is row j of SPECIAL_ROWS
        n = len(SPECIAL_ROWS)
        vol = torch.tensor([row[0] for row in SPECIAL_ROWS])
        frac = torch.tensor([row[1] for row in SPECIAL_ROWS])
        data["sea_ice_volume"].view(B, T, HW)[0, 0, :n] = vol
        forcing["sea_surface_fraction"].view(B, T, HW)[0, 0, :n] = 1.0
        if special == "ocean_fraction":
            data["ocean_sea_ice_fraction"].view(B, T, HW)[0, 0, :n] = frac
        else:                                               # frac = sif * 1 / (1 - 0); then 1 - land NaN and 1 - land = 0 on step 1
            data["sea_ice_fraction"].view(B, T, HW)[0, 0, :n] = frac
            forcing["land_fraction"].view(B, T, HW)[0, 0, :n] = 0.0
            forcing["land_fraction"].view(B, T, HW)[0, 1, 0] = float("nan")
            forcing["land_fraction"].view(B, T, HW)[0, 1, 1] = 1.0
    return data, forcing


def area_factor(case):
    """(H, W) factor on the grid's cell areas: 1 but at the special pixels"""
    f = torch.ones(HW)
    if case.get("special"):
        f[:len(SPECIAL_ROWS)] = torch.tensor([row[2] for row in SPECIAL_ROWS])
    return f.view(H, W)


def case_inputs(i: int, name: str):
    case = CASES[name]
    idepth, mask, deptho = geometry(500 + i, case["deptho"], case["land"])
    data, forcing = fields(600 + i, case, mask)
    return case, idepth, mask, deptho, data, forcing
