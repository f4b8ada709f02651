"""Synthetic oceans of any shape and their fp64 truth for the fused ocean corrector (csrc/ocean_phys.hip: launches O1 and O2).

``case`` generalises ``_cm4`` of test_gpu_ocean_corrector.py - land columns, NaN below the sea floor in the input's thetao,
fractions drawn outside [0, 1], negative values in the force-positive fields - to any grid, level count and combination of the
corrector's switches (``VARIANTS``); ``truth`` is ``OceanCorrector.torch_apply`` - the restatement that
test_ocean_corrector_cpu.py holds to the reference's golden outputs - run in fp64 and in fp32; ``ocean_buffers`` lays the planes
out on the device as the OceanRolloutEngine does and calls the corrector's fused path on them.  CPU only but for the last.

Three choices make a lost partial sum, a lost grid-stride tail or a wrong sample offset in the heat-content reduction move the
answer by much more than the bar (test_ocean_phys_ref_cpu.py measures each):
  - latitudes -60 .. 60: on a pole-to-pole grid the rows the last workgroups cover weigh almost nothing;
  - the generated temperatures are the draw times 1 + 0.01 (b + 1) + GRADIENT px / (H W): the local ratio of input to generated
    heat content then differs from the global one everywhere, and each sample's ratio from its neighbour's by about 1 %;
  - a 120-day step and a geothermal flux and an unaccounted heating of watts, not hundredths: the flux terms of the budget are
    1e-3 of the heat content, not 1e-6, so a wrong flux source or sea-surface fraction is visible too."""
import datetime
import functools
import zlib

import torch

# B, H, W, L: the smallest shapes at which each branch of the kernels is live (NT = 256 threads, NBLK_MAX = 512 workgroups)
SMALL_SHAPES = [
    (1, 4, 8, 1),        # one level, half a wave
    (2, 5, 13, 2),       # HW = 65: wave 1 holds one lane, waves 2 and 3 are empty
    (3, 9, 57, 4),       # 3 workgroups, the last holds one thread, odd W under px / W, max_batch = 3
]
LARGE_SHAPES = [
    (2, 180, 365, 8),    # 257 workgroups: second trip of O2's partial re-sum, at b = 1 too
    (2, 256, 512, 8),    # HW = NBLK_MAX * NT exactly
    (1, 182, 721, 64),   # capped at 512 workgroups, 150 threads make a second column trip in O1 and O2, ACE_OCEAN_MAX_LEVELS
]
BUDGET_VARIANTS = ["gen_total_area", "gen_hfds", "input_hfds", "input_total_area_ssf", "input_total_area_land"]
VARIANTS = BUDGET_VARIANTS + ["column_local"]
MAX_POSITIVE, MAX_ZERO = 40, 8       # ACE_OCEAN_MAX_POSITIVE, ACE_OCEAN_MAX_ZERO (include/ace_sfno.h)
BAR = 2e-6               # the bar _physics_ref.py holds the atmosphere kernels to
FLOOR_CAP = 1e-5         # 3 * floor may not pass this: keeps the GPU tolerance from growing quietly
GRADIENT = 0.5           # tuned until test_bar_sees_a_lost_partial holds (0.05: the grid-stride tail moves thetao by 6.8 x the bar only)
FLUXES = ["DLWRFsfc", "ULWRFsfc", "DSWRFsfc", "USWRFsfc", "LHTFLsfc", "SHTFLsfc", "PRATEsfc"]


def shape_variant_grid():
    return [(sh, v) for sh in SMALL_SHAPES for v in VARIANTS] + [(sh, v) for sh in LARGE_SHAPES for v in BUDGET_VARIANTS]


def shape_id(sh):
    return "B%d-%dx%dx%d" % sh


def variant(name, L):
    """what a variant puts into the step's output, input and forcing, its geometry switches and its corrector configuration"""
    so = [f"so_{k}" for k in range(min(L, 8))]
    th = [f"thetao_{k}" for k in range(L)]
    sif = {"sea_ice_fraction_name": "ocean_sea_ice_fraction", "land_fraction_name": "land_fraction"}
    ohc = lambda heating: {"method": "scaled_temperature", "constant_unaccounted_heating": heating}       # noqa: E731
    if name == "gen_total_area":
        # every correction; hfds "prescribed" on hfds_total_area (sea_surface_fraction in the forcing); flux source 0; hfgeou;
        # a provider mask for the heat content; unaccounted heating; sst in the output; the frozen rate as its total
        return dict(land=True, deptho=True, mask="mask_ocean_heat_content",
                    gen=so + th + ["sst", "zos", "HI", "ocean_sea_ice_fraction", "hfds_total_area"],
                    inp=th + ["sst", "ocean_sea_ice_fraction", "land_fraction", "HI"],
                    forcing=FLUXES + ["total_frozen_precipitation_rate", "sea_surface_fraction", "hfgeou"],
                    config={"force_positive_names": so + ["HI"],
                            "sea_ice_fraction_correction": {**sif, "zero_where_ice_free_names": ["HI"]},
                            "surface_energy_flux_correction": {"method": "prescribed"},
                            "ocean_heat_content_correction": ohc(3.0)})
    if name == "gen_hfds":
        # hfds "residual_prediction" on hfds (land_fraction in the forcing); sea_ice_fraction in the input; the frozen rate as its
        # three parts; flux source 1; no mask for the heat content (so no land columns), no deptho
        return dict(land=False, deptho=False, mask=None,
                    gen=so + th + ["sst", "zos", "hfds"],
                    inp=th + ["sst", "sea_ice_fraction", "land_fraction"],
                    forcing=FLUXES + ["ICEsfc", "GRAUPELsfc", "SNOWsfc", "land_fraction", "hfgeou"],
                    config={"force_positive_names": so, "surface_energy_flux_correction": {"method": "residual_prediction"},
                            "ocean_heat_content_correction": ohc(0.0)})
    if name == "input_hfds":
        # no flux correction; flux source 2; no sst in the output; no hfgeou; the sea-ice rebalance off
        return dict(land=True, deptho=True, mask="mask_2d",
                    gen=so + th + ["zos", "HI", "ocean_sea_ice_fraction"],
                    inp=th + ["sst", "hfds", "land_fraction"],
                    forcing=["land_fraction"],
                    config={"force_positive_names": so + ["HI"],
                            "sea_ice_fraction_correction": {**sif, "zero_where_ice_free_names": ["HI"],
                                                            "remove_negative_ocean_fraction": False},
                            "ocean_heat_content_correction": ohc(0.0)})
    if name == "input_total_area_ssf":
        return dict(land=True, deptho=True, mask="mask_2d", gen=th + ["sst", "zos"],
                    inp=th + ["hfds_total_area", "sea_surface_fraction"], forcing=["sea_surface_fraction", "hfgeou"],
                    config={"ocean_heat_content_correction": ohc(3.0)})
    if name == "input_total_area_land":
        return dict(land=False, deptho=True, mask=None, gen=th + ["sst"],
                    inp=th + ["hfds_total_area", "land_fraction"], forcing=["land_fraction", "hfgeou"],
                    config={"ocean_heat_content_correction": ohc(0.0)})
    if name == "column_local":
        # as many clamped and zeroed fields as the kernel takes, hfds without a frozen field (the zero fallback) and without the
        # heat budget: one launch.  tracer_39 and icevar_7 are in the output but in no list: they come back bitwise.
        tracers = [f"tracer_{i}" for i in range(MAX_POSITIVE)]
        icevars = [f"icevar_{i}" for i in range(MAX_ZERO)]
        return dict(land=True, deptho=True, mask="mask_2d",
                    gen=tracers + icevars + ["HI", "ocean_sea_ice_fraction", "hfds", "zos"],
                    inp=["sst", "ocean_sea_ice_fraction", "land_fraction"], forcing=FLUXES + ["PRESsfc"],
                    config={"force_positive_names": tracers[:MAX_POSITIVE - 1] + ["HI"],
                            "sea_ice_fraction_correction": {**sif, "zero_where_ice_free_names": ["HI"] + icevars[:MAX_ZERO - 1]},
                            "surface_energy_flux_correction": {"method": "residual_prediction"}})
    raise KeyError(name)


def _draw(part, name, B, H, W, L, mask):
    """one field, from a generator seeded by the shape, the part and the name: a name means the same data in every variant"""
    g = torch.Generator().manual_seed(zlib.crc32(f"{B}x{H}x{W}x{L}/{part}/{name}".encode()))
    r = lambda s=1.0, m=0.0: torch.randn(B, H, W, generator=g) * s + m                                 # noqa: E731
    u = lambda: torch.rand(B, H, W, generator=g)                                                      # noqa: E731
    if name in ("land_fraction", "sea_surface_fraction"):         # static: the same plane in the input and in the forcing
        land = 0.5 * torch.rand(B, H, W, generator=torch.Generator().manual_seed(zlib.crc32(f"{B}x{H}x{W}/land".encode())))
        return land if name == "land_fraction" else 1.0 - land
    if name.startswith("thetao_"):
        k = int(name[7:])
        t = r(2.0, 15.0 - 13.3 * k / L)                           # at 19 levels _cm4's 15 - 0.7 k
        if part == "input":
            return t.where(mask[..., k] > 0, float("nan"))        # NaN below the sea floor and on land
        px = torch.arange(H * W, dtype=torch.float32).reshape(H, W) / (H * W)
        b = torch.arange(1, B + 1, dtype=torch.float32).reshape(B, 1, 1)
        return t * (1.0 + 0.01 * b + GRADIENT * px)
    if name.startswith(("so_", "tracer_")):
        return r(1.0, 0.5)                                        # some negative
    if name.startswith("icevar_"):
        return r(0.5, 0.2)
    table = {
        "gen": {"sst": lambda: r(3.0, 290.0), "zos": lambda: r(0.3), "HI": lambda: r(0.5, 0.2),
                "ocean_sea_ice_fraction": lambda: 1.4 * u() - 0.2, "hfds": lambda: r(40.0, 25.0),
                "hfds_total_area": lambda: r(40.0, 20.0)},
        "input": {"sst": lambda: r(3.0, 290.0), "ocean_sea_ice_fraction": u, "sea_ice_fraction": lambda: 0.5 * u(),
                  "HI": lambda: r(0.5), "hfds": lambda: r(30.0, 25.0), "hfds_total_area": lambda: r(30.0, 15.0)},
        "forcing": {"DLWRFsfc": lambda: r(30.0, 330.0), "ULWRFsfc": lambda: r(30.0, 390.0), "DSWRFsfc": lambda: r(40.0, 180.0).abs(),
                    "USWRFsfc": lambda: r(10.0, 30.0).abs(), "LHTFLsfc": lambda: r(40.0, 80.0), "SHTFLsfc": lambda: r(15.0, 20.0),
                    "PRATEsfc": lambda: r(2e-5, 3e-5).abs(), "PRESsfc": lambda: r(1500.0, 98000.0),
                    "total_frozen_precipitation_rate": lambda: r(2e-5, 1e-5).abs(), "ICEsfc": lambda: r(1e-5, 4e-6).abs(),
                    "GRAUPELsfc": lambda: r(1e-5, 4e-6).abs(), "SNOWsfc": lambda: r(1e-5, 4e-6).abs(),
                    "hfgeou": lambda: r(0.5, 2.0)},
    }
    return table[part][name]()


def geometry(H, W, L, land):
    """interface depths whose thicknesses scale with 19 / L (4800 m in all at any L > 1, _cm4's at L = 19), a sea floor between 0
    and 1.25 times that - so every level is open in some columns and closed in others - and 30 % land columns or none"""
    g = torch.Generator().manual_seed(zlib.crc32(f"{H}x{W}x{L}/geometry".encode()))
    idepth = torch.cat([torch.zeros(1), torch.cumsum(torch.linspace(5.0, 500.0, L) * (19.0 / L), 0)])
    deptho = torch.rand(H, W, generator=g) * 1.25 * idepth[-1]
    dry = torch.rand(H, W, generator=g) < 0.3
    deptho = deptho.masked_fill(dry, 0.0) if land else deptho.clamp(min=0.5 * float(idepth[1]))
    mask = (deptho.unsqueeze(-1) > idepth[:-1]).float()
    return idepth, mask, deptho


@functools.lru_cache(maxsize=2)
def case(B, H, W, L, name):
    """the layout of tests/golden/gen_ocean_corrector_*.pt: config, grid, depth coordinate, provider masks, input / gen / forcing"""
    v = variant(name, L)
    idepth, mask, deptho = geometry(H, W, L, v["land"])
    masks = {v["mask"]: mask[..., 0].clone()} if v["mask"] else {}
    draw = lambda part, names: {n: _draw(part, n, B, H, W, L, mask) for n in names}                   # noqa: E731
    return {"config": v["config"], "lat": torch.linspace(-60.0, 60.0, H), "lon": torch.arange(W, dtype=torch.float32) * (360.0 / W),
            "idepth": idepth, "mask": mask, "deptho": deptho if v["deptho"] else None, "masks": masks,
            "timestep_seconds": datetime.timedelta(days=120).total_seconds(),
            "input": draw("input", v["inp"]), "gen": draw("gen", v["gen"]), "forcing": draw("forcing", v["forcing"])}


# ---- the truth ---------------------------------------------------------------------------------------------------------------
def _config(config):
    from ace_amd.ocean_corrector import OceanCorrectorConfig
    if isinstance(config, OceanCorrectorConfig):
        return config
    return OceanCorrectorConfig.from_state({"type": "ocean_corrector", "config": config})


def dataset_info(c, dtype=torch.float32, drop=None):
    """the geometry of a case.  In fp64 the fp32 area weights, dz and masks - what the kernels are given - are upcast, not
    recomputed.  ``drop`` (H x W bool): columns whose heat-content weight is zeroed, through the provider's own mask for
    "ocean_heat_content" (the area weights themselves must stay uniform along a row)."""
    from ace_amd.dataset_info import DatasetInfo
    from ace_amd.masking import SpatialMaskProvider
    from ace_amd.ocean_corrector import DepthCoordinate
    H, W = c["mask"].shape[:2]
    kw = dict(timestep=datetime.timedelta(seconds=c["timestep_seconds"]), lat=c["lat"], lon=c["lon"])
    depth = DepthCoordinate(c["idepth"], c["mask"], c["deptho"])
    masks = dict(c["masks"])
    if drop is not None:
        held = SpatialMaskProvider(masks).get_mask_tensor_for("ocean_heat_content")
        masks["mask_ocean_heat_content"] = (torch.ones(H, W) if held is None else held.clone()).masked_fill(drop, 0.0)
    if dtype == torch.float32:
        return DatasetInfo((H, W), mask_provider=SpatialMaskProvider(masks), depth_coordinate=depth, **kw)

    class Upcast(DepthCoordinate):
        def __init__(self):              # no recomputation: dz is the fp32 table, widened
            self.idepth, self.mask = depth.idepth.to(dtype), depth.mask.to(dtype)
            self.deptho = depth.deptho.to(dtype) if depth.deptho is not None else None
            self._dz = depth.dz.to(dtype)

        def to(self, device):
            return self

    area = DatasetInfo((H, W), **kw).area_weights
    assert area.dtype == torch.float32
    return DatasetInfo((H, W), area_weights=area.to(dtype), mask_provider=SpatialMaskProvider({k: m.to(dtype) for k, m in masks.items()}),
                       depth_coordinate=Upcast(), **kw)


def run(config, c, dtype, drop=None):
    corrector = _config(config).get_corrector(dataset_info(c, dtype, drop))
    cast = lambda d: {k: v.to(dtype) for k, v in d.items()}                                           # noqa: E731
    out = corrector.torch_apply(cast(c["input"]), cast(c["gen"]), cast(c["forcing"]))
    assert all(v.dtype == dtype for v in out.values())      # the restatement stays in the precision it is given
    return out


def truth(config, c):
    """The restatement on case ``c`` in fp64 and in fp32.  Returns
      fields    the fp64 corrected fields the truth CHANGES (every other field of gen comes back as it went in),
      nan       their NaN patterns (the fp32 leg's are the same: asserted),
      floor[k]  max|fp32 - fp64| / max|fp64| over the non-NaN points: how far the restatement's own fp32 arithmetic is from exact,
      fp32      every corrected field of the fp32 leg."""
    f64, f32 = run(config, c, torch.float64), run(config, c, torch.float32)
    gen = c["gen"]
    assert set(f64) == set(gen) == set(f32)
    fields = {k: v for k, v in f64.items() if not torch.equal(v, gen[k].double())}
    nan, floor = {}, {}
    for k, v in fields.items():
        nan[k] = torch.isnan(v)
        assert torch.equal(nan[k], torch.isnan(f32[k])), k
        ok = ~nan[k]
        floor[k] = float((f32[k].double() - v)[ok].abs().max() / v[ok].abs().max()) if ok.any() else 0.0
    return {"fields": fields, "nan": nan, "floor": floor, "fp32": f32}


@functools.lru_cache(maxsize=4)
def truth_for(shape, name):
    """``truth`` of the synthetic case of ``shape`` and variant ``name``, without the fp32 leg's fields (a large case is ~35 MB)"""
    c = case(*shape, name)
    t = truth(c["config"], c)
    del t["fp32"]
    return t


def tolerance(floor):
    return max(BAR, 3.0 * floor)


def rel_err(got, want):
    """max|got - want| / max|want| over the points where ``want`` is not NaN (0 when there is none)"""
    ok = ~torch.isnan(want)
    return float((got.double() - want)[ok].abs().max() / want[ok].abs().max()) if ok.any() else 0.0


# ---- the device side ---------------------------------------------------------------------------------------------------------
def ocean_buffers(dev, c, T=2):
    """The planes of a case laid out as the OceanRolloutEngine lays them out: every output a (B, T, H, W) tensor whose step
    T - 1 holds the generated field (a view with per-sample stride T * HW), the step's input a separate (B, 1, H, W) tensor, the
    forcing (B, T + 1, H, W) with the step's data at T.  The other steps hold different data, so that a read or a write at the
    wrong step shows.  Returns (inp, gen, forcing) dicts of views and ``whole``, the tensors they are views of."""
    s = T - 1
    whole = {"gen": {}, "input": {}, "forcing": {}}
    gen, inp, forcing = {}, {}, {}
    for n, v in c["gen"].items():
        t = whole["gen"][n] = torch.stack([v + 1.0 + i for i in range(s)] + [v], dim=1).to(dev).contiguous()
        gen[n] = t[:, s]
    for n, v in c["input"].items():
        t = whole["input"][n] = v.unsqueeze(1).to(dev).contiguous()
        inp[n] = t[:, 0]
    for n, v in c["forcing"].items():
        t = whole["forcing"][n] = torch.stack([v + 1.0 + i for i in range(T)] + [v], dim=1).to(dev).contiguous()
        forcing[n] = t[:, T]
    return inp, gen, forcing, whole


def fused_corrector(c):
    corrector = _config(c["config"]).get_corrector(dataset_info(c))
    assert corrector.fused
    return corrector
