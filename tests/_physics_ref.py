"""Synthetic atmospheres of any shape and their fp64 truth for the fused post-step physics kernels (csrc/physics.hip).

``synthetic`` is the generator of tests/golden/make_golden_corrector.py with the grid and the layer count free (at 2 x 8 x 16 x 4 it
is that generator, bit for bit: test_physics_ref_cpu.py), ``case`` arranges four draws as the golden file arranges them (step
input, two generated states, next-step forcing), ``truth`` is ``ace_amd.corrector.AtmosphereCorrector`` - the torch restatement
that test_corrector_cpu.py holds to the reference's own vectors at 1e-6 - run in fp64 and in fp32, and ``physics_buffers`` lays
the fields out on the device as the RolloutEngine does and puts a ``FusedPhysics`` over them.  CPU only but for the last."""
import datetime
import functools

import torch

from test_corrector_cpu import CONFIGS

# B, H, W, NZ: the smallest shapes at which each branch of the kernels is live (NT = 256 threads, NBLK_MAX = 512 workgroups)
SMALL_SHAPES = [
    (1, 4, 8, 1),        # one layer, half a wave
    (2, 5, 13, 2),       # HW = 65: wave 1 holds one lane, waves 2 and 3 are empty
    (3, 9, 57, 4),       # nblk = 3, last block one thread, odd W, max_batch = 3
]
LARGE_SHAPES = [
    (2, 180, 360, 8),    # the headline grid, nblk = 254
    (2, 180, 365, 8),    # nblk = 257: second trip of block_load_sums
    (2, 256, 512, 8),    # HW = NBLK_MAX * NT exactly: no second column trip
    (1, 182, 721, 16),   # nblk capped at 512, grid-stride second trip for 150 threads, ACE_PHYS_MAX_LEVELS
]
LARGE_CONFIGS = ["ace2_like", "moisture_advection_and_evaporation", "zero_advection", "energy"]   # every reduction slot of every pass
VARIANT_SHAPES = [(3, 9, 57, 4), (2, 180, 365, 8)]      # frozen parts + geopotential; carried dry-air reference
# The draws of a case are seeds SEED0 + 1 .. + 4 (the golden file: 1 .. 4).  At 4 x 8 x 1 seeds 1 .. 4 happen to make the global
# tendency of the water path cancel the precipitation to 1 %, so the evaporation scale - and with it the whole corrected
# LHTFLsfc, the denominator of its relative error - is near zero and the restatement's own fp32 floor is 1.8e-5.  The next four
# seeds give an ordinary sample (floors <= 2.1e-7): the inputs change, not the cap.
SEED0 = {(1, 4, 8, 1): 4}
BAR = 2e-6               # the bar test_fused_physics_vs_reference_corrector holds at 8 x 16
FLOOR_CAP = 1e-5         # 3 * floor may not pass this: keeps the GPU tolerance from growing quietly


def shape_config_grid():
    return [(sh, name) for sh in SMALL_SHAPES for name in sorted(CONFIGS)] + [(sh, name) for sh in LARGE_SHAPES for name in LARGE_CONFIGS]


def shape_id(sh):
    return "B%d-%dx%dx%d" % sh


def synthetic(seed, B=2, H=8, W=16, NZ=4, frozen="total", height="HGTsfc"):
    """make_golden_corrector.synthetic: same fields, draw order and magnitudes; the vertical profiles scale with NZ so that a
    column stays physical (at NZ = 4 they are the golden's)."""
    assert frozen in ("total", "parts") and height in ("HGTsfc", "PHIS")
    g = torch.Generator().manual_seed(seed)
    r = lambda scale=1.0, shift=0.0: torch.randn(B, H, W, generator=g) * scale + shift            # noqa: E731
    d = {"PRESsfc": r(1500.0, 98000.0), "HGTsfc": r(300.0, 200.0), "DSWRFtoa": r(50.0, 340.0).abs(),
         "PRATEsfc": (r(2e-5, 3e-5)), "LHTFLsfc": r(40.0, 80.0), "SHTFLsfc": r(15.0, 20.0),
         "tendency_of_total_water_path_due_to_advection": r(2e-5)}
    if frozen == "total":
        d["total_frozen_precipitation_rate"] = r(2e-5, 1e-5).abs()
    else:
        for n in ("ICEsfc", "GRAUPELsfc", "SNOWsfc"):
            d[n] = r(1e-5, 4e-6).abs()
    d.update({"DSWRFsfc": r(40.0, 180.0).abs(), "USWRFsfc": r(10.0, 30.0).abs(), "DLWRFsfc": r(30.0, 330.0),
              "ULWRFsfc": r(30.0, 390.0), "ULWRFtoa": r(20.0, 240.0), "USWRFtoa": r(15.0, 100.0).abs()})
    for k in range(NZ):
        d[f"specific_total_water_{k}"] = r(4e-3 / NZ, 8e-3 * (k + 1) / NZ)
        d[f"air_temperature_{k}"] = r(5.0, 220.0 + 80.0 * k / NZ)
    if height == "PHIS":
        d["PHIS"] = 9.80616 * d.pop("HGTsfc")
    return d


def geometry(H, W, NZ):
    """cell-centred latitudes (a pole at exactly +-90 has a tiny negative cosine weight in fp32), ak piecewise linear
    100 -> 12000 -> 0 Pa and bk quadratic over the NZ + 1 interfaces, six-hour step"""
    x = torch.linspace(0.0, 1.0, NZ + 1)
    ak = torch.where(x <= 0.5, 100.0 + (12000.0 - 100.0) * x / 0.5, 12000.0 * (1.0 - x) / 0.5)
    return {"lat": torch.linspace(-90.0 + 90.0 / H, 90.0 - 90.0 / H, H), "lon": torch.arange(W, dtype=torch.float32) * 360.0 / W,
            "ak": ak, "bk": x ** 2, "timestep_seconds": datetime.timedelta(hours=6).total_seconds()}


@functools.lru_cache(maxsize=2)
def case(B, H, W, NZ, frozen="total", height="HGTsfc"):
    """the layout of gen_corrector.pt: input0 (state + forcing), gen0, gen1 (no forcing-only fields), forcing"""
    hname = height
    kw = dict(B=B, H=H, W=W, NZ=NZ, frozen=frozen, height=height)
    s0 = SEED0.get((B, H, W, NZ), 0)
    inp0, gen0, gen1 = synthetic(s0 + 1, **kw), synthetic(s0 + 2, **kw), synthetic(s0 + 3, **kw)
    forcing = {"DSWRFtoa": synthetic(s0 + 4, **kw)["DSWRFtoa"], hname: inp0[hname]}
    for d in (gen0, gen1):
        del d["DSWRFtoa"], d[hname]
    return {**geometry(H, W, NZ), "input0": {**inp0, **forcing}, "gen0": gen0, "gen1": gen1, "forcing": forcing}


def config_for(name, NZ):
    """CONFIGS[name] with only the levels that exist in force_positive_names"""
    cfg = dict(CONFIGS[name])
    if "force_positive_names" in cfg:
        cfg["force_positive_names"] = [n for n in cfg["force_positive_names"]
                                       if not n.startswith("specific_total_water_") or int(n.rsplit("_", 1)[1]) < NZ]
    return cfg


def dataset_info(c, dtype=torch.float32):
    """the geometry of a case; in fp64 the fp32 weights and coefficients (what the kernels are given) upcast, not recomputed"""
    import ace_amd
    H, W = c["input0"]["PRESsfc"].shape[-2:]
    info = ace_amd.DatasetInfo((H, W), timestep=datetime.timedelta(seconds=c["timestep_seconds"]), lat=c["lat"], lon=c["lon"],
                               ak=c["ak"], bk=c["bk"])
    if dtype == torch.float32:
        return info
    return ace_amd.DatasetInfo((H, W), timestep=datetime.timedelta(seconds=c["timestep_seconds"]), lat=c["lat"], lon=c["lon"],
                               ak=c["ak"].to(dtype), bk=c["bk"].to(dtype), area_weights=info.area_weights.to(dtype))


def _run(config, c, dtype, steps, mass):
    from ace_amd.corrector import AtmosphereCorrectorConfig, CorrectorState
    corrector = AtmosphereCorrectorConfig.from_state(config).get_corrector(dataset_info(c, dtype))
    cast = lambda d: {k: v.to(dtype) for k, v in d.items()}                                       # noqa: E731
    forcing = cast(c["forcing"])
    inp = cast(c["input0"])
    state = None if mass is None else CorrectorState(global_dry_air_mass=mass.reshape(-1, 1, 1).to(torch.float64))
    out = []
    for s in range(steps):
        corrected, state = corrector(inp, cast(c[f"gen{s}"]), forcing, state)
        out.append(corrected)
        inp = {**corrected, **forcing}          # the next step's input: this step's corrected output plus the forcing
    got = None if state is None else state.global_dry_air_mass
    assert all(v.dtype == dtype for st in out for v in st.values())     # the restatement stays in the precision it is given
    assert got is None or got.dtype == torch.float64
    return out, got


def truth(config, c, steps=2, mass=None):
    """The restatement on ``steps`` chained steps of case ``c``, in fp64 and in fp32.  Returns
      fields[s]   the fp64 corrected fields the truth CHANGES (every other field of gen{s} comes back as it went in),
      mass        the fp64 global dry-air mass the state carries (None when conserve_dry_air is off),
      floor[s][k] max|fp32 - fp64| / max|fp64|: how far the restatement's own fp32 arithmetic is from exact (the same idea as
                  _util.conditioning_floor),
      fp32[s]     every corrected field of the fp32 leg; mass32 its carried mass (fp64 mean of fp32 columns).
    ``mass`` carries a CorrectorState in from a previous window."""
    f64, m64 = _run(config, c, torch.float64, steps, mass)
    f32, m32 = _run(config, c, torch.float32, steps, mass)
    fields, floor = [], []
    for s in range(steps):
        gen = c[f"gen{s}"]
        assert set(f64[s]) == set(gen) == set(f32[s])
        changed = {k: v for k, v in f64[s].items() if not torch.equal(v, gen[k].double())}
        fields.append(changed)
        floor.append({k: float((f32[s][k].double() - v).abs().max() / v.abs().max()) for k, v in changed.items()})
    return {"fields": fields, "mass": m64, "floor": floor, "fp32": f32, "mass32": m32}


@functools.lru_cache(maxsize=4)
def truth_for(shape, name, frozen="total", height="HGTsfc"):
    """``truth`` of CONFIGS[name] on the synthetic case of ``shape``, without the fp32 leg's fields (a large case is ~100 MB)"""
    t = truth(config_for(name, shape[3]), case(*shape, frozen=frozen, height=height))
    del t["fp32"]
    return t


def tolerance(floor):
    return max(BAR, 3.0 * floor)


# ---- the device side ---------------------------------------------------------------------------------------------------------
def physics_buffers(dev, c, config, T=2):
    """Static buffers laid out as the RolloutEngine lays them out - (B, T, H, W) output planes with per-sample stride T * HW, the
    initial condition with stride HW, forcing with T + 1 steps, the input of step s > 0 inside step s - 1's output - and a
    FusedPhysics over them.  Returns (phys, out, keep); ``keep`` holds what the field tables point into."""
    from ace_amd.corrector import AtmosphereCorrectorConfig
    from ace_amd.physics import FusedPhysics
    corrector = AtmosphereCorrectorConfig.from_state(config).get_corrector(dataset_info(c)) if config is not None else None
    prog = sorted(c["gen0"])
    B, H, W = c["gen0"]["PRESsfc"].shape
    HW = H * W
    out = {n: torch.zeros(B, T, H, W, device=dev) for n in prog}
    ic = {n: c["input0"][n].reshape(B, 1, H, W).to(dev).contiguous() for n in prog}
    forcing = {n: torch.stack([c["forcing"][n]] * (T + 1), dim=1).to(dev).contiguous() for n in c["forcing"]}

    def locate_gen(name, s):
        return (out[name].data_ptr() + 4 * s * HW, T * HW) if name in out else None

    def locate_in(name, s):
        if name in ic:
            return (ic[name].data_ptr(), HW) if s == 0 else (out[name].data_ptr() + 4 * (s - 1) * HW, T * HW)
        return (forcing[name].data_ptr() + 4 * s * HW, (T + 1) * HW) if name in forcing else None

    def locate_next(name, s):
        return (forcing[name].data_ptr() + 4 * (s + 1) * HW, (T + 1) * HW) if name in forcing else None

    phys = FusedPhysics(corrector, None, [], B, (H, W), T, gen_names=prog, in_names=prog + list(forcing),
                        next_names=list(forcing), locate_gen=locate_gen, locate_in=locate_in, locate_next=locate_next, device=dev)
    return phys, out, (ic, forcing)
