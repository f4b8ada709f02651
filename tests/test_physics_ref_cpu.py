"""tests/_physics_ref.py pinned on the CPU: its generator to the golden inputs the reference's corrector was run on, the fp32 leg
of its truth to the reference's golden outputs, its frozen-parts / geopotential variants to their twins, and the conditioning of
every case test_gpu_physics_shapes.py uses to a cap."""
import os

import pytest
import torch

import _physics_ref as R
from test_corrector_cpu import CONFIGS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_corrector.pt")


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, map_location="cpu", weights_only=False)


def test_generator_reproduces_the_golden_inputs(gold):
    c = R.case(2, 8, 16, 4)
    for part in ("gen0", "gen1", "input0", "forcing"):
        assert set(c[part]) == set(gold[part]), part
        for k, v in gold[part].items():
            assert torch.equal(c[part][k], v), (part, k)
    assert torch.equal(c["lat"], gold["lat"]) and torch.equal(c["lon"], gold["lon"])
    assert c["timestep_seconds"] == gold["timestep_seconds"]


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_fp32_leg_of_the_truth_matches_the_reference(gold, name):
    """on the golden inputs AND the golden geometry: the fp32 leg is the restatement test_corrector_cpu.py holds, here through
    the chaining of ``truth``"""
    t = R.truth(CONFIGS[name], gold)
    exp = gold["expected"][name]
    for s in range(2):
        assert set(t["fp32"][s]) == set(exp[f"step{s}"])
        for k, v in exp[f"step{s}"].items():
            torch.testing.assert_close(t["fp32"][s][k], v, rtol=1e-6, atol=0.0, msg=lambda m: f"{name} step{s} {k}: {m}")
        # the fp64 leg is the same computation: no further from the reference than the reference's fp32 is from exact
        for k, v in t["fields"][s].items():
            scale = float(v.abs().max())
            assert float((exp[f"step{s}"][k].double() - v).abs().max()) / scale <= 1e-5, (name, s, k)
    if exp["global_dry_air_mass"] is None:
        assert t["mass"] is None and t["mass32"] is None
    else:
        torch.testing.assert_close(t["mass32"], exp["global_dry_air_mass"], rtol=1e-12, atol=0.0)
        torch.testing.assert_close(t["mass"], exp["global_dry_air_mass"], rtol=1e-6, atol=0.0)


def test_truth_lists_exactly_the_fields_it_changes():
    c = R.case(3, 9, 57, 4)
    t = R.truth(R.config_for("moisture_evaporation", 4), c)
    assert set(t["fields"][0]) == {"LHTFLsfc"}
    t = R.truth(R.config_for("dry_air", 4), c)
    assert set(t["fields"][0]) == {"PRESsfc"} and t["mass"].shape == (3, 1, 1) and t["mass"].dtype == torch.float64
    carried = R.truth(R.config_for("dry_air", 4), c, steps=1, mass=t["mass"] * 1.0001)
    assert torch.equal(carried["mass"], t["mass"] * 1.0001)
    shift = (carried["fields"][0]["PRESsfc"] - t["fields"][0]["PRESsfc"]).mean(dim=(-2, -1))
    torch.testing.assert_close(shift, 1e-4 * t["mass"].reshape(-1), rtol=1e-2, atol=0.0)      # a heavier reference lifts every column


@pytest.mark.parametrize("shape", [(3, 9, 57, 4), (1, 4, 8, 1)], ids=R.shape_id)
def test_frozen_parts_and_geopotential_are_wired(shape):
    """ICEsfc + GRAUPELsfc + SNOWsfc for the frozen rate and PHIS / 9.80616 for the surface height give what their sum and
    quotient give as total_frozen_precipitation_rate and HGTsfc; and the fields matter (without them the answer moves)."""
    cfg = R.config_for("energy", shape[3])
    v = R.case(*shape, frozen="parts", height="PHIS")
    twin = {k: ({n: t.double() for n, t in d.items()} if isinstance(d, dict) else d) for k, d in v.items()}
    for part in ("input0", "gen0", "gen1", "forcing"):
        d = twin[part]
        if "ICEsfc" in d:
            d["total_frozen_precipitation_rate"] = d.pop("ICEsfc") + d.pop("GRAUPELsfc") + d.pop("SNOWsfc")
        if "PHIS" in d:
            d["HGTsfc"] = d.pop("PHIS") / 9.80616
    a, _ = R._run(cfg, v, torch.float64, 2, None)
    b, _ = R._run(cfg, twin, torch.float64, 2, None)
    bare = {k: ({n: t for n, t in d.items() if n not in ("ICEsfc", "GRAUPELsfc", "SNOWsfc")} if isinstance(d, dict) else d)
            for k, d in v.items()}
    c, _ = R._run(cfg, bare, torch.float64, 2, None)
    for s in range(2):
        for k in a[s]:
            if k.startswith(("air_temperature_", "specific_total_water_")):
                torch.testing.assert_close(a[s][k], b[s][k], rtol=1e-13, atol=0.0)
        assert float((a[s]["air_temperature_0"] - c[s]["air_temperature_0"]).abs().max()) > 1e-3     # kelvin
    flat = {k: ({**d, "PHIS": torch.zeros_like(d["PHIS"])} if isinstance(d, dict) and "PHIS" in d else d) for k, d in v.items()}
    c, _ = R._run(cfg, flat, torch.float64, 1, None)
    # step 0: the heights of input and forcing are the same draw, and with both at zero the energy paths move apart
    assert float((a[0]["air_temperature_0"] - c[0]["air_temperature_0"]).abs().max()) > 1e-6


def _floor_cases():
    grid = [(sh, name, "total", "HGTsfc") for sh, name in R.shape_config_grid()]
    return grid + [(sh, "ace2_like", "parts", "PHIS") for sh in R.VARIANT_SHAPES]


@pytest.mark.parametrize("shape,name,frozen,height", _floor_cases(),
                         ids=lambda v: R.shape_id(v) if isinstance(v, tuple) else str(v))
def test_floor_cap(shape, name, frozen, height):
    """A condition on the inputs, not a measurement of the kernels: 3 * floor <= 1e-5 for every field and step of every case the
    GPU tests use, so that their bar max(2e-6, 3 * floor) cannot grow quietly.  Measured floors, the largest over configurations,
    steps and fields (PHYSFLOOR lines of a run with -s):
      1 x 4 x 8 x 1        2.1e-7  LHTFLsfc, moisture_advection_and_evaporation (seeds 5 .. 8; 1.8e-5 with seeds 1 .. 4: _physics_ref.SEED0)
      2 x 5 x 13 x 2       3.8e-7  total_frozen_precipitation_rate, ace2_like
      3 x 9 x 57 x 4       8.5e-7  total_frozen_precipitation_rate, ace2_like     (parts / PHIS: 7.2e-7)
      2 x 180 x 360 x 8    1.4e-6  tendency_of_total_water_path_due_to_advection, ace2_like
      2 x 180 x 365 x 8    1.6e-6  the same                                       (parts / PHIS: 1.5e-6)
      2 x 256 x 512 x 8    1.3e-6  the same
      1 x 182 x 721 x 16   2.5e-6  the same: 3 x 2.5e-6 = 7.4e-6
    Every field but the advective tendency (a residual of nearly cancelling terms) stays below 8.5e-7 at every shape."""
    t = R.truth_for(shape, name, frozen, height)
    worst = max(((f, s, k) for s, st in enumerate(t["floor"]) for k, f in st.items()), default=(0.0, 0, "-"))
    print(f"PHYSFLOOR {R.shape_id(shape)} {name} {frozen} {height}: worst floor {worst[0]:.3e} (step {worst[1]}, {worst[2]})")
    for s, st in enumerate(t["floor"]):
        for k, f in st.items():
            assert 3.0 * f <= R.FLOOR_CAP, (shape, name, s, k, f)
