"""tests/_ocean_phys_ref.py pinned on the CPU: the fp64 leg of its truth to the reference's own fp64 outputs on the golden cases,
the conditioning of every case test_gpu_ocean_phys_shapes.py uses to a cap, and - in fp64, no kernel involved - the proof that the
bar those tests hold can see what a multi-block reduction gets wrong: a lost partial sum, a lost grid-stride tail, another
sample's means, a dropped flux term."""
import pytest
import torch

import _ocean_phys_ref as R
from test_ocean_corrector_cpu import CASES, assert_matches_fp64, load_case

NT, NBLK_MAX = 256, 512          # csrc/ocean_phys.hip


@pytest.mark.parametrize("name", CASES)
def test_fp64_leg_matches_the_references_fp64(name):
    """the reference's fp64 run recomputes its geometry in fp64, the truth's upcasts the fp32 geometry the kernels are given: both
    within assert_matches_fp64's 1e-5 of each other, and the fp32 leg is the restatement test_ocean_corrector_cpu.py holds"""
    c = load_case(name)
    t = R.truth(c["config"], c)
    assert set(t["fields"]) == set(c["expected"])
    assert_matches_fp64(t["fields"], c)
    assert_matches_fp64(t["fp32"], c)
    for k, f in t["floor"].items():
        assert f <= 1e-5, (name, k, f)


def test_truth_lists_exactly_the_fields_it_changes():
    L = 4
    th = {f"thetao_{k}" for k in range(L)}
    so = {f"so_{k}" for k in range(L)}
    want = {"gen_total_area": th | so | {"sst", "HI", "ocean_sea_ice_fraction", "hfds_total_area"},
            "gen_hfds": th | so | {"sst", "hfds"},
            "input_hfds": th | so | {"HI", "ocean_sea_ice_fraction"},
            "input_total_area_ssf": th | {"sst"},
            "input_total_area_land": th | {"sst"},
            "column_local": {f"tracer_{i}" for i in range(R.MAX_POSITIVE - 1)} | {f"icevar_{i}" for i in range(R.MAX_ZERO - 1)}
            | {"HI", "ocean_sea_ice_fraction", "hfds"}}
    assert set(want) == set(R.VARIANTS)
    for name, fields in want.items():
        assert set(R.truth_for((3, 9, 57, L), name)["fields"]) == fields, name


def test_every_branch_of_o1_is_taken_by_some_variant():
    """the switches FusedOceanCorrector.fields derives, read off the cases themselves"""
    from ace_amd.ocean_corrector import ohc_flux_source
    seen = set()
    for name in R.VARIANTS:
        c = R.case(2, 5, 13, 2, name)
        cfg, inp, gen, forcing = c["config"], c["input"], c["gen"], c["forcing"]
        if "ocean_heat_content_correction" in cfg:
            src = ohc_flux_source(gen, forcing)
            seen.add(("flux", {"gen_total_area": 0, "gen": 1}.get(src, 2 if "hfds" in inp else 3)))
            if src == "input" and "hfds" not in inp:
                seen.add(("in_ssf_is_land", "sea_surface_fraction" not in inp))
            seen.add(("f_ssf_is_land", "sea_surface_fraction" not in forcing))
            seen.add(("hfgeou", "hfgeou" in forcing))
            seen.add(("ohc_mask", bool(c["masks"])))
            seen.add(("sst_out", "sst" in gen))
            seen.add(("heating", cfg["ocean_heat_content_correction"]["constant_unaccounted_heating"] != 0))
            seen.add(("deptho", c["deptho"] is not None))
        if "surface_energy_flux_correction" in cfg:
            seen.add(("hfds", cfg["surface_energy_flux_correction"]["method"], "hfds" in gen))
            seen.add(("in_sif_is_ocean_sif", "sea_ice_fraction" not in inp))
            seen.add(("frozen", "total" if "total_frozen_precipitation_rate" in forcing else "parts" if "ICEsfc" in forcing else "none"))
        else:
            seen.add(("hfds", None))
        if "sea_ice_fraction_correction" in cfg:
            seen.add(("rebalance", cfg["sea_ice_fraction_correction"].get("remove_negative_ocean_fraction", True)))
    want = {("flux", 0), ("flux", 1), ("flux", 2), ("flux", 3), ("in_ssf_is_land", False), ("in_ssf_is_land", True),
            ("f_ssf_is_land", False), ("f_ssf_is_land", True), ("hfgeou", False), ("hfgeou", True), ("ohc_mask", False),
            ("ohc_mask", True), ("sst_out", False), ("sst_out", True), ("heating", False), ("heating", True), ("deptho", False),
            ("deptho", True), ("hfds", "prescribed", False), ("hfds", "residual_prediction", True), ("hfds", None),
            ("in_sif_is_ocean_sif", False), ("in_sif_is_ocean_sif", True), ("frozen", "total"), ("frozen", "parts"),
            ("frozen", "none"), ("rebalance", False), ("rebalance", True)}
    assert want <= seen, want - seen


def test_the_cases_keep_what_cm4_has():
    """land columns, NaN below the sea floor in the input's thetao, fractions outside [0, 1], negative force-positive fields, and
    at 64 levels columns that are partly open"""
    c = R.case(1, 182, 721, 64, "gen_total_area")
    mask = c["mask"]
    assert 0.2 < float((mask[..., 0] == 0).float().mean()) < 0.4
    open_levels = mask.sum(-1)
    assert float(open_levels.max()) == 64 and 0.5 < float(((open_levels > 0) & (open_levels < 64)).float().mean())
    assert torch.equal(torch.isnan(c["input"]["thetao_63"][0]), mask[..., 63] == 0)
    assert not any(torch.isnan(v).any() for v in c["gen"].values())
    sif = c["gen"]["ocean_sea_ice_fraction"]
    assert float(sif.min()) < 0 and float(sif.max()) > 1
    assert float(c["gen"]["so_0"].min()) < 0 and float(c["gen"]["HI"].min()) < 0
    assert not R.case(2, 5, 13, 2, "gen_hfds")["mask"][..., 0].eq(0).any()          # no mask for the mean: no land column


@pytest.mark.parametrize("shape", R.SMALL_SHAPES + R.LARGE_SHAPES, ids=R.shape_id)
def test_floor_cap(shape):
    """A condition on the inputs, not a measurement of the kernels: 3 * floor <= 1e-5 for every field of every case the GPU tests
    use, so that their bar max(2e-6, 3 * floor) cannot grow quietly.  Measured floors, the largest over variants and fields
    (OCEANFLOOR lines of a run with -s):
      1 x 4 x 8 x 1        2.6e-7  hfds, gen_hfds
      2 x 5 x 13 x 2       1.7e-7  hfds, column_local
      3 x 9 x 57 x 4       1.7e-7  hfds_total_area, gen_total_area
      2 x 180 x 365 x 8    2.0e-7  hfds_total_area, gen_total_area
      2 x 256 x 512 x 8    1.9e-7  hfds_total_area, gen_total_area
      1 x 182 x 721 x 64   2.1e-7  hfds_total_area, gen_total_area
    The temperatures alone stay below 2.0e-7.  So 3 * floor < 2e-6 everywhere and the bar is 2e-6."""
    variants = R.VARIANTS if shape in R.SMALL_SHAPES else R.BUDGET_VARIANTS
    worst = (0.0, "-", "-")
    for name in variants:
        for k, f in R.truth_for(shape, name)["floor"].items():
            worst = max(worst, (f, k, name))
            assert 3.0 * f <= R.FLOOR_CAP, (shape, name, k, f)
    print(f"OCEANFLOOR {R.shape_id(shape)}: worst floor {worst[0]:.3e} ({worst[1]}, {worst[2]})")


# ---- what the bar can see ---------------------------------------------------------------------------------------------------
def _moved(shape, name, drop):
    """the largest move of a thetao level, as a multiple of that level's tolerance, when the columns ``drop`` leave the three
    means (fp64 against fp64: nothing but the omission)"""
    c = R.case(*shape, name)
    t = R.truth_for(shape, name)
    out = R.run(c["config"], c, torch.float64, drop=drop.reshape(shape[1], shape[2]))
    return max(R.rel_err(out[k], v) / R.tolerance(t["floor"][k]) for k, v in t["fields"].items() if k.startswith("thetao_"))


def test_bar_sees_a_lost_partial():
    """Zeroing the heat-content weight of (a) the columns of workgroup 256 at 2 x 180 x 365 x 8 - the partial O2's second re-sum
    trip adds; (b) the columns px >= 512 * 256 at 1 x 182 x 721 x 64 - the second grid-stride trip of O1; (c) the columns of one
    interior workgroup at 2 x 256 x 512 x 8, moves some thetao level by at least 10 x its tolerance.  Measured, with
    GRADIENT = 0.5 (OCEANSEES lines):
      (a) 170 x the tolerance   (b) 79 x   (c) 126 x
    With GRADIENT = 0.2 they are 86, 34 and 64; with 0.05 they are 35, 6.8 and 27: the tail of (b) is 150 columns of 131222."""
    px = lambda hw: torch.arange(hw)                                                                  # noqa: E731
    a = _moved((2, 180, 365, 8), "gen_total_area", px(180 * 365) // NT == 256)
    b = _moved((1, 182, 721, 64), "gen_total_area", px(182 * 721) >= NBLK_MAX * NT)
    c = _moved((2, 256, 512, 8), "gen_total_area", px(256 * 512) // NT == 100)
    print(f"OCEANSEES lost partial: (a) {a:.1f} (b) {b:.1f} (c) {c:.1f} x the tolerance")
    assert a >= 10 and b >= 10 and c >= 10, (a, b, c)


@pytest.mark.parametrize("shape", [(3, 9, 57, 4), (2, 180, 365, 8)], ids=R.shape_id)
def test_bar_sees_a_wrong_sample_offset(shape):
    """Scaling sample 1 by the ratio sample 0's three means give moves its thetao by at least 10 x the tolerance.  Measured:
    1.4e4 x at 3 x 9 x 57 x 4, 3.4e3 x at 2 x 180 x 365 x 8 (the generated temperatures of neighbouring samples differ by 1 %)."""
    from ace_amd.ocean_corrector import ohc_ratio
    name = "gen_total_area"
    c = R.case(*shape, name)
    t = R.truth_for(shape, name)
    out = R.run(c["config"], c, torch.float64)
    gen = {**{k: v.double() for k, v in c["gen"].items()}, **{k: out[k] for k in ("hfds_total_area",)}}     # after the local links
    corrector = R._config(c["config"]).get_corrector(R.dataset_info(c, torch.float64))
    ratio = ohc_ratio({k: v.double() for k, v in c["input"].items()}, gen, {k: v.double() for k, v in c["forcing"].items()},
                      corrector._mean, corrector._depth_on("cpu"), corrector._dt, 3.0)
    torch.testing.assert_close(gen["thetao_0"] * ratio, t["fields"]["thetao_0"], rtol=1e-14, atol=0.0)      # the truth's own ratio
    wrong = gen["thetao_0"][1] * ratio[0]
    moved = R.rel_err(wrong, t["fields"]["thetao_0"][1]) / R.tolerance(t["floor"]["thetao_0"])
    print(f"OCEANSEES wrong sample offset {R.shape_id(shape)}: {moved:.1f} x the tolerance")
    assert moved >= 10


def test_bar_sees_the_flux_terms():
    """The flux side of the budget at 3 x 9 x 57 x 4, each change moving thetao_0 by at least 10 x the tolerance: no geothermal
    flux, no unaccounted heating, the flux not weighted by the sea-surface fraction (sources 0 and 1 differ in exactly that), the
    input's flux for the output's.  Measured: 83 x, 159 x, 61 x, 558 x."""
    shape, name = (3, 9, 57, 4), "gen_total_area"
    c = R.case(*shape, name)
    t = R.truth_for(shape, name)
    tol = R.tolerance(t["floor"]["thetao_0"])
    moved = {}

    def rerun(label, **changes):
        out = R.run(changes.pop("config", c["config"]), {**c, **changes}, torch.float64)
        moved[label] = R.rel_err(out["thetao_0"], t["fields"]["thetao_0"]) / tol

    rerun("no hfgeou", forcing={k: v for k, v in c["forcing"].items() if k != "hfgeou"})
    rerun("no heating", config={**c["config"], "ocean_heat_content_correction": {"method": "scaled_temperature"}})
    rerun("no sea-surface fraction", forcing={**c["forcing"], "sea_surface_fraction": torch.ones_like(c["forcing"]["hfgeou"])})
    o = R.case(*shape, "input_hfds")
    to = R.truth_for(shape, "input_hfds")
    out = R.run(o["config"], {**o, "input": {**o["input"], "hfds": 0.5 * o["input"]["hfds"]}}, torch.float64)
    moved["half the input's flux"] = R.rel_err(out["thetao_0"], to["fields"]["thetao_0"]) / R.tolerance(to["floor"]["thetao_0"])
    print("OCEANSEES flux terms: " + ", ".join(f"{k} {v:.1f}" for k, v in moved.items()) + " x the tolerance")
    assert all(v >= 10 for v in moved.values()), moved
