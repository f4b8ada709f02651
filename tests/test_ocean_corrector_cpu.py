"""The ocean corrector's torch restatement (ace_amd/ocean_corrector.py) against the reference's own outputs
(tests/golden/gen_ocean_corrector_*.pt, tests/golden/make_golden_ocean_corrector.py), its geometry, its configuration and its
loading from a Samudra stepper checkpoint."""
import datetime
import glob
import os

import pytest
import torch

from ace_amd.dataset_info import DatasetInfo
from ace_amd.masking import SpatialMaskProvider
from ace_amd.ocean_corrector import (DepthCoordinate, MaskedAreaWeightedMean, OceanCorrector, OceanCorrectorConfig,
                                     OceanHeatContentBudgetConfig, corrector_config_from_state)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = sorted(os.path.basename(p)[len("gen_ocean_corrector_"):-3] for p in glob.glob(os.path.join(GOLDEN, "gen_ocean_corrector_*.pt")))


def load_case(name):
    case = torch.load(os.path.join(GOLDEN, f"gen_ocean_corrector_{name}.pt"), weights_only=False)
    case["mask"] = case["mask"].float()                   # 0 / 1 masks are stored as bool
    case["masks"] = {k: v.float() for k, v in case["masks"].items()}
    return case


def dataset_info(case) -> DatasetInfo:
    return DatasetInfo(tuple(case["mask"].shape[:2]), timestep=datetime.timedelta(seconds=case["timestep_seconds"]),
                       lat=case["lat"], lon=case["lon"], mask_provider=SpatialMaskProvider(case["masks"]),
                       depth_coordinate={"idepth": case["idepth"], "mask": case["mask"],
                                         **({"deptho": case["deptho"]} if case["deptho"] is not None else {})})


def build(case) -> OceanCorrector:
    return OceanCorrectorConfig.from_state({"type": "ocean_corrector", "config": case["config"]}).get_corrector(dataset_info(case))


def assert_matches_fp64(out, case, rtol=1e-5):
    for k, v32 in case["expected"].items():
        ref = v32.double() + case["expected64_minus_32"][k].double()
        got = out[k].double().cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), k
        ok = ~torch.isnan(ref)
        # relative to the field's magnitude (a flux that cancels to ~0 in a column has no relative precision of its own)
        err = ((got - ref).abs()[ok].max() / ref.abs()[ok].max()).item() if ok.any() else 0.0
        assert err <= rtol, (k, err)


def test_every_case_is_present():
    assert len(CASES) >= 9, CASES


@pytest.mark.parametrize("name", CASES)
def test_torch_restatement_matches_the_reference(name):
    case = load_case(name)
    corrector = build(case)
    out, state = corrector(case["input"], case["gen"], case["forcing"], None)
    assert state is None
    assert_matches_fp64(out, case)
    for k in case["gen"]:                                  # fields the reference leaves alone stay the same tensors
        if k not in case["expected"]:
            assert out[k] is case["gen"][k]


def test_inputs_are_not_modified():
    case = load_case("legacy_bool_all")
    before = {k: {n: t.clone() for n, t in case[k].items()} for k in ("input", "gen", "forcing")}
    build(case)(case["input"], case["gen"], case["forcing"])
    for k, d in before.items():
        for n, t in d.items():
            assert torch.equal(t, case[k][n]) or (torch.isnan(t) == torch.isnan(case[k][n])).all(), (k, n)


@pytest.mark.parametrize("name", ["ohc_gen_total_area_deptho_mask2d", "ohc_gen_hfds_no_deptho", "ohc_input_total_area"])
def test_depth_coordinate_dz_matches_the_reference(name):
    case = load_case(name)
    dc = DepthCoordinate(case["idepth"], case["mask"], case["deptho"])
    torch.testing.assert_close(dc.dz, case["dz"], rtol=1e-6, atol=1e-4)
    assert dc.nlev == 7 and len(dc) == 8
    x = torch.ones(2, *case["mask"].shape)
    x[..., 3] = float("nan")                               # NaN counts as zero
    integral = dc.depth_integral(x)
    top = case["mask"][..., 0] > 0
    expected = (case["dz"].double().sum(-1) - case["dz"].double()[..., 3]).float()
    torch.testing.assert_close(integral[:, top], expected[top].expand(2, -1), rtol=1e-5, atol=1e-3)
    assert torch.isnan(integral[:, ~top]).all()
    with pytest.raises(ValueError, match="one shorter"):
        DepthCoordinate(case["idepth"], case["mask"][..., :-1])
    with pytest.raises(ValueError, match="must match"):
        dc.depth_integral(x[..., :-1])


def test_partial_bottom_cells():
    idepth = torch.tensor([0.0, 10.0, 30.0, 60.0])
    mask = torch.tensor([[1.0, 1.0, 1.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    dc = DepthCoordinate(idepth, mask, torch.tensor([45.0, 25.0, 0.0]))
    torch.testing.assert_close(dc.dz, torch.tensor([[10.0, 20.0, 15.0], [10.0, 15.0, 0.0], [0.0, 0.0, 0.0]]))
    dc = DepthCoordinate(idepth, mask)                    # no deptho: the deepest valid interface
    torch.testing.assert_close(dc.dz, torch.tensor([[10.0, 20.0, 30.0], [10.0, 20.0, 0.0], [0.0, 0.0, 0.0]]))


def test_masked_area_weighted_mean():
    H, W = 4, 6
    area = torch.linspace(1.0, 2.0, H).unsqueeze(-1).expand(H, W)
    area = area / area.sum()
    mask = (torch.arange(W) % 2 == 0).float().expand(H, W)
    mean = MaskedAreaWeightedMean(area, SpatialMaskProvider({"mask_2d": mask, "mask_sst": torch.ones(H, W)}))
    x = torch.randn(3, H, W)
    x_nan = x.where(mask > 0, float("nan"))               # NaNs with weight 0 are dropped
    w = area * mask
    expected = (x * w).sum((-2, -1)) / w.sum()
    torch.testing.assert_close(mean(x_nan, name="ocean_heat_content"), expected)
    torch.testing.assert_close(mean(x, keepdim=True, name="sst"), ((x * area).sum((-2, -1)) / area.sum()).reshape(3, 1, 1))
    torch.testing.assert_close(mean(x), (x * area).sum((-2, -1)) / area.sum())      # no name: the plain area mean
    assert torch.isnan(mean(x_nan, name="sst")).all()


def test_deprecated_keys():
    cfg = OceanCorrectorConfig.from_state({
        "masking": {"mask_value": 0}, "ocean_heat_content_correction": True,
        "sea_ice_fraction_correction": {"sea_ice_fraction_name": "sif", "land_fraction_name": "lf",
                                        "zero_where_ice_free_names": ["x"], "sea_ice_thickness_name": "HI"}})
    assert cfg.ocean_heat_content_correction == OceanHeatContentBudgetConfig(method="scaled_temperature")
    assert cfg.sea_ice_fraction_correction.zero_where_ice_free_names == ["x", "HI"]
    assert cfg.sea_ice_fraction_correction.remove_negative_ocean_fraction is True
    cfg = OceanCorrectorConfig.from_state({"ocean_heat_content_correction": False,
                                           "sea_ice_fraction_correction": {"sea_ice_fraction_name": "sif", "land_fraction_name": "lf",
                                                                           "sea_ice_thickness_name": None}})
    assert cfg.ocean_heat_content_correction is None
    assert cfg.sea_ice_fraction_correction.zero_where_ice_free_names == []
    # the straight-through option changes gradients only: accepted
    assert OceanCorrectorConfig.from_state({"keep_gradient_through_clamps": True}).keep_gradient_through_clamps
    with pytest.raises(ValueError, match="unknown"):
        OceanCorrectorConfig.from_state({"nonsense": 1})
    with pytest.raises(NotImplementedError):
        OceanCorrectorConfig.from_state({"ocean_heat_content_correction": {"method": "other"}})


def test_selection_by_type():
    from ace_amd.corrector import AtmosphereCorrectorConfig
    assert isinstance(corrector_config_from_state({"type": "ocean_corrector", "config": {}}), OceanCorrectorConfig)
    atm = corrector_config_from_state({"type": "atmosphere_corrector", "config": {"conserve_dry_air": True}})
    assert atm == AtmosphereCorrectorConfig(conserve_dry_air=True)
    assert corrector_config_from_state(None) == AtmosphereCorrectorConfig()
    assert corrector_config_from_state({"force_positive_names": ["a"]}) == AtmosphereCorrectorConfig(force_positive_names=["a"])


def test_heat_content_without_depth_coordinate_raises_the_references_error():
    case = load_case("ohc_gen_hfds_no_deptho")
    di = DatasetInfo(tuple(case["mask"].shape[:2]), timestep=datetime.timedelta(days=5), lat=case["lat"], lon=case["lon"])
    corrector = OceanCorrectorConfig.from_state(case["config"]).get_corrector(di)
    with pytest.raises(ValueError, match="no vertical coordinate"):
        corrector(case["input"], case["gen"], case["forcing"])
    with pytest.raises(NotImplementedError, match="area weights"):
        OceanCorrectorConfig.from_state(case["config"]).get_corrector(DatasetInfo((4, 8)))


def test_hfds_in_output_and_forcing_is_refused():
    case = load_case("ohc_gen_hfds_no_deptho")
    with pytest.raises(ValueError, match="both gen_data and forcing_data"):
        build(case)(case["input"], case["gen"], {**case["forcing"], "hfds": case["gen"]["hfds"]})


# ---- the stepper around it --------------------------------------------------------------------------------------------
NAMES_IN = ["sst", "thetao_0", "thetao_1", "thetao_2", "so_0", "HI", "ocean_sea_ice_fraction", "land_fraction", "hfds"]
NAMES_OUT = ["sst", "thetao_0", "thetao_1", "thetao_2", "so_0", "HI", "ocean_sea_ice_fraction"]


def samudra_ocean_state(H=12, W=24, vertical=True):
    from ace_amd.samudra import Samudra
    torch.manual_seed(0)
    cfg = {"ch_width": [8, 8], "dilation": [1, 2], "n_layers": [1, 1], "pad": "circular", "norm": "instance"}
    net = Samudra(len(NAMES_IN), len(NAMES_OUT), **cfg)
    names = sorted(set(NAMES_IN) | set(NAMES_OUT))
    mask = torch.ones(H, W, 3)
    mask[:2] = 0.0
    mask[5:, :, 2] = 0.0
    ds = {"horizontal_coordinates": {"lat": torch.linspace(-80, 80, H), "lon": torch.linspace(0, 345, W)},
          "timestep": datetime.timedelta(days=5) // datetime.timedelta(microseconds=1),
          "mask_provider": {"masks": {"mask_2d": mask[..., 0], **{f"mask_{k}": mask[..., k] for k in range(3)}}}}
    if vertical:
        ds["vertical_coordinate"] = {"idepth": torch.tensor([0.0, 10.0, 50.0, 200.0]), "mask": mask,
                                     "deptho": torch.full((H, W), 120.0)}
    corrector = {"type": "ocean_corrector", "config": {
        "force_positive_names": ["so_0", "HI"],
        "sea_ice_fraction_correction": {"sea_ice_fraction_name": "ocean_sea_ice_fraction", "land_fraction_name": "land_fraction",
                                        "remove_negative_ocean_fraction": False},
        "ocean_heat_content_correction": {"method": "scaled_temperature"}}}
    return {"stepper": {
        "config": {"input_masking": {"mask_value": 0, "fill_value": 0.0, "exclude_names_and_prefixes": ["land_fraction"]},
                   "step": {"type": "single_module", "config": {
                       "builder": {"type": "Samudra", "config": cfg}, "in_names": NAMES_IN, "out_names": NAMES_OUT,
                       "normalization": {"network": {"means": {n: 0.1 * i for i, n in enumerate(names)},
                                                     "stds": {n: 1.0 + 0.5 * i for i, n in enumerate(names)}}},
                       "ocean": None, "corrector": corrector}}},
        "dataset_info": ds,
        "step": {"module": {**{f"module.{k}": v for k, v in net.state_dict().items()}, "label_encoding": None}}}}


def test_load_stepper_with_an_ocean_corrector():
    from ace_amd.checkpoint import load_stepper
    loaded = load_stepper(samudra_ocean_state(), device="cpu")
    step = loaded.stepper._step_obj
    corrector = step._corrector
    assert isinstance(corrector, OceanCorrector)
    assert corrector.corrections == ["force_positive", "sea_ice_fraction_correction", "ocean_heat_content_correction"]
    assert not loaded.ignored
    dc = loaded.dataset_info.ocean_vertical_coordinate
    assert isinstance(dc, DepthCoordinate) and dc.nlev == 3
    assert loaded.dataset_info.vertical_coordinate is None       # the atmosphere's hybrid coordinate stays separate
    torch.testing.assert_close(dc.dz[0, 0], torch.zeros(3))
    torch.testing.assert_close(dc.dz[6, 0], torch.tensor([10.0, 40.0, 0.0]))
    # the corrector as the step calls it, on the CPU: torch ops
    g = torch.Generator().manual_seed(3)
    H, W = 12, 24
    gen = {n: torch.randn(2, H, W, generator=g) + (280.0 if n == "sst" else 5.0) for n in NAMES_OUT}
    inp = {n: torch.randn(2, H, W, generator=g) + (280.0 if n == "sst" else 5.0) for n in NAMES_IN}
    inp["hfds"] = torch.zeros(2, H, W)                  # no net flux into the ocean: the heat content is conserved
    out, _ = corrector(inp, gen, {"land_fraction": torch.rand(2, H, W, generator=g)})
    assert (out["so_0"] >= 0).all() and (out["ocean_sea_ice_fraction"] <= 1).all()
    mean = corrector._mean
    ohc = lambda d: mean(dc.depth_integral(torch.stack([d[f"thetao_{k}"] for k in range(3)], -1) * 3992.0 * 1035.0),
                         name="ocean_heat_content")
    torch.testing.assert_close(ohc(out), ohc(inp), rtol=1e-5, atol=0.0)


def test_load_stepper_needs_a_depth_or_null_vertical_coordinate():
    from ace_amd.checkpoint import load_stepper
    with pytest.raises(NotImplementedError, match="ocean_corrector"):
        load_stepper(samudra_ocean_state(vertical=False), device="cpu")


def test_rollout_engine_refuses_an_ocean_corrector():
    from ace_amd.checkpoint import load_stepper
    from ace_amd.rollout import RolloutEngine
    loaded = load_stepper(samudra_ocean_state(), device="cpu")
    with pytest.raises(NotImplementedError, match="ocean corrector"):
        RolloutEngine(loaded.stepper, batch=1, n_forward_steps=1)
