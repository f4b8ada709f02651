"""The fused ocean corrector (ace_amd/csrc/ocean_phys.hip through ace_amd/ocean_phys.py) on the MI355X: against the reference's
fp64 outputs (tests/golden/gen_ocean_corrector_*.pt), against the torch restatement, bitwise repeatability, read-only inputs,
strided output views, the CM4 shape, and a Samudra stepper rollout with the corrector."""
import datetime

import pytest
import torch

from ace_amd.ocean_corrector import OceanCorrectorConfig
from tests.test_ocean_corrector_cpu import CASES, assert_matches_fp64, build, dataset_info, load_case, samudra_ocean_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def to_dev(d, dtype=None):
    return {k: v.to(DEV, dtype=dtype) if dtype else v.to(DEV).clone() for k, v in d.items()}


@pytest.mark.parametrize("name", CASES)
def test_hip_path_matches_the_reference(name):
    case = load_case(name)
    corrector = build(case)
    inp, gen, forcing = to_dev(case["input"]), to_dev(case["gen"]), to_dev(case["forcing"])
    out, _ = corrector(inp, gen, forcing)
    torch.cuda.synchronize()
    o1, o2 = corrector.launches()
    assert o1 == 1 and o2 == int("ocean_heat_content_correction" in corrector.corrections)
    assert_matches_fp64(out, case)
    # and against the torch restatement on the same device
    corrector.fused = False
    ref, _ = corrector(to_dev(case["input"]), to_dev(case["gen"]), to_dev(case["forcing"]))
    assert corrector.launches() == (o1, o2)
    for k in case["expected"]:
        torch.testing.assert_close(out[k], ref[k], rtol=2e-6, atol=1e-5 * ref[k].nan_to_num().abs().max().item(), equal_nan=True)


def test_repeat_calls_are_bitwise_identical_and_inputs_are_read_only():
    case = load_case("legacy_bool_all")
    corrector = build(case)
    inp, forcing = to_dev(case["input"]), to_dev(case["forcing"])
    inp0, forcing0 = {k: v.clone() for k, v in inp.items()}, {k: v.clone() for k, v in forcing.items()}
    a, _ = corrector(inp, to_dev(case["gen"]), forcing)
    b, _ = corrector(inp, to_dev(case["gen"]), forcing)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k].nan_to_num(1234.5), b[k].nan_to_num(1234.5)), k
    for k in inp:
        assert torch.equal(inp[k].nan_to_num(1234.5), inp0[k].nan_to_num(1234.5)), k
    for k in forcing:
        assert torch.equal(forcing[k], forcing0[k]), k
    assert corrector.launches() == (2, 2)


def test_strided_output_views_are_corrected_in_place():
    case = load_case("legacy_bool_all")
    corrector = build(case)
    names = sorted(case["gen"])
    packed = torch.stack([case["gen"][n] for n in names], dim=1).to(DEV)       # (B, C, H, W): views with stride C * H * W
    gen = {n: packed[:, i] for i, n in enumerate(names)}
    out, _ = corrector(to_dev(case["input"]), gen, to_dev(case["forcing"]))
    for i, n in enumerate(names):
        assert out[n].data_ptr() == packed[:, i].data_ptr()
    assert_matches_fp64({n: packed[:, i] for i, n in enumerate(names)}, case)


def test_wrong_layout_is_loud():
    case = load_case("cm4_shipped")
    corrector = build(case)
    gen = to_dev(case["gen"])
    gen["HI"] = gen["HI"].transpose(-1, -2).contiguous().transpose(-1, -2)     # column-major rows
    with pytest.raises(ValueError, match="contiguous rows"):
        corrector(to_dev(case["input"]), gen, to_dev(case["forcing"]))
    gen = to_dev(case["gen"])
    gen["HI"] = gen["HI"].double()
    with pytest.raises(TypeError, match="float32"):
        corrector(to_dev(case["input"]), gen, to_dev(case["forcing"]))


def _cm4(B=2, H=180, W=360, L=19, seed=0):
    """the CM4 piControl ocean's names at 1 degree, with every correction on"""
    from ace_amd.dataset_info import DatasetInfo
    from ace_amd.masking import SpatialMaskProvider
    g = torch.Generator().manual_seed(seed)
    idepth = torch.cat([torch.zeros(1), torch.cumsum(torch.linspace(5.0, 500.0, L), 0)])
    deptho = torch.rand(H, W, generator=g) * 6000.0
    deptho[torch.rand(H, W, generator=g) < 0.3] = 0.0
    mask = (deptho.unsqueeze(-1) > idepth[:-1]).float()
    r = lambda s=1.0, m=0.0: torch.randn(B, H, W, generator=g) * s + m
    u = lambda: torch.rand(B, H, W, generator=g)
    thetao = lambda: {f"thetao_{k}": r(2.0, 15.0 - 0.7 * k).where(mask[..., k] > 0, float("nan")) for k in range(L)}
    gen = {**{f"so_{k}": r(1.0, 0.5) for k in range(L)}, **{f"thetao_{k}": r(2.0, 15.0 - 0.7 * k) for k in range(L)},
           "sst": r(3.0, 290.0), "zos": r(0.3), "HI": r(0.5, 0.2), "ocean_sea_ice_fraction": 1.4 * u() - 0.2, "hfds": r(40.0)}
    land = 0.5 * u()
    inp = {**thetao(), "sst": r(3.0, 290.0), "ocean_sea_ice_fraction": u(), "land_fraction": land, "HI": r(0.5)}
    forcing = {"DLWRFsfc": r(30.0, 330.0), "ULWRFsfc": r(30.0, 390.0), "DSWRFsfc": r(40.0, 180.0).abs(), "USWRFsfc": r(10.0, 30.0).abs(),
               "LHTFLsfc": r(40.0, 80.0), "SHTFLsfc": r(15.0, 20.0), "PRATEsfc": r(2e-5, 3e-5).abs(), "PRESsfc": r(1500.0, 98000.0),
               "land_fraction": land, "hfgeou": r(0.02, 0.08)}
    cfg = {"force_positive_names": [f"so_{k}" for k in range(L)] + ["HI"],
           "sea_ice_fraction_correction": {"sea_ice_fraction_name": "ocean_sea_ice_fraction", "land_fraction_name": "land_fraction",
                                           "zero_where_ice_free_names": ["HI"]},
           "surface_energy_flux_correction": {"method": "prescribed"},
           "ocean_heat_content_correction": {"method": "scaled_temperature", "constant_unaccounted_heating": 0.3}}
    di = DatasetInfo((H, W), timestep=datetime.timedelta(days=5), lat=torch.linspace(-89.5, 89.5, H), lon=torch.arange(W) * 1.0,
                     mask_provider=SpatialMaskProvider({"mask_2d": mask[..., 0]}),
                     depth_coordinate={"idepth": idepth, "mask": mask, "deptho": deptho})
    return OceanCorrectorConfig.from_state(cfg), di, inp, gen, forcing


def test_cm4_shape_batch2_against_float64_torch():
    """On this pole-to-pole grid a lost last partial sum moves the answer by about 4e-7, far inside the bar below: what guards the
    multi-block reduction is test_gpu_ocean_phys_shapes.py."""
    cfg, di, inp, gen, forcing = _cm4()
    corrector = cfg.get_corrector(di)
    out, _ = corrector(to_dev(inp), to_dev(gen), to_dev(forcing))
    ref = corrector.torch_apply(to_dev(inp, torch.float64), to_dev(gen, torch.float64), to_dev(forcing, torch.float64))
    torch.cuda.synchronize()
    assert corrector.launches() == (1, 1)
    for k in gen:
        a, b = out[k].double(), ref[k]
        assert torch.equal(torch.isnan(a), torch.isnan(b)), k
        ok = ~torch.isnan(b)
        err = ((a - b).abs()[ok].max() / b.abs()[ok].max()).item()
        assert err <= 1e-5, (k, err)


def test_samudra_stepper_rollout_with_the_fused_corrector():
    from ace_amd.checkpoint import load_stepper
    H, W = 12, 24
    state = samudra_ocean_state(H, W)
    g = torch.Generator().manual_seed(5)
    names_in = state["stepper"]["config"]["step"]["config"]["in_names"]
    names_out = state["stepper"]["config"]["step"]["config"]["out_names"]
    ic = {n: (torch.rand(2, 1, H, W, generator=g) + (280.0 if n == "sst" else 2.0)).to(DEV) for n in names_out}
    forcing = {n: (torch.rand(2, 4, H, W, generator=g) * 0.5).to(DEV) for n in names_in if n not in names_out}
    forcing["hfds"] = 10.0 * torch.randn(2, 4, H, W, generator=g).to(DEV)      # the heat budget's flux: the input's hfds
    outs = []
    for fused in (True, False):
        stepper = load_stepper(state, device=DEV).stepper
        corrector = stepper._step_obj._corrector
        corrector.fused = fused
        with torch.no_grad():
            data, _ = stepper.predict({k: v.clone() for k, v in ic.items()}, {k: v.clone() for k, v in forcing.items()},
                                      n_forward_steps=3)
        torch.cuda.synchronize()
        outs.append((data, corrector.launches()))
    (fused, launches_f), (plain, launches_p) = outs
    assert launches_f == (3, 3) and launches_p == (0, 0)
    for k in fused:
        torch.testing.assert_close(fused[k], plain[k], rtol=1e-5, atol=1e-4, equal_nan=True)
