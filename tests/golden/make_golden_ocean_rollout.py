"""tests/golden/gen_ocean_rollout.pt: B = 2, T = 4 steps of a small Samudra ocean stepper with input masking, the provider's output
masking and the ocean corrector with the heat-content budget, emitted by the REAL reference's pieces - build container only.

The reference ``Stepper`` does not come up under oracle/ref_loader's stubs, so the step is composed here from the reference's own
modules in the order of fme/ace/stepper/single_module.py:1045-1075 (``Stepper.step``) and fme/core/step/single_module.py:595-733
(``step_with_adjustments``):
  input masking of the input AND the next-step data (fme/core/spatial_masking.py) -> normalise (fme/core/normalizer.py) -> pack
  (fme/core/packer.py) -> Samudra (fme/ace/models/ocean/m2lines/samudra.py) -> unpack -> denormalise -> ocean corrector on
  (masked input, output, masked next-step data) (fme/core/corrector/ocean.py) -> the provider's output masker (NaN where the mask
  is 0); the masked output is the next step's state (single_module.py:1124-1167).
Stored: the stepper checkpoint in ace_amd's load_stepper layout (the reference's state_dict, names, normalisation, masks, depth
coordinate, corrector config; the weights bfloat16-exact, stored as bfloat16), the initial condition and forcing, the fp32 rollout, and the same rollout with every piece in fp64,
stored as its fp16 difference from the fp32 one under a power-of-two scale (see fp64_output)."""
import datetime
import importlib
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from oracle import ref_loader  # noqa: E402

H, W, L, B, T = 16, 32, 3, 2, 4
CFG = {"ch_width": [8, 8], "dilation": [1, 2], "n_layers": [1, 1], "pad": "circular", "norm": "instance", "upscale_factor": 1}
OUT = ["sst", "zos"] + [f"thetao_{k}" for k in range(L)] + [f"so_{k}" for k in range(L)] + ["ocean_sea_ice_fraction", "HI"]
FORCING = ["land_fraction", "hfds", "hfgeou", "DLWRFsfc"]
IN = FORCING + OUT
NEXT_STEP_FORCING = ["hfds"]
INPUT_MASKING = {"mask_value": 0, "fill_value": "mean", "exclude_names_and_prefixes": ["land_fraction"]}
CORRECTOR = {"force_positive_names": [f"so_{k}" for k in range(L)] + ["HI"],
             "sea_ice_fraction_correction": {"sea_ice_fraction_name": "ocean_sea_ice_fraction", "land_fraction_name": "land_fraction",
                                             "remove_negative_ocean_fraction": False},
             "ocean_heat_content_correction": {"method": "scaled_temperature"}}
TIMESTEP = datetime.timedelta(days=5)


def fp64_output(case, name) -> torch.Tensor:
    return case["output"][name].double() + case["output64_delta"][name].double() / case["output64_delta_scale"]


def setup():
    g = torch.Generator().manual_seed(11)
    idepth = torch.tensor([0.0, 10.0, 40.0, 120.0])
    deptho = torch.rand(H, W, generator=g) * 150.0
    deptho[torch.rand(H, W, generator=g) < 0.2] = 0.0
    deptho[:2] = 0.0
    mask = (deptho.unsqueeze(-1) > idepth[:-1]).float()
    masks = {"mask_2d": mask[..., 0].clone(), **{f"mask_{k}": mask[..., k].clone() for k in range(L)}}
    stats = {"sst": (285.0, 5.0), "zos": (0.0, 0.3), "ocean_sea_ice_fraction": (0.3, 0.3), "HI": (0.8, 0.5), "land_fraction": (0.3, 0.4),
             "hfds": (0.0, 30.0), "hfgeou": (0.08, 0.02), "DLWRFsfc": (330.0, 20.0),
             **{f"thetao_{k}": (12.0 - 2.0 * k, 3.0) for k in range(L)}, **{f"so_{k}": (34.5 + 0.1 * k, 0.5) for k in range(L)}}
    means = {n: v[0] for n, v in stats.items()}
    stds = {n: v[1] for n, v in stats.items()}
    lat = torch.linspace(-80.0, 80.0, H)
    lon = torch.arange(W) * (360.0 / W)
    return idepth, deptho, mask, masks, means, stds, lat, lon


def data(mask):
    g = torch.Generator().manual_seed(12)
    r = lambda *shape, scale=1.0, shift=0.0: torch.randn(*shape, generator=g) * scale + shift
    ic = {n: r(B, 1, H, W, scale=2.0 if n in ("sst", "thetao_0") else 0.3,
                shift=285.0 if n == "sst" else 12.0 if n.startswith("thetao") else 34.5 if n.startswith("so") else 0.5) for n in OUT}
    ic["ocean_sea_ice_fraction"] = torch.rand(B, 1, H, W, generator=g) * 1.2 - 0.1
    forcing = {"land_fraction": (1.0 - mask[..., 0]).expand(B, T + 1, H, W).clone() * 0.9 + 0.05 * torch.rand(B, T + 1, H, W, generator=g),
               "hfds": r(B, T + 1, H, W, scale=30.0), "hfgeou": r(B, T + 1, H, W, scale=0.02, shift=0.08),
               "DLWRFsfc": r(B, T + 1, H, W, scale=20.0, shift=330.0)}
    return ic, forcing


def rollout(mods, net, dtype, setup_, ic, forcing):
    sm, smp, norm_mod, packer_mod, oc, coords, ref = mods
    idepth, deptho, mask, masks, means, stds, lat, lon = setup_
    c = lambda d: {k: v.to(dtype) for k, v in d.items()}
    provider = smp.SpatialMaskProvider(c(masks))
    normalizer = norm_mod.StandardNormalizer(means={k: torch.tensor(v, dtype=dtype) for k, v in means.items()},
                                             stds={k: torch.tensor(v, dtype=dtype) for k, v in stds.items()})
    in_mask = sm.StaticSpatialMaskingConfig(**INPUT_MASKING).build(mask=provider, means=normalizer.means)
    out_mask = provider.build_output_spatial_masker()
    ops = ref.LatLonCoordinates(lat=lat.to(dtype), lon=lon.to(dtype)).get_gridded_operations(provider)
    depth = coords.DepthCoordinate(idepth.to(dtype), mask.to(dtype), deptho.to(dtype))
    from make_golden_ocean_corrector import build_config
    corrector = build_config(oc, CORRECTOR)._build(ops, depth, TIMESTEP)
    in_packer, out_packer = packer_mod.Packer(IN), packer_mod.Packer(OUT)
    net = net.to(dtype)
    state = {k: v[:, 0].to(dtype) for k, v in ic.items()}
    forcing = c(forcing)
    outs = []
    for s in range(T):
        inp = {**state, **{k: forcing[k][:, s + 1 if k in NEXT_STEP_FORCING else s] for k in FORCING}}
        nxt = {k: forcing[k][:, s + 1] for k in FORCING}
        inp, nxt = in_mask(inp), in_mask(nxt)
        x = in_packer.pack(normalizer.normalize(inp), axis=-3)
        with torch.no_grad():
            y = net(x)
        gen = normalizer.denormalize(out_packer.unpack(y, axis=-3))
        gen = corrector(inp, gen, nxt, None).corrected
        state = out_mask(gen)
        outs.append(state)
    return {k: torch.stack([o[k] for o in outs], dim=1) for k in OUT}


def main():
    ref = ref_loader.load_corrector()
    sm = importlib.import_module("fme.core.spatial_masking")
    smp = importlib.import_module("fme.core.spatial_mask_provider")
    try:
        import xarray  # noqa: F401
    except ImportError:          # fme.core.normalizer reads statistics files through xarray; the in-memory normaliser does not
        ref_loader._ns("xarray")
    norm_mod = importlib.import_module("fme.core.normalizer")
    packer_mod = importlib.import_module("fme.core.packer")
    oc = importlib.import_module("fme.core.corrector.ocean")
    coords = importlib.import_module("fme.core.coordinates")
    from make_golden_samudra import load_reference
    samudra = load_reference()
    mods = (sm, smp, norm_mod, packer_mod, oc, coords, ref)
    setup_ = setup()
    idepth, deptho, mask, masks, means, stds, lat, lon = setup_
    torch.manual_seed(13)
    net = samudra.Samudra(input_channels=len(IN), output_channels=len(OUT), norm_kwargs=None, **CFG).eval()
    with torch.no_grad():         # weights exactly representable in bfloat16, stored so (the file stays under 0.5 MB)
        for p in net.parameters():
            p.copy_(p.bfloat16().float())
    state_dict = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ic, forcing = data(mask)
    out32 = rollout(mods, net, torch.float32, setup_, ic, forcing)
    net.load_state_dict(state_dict)
    out64 = rollout(mods, net.double(), torch.float64, setup_, ic, forcing)
    dmax = max(float((out64[k] - out32[k].double()).nan_to_num().abs().max()) for k in OUT)
    scale = 2.0 ** (14 - math.frexp(dmax)[1]) if dmax > 0 else 1.0
    stepper = {"config": {"input_masking": INPUT_MASKING, "step": {"type": "single_module", "config": {
                   "builder": {"type": "Samudra", "config": CFG}, "in_names": IN, "out_names": OUT,
                   "next_step_forcing_names": NEXT_STEP_FORCING,
                   "normalization": {"network": {"means": means, "stds": stds}}, "ocean": None,
                   "corrector": {"type": "ocean_corrector", "config": CORRECTOR}}}},
               "dataset_info": {"horizontal_coordinates": {"lat": lat, "lon": lon},
                                "timestep": TIMESTEP // datetime.timedelta(microseconds=1),
                                "mask_provider": {"masks": {k: v.bool() for k, v in masks.items()}},
                                "vertical_coordinate": {"idepth": idepth, "mask": mask.bool(), "deptho": deptho}},
               "step": {"module": {**{f"module.{k}": v.bfloat16() if v.is_floating_point() else v for k, v in state_dict.items()},
                                   "label_encoding": None}}}
    rec = {"stepper": stepper, "initial_condition": ic, "forcing": forcing, "output": out32,
           "output64_delta": {k: ((out64[k] - out32[k].double()) * scale).half() for k in OUT}, "output64_delta_scale": scale}
    for k in OUT:
        ref64 = out64[k]
        err = float((fp64_output(rec, k) - ref64).nan_to_num().abs().max() / ref64.nan_to_num().abs().max().clamp_min(1e-30))
        assert err <= 1e-9, (k, err)
        assert torch.equal(torch.isnan(out32[k]), torch.isnan(ref64)), k
    path = os.path.join(HERE, "gen_ocean_rollout.pt")
    torch.save(rec, path)
    print("fp32 vs fp64:", {k: float((out32[k].double() - out64[k]).nan_to_num().abs().max() / out64[k].nan_to_num().abs().max())
                            for k in OUT})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
