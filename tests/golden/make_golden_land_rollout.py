"""tests/golden/gen_land_rollout.pt: B = 2, T = 3 steps of a small LandNet land stepper with input masking and the provider's
output masking, emitted by the REAL reference's pieces - build container only.

The reference ``Stepper`` does not come up under oracle/ref_loader's stubs, so the step is composed here from the reference's own
modules in the order of fme/ace/stepper/single_module.py:1045-1075 (``Stepper.step``) and fme/core/step/single_module.py:595-733
(``step_with_adjustments``), as make_golden_ocean_rollout.py does:
  input masking (fme/core/spatial_masking.py; fill "mean", one excluded name) -> normalise (fme/core/normalizer.py) -> pack
  (fme/core/packer.py) -> LandNet (fme/ace/models/land/land_net.py) -> unpack -> denormalise -> the provider's output masker (NaN
  where mask_2d is 0); the masked output is the next step's state (single_module.py:1124-1167).  No corrector is configured.
Stored: the stepper checkpoint in ace_amd's load_stepper layout (the reference's state_dict bfloat16-exact, stored as bfloat16),
the initial condition (NaN where masked) and forcing, the fp32 rollout, and the same rollout with every piece in fp64, stored as
its fp16 difference from the fp32 one under a power-of-two scale (see fp64_output)."""
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

H, W, B, T = 9, 15, 2, 3
CFG = {"hidden_dims": [16, 8], "network_type": "MLP", "use_positional_embedding": True}
PROGNOSTIC = ["TSOIL", "SOILM", "SNOWD"]
DIAGNOSTIC = ["LHTFLsfc"]
OUT = PROGNOSTIC + DIAGNOSTIC
FORCING = ["land_fraction", "PRATEsfc", "DSWRFsfc", "TMP2m"]
IN = FORCING + PROGNOSTIC
NEXT_STEP_FORCING = ["DSWRFsfc"]
INPUT_MASKING = {"mask_value": 0, "fill_value": "mean", "exclude_names_and_prefixes": ["land_fraction"]}
TIMESTEP = datetime.timedelta(hours=6)


def fp64_output(case, name) -> torch.Tensor:
    return case["output"][name].double() + case["output64_delta"][name].double() / case["output64_delta_scale"]


def setup():
    g = torch.Generator().manual_seed(21)
    masks = {"mask_2d": (torch.rand(H, W, generator=g) < 0.5).float()}       # 1: land (valid), 0: masked
    stats = {"TSOIL": (285.0, 8.0), "SOILM": (0.3, 0.1), "SNOWD": (0.05, 0.1), "LHTFLsfc": (60.0, 40.0), "land_fraction": (0.4, 0.45),
             "PRATEsfc": (3e-5, 5e-5), "DSWRFsfc": (200.0, 120.0), "TMP2m": (287.0, 10.0)}
    return masks, {n: v[0] for n, v in stats.items()}, {n: v[1] for n, v in stats.items()}


def data(masks, means, stds):
    g = torch.Generator().manual_seed(22)
    r = lambda n, t: torch.randn(B, t, H, W, generator=g) * stds[n] + means[n]     # noqa: E731
    ic = {n: r(n, 1) for n in PROGNOSTIC}
    for n in PROGNOSTIC:                                                           # the prognostic state has no data off the land
        ic[n][:, :, masks["mask_2d"] == 0] = float("nan")
    forcing = {n: r(n, T + 1) for n in FORCING}
    forcing["land_fraction"] = masks["mask_2d"].expand(B, T + 1, H, W).clone()
    return ic, forcing


def rollout(mods, net, dtype, masks, means, stds, ic, forcing):
    sm, smp, norm_mod, packer_mod = mods
    c = lambda d: {k: v.to(dtype) for k, v in d.items()}     # noqa: E731
    provider = smp.SpatialMaskProvider(c(masks))
    normalizer = norm_mod.StandardNormalizer(means={k: torch.tensor(v, dtype=dtype) for k, v in means.items()},
                                             stds={k: torch.tensor(v, dtype=dtype) for k, v in stds.items()})
    in_mask = sm.StaticSpatialMaskingConfig(**INPUT_MASKING).build(mask=provider, means=normalizer.means)
    out_mask = provider.build_output_spatial_masker()
    in_packer, out_packer = packer_mod.Packer(IN), packer_mod.Packer(OUT)
    net = net.to(dtype)
    state = {k: v[:, 0].to(dtype) for k, v in ic.items()}
    forcing = c(forcing)
    outs = []
    for s in range(T):
        inp = {**state, **{k: forcing[k][:, s + 1 if k in NEXT_STEP_FORCING else s] for k in FORCING}}
        inp = in_mask(inp)
        x = in_packer.pack(normalizer.normalize(inp), axis=-3)
        with torch.no_grad():
            y = net(x)
        gen = out_mask(normalizer.denormalize(out_packer.unpack(y, axis=-3)))
        outs.append(gen)
        state = {k: gen[k] for k in PROGNOSTIC}
    return {k: torch.stack([o[k] for o in outs], dim=1) for k in OUT}


def main():
    ref_loader.load_corrector()
    sm = importlib.import_module("fme.core.spatial_masking")
    smp = importlib.import_module("fme.core.spatial_mask_provider")
    try:
        import xarray  # noqa: F401
    except ImportError:          # fme.core.normalizer reads statistics files through xarray; the in-memory normaliser does not
        ref_loader._ns("xarray")
    norm_mod = importlib.import_module("fme.core.normalizer")
    packer_mod = importlib.import_module("fme.core.packer")
    from make_golden_landnet import load_reference
    land = load_reference()
    mods = (sm, smp, norm_mod, packer_mod)
    masks, means, stds = setup()
    torch.manual_seed(23)
    net = land.LandNet(img_shape=(H, W), input_channels=len(IN), output_channels=len(OUT), **CFG).eval()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p.bfloat16().float())
    state_dict = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ic, forcing = data(masks, means, stds)
    out32 = rollout(mods, net, torch.float32, masks, means, stds, ic, forcing)
    net.load_state_dict(state_dict)
    out64 = rollout(mods, net.double(), torch.float64, masks, means, stds, ic, forcing)
    dmax = max(float((out64[k] - out32[k].double()).nan_to_num().abs().max()) for k in OUT)
    scale = 2.0 ** (14 - math.frexp(dmax)[1]) if dmax > 0 else 1.0
    stepper = {"config": {"input_masking": INPUT_MASKING, "step": {"type": "single_module", "config": {
                   "builder": {"type": "LandNet", "config": CFG}, "in_names": IN, "out_names": OUT,
                   "next_step_forcing_names": NEXT_STEP_FORCING,
                   "normalization": {"network": {"means": means, "stds": stds}}, "ocean": None}}},
               "dataset_info": {"img_shape": [H, W], "timestep": TIMESTEP // datetime.timedelta(microseconds=1),
                                "mask_provider": {"masks": {k: v.bool() for k, v in masks.items()}}},
               "step": {"module": {**{f"module.{k}": v.bfloat16() for k, v in state_dict.items()}, "label_encoding": None}}}
    rec = {"stepper": stepper, "initial_condition": ic, "forcing": forcing, "output": out32,
           "output64_delta": {k: ((out64[k] - out32[k].double()) * scale).half() for k in OUT}, "output64_delta_scale": scale}
    for k in OUT:
        ref64 = out64[k]
        err = float((fp64_output(rec, k) - ref64).nan_to_num().abs().max() / ref64.nan_to_num().abs().max().clamp_min(1e-30))
        assert err <= 1e-9, (k, err)
        assert torch.equal(torch.isnan(out32[k]), torch.isnan(ref64)), k
        assert bool(torch.isnan(out32[k]).any()) and not bool(torch.isnan(out32[k]).all()), k
    path = os.path.join(HERE, "gen_land_rollout.pt")
    torch.save(rec, path)
    print("fp32 vs fp64:", {k: float((out32[k].double() - out64[k]).nan_to_num().abs().max() / out64[k].nan_to_num().abs().max())
                            for k in OUT})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
