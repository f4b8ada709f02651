"""tests/golden/gen_ice_rollout.pt: B = 2, T = 4 steps at 16 x 32 of a small Samudra stepper over the sea-ice names of the reference's
fme/ace/test_ice_train.py (siconc and its budget terms LSRCc / LSNKc / XPRTc) plus simass / sisnmass with theirs, with input masking
on mask_2d, the provider's output masking and the ice corrector over all three variables, emitted by the REAL reference's pieces -
build container only.

Composed as tests/golden/make_golden_ocean_rollout.py composes its stepper (the reference ``Stepper`` does not come up under
oracle/ref_loader's stubs): input masking of the input -> normalise -> pack -> Samudra -> unpack -> denormalise -> ice corrector
on (masked input, output) (fme/core/corrector/ice.py) -> the provider's output masker; the masked output is the next step's state.
Stored: the stepper checkpoint in ace_amd's load_stepper layout (weights bfloat16-exact, stored as bfloat16), the initial condition
and forcing, the fp32 rollout, the same rollout with every piece in fp64 as its fp16 difference from the fp32 one under a
power-of-two scale (make_golden_ocean_rollout.fp64_output), and the flag path the reference's corrector took at every step."""
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
from make_golden_ice_corrector import paths_from_any, plan_of  # noqa: E402
from make_golden_ocean_rollout import fp64_output  # noqa: E402

H, W, B, T = 16, 32, 2, 4
CFG = {"ch_width": [8, 8], "dilation": [1, 2], "n_layers": [1, 1], "pad": "circular", "norm": "instance", "upscale_factor": 1}
CORRECTED = {"siconc": ["LSRCc", "LSNKc", "XPRTc"], "simass": ["SIMSRC", "SIMSNK", "SIMXPRT"], "sisnmass": ["SNSRC", "SNSNK", "SNXPRT"]}
OUT = [n for name, terms in CORRECTED.items() for n in (name, *terms)]
FORCING = ["DSWRFsfc"]
IN = FORCING + OUT
INPUT_MASKING = {"mask_value": 0, "fill_value": 0.0}
CORRECTOR = {"budget_correction": {"corrected_variables": CORRECTED}}
TIMESTEP = datetime.timedelta(days=2)
DT = TIMESTEP.total_seconds()
SCALE = {"siconc": 1.0, "simass": 40.0, "sisnmass": 7.0}


def setup():
    g = torch.Generator().manual_seed(21)
    mask = (torch.rand(H, W, generator=g) > 0.2).float()
    mask[:2] = 0.0
    masks = {"mask_2d": mask}
    stats = {"DSWRFsfc": (180.0, 90.0)}
    for name, terms in CORRECTED.items():
        c = SCALE[name]
        stats[name] = (0.45 * c, 0.3 * c)
        # the ice mass keeps well away from zero over the ocean: "ice mass == 0" is decided by the last bit of an fp64 sum wherever
        # stage 1 has emptied a pixel, and a rollout compared at a tolerance must not hang on it.  It is so decided on the land
        # pixels (a zero fill as the old mass), which raise the flags of every stage and come out NaN.
        w = 0.02 if name == "simass" else 0.1
        stats[terms[0]], stats[terms[1]], stats[terms[2]] = (w * c / DT, w * c / DT), (-w * c / DT, w * c / DT), (0.0, 1.5 * w * c / DT)
    means = {n: v[0] for n, v in stats.items()}
    stds = {n: v[1] for n, v in stats.items()}
    return mask, masks, means, stds


def data(means, stds):
    g = torch.Generator().manual_seed(22)
    ic = {n: torch.randn(B, 1, H, W, generator=g) * stds[n] + means[n] for n in OUT}
    for name in CORRECTED:
        ic[name] = torch.rand(B, 1, H, W, generator=g) * SCALE[name]
    ic["simass"] = (0.3 + 0.7 * torch.rand(B, 1, H, W, generator=g)) * SCALE["simass"]
    forcing = {"DSWRFsfc": torch.randn(B, T + 1, H, W, generator=g) * 90.0 + 180.0}
    return ic, forcing


def rollout(mods, net, dtype, setup_, ic, forcing):
    sm, smp, norm_mod, packer_mod, ice = mods
    mask, masks, means, stds = setup_
    c = lambda d: {k: v.to(dtype) for k, v in d.items()}
    provider = smp.SpatialMaskProvider(c(masks))
    normalizer = norm_mod.StandardNormalizer(means={k: torch.tensor(v, dtype=dtype) for k, v in means.items()},
                                             stds={k: torch.tensor(v, dtype=dtype) for k, v in stds.items()})
    in_mask = sm.StaticSpatialMaskingConfig(**INPUT_MASKING).build(mask=provider, means=normalizer.means)
    out_mask = provider.build_output_spatial_masker()
    corrector = ice.IceCorrectorConfig(budget_correction=ice.IceBudgetCorrectionConfig(**CORRECTOR["budget_correction"]))._build(None, TIMESTEP)
    in_packer, out_packer = packer_mod.Packer(IN), packer_mod.Packer(OUT)
    net = net.to(dtype)
    state = {k: v[:, 0].to(dtype) for k, v in ic.items()}
    forcing = c(forcing)
    plan = plan_of(CORRECTED)
    outs, paths = [], []
    real_any = torch.any
    for s in range(T):
        inp = {**state, **{k: forcing[k][:, s] for k in FORCING}}
        nxt = {k: forcing[k][:, s + 1] for k in FORCING}
        inp, nxt = in_mask(inp), in_mask(nxt)
        x = in_packer.pack(normalizer.normalize(inp), axis=-3)
        with torch.no_grad():
            y = net(x)
        gen = normalizer.denormalize(out_packer.unpack(y, axis=-3))
        seen = []

        def recording_any(*a, **k):
            r = real_any(*a, **k)
            seen.append(bool(r))
            return r
        torch.any = recording_any
        try:
            gen = corrector(inp, gen, nxt, None).corrected
        finally:
            torch.any = real_any
        paths.append(paths_from_any(plan, seen))
        state = out_mask(gen)
        outs.append(state)
    return {k: torch.stack([o[k] for o in outs], dim=1) for k in OUT}, paths


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
    ice = importlib.import_module("fme.core.corrector.ice")
    from make_golden_samudra import load_reference
    samudra = load_reference()
    mods = (sm, smp, norm_mod, packer_mod, ice)
    setup_ = setup()
    mask, masks, means, stds = setup_
    torch.manual_seed(23)
    net = samudra.Samudra(input_channels=len(IN), output_channels=len(OUT), norm_kwargs=None, **CFG).eval()
    with torch.no_grad():         # weights exactly representable in bfloat16, stored so
        for p in net.parameters():
            p.copy_(p.bfloat16().float())
    state_dict = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ic, forcing = data(means, stds)
    out32, paths32 = rollout(mods, net, torch.float32, setup_, ic, forcing)
    net.load_state_dict(state_dict)
    out64, paths64 = rollout(mods, net.double(), torch.float64, setup_, ic, forcing)
    print("paths fp32:", paths32)
    print("paths fp64:", paths64)
    assert any(any(p) for step in paths32 for p in step.values()), "no stage ever ran"
    dmax = max(float((out64[k] - out32[k].double()).nan_to_num().abs().max()) for k in OUT)
    scale = 2.0 ** (14 - math.frexp(dmax)[1]) if dmax > 0 else 1.0
    stepper = {"config": {"input_masking": INPUT_MASKING, "step": {"type": "single_module", "config": {
                   "builder": {"type": "Samudra", "config": CFG}, "in_names": IN, "out_names": OUT,
                   "normalization": {"network": {"means": means, "stds": stds}}, "ocean": None,
                   "corrector": {"type": "ice_corrector", "config": CORRECTOR}}}},
               "dataset_info": {"img_shape": [H, W], "timestep": TIMESTEP // datetime.timedelta(microseconds=1),
                                "mask_provider": {"masks": {k: v.bool() for k, v in masks.items()}}},
               "step": {"module": {**{f"module.{k}": v.bfloat16() if v.is_floating_point() else v for k, v in state_dict.items()},
                                   "label_encoding": None}}}
    rec = {"stepper": stepper, "initial_condition": ic, "forcing": forcing, "output": out32, "paths": paths32,
           "output64_delta": {k: ((out64[k] - out32[k].double()) * scale).half() for k in OUT}, "output64_delta_scale": scale}
    for k in OUT:
        assert torch.equal(torch.isnan(out32[k]), torch.isnan(out64[k])), k
    path = os.path.join(HERE, "gen_ice_rollout.pt")
    torch.save(rec, path)
    print("fp32 vs fp64:", {k: float((out32[k].double() - out64[k]).nan_to_num().abs().max() / out64[k].nan_to_num().abs().max())
                            for k in OUT})
    print("stored fp64:", {k: float((fp64_output(rec, k) - out64[k]).nan_to_num().abs().max() / out64[k].nan_to_num().abs().max())
                           for k in ("siconc", "simass", "LSRCc")})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
