"""Golden vectors for the Samudra ocean emulator, emitted by the REAL reference module (fme/ace/models/ocean/m2lines/samudra.py,
layers.py, activations.py) imported under namespace stubs - build container only.  Each case stores the builder configuration as
the plain dict the registry takes, the reference's seeded state_dict (batch-norm running statistics and norm affines made
non-trivial), the input (bfloat16 values, exact in fp32), and the reference output in fp32 and in fp64 (the same module after
.double(); stored as its difference from the fp32 output, see fp64_output).  One file per case: tests/golden/gen_samudra_<case>.pt;
a case that differs from another only in options without parameters names it in "same_as" and takes its input and
state_dict from that case's file."""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader  # noqa: E402

CASES = {
    # 4 levels, odd sizes on both axes (92 x 184 -> 46 x 92 -> 23 x 46 -> 11 x 23 -> 5 x 11): skip pads of one row / column
    "l4_instance_circular": dict(H=92, W=184, batch=2, n_in=1, n_out=1,
                                 config=dict(ch_width=[8, 8, 8, 8], dilation=[1, 2, 4, 8], n_layers=[1, 1, 1, 1], norm="instance",
                                             upscale_factor=1)),
    "l4_instance_circular_periodic_upsample": dict(same_as="l4_instance_circular",
                                                   config=dict(ch_width=[8, 8, 8, 8], dilation=[1, 2, 4, 8], n_layers=[1, 1, 1, 1],
                                                               norm="instance", upscale_factor=1, zonally_periodic_upsample=True)),
    "l3_nonorm_constant": dict(H=46, W=92, batch=1, n_in=3, n_out=1,
                               config=dict(ch_width=[8, 8, 12], dilation=[1, 2, 4], n_layers=[1, 1, 1], norm=None, pad="constant",
                                           upscale_factor=1)),
    "l3_batch": dict(H=46, W=92, batch=1, n_in=3, n_out=1,
                     config=dict(ch_width=[8, 8, 12], dilation=[1, 2, 4], n_layers=[1, 1, 1], norm="batch", upscale_factor=1)),
    "l2_instance_affine_eps": dict(H=30, W=60, batch=2, n_in=4, n_out=2,
                                   config=dict(ch_width=[8, 12], dilation=[2, 4], n_layers=[1, 1], norm="instance", upscale_factor=1,
                                               norm_kwargs={"affine": True, "eps": 1e-3})),
    # one level, 4 a % 8 == 4 for every block (a = 3, 9): the widest activation's last channel group is half-filled; identity skips
    "l1_width_mod8_4": dict(H=26, W=54, batch=1, n_in=3, n_out=2,
                            config=dict(ch_width=[9], dilation=[2], n_layers=[1], norm="instance", upscale_factor=4)),
}


def path_of(name: str) -> str:
    return os.path.join(HERE, f"gen_samudra_{name}.pt")


def load_case(name: str, directory: str = HERE) -> dict:
    """one stored case, with the input and state_dict of its "same_as" case filled in"""
    case = torch.load(os.path.join(directory, f"gen_samudra_{name}.pt"), map_location="cpu", weights_only=False)
    if "same_as" in case:
        src = torch.load(os.path.join(directory, f"gen_samudra_{case['same_as']}.pt"), map_location="cpu", weights_only=False)
        case = {**case, "state_dict": src["state_dict"], "input": src["input"]}
    return case


def fp64_output(case) -> torch.Tensor:
    """the reference's fp64 output of a stored case: output_fp32 + the fp16 difference / its power-of-two scale"""
    return case["output_fp32"].double() + case["output_fp64_delta"].double() / case["output_fp64_delta_scale"]


def load_reference():
    for pkg in ("fme", "fme.ace", "fme.ace.models", "fme.ace.models.ocean", "fme.ace.models.ocean.m2lines"):
        ref_loader._ns(pkg, os.path.join(ref_loader.REF, *pkg.split(".")))
    import importlib
    return importlib.import_module("fme.ace.models.ocean.m2lines.samudra")


def main():
    ref = load_reference()
    shared = {}
    total = 0
    for i, (name, case) in enumerate(CASES.items()):
        base = CASES[case["same_as"]] if "same_as" in case else case
        cfg = dict(case["config"])
        torch.manual_seed(100 + (list(CASES).index(case["same_as"]) if "same_as" in case else i))
        kw = dict(cfg)
        kw.setdefault("norm_kwargs", None)
        model = ref.Samudra(input_channels=base["n_in"], output_channels=base["n_out"], **kw)
        if "same_as" in case:
            model.load_state_dict(shared[case["same_as"]][0])
        if cfg.get("norm") == "batch":
            with torch.no_grad():
                for m in model.modules():
                    if isinstance(m, torch.nn.BatchNorm2d):
                        m.running_mean.normal_(0.0, 0.5)
                        m.running_var.uniform_(0.5, 2.0)
                        m.weight.normal_(1.0, 0.2)
                        m.bias.normal_(0.0, 0.2)
        if cfg.get("norm_kwargs", {}).get("affine"):
            with torch.no_grad():
                for m in model.modules():
                    if isinstance(m, torch.nn.InstanceNorm2d):
                        m.weight.normal_(1.0, 0.2)
                        m.bias.normal_(0.0, 0.2)
        model.eval()
        if "same_as" in case:
            state, x = shared[case["same_as"]]
        else:
            state = {k: v.detach().clone() for k, v in model.state_dict().items()}
            # values exactly representable in bfloat16, stored so (the file stays small; the network sees them as fp32)
            x = torch.randn(base["batch"], base["n_in"], base["H"], base["W"], generator=torch.Generator().manual_seed(7 + i)).bfloat16()
            shared[name] = (state, x)
        with torch.no_grad():
            y32 = model(x.float())
            y64 = model.double()(x.double())
        # the fp64 output as output_fp32 + a small difference (~1e-6 of the output), kept in fp16 under a power-of-two scale that
        # puts its maximum near 2^14: the fp64 result to ~1e-9 of the output at a quarter of the bytes (read with fp64_output())
        delta = y64 - y32.double()
        dmax = float(delta.abs().max())
        scale = 2.0 ** (14 - math.frexp(dmax)[1]) if dmax > 0 else 1.0
        rec = dict(config=cfg, n_in=base["n_in"], n_out=base["n_out"], H=base["H"], W=base["W"], batch=base["batch"],
                   output_fp32=y32, output_fp64_delta=(delta * scale).half(), output_fp64_delta_scale=scale)
        err = float((fp64_output(rec) - y64).abs().max() / y64.abs().max())
        assert err <= 1e-9, err
        if "same_as" in case:
            rec["same_as"] = case["same_as"]        # state_dict and input: those of that case's file
        else:
            rec.update(state_dict=state, input=x)
        torch.save(rec, path_of(name))
        size = os.path.getsize(path_of(name))
        total += size
        print(name, tuple(x.shape), "->", tuple(y32.shape), "params", sum(v.numel() for v in state.values()), "max|y|",
              float(y64.abs().max()), "fp32 vs fp64", float((y32.double() - y64).abs().max() / y64.abs().max()), "stored fp64 err", err,
              "bytes", size)
    print("wrote", len(CASES), "files,", total, "bytes")


if __name__ == "__main__":
    main()
