"""tests/golden/gen_landnet_<case>.pt: the REAL reference LandNet (fme/ace/models/land/land_net.py) on seeded weights - build
container only.  Per case: the builder config (fme/ace/registry/land_net.py's fields), the reference's seeded state_dict and the
input, both exactly representable in bfloat16 and stored so, the reference's fp32 output, and its output with the module and the
input in fp64, stored as the fp16 difference from the fp32 one under a power-of-two scale (see fp64_output)."""
import importlib
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader  # noqa: E402

# name -> (in, hidden_dims, out, use_positional_embedding, H, W, B)
CASES = {
    "small_embed": (5, [20, 7], 3, True, 9, 15, 2),
    "shipped_embed": (30, [64, 64], 10, True, 33, 65, 1),
    "one_hidden": (4, [16], 16, False, 6, 10, 1),
    "no_hidden": (3, [], 2, False, 5, 7, 1),
}


def fp64_output(case) -> torch.Tensor:
    return case["output"].double() + case["output64_delta"].double() / case["output64_delta_scale"]


def load_reference():
    for pkg in ("fme", "fme.ace", "fme.ace.models", "fme.ace.models.land"):
        if pkg not in sys.modules:
            ref_loader._ns(pkg, os.path.join(ref_loader.REF, *pkg.split(".")))
    return importlib.import_module("fme.ace.models.land.land_net")


def main():
    ref = load_reference()
    for i, (name, (cin, hidden, cout, embed, H, W, B)) in enumerate(CASES.items()):
        torch.manual_seed(300 + i)
        net = ref.LandNet(img_shape=(H, W), input_channels=cin, hidden_dims=list(hidden), output_channels=cout, network_type="MLP",
                          use_positional_embedding=embed).eval()
        with torch.no_grad():
            for p in net.parameters():
                p.copy_(p.bfloat16().float())
        state = {k: v.detach().clone() for k, v in net.state_dict().items()}
        x = torch.randn(B, cin, H, W, generator=torch.Generator().manual_seed(400 + i)).bfloat16().float()
        with torch.no_grad():
            y32 = net(x)
            y64 = net.double()(x.double())
        d = y64 - y32.double()
        dmax = float(d.abs().max())
        scale = 2.0 ** (14 - math.frexp(dmax)[1]) if dmax > 0 else 1.0
        rec = {"config": {"hidden_dims": list(hidden), "network_type": "MLP", "use_positional_embedding": embed},
               "n_in_channels": cin, "n_out_channels": cout, "img_shape": (H, W),
               "state_dict": {k: v.bfloat16() for k, v in state.items()}, "input": x.bfloat16(), "output": y32,
               "output64_delta": (d * scale).half(), "output64_delta_scale": scale}
        err = float((fp64_output(rec) - y64).abs().max() / y64.abs().max())
        assert err <= 1e-9, (name, err)
        path = os.path.join(HERE, f"gen_landnet_{name}.pt")
        torch.save(rec, path)
        print(name, "fp32 vs fp64:", float(d.abs().max() / y64.abs().max()), "wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
