"""tests/golden/gen_fill.pt from the reference's own SmoothFloodFill(num_steps=4) (fme/core/fill.py; imported through
oracle/ref_loader.load_stepper_ref's stubs): four masks, each with a (1, 2, H, W) fp32 field that is NaN exactly on the masked
pixels, and the reference's filled output.
  "continent" 24 x 40: a continent across the dateline that touches the north pole, a southern block and a one-pixel lake inside
              the continent; every layer 0..5 is populated.  Offset 290, scale 10.
  "single"    17 x 34: one valid pixel.  Offset 1e5, scale 900.
  "seam"      45 x 90: an interior block, the whole seam column 0 and the whole north pole row masked.  Offset -3, scale 2.
  "random"     9 x 18: random 30 % land without an interior.  Offset 290, scale 10.
Stored per case: ``mask`` (H, W) fp32 with 1 = valid, ``input``, ``output``."""
import importlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader  # noqa: E402


def masks():
    c = torch.ones(24, 40)
    c[0:13, 33:] = 0                     # the continent: 13 rows from the pole, 14 columns across the dateline
    c[0:13, :7] = 0
    c[6, 37] = 1                         # the lake
    c[16:23, 14:25] = 0                  # the southern block
    s = torch.zeros(17, 34)
    s[9, 20] = 1
    m = torch.ones(45, 90)
    m[15:31, 30:52] = 0
    m[:, 0] = 0
    m[0, :] = 0
    r = (torch.rand(9, 18, generator=torch.Generator().manual_seed(99)) >= 0.3).float()
    return {"continent": (c, 290.0, 10.0), "single": (s, 1e5, 900.0), "seam": (m, -3.0, 2.0), "random": (r, 290.0, 10.0)}


def main():
    ref_loader.load_stepper_ref()
    fill = importlib.import_module("fme.core.fill")
    g = torch.Generator().manual_seed(7)
    out = {}
    for name, (mask, offset, scale) in masks().items():
        H, W = mask.shape
        # a smooth part and noise, so that neighbouring pixels differ by the field's own variability
        lat = torch.linspace(-1.5, 1.5, H)[:, None]
        lon = torch.linspace(0, 6.283, W + 1)[None, :-1]
        x = offset + scale * (torch.cos(lat) * torch.sin(2 * lon) + 0.5 * torch.randn(1, 2, H, W, generator=g))
        x = x.float().where(mask != 0, torch.tensor(float("nan")))
        y = fill.SmoothFloodFill(num_steps=4)(x.clone(), name)
        assert bool(torch.isfinite(y).all()), name
        interior = fill._get_interior_mask(mask == 0, 4)
        print(name, tuple(mask.shape), "valid", int((mask != 0).sum()), "interior", int(interior.sum()))
        out[name] = {"mask": mask, "input": x, "output": y.float()}
    dst = os.path.join(HERE, "gen_fill.pt")
    torch.save(out, dst)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 200 * 1024


if __name__ == "__main__":
    main()
