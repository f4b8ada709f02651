"""tests/golden/gen_ankur_<case>.pt and gen_ankur_tables.pt: the REAL reference AnkurLocalNet
(fme/core/models/conditional_sfno/ankur.py under fme/ace/registry/local_net.py's wrapper keys) and the reference's own DISCO tables
(fme/core/disco/_convolution.py) - build container only.

Per case: the builder config, the seeded state_dict and the input (both exactly representable in bfloat16 and stored so), the
reference's fp32 output, and the fp64 truth stored as the fp16 difference from the fp32 output under a power-of-two scale (see
fp64_output).  The reference's DISCO casts whatever it is given to fp32, so the truth is not the module in fp64: it is the direct
fp64 sum  z[b, c, k, ho, wo] = sum psi[k, ho, hi, wi] x[b, c, hi, (wi + wo) mod W]  over the reference's own psi_idx / psi_vals,
the fp64 grouped mix with the weight, and the fp64 rest of the network.

gen_ankur_tables.pt: per grid the reference's row offsets, column indices (hi * W + wi) and fp32 values [K][points of the row] of
kernel index 0 .. K - 1 (all K share one support; asserted here)."""
import importlib
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader  # noqa: E402

# name -> (H, W, kernel_size, in, embed_dim, out, use_disco_encoder, pos_embed, activation, B)
CASES = {
    "disco_gelu": (8, 16, 3, 6, 24, 4, True, False, "gelu", 2),
    "disco_relu_embed": (9, 20, 2, 12, 32, 5, True, True, "relu", 1),
    "disco_silu_embed": (6, 8, 3, 5, 24, 3, True, True, "silu", 2),
    "depthwise_relu": (16, 36, 3, 8, 8, 8, True, False, "relu", 1),
    "conv_gelu_embed": (6, 8, 3, 5, 24, 3, False, True, "gelu", 1),
    "conv_relu_embed": (9, 20, 3, 7, 65, 4, False, True, "relu", 2),
}
# (H, W, kernel_size)
TABLE_GRIDS = [(6, 8, 3), (8, 16, 3), (9, 20, 2), (16, 36, 3), (24, 70, 4), (180, 360, 3)]


def fp64_output(case) -> torch.Tensor:
    return case["output"].double() + case["output64_delta"].double() / case["output64_delta_scale"]


def load_reference():
    """(ankur module, DiscreteContinuousConvS2): the stub Distributed of ref_loader gets the DISCO factory in this process."""
    ref_loader.load_csfno()
    for pkg in ("fme.core.disco",):
        if pkg not in sys.modules:
            ref_loader._ns(pkg, os.path.join(ref_loader.REF, *pkg.split(".")))
    conv = importlib.import_module("fme.core.disco._convolution")
    D = sys.modules["fme.core.distributed"].Distributed
    D.get_disco_conv_s2 = lambda self, *a, **k: conv.DiscreteContinuousConvS2(*a, **k)
    ankur = importlib.import_module("fme.core.models.conditional_sfno.ankur")
    return ankur, conv.DiscreteContinuousConvS2


def reference_table(disco):
    """(row offsets [H + 1], column index [P], values [K][P]) from a reference DISCO module, the K kernels' supports asserted equal."""
    ker, row, col, vals = disco.psi_ker_idx, disco.psi_row_idx, disco.psi_col_idx, disco.psi_vals
    K, H = disco.kernel_size, disco.nlat_out
    per_k = []
    for k in range(K):
        m = ker == k
        per_k.append((row[m], col[m], vals[m]))
    r0, c0, _ = per_k[0]
    for r, c, _ in per_k[1:]:
        assert torch.equal(r, r0) and torch.equal(c, c0), "the supports of the K basis functions differ"
    assert torch.equal(r0, torch.sort(r0, stable=True)[0])
    offs = torch.zeros(H + 1, dtype=torch.int64)
    offs[1:] = torch.cumsum(torch.bincount(r0, minlength=H), 0)
    return offs, c0.to(torch.int32), torch.stack([v for _, _, v in per_k]).float()


def truth64(net, x, cfg):
    """The fp64 truth of the net on x (see the module docstring)."""
    x = x.double()
    mods = list(net.mlp)
    i = 0
    if cfg["use_disco_encoder"]:
        d = mods[0].conv
        offs, col, vals = reference_table(d)
        K, H, W = d.kernel_size, d.nlat_in, d.nlon_in
        B, C = x.shape[:2]
        z = torch.zeros(B, C, K, H, W, dtype=torch.float64)
        v64 = vals.double()
        for ho in range(H):
            for e in range(int(offs[ho]), int(offs[ho + 1])):
                hi, wi = int(col[e]) // W, int(col[e]) % W
                z[:, :, :, ho, :] += v64[:, e][None, None, :, None] * torch.roll(x[:, :, hi, :], -wi, dims=-1)[:, :, None, :]
        w = d.weight.detach().double()
        G = d.groups
        h = torch.einsum("bgckxy,gock->bgoxy", z.reshape(B, G, d.groupsize, K, H, W), w.reshape(G, -1, w.shape[1], w.shape[2]))
        x = h.reshape(B, -1, H, W)
        i = 1
    for m in mods[i:]:
        x = m.double()(x)
    return x


def main():
    ankur, Disco = load_reference()
    for i, (name, (H, W, ks, cin, embed, cout, use_disco, pos, act, B)) in enumerate(CASES.items()):
        torch.manual_seed(700 + i)
        cfg = {"embed_dim": embed, "use_disco_encoder": use_disco, "disco_kernel_size": ks, "pos_embed": pos,
               "activation_function": act}
        net = ankur.AnkurLocalNet(ankur.AnkurLocalNetConfig(**cfg), img_shape=(H, W), in_chans=cin, out_chans=cout,
                                  data_grid="legendre-gauss").eval()
        with torch.no_grad():
            for p in net.parameters():
                if p.dim() == 4 and p.shape[0] == 1:                     # the positional embedding: std 0.02, seen at full size
                    p.copy_(torch.randn_like(p))
                p.copy_(p.bfloat16().float())
        state = {"module." + k: v.detach().clone() for k, v in net.state_dict().items()}
        x = torch.randn(B, cin, H, W, generator=torch.Generator().manual_seed(800 + i)).bfloat16().float()
        with torch.no_grad():
            y32 = net(x, None)
            y64 = truth64(net, x, cfg)
        d = y64 - y32.double()
        dmax = float(d.abs().max())
        scale = 2.0 ** (14 - math.frexp(dmax)[1]) if dmax > 0 else 1.0
        rec = {"config": cfg, "n_in_channels": cin, "n_out_channels": cout, "img_shape": (H, W),
               "state_dict": {k: v.bfloat16() for k, v in state.items()}, "input": x.bfloat16(), "output": y32,
               "output64_delta": (d * scale).half(), "output64_delta_scale": scale,
               "reference_error": float(d.abs().max() / y64.abs().max())}
        err = float((fp64_output(rec) - y64).abs().max() / y64.abs().max())
        assert err <= 1e-9, (name, err)
        path = os.path.join(HERE, f"gen_ankur_{name}.pt")
        torch.save(rec, path)
        print(name, "keys", sorted(state), "fp32 vs fp64:", rec["reference_error"], "wrote", path, os.path.getsize(path), "bytes")
    tables = {}
    for H, W, ks in TABLE_GRIDS:
        d = Disco(1, 1, (H, W), (H, W), (ks, ks), basis_type="morlet", basis_norm_mode="mean", groups=1, grid_in="legendre-gauss",
                  grid_out="legendre-gauss", bias=False, theta_cutoff=(ks + 1) * 0.5 * math.pi / float(H - 1))
        offs, col, vals = reference_table(d)
        tables[(H, W, ks)] = {"row_offsets": offs, "col_idx": col, "vals": vals}
        print((H, W, ks), "points", int(offs[-1]), "per row", (offs[1:] - offs[:-1])[:6].tolist())
    path = os.path.join(HERE, "gen_ankur_tables.pt")
    torch.save(tables, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
