"""TEST INFRASTRUCTURE: the contract of ``ace_pixel_mlp_forward`` (include/ace_sfno.h, "Per-pixel MLP") restated in numpy, bit for
bit: per pixel and layer ``acc = bias``, then ``acc = fmaf(w[o][k], a[k], acc)`` over k in the header's order ("for tile t, for r,
for g: k = 16 t + 4 g + r", k < K only), then relu(v) = v < 0 ? +0 : v, then one fp32 addition of the embedding.

``fmaf`` is formed without a fused instruction: the product of two fp32 numbers is exact in fp64; the sum with the addend is
rounded TO ODD in fp64 (round-to-nearest sum, then - where the TwoSum error term says the sum was inexact and its last bit is even -
one step towards the error), and that rounds to fp32 as the exact sum would (53 >= 2 * 24 + 2 bits)."""
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ace_sfno.h")


def constants() -> dict:
    """The ACE_PIXEL_MLP_* macros of the header."""
    text = open(HEADER).read()
    return {k: int(v) for k, v in re.findall(r"#define ACE_PIXEL_MLP_(\w+) (\d+)", text)}


TILE = constants()["TILE"]


def k_order(K: int):
    """The header's summation order of a layer with K inputs."""
    return [TILE * t + 4 * g + r for t in range((K + TILE - 1) // TILE) for r in range(4) for g in range(4) if TILE * t + 4 * g + r < K]


def fmaf(a, b, c):
    """round_fp32(a * b + c) with a single rounding, elementwise on fp32 arrays (Inf / NaN as IEEE)."""
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)          # exact
        c = c.astype(np.float64)
        s = p + c
        bb = s - p                                               # TwoSum: s + e == p + c exactly
        e = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.int64) & 1) != 0
        fix = np.isfinite(s) & (e != 0) & ~odd
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def relu(v):
    return np.where(v < 0, np.float32(0.0), v)      # NaN < 0 and -0 < 0 are false: both stay


def pixel_mlp(x, weights, biases, acts, embed_layer=-1, embed=None):
    """x [B][dims[0]][hw] fp32; weights[l] [O][K]; biases[l] [O] or None; acts[l] 0 / 1; embed [dims[embed_layer + 1]][hw]."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    B, _, hw = a.shape
    for l, w in enumerate(weights):
        w = np.asarray(w, dtype=np.float32)
        O, K = w.shape
        assert a.shape[1] == K
        bias = np.zeros(O, np.float32) if biases is None or biases[l] is None else np.asarray(biases[l], dtype=np.float32)
        acc = np.broadcast_to(bias[None, :, None], (B, O, hw)).copy()
        for k in k_order(K):
            acc = fmaf(np.broadcast_to(w[None, :, k, None], acc.shape), np.broadcast_to(a[:, None, k, :], acc.shape), acc)
        if acts[l]:
            acc = relu(acc)
        if l == embed_layer:
            with np.errstate(all="ignore"):
                acc = (acc + np.asarray(embed, dtype=np.float32)[None]).astype(np.float32)
        a = acc
    return a


def landnet_statement(state_dict, x, use_embed: bool):
    """The statement on a LandNet state_dict (torch tensors, the reference's keys) and a (B, C, H, W) input -> (B, O, H, W) numpy."""
    n = len([k for k in state_dict if k.endswith(".weight")])
    ws = [state_dict[f"model.{l}.layers.0.weight"].float().numpy().reshape(state_dict[f"model.{l}.layers.0.weight"].shape[:2]) for l in range(n)]
    bs = [state_dict[f"model.{l}.layers.0.bias"].float().numpy() for l in range(n)]
    B, C, H, W = x.shape
    embed = state_dict["pos_embed.pos_embed"].float().numpy().reshape(-1, H * W) if use_embed else None
    y = pixel_mlp(x.float().numpy().reshape(B, C, H * W), ws, bs, [1] * (n - 1) + [0], 0 if use_embed else -1, embed)
    return y.reshape(B, -1, H, W)
