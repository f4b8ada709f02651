"""TEST INFRASTRUCTURE: the contract of ``ace_disco_forward`` (include/ace_sfno.h, "DISCO convolution") restated in numpy, bit for
bit: z[c][k] = fmaf(psi[ho][e][k], x[c][hi_e][(wi_e + wo) mod W], z[c][k]) over the row's points in table order from +0, then per
output acc = fmaf(w[o][c'][k], z[g gs + c'][k], acc) over j = c' K + k ascending from +0, one fp32 addition of the embedding, the
activation.  ``fmaf`` is tests/_pixel_mlp_ref.py's (exact product in fp64, sum rounded to odd, then to fp32).

GELU and SiLU are not part of the bit-for-bit statement (the kernel's erff / expf are its toolchain's): ``disco`` returns the
pre-activation for them when asked (``pre_activation=True``) and the tests apply an fp64 activation to it."""
import os
import re

import numpy as np

from _pixel_mlp_ref import fmaf, relu

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ace_sfno.h")
ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU = 0, 1, 2, 3


def constants() -> dict:
    """The ACE_DISCO_* macros of the header."""
    text = open(HEADER).read()
    return {k: int(v) for k, v in re.findall(r"#define ACE_DISCO_(\w+) (\d+)", text)}


def disco_z(x, table, rows=None):
    """x [B][C][H][W] fp32 -> z [B][C][K][H][W] fp32 by the statement's chain (``rows``: only these output rows, in this order)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, C, H, W = x.shape
    K = table.vals.shape[1]
    rows = list(range(H)) if rows is None else list(rows)
    z = np.zeros((B, C, K, len(rows), W), np.float32)
    for i, ho in enumerate(rows):
        acc = np.zeros((B, C, K, W), np.float32)
        for e in range(int(table.row_offsets[ho]), int(table.row_offsets[ho + 1])):
            xr = np.roll(x[:, :, int(table.hi[e]), :], -int(table.wi[e]), axis=-1)            # xr[wo] = x[(wi + wo) mod W]
            acc = fmaf(np.broadcast_to(table.vals[e][None, None, :, None], acc.shape), np.broadcast_to(xr[:, :, None, :], acc.shape), acc)
        z[:, :, :, i, :] = acc
    return z


def disco_mix(z, w, groups):
    """z [B][C][K][H][W], w [O][gs][K] -> [B][O][H][W]: per output the fmaf chain over j = c' K + k ascending, from +0."""
    B, C, K, H, W = z.shape
    O, gs, _ = w.shape
    opg = O // groups
    out = np.zeros((B, O, H, W), np.float32)
    for g in range(groups):
        acc = np.zeros((B, opg, H, W), np.float32)
        wg = w[g * opg:(g + 1) * opg]
        for cp in range(gs):
            for k in range(K):
                acc = fmaf(np.broadcast_to(wg[None, :, cp, k, None, None], acc.shape),
                           np.broadcast_to(z[:, None, g * gs + cp, k], acc.shape), acc)
        out[:, g * opg:(g + 1) * opg] = acc
    return out


def disco(x, table, w, groups, act=ACT_NONE, embed=None, pre_activation=False, rows=None):
    """The statement: x [B][C][H][W], w [O][C / groups][K], embed [O][H][W] or None -> y [B][O][H][W] (or [B][O][rows][W])."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    acc = disco_mix(disco_z(x, table, rows), w, groups)
    if embed is not None:
        e = np.asarray(embed, dtype=np.float32)
        with np.errstate(all="ignore"):
            acc = (acc + (e if rows is None else e[:, list(rows)])[None]).astype(np.float32)
    if pre_activation or act == ACT_NONE:
        return acc
    if act == ACT_RELU:
        return relu(acc)
    raise ValueError("GELU / SiLU are held to an fp64 activation of the pre-activation, not stated bit for bit")


def gelu64(v):
    import math
    v = np.asarray(v, dtype=np.float64)
    erf = np.vectorize(math.erf, otypes=[np.float64])
    with np.errstate(all="ignore"):
        return 0.5 * v * (1.0 + erf(v / math.sqrt(2.0)))


def silu64(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        return v / (1.0 + np.exp(-v))
