"""Cases for the instance-norm statistics under a large per-channel mean (DC), and their truth.

A trained pos_embed, fc2 bias or inner-skip bias puts an arbitrary per-channel constant on the tensor an instance norm sees.  The
norm removes it, so a constant added at ONE of the three sites below reaches exactly one norm at full size and no later one:

  site "h0": pos_embed                        -> blocks.0.norm0        (statistics from the encoder's epilogue)
  site "t" : blocks.{last}.inner_skip.bias    -> blocks.{last}.norm1   (statistics from the inner skip's epilogue, after GELU)
  site "h1": blocks.0.mlp.fwd.2.bias          -> blocks.1.norm0        (statistics from fc2's epilogue)

Plain torch and oracle/sfno.py; the oracle's arithmetic is untouched - its `_norm` is wrapped from outside to record every norm's
input and output.  Cases and oracle passes are cached: the CPU conditions test and every GPU routing / precision share them."""

import dataclasses
import functools

import torch

from oracle.sfno import SFNOConfig, SFNOOracle, init_state

SITES = ("h0", "t", "h1")
IN_CHANS, OUT_CHANS, BATCH = 5, 4, 2


class _Reached(Exception):
    pass


def target_norm(site: str, num_layers: int) -> str:
    return {"h0": "blocks.0.norm0", "t": f"blocks.{num_layers - 1}.norm1", "h1": "blocks.1.norm0"}[site]


def site_param(site: str, num_layers: int) -> str:
    return {"h0": "pos_embed", "t": f"blocks.{num_layers - 1}.inner_skip.bias", "h1": "blocks.0.mlp.fwd.2.bias"}[site]


def run_oracle(cfg, state, x, dtype, stop_at=None):
    """One oracle forward with every norm's (input, output) recorded.  stop_at: leave once that norm has run (the calibration
    passes need nothing behind it).  Returns (records, taps, y); taps and y are None after an early exit."""
    orc = SFNOOracle(cfg, state, dtype=dtype)
    inner, rec = orc._norm, {}

    def recording_norm(t, prefix):
        out = inner(t, prefix)
        rec[prefix] = (t, out)
        if prefix == stop_at:
            raise _Reached
        return out

    orc._norm = recording_norm
    try:
        with torch.no_grad():
            y, taps = orc.forward(x, return_blocks=True)
    except _Reached:
        return rec, None, None
    return rec, taps, y


def channel_stats(t):
    """per-channel |mean| and std of a (B, C, H, W) norm input: per (sample, channel) plane, then the mean over the samples"""
    t = t.double()
    return t.mean(dim=(2, 3)).abs().mean(0), t.std(dim=(2, 3), unbiased=False).mean(0)


def realised(t):
    """(median ratio, min ratio, min std / max std) of |mean| / std over the channels of a norm input"""
    m, s = channel_stats(t)
    r = m / s
    return float(r.median()), float(r.min()), float(s.min() / s.max())


@functools.lru_cache(maxsize=None)
def _base(C, hw, num_layers, seed):
    cfg = SFNOConfig(in_chans=IN_CHANS, out_chans=OUT_CHANS, img_shape=tuple(hw), embed_dim=C, num_layers=num_layers,
                     operator_type="dhconv")
    state = init_state(cfg, seed=seed)
    x = torch.randn(BATCH, IN_CHANS, *hw, generator=torch.Generator().manual_seed(seed + 1))
    return cfg, state, x


@functools.lru_cache(maxsize=None)
def _zero_dc_std(C, hw, num_layers, site, seed):
    cfg, state, x = _base(C, hw, num_layers, seed)
    name = target_norm(site, num_layers)
    rec, _, _ = run_oracle(cfg, state, x, torch.float64, stop_at=name)
    return channel_stats(rec[name][0])[1]


@dataclasses.dataclass
class Case:
    cfg: SFNOConfig
    state: dict
    x: torch.Tensor
    target: str          # name of the norm the constant reaches
    rec64: dict          # norm name -> (input, output), fp64 oracle
    taps64: list
    y64: torch.Tensor
    rec32: dict          # the same from the fp32 oracle: the reference floor
    taps32: list
    y32: torch.Tensor


@functools.lru_cache(maxsize=None)
def make_case(C, hw, num_layers, site, ratio, seed=0) -> Case:
    """A net whose `target_norm(site)` input has |mean| / std = ratio in every channel (ratio 0: init_state as it is)."""
    cfg, state, x = _base(C, tuple(hw), num_layers, seed)
    state = dict(state)
    name = target_norm(site, num_layers)
    if ratio:
        std = _zero_dc_std(C, tuple(hw), num_layers, site, seed)
        g = torch.Generator().manual_seed(seed + 2)
        # "t": positive only - a negative constant sends the channel through GELU to ~0 (degenerate)
        sign = torch.ones(C, dtype=torch.float64) if site == "t" else (torch.randint(0, 2, (C,), generator=g).double() * 2 - 1)
        dc = sign * ratio * std
        key = site_param(site, num_layers)
        base = state[key].double()
        shape = (1, C, 1, 1) if site == "h0" else (C,)
        state[key] = (base + dc.reshape(shape)).float()
        if site == "t":
            # GELU halves the zero-DC std and is linear once the constant is on: the naive recipe realises about ratio / 2.
            # One more pass measures what it realised, the constant is rescaled per channel to hit the target.
            rec, _, _ = run_oracle(cfg, state, x, torch.float64, stop_at=name)
            m, s = channel_stats(rec[name][0])
            state[key] = (base + dc * (ratio * s / m)).float()
    rec64, taps64, y64 = run_oracle(cfg, state, x, torch.float64)
    rec32, taps32, y32 = run_oracle(cfg, state, x, torch.float32)
    return Case(cfg, state, x, name, rec64, taps64, y64, rec32, taps32, y32)


def z_from_affine(scale, shift, x64):
    """the normalised tensor an affine (scale, shift) per (sample, channel) gives on the fp64 norm input, evaluated in fp64"""
    return scale.double()[:, :, None, None] * x64.double() + shift.double()[:, :, None, None]


def stat_err(z, z64):
    """(overall, worst channel) of max|z - z64| / max|z64|; the channel measure takes both maxima over that channel"""
    d = (z.double() - z64).abs()
    per = d.amax(dim=(0, 2, 3)) / z64.abs().amax(dim=(0, 2, 3))
    return float(d.max() / z64.abs().max()), float(per.max())


def floor_of(case: Case, name: str):
    """stat_err of the fp32 oracle's output of norm `name` against the fp64 one: what fp32 two-pass statistics on fp32 data give"""
    return stat_err(case.rec32[name][1], case.rec64[name][1])


# ---- the grid the GPU tests and the CPU conditions test share
RATIOS = (10, 30, 300)
SITE_DEPTH = (("h0", 1), ("t", 1), ("t", 2), ("h1", 2))
# C = 128 at 24 x 48: every fast kernel eligible.  C = 384 at 45 x 90: K = 384, ragged last tile (4050 = 126 * 32 + 18) - but H W % 4
# != 0 keeps the packed-operand engines out, so there the statistics come from the stand-alone instnorm_stats_kernel.  C = 384 at
# 46 x 92 (4232 = 132 * 32 + 8, a multiple of 4) is the K = 384 shape whose partials DO come from the producers' epilogues: extra
# workgroups and two-tile segments on conv_ws.hip (ws_plan.h), a ragged last strip on the tile engine.
SHAPES = ((128, (24, 48)), (384, (45, 90)), (384, (46, 92)))
LONG_RUN = ((128, (180, 360), 1, "t", 30), (128, (180, 360), 2, "h1", 30))


def grid_cases():
    return [(C, hw, nl, site, ratio) for C, hw in SHAPES for site, nl in SITE_DEPTH for ratio in RATIOS]


def ws_tiles_per_segment(M, HW, allow_extra):
    """pixel tiles per segment of a conv_ws launch's regular workgroups: `g` of ws_plan (csrc/ws_plan.h), restated"""
    nslice = M // 128
    tiles = (HW + 31) // 32
    tpx = (tiles + 7) // 8
    F0 = max(32 // nslice, 1)
    if tpx <= F0:
        return 1
    left = max(32 - F0 * nslice, 0)
    if not allow_extra and left > 0 and 8 * left >= nslice:
        XG = 8 * left // nslice
        return (tiles + 8 * F0 + XG - 1) // (8 * F0 + XG)
    R = left if allow_extra else 0
    e = (tpx * R + 16) // 32 if R > 0 else 0
    if e * nslice < R:
        e = 0
    return (tpx - e + F0 - 1) // F0
