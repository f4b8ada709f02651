"""The records the step-mean and ensemble-metric tests run on, made of exact arithmetic only (integer hashes and rationals) so that
tests/golden/make_golden_ensemble.py and every test machine build the same fp32 bits: a 5 x 7 grid (35 pixels, not a multiple of
4), 3 initial conditions x 5 members (sample b = i * 5 + e), ``n_ic_steps`` initial-condition steps (1 by default) and 6 forward
steps in windows of 3 + 3.  The prediction is the target's field plus a bias of 0.9 + 0.3 lat / 90 standard deviations and member
noise of 0.8 x U(-0.5, 0.5) standard deviations, so the squared error of the ensemble mean (0.5 to 1.2 sigma^2) is far above the
variance / E that the spread-skill ratio takes off it (0.011 sigma^2): spread / sqrt(mse - var / E) is well conditioned and fp32
and fp64 statements of it can be compared.  Over a "calm" patch of every name the bias is 0 and the member noise sums to zero, so the
ensemble mean is the target up to rounding, mse - var / E is -var / E, clamped, and the ratio reports -1 by convention - again far
from the clamp's edge, where the ratio is a 0 / 0.  Names:
  * ``a``: over a "prescribed" patch every member equals the target (spread and error exactly 0);
  * ``b``: one NaN in one member (sample 7 = initial condition 1, member 2) at one pixel of the time indices below 4;
  * ``c``: the target is NaN everywhere (the reference's filled missing variable), the prediction is not."""
import numpy as np
import torch

from ace_amd.dataset_info import DatasetInfo

H, W = 5, 7
N_IC, E = 3, 5
B = N_IC * E
N_FORWARD = 6
NAMES = ["a", "b", "c"]
PRESCRIBED = (slice(1, 3), slice(2, 5))
CALM = (slice(3, 5), slice(0, 3))
NAN_AT = (7, 3, 4)                                       # sample, row, column
NAN_UNTIL = 4                                            # the time indices 0 .. 3 hold the NaN
LAT = np.arange(-60.0, 61.0, 30.0)
MEANS = {"a": 280.0, "b": 2.0, "c": -1.0}
STDS = {"a": 4.0, "b": 0.5, "c": 3.0}


def _noise(shape, salt):
    """uniform in [-0.5, 0.5) from a 64-bit multiplicative hash of the element index: the same bits on every machine"""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        h = (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(6364136223846793005) + np.uint64(1442695040888963407)
        h ^= h >> np.uint64(29)
        h = h * np.uint64(0x9E3779B97F4A7C15)
    return ((h >> np.uint64(40)).astype(np.float64) / 2.0 ** 24 - 0.5).reshape(shape)


def info():
    return DatasetInfo((H, W), lat=torch.tensor(LAT, dtype=torch.float32))


def stats(device="cpu"):
    """the normaliser: per-name means and standard deviations on ``device``, where the windows live (torch on a GPU divides by a
    0-dim tensor of its own device as written, but turns a division by a CPU scalar into a multiplication by its reciprocal)"""
    from ace_amd.normalizer import StandardNormalizer
    return StandardNormalizer(MEANS, STDS, device=device)


def case(n_ic_steps=1, cuts=(3,)):
    """``gen`` / ``target``: name -> (B, n_ic_steps + 6, H, W) fp32; ``ic``: the pair of initial-condition windows; ``windows``:
    the (gen, target) pairs of the forward steps, cut at ``cuts`` (forward-step offsets)"""
    n_time = n_ic_steps + N_FORWARD
    lat = LAT[:, None] / 90.0
    bias = np.broadcast_to(0.9 + 0.3 * lat, (H, W)).copy()
    bias[CALM] = 0.0
    out = []
    for side in range(2):
        d = {}
        for k, name in enumerate(NAMES):
            ic = np.repeat(_noise((N_IC, 1, n_time, H, W), 11 + 100 * k), E, axis=1)          # what the members of one i share
            x = MEANS[name] + STDS[name] * (1.5 * lat + ic) + side * STDS[name] * bias
            if side == 0:
                member = _noise((N_IC, E, n_time, H, W), 1000 + 100 * k)
                member[..., CALM[0], CALM[1]] -= member[..., CALM[0], CALM[1]].mean(axis=1, keepdims=True)
                x = x + STDS[name] * 0.8 * member
            d[name] = x.reshape(B, n_time, H, W).astype(np.float32)
        out.append(d)
    gen, target = out
    gen["a"][:, :, PRESCRIBED[0], PRESCRIBED[1]] = target["a"][:, :, PRESCRIBED[0], PRESCRIBED[1]]
    gen["b"][NAN_AT[0], :NAN_UNTIL, NAN_AT[1], NAN_AT[2]] = np.nan
    target["c"][:] = np.nan
    gen, target = ({n: torch.from_numpy(v) for n, v in d.items()} for d in (gen, target))
    bounds = [n_ic_steps] + [n_ic_steps + c for c in cuts] + [n_time]
    cut = lambda d, a, b: {n: v[:, a:b] for n, v in d.items()}          # noqa: E731
    return {"info": info(), "gen": gen, "target": target, "n_ic_steps": n_ic_steps, "n_time": n_time,
            "ic": (cut(gen, 0, n_ic_steps), cut(target, 0, n_ic_steps)),
            "windows": [(cut(gen, a, b), cut(target, a, b), a) for a, b in zip(bounds[:-1], bounds[1:])]}


def checksum(c):
    """a few exact numbers of the record a golden file can pin: the fp64 sum of the finite values of every field"""
    return {f"{side}/{n}": float(torch.nan_to_num(c[side][n].double()).sum()) for side in ("gen", "target") for n in NAMES}
