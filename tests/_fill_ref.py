"""The header contract of ``ace_diag_fill_planes`` (include/ace_sfno.h) in plain numpy fp64, written from the header: the layer plane
of a valid set from its two simulations, the blurred valid plane, and per plane the mean at the interior, the four rings of
neighbour averages, the separable blur and the blend.  Nothing is rounded to fp32 on the way except the blurred valid plane, which
the contract stores as fp32.  tests/test_fill_ref_cpu.py holds this statement to the reference's own SmoothFloodFill
(tests/golden/gen_fill.pt); the GPU kernel tests hold the kernel to this statement."""
import numpy as np

STEPS, INTERIOR = 4, 5
OFFSETS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def taps():
    q = np.arange(-2.0, 3.0)
    g = np.exp(-q * q / 2.0)
    return g / g.sum()


def shifted(x, dy, dx, outside):
    """y[r, c] = x[r + dy, (c + dx) mod W], ``outside`` where row r + dy does not exist"""
    y = np.roll(x, -dx, axis=1)
    out = np.full_like(y, outside)
    H = x.shape[0]
    lo, hi = max(0, -dy), min(H, H - dy)
    out[lo:hi] = y[lo + dy:hi + dy]
    return out


def grow(s):
    out = np.zeros_like(s)
    for dy, dx in OFFSETS:
        out |= shifted(s, dy, dx, False)
    return out


def reach(start):
    """the step (1..4) at which growing ``start`` first covers each pixel; 0 inside ``start``, 5 where four steps do not reach"""
    step = np.where(start, 0, INTERIOR).astype(np.uint8)
    known = start.copy()
    for k in range(1, STEPS + 1):
        g = grow(known)
        step[g & ~known] = k
        known = g
    return step


def layers_a_only(valid):
    """the trap: layers read off simulation A alone"""
    return reach(np.asarray(valid, bool))


def layers(valid):
    valid = np.asarray(valid, bool)
    interior = reach(valid) == INTERIOR                           # simulation A
    lay = reach(valid | interior)                                  # simulation B
    lay[interior] = INTERIOR
    return lay


def blur(x):
    g = taps()
    H = x.shape[-2]
    v = np.zeros_like(x)
    for i, q in enumerate(range(-2, 3)):
        rows = np.clip(np.arange(H) + q, 0, H - 1)
        v = v + g[i] * x[..., rows, :]
    out = np.zeros_like(x)
    for i, q in enumerate(range(-2, 3)):
        out = out + g[i] * np.roll(v, -q, axis=-1)
    return out


def blurred_valid(valid):
    return blur(np.asarray(valid, bool).astype(np.float64)).astype(np.float32)


def fill(plane, valid, lay=None):
    """one (H, W) plane in fp64; values at masked pixels are not read"""
    valid = np.asarray(valid, bool)
    lay = layers(valid) if lay is None else lay
    bv = blurred_valid(valid).astype(np.float64)
    x = np.where(valid, np.asarray(plane, np.float64), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = x[valid].sum() / valid.sum()
        x = np.where(lay == INTERIOR, mean, x)
        for k in range(1, STEPS + 1):
            known = (lay < k) | (lay == INTERIOR)
            total, count = np.zeros_like(x), np.zeros_like(x)
            for dy, dx in OFFSETS:
                kn = shifted(known, dy, dx, False)
                total += np.where(kn, shifted(x, dy, dx, 0.0), 0.0)
                count += kn
            x = np.where(lay == k, total / count, x)
        return x * bv + blur(x) * (1.0 - bv)


def fill_planes(field, valid):
    """every plane of a (..., H, W) field"""
    field = np.asarray(field)
    flat = field.reshape(-1, *field.shape[-2:])
    lay = layers(valid)
    return np.stack([fill(p, valid, lay) for p in flat]).reshape(field.shape)


def scale(field, valid):
    """M of the bars: max |valid value| per plane, shaped to broadcast against the field"""
    field = np.asarray(field, np.float64)
    v = np.abs(field[..., np.asarray(valid, bool)])
    return (v.max(axis=-1) if v.shape[-1] else np.zeros(field.shape[:-2]))[..., None, None]
