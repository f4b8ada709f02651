"""The longitude DFT stage (ace_amd/csrc/fft.hip and the matrix-form kernels of kernels.hip, C ABI `ace_dft_stage`) stated in numpy: the
cases tests/test_gpu_dft_stage.py holds the four kernels to, their seeded inputs and the fp64 truth.  tests/test_dft_ref_cpu.py holds
this file itself.

    forward   X[m] = 2 pi * rfft(in_scale * x + in_shift, norm="forward")[m],  m < Mm, laid out X[m][lat][b][re | im][c]
    inverse   y = irfft(T, n=W, norm="forward") + bias, T = the spectrum with the entries from min(Mm, mcut[lat]) on zeroed, the
              imaginary parts of m = 0 and - for even W, when stored - of m = W / 2 zeroed          (fme/fft.py:78-96)

With the planes input the truth is taken from the values the planes REPRESENT, (hi + lo) / scale, not from the field they were made
from (`planes_from`: exactly what a producer kernel does).

Two norms.  Whole tensor: max|err| / max|ref| over every compared entry, on every case.  Per wavenumber (forward only): the worst m of
max|err| over that m / max|ref| over that m - the whole-tensor norm alone lets a wrong high wavenumber hide behind the DC.  It applies to
CENTRED cases only (white noise, |in_shift| <= 0.05), and not to the matrix form at W >= 360: a plain fp32 matrix product of that
length is past OP_TOL / 2 per wavenumber by itself (1.14e-6 with a BLAS product at W = 360; 9.7e-7 summed in order at W = 256)."""

import dataclasses
import functools
import zlib

import numpy as np

OP_TOL = 2e-6   # the operator bar of tests/test_gpu_parity.py
FFT_WIDTHS = (16, 24, 48, 360, 720, 1440)
N1 = {16: 4, 24: 6, 48: 8, 360: 20, 720: 30, 1440: 40}      # W = N1 * N2 (fft.hip: launch_fwd / launch_inv)
N2 = {16: 4, 24: 4, 48: 6, 360: 18, 720: 24, 1440: 36}
ROWS = ({16: 16, 24: 16, 48: 16, 360: 16, 720: 8, 1440: 8},  # channel rows per workgroup, forward
        {16: 16, 24: 16, 48: 16, 360: 32, 720: 8, 1440: 8})  # ... inverse
NYQ_POISON = 7e3   # what the inverse cases hold in the imaginary parts of m = 0 and of a stored m = W / 2


@dataclasses.dataclass(frozen=True)
class Case:
    sweep: str
    inverse: bool
    engine: int            # 0 matrix form, 1 two-level FFT form
    H: int
    W: int
    Mm: int
    bt: int
    c: int
    opts: tuple = ()       # forward: affine, absmax, planes, mcut, rider;  inverse: bias, absmax, mcut
    mcut: str = "edges"    # with "mcut": per-latitude cutoffs at the kernels' edges, or "random"
    shift: str = "small"   # with "affine": |in_shift| <= 0.05 (centred), or "large" (N(0, 1) * 3: whole-tensor norm only)
    mis_grid: bool = False   # x (forward) / y (inverse) starts 4 bytes off a 16-byte boundary
    mis_spec: bool = False   # spec_out (forward) / spec (inverse) does
    ride: tuple = ()       # with "rider": (O, I, order) of the weight-packing job

    @property
    def id(self):
        o = "+".join(self.opts) if self.opts else "plain"
        s = f"{self.sweep}-{'inv' if self.inverse else 'fwd'}{self.engine}-H{self.H}-W{self.W}-Mm{self.Mm}-bt{self.bt}-c{self.c}-{o}"
        if "mcut" in self.opts and self.mcut != "edges":
            s += f"-{self.mcut}"
        if self.shift != "small":
            s += f"-{self.shift}shift"
        if self.ride:
            s += "-ride%dx%do%d" % self.ride
        return s + ("-misgrid" if self.mis_grid else "") + ("-misspec" if self.mis_spec else "")

    @property
    def per_wavenumber(self):
        """does the per-wavenumber norm apply (centred forward cases; not the matrix form at W >= 360)"""
        return not self.inverse and self.shift == "small" and not (self.engine == 0 and self.W >= 360)


def rows(case):
    return ROWS[1 if case.inverse else 0][case.W] if case.engine == 1 else 0


def takes(case):
    """does the named engine take the case (ace_dft_stage returns ACE_ERR_INVALID otherwise)"""
    if case.engine == 1:
        return case.W in FFT_WIDTHS and not case.mis_grid and ("planes" not in case.opts or case.c % 8 == 0)
    return not ({"planes", "mcut", "rider"} & set(case.opts))


def rider_blocks(case):
    return (case.ride[0] // 32) * (case.ride[1] // 16) if case.ride else 0


def rides(case):
    """a rider job rides only where the workgroup has at least four waves (W = 360, 1440)"""
    return bool(case.ride) and case.engine == 1 and ROWS[0][case.W] * N2[case.W] >= 256


def expected_route(case):
    """(form, rows, units, rode) the launch must report: form 0 matrix with 4-byte loads, 1 matrix with 16-byte loads, 2 FFT; the
    operands of the tests are 16-byte aligned unless the case says otherwise"""
    if case.engine == 1:
        R = rows(case)
        gx = -(-case.c // R)
        extra = -(-rider_blocks(case) // gx) if rides(case) else 0
        return (2, R, gx * (case.H + extra), int(rides(case)))
    cols = case.H * case.bt * case.c
    if case.inverse:
        return (1 if (not case.mis_spec and case.c % 4 == 0) else 0, 0, -(-cols // 128) * -(-(case.W // 2 + 1) // 64), 0)
    return (1 if (not case.mis_grid and case.W % 4 == 0 and case.W >= 8) else 0, 0, -(-case.Mm // 64) * -(-cols // 128), 0)


# --------------------------------------------------------------------------------------------- the case lists
def _mm_list(W):
    """every wavenumber kept, the Nyquist entry dropped (and one more), across the first wavenumber block (N1) and across the
    self-conjugate column (N1 / 2), and the DC alone"""
    n1 = N1[W]
    out = []
    for mm in (W // 2 + 1, W // 2, W // 2 - 1, n1 + 1, n1, n1 // 2 + 1, n1 // 2, 1):
        if 1 <= mm <= W // 2 + 1 and mm not in out:
            out.append(mm)
    return out


def _both(sweep, inverse, engine, H, W, Mm, c, bt_all=3, **kw):
    """a shape once bare at batch 1 and once with every option it takes at batch 3 (the per-sample strides are used)"""
    if inverse:
        allo = ("bias", "absmax") + (("mcut",) if engine == 1 else ())
    else:
        allo = ("affine", "absmax") + (("mcut",) if engine == 1 else ())
    return [Case(sweep, inverse, engine, H, W, Mm, 1, c, **kw),
            Case(sweep, inverse, engine, H, W, Mm, bt_all, c, opts=allo, mcut="random", **kw)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for inv in (False, True):
        # ---------------- engine 1, the two-level FFT form
        for W in FFT_WIDTHS:
            R = ROWS[1 if inv else 0][W]
            full = W // 2 + 1
            # channels: one row, a ragged block, a whole block, a block and one row, two blocks and three rows; H = 5: launch order
            for c in (1, R - 1, R, R + 1, 2 * R + 3):
                out += _both("chan", inv, 1, 5, W, full, c)
            # units: H = 8 makes gx * H a multiple of 8 (XCD-contiguous where the kernel has that branch), H = 7 with gx = 2 does not
            for H in (8, 7):
                out += _both("unit", inv, 1, H, W, full, R + 1)
            out += _both("unit", inv, 1, 8, W, full, 1)
            for Mm in _mm_list(W):
                if Mm != full:
                    out += _both("mm", inv, 1, 5, W, Mm, R + 1)
            # the polar cut at every edge of the register algebra, all in one call (H = 10 latitudes); FULLM and truncated kernels
            for Mm in (full, W // 2 - 1):
                out.append(Case("cut", inv, 1, 10, W, Mm, 1, R + 1, opts=("mcut",)))
            if W in (360, 1440):
                out.append(Case("cut", inv, 1, 10, W, full, 2, R + 1, opts=("mcut",), mcut="random"))
            # options, each alone
            for o in (("bias",), ("absmax",)) if inv else (("affine",), ("absmax",)):
                out.append(Case("opt", inv, 1, 5, W, full, 3, R + 1, opts=o))
                out.append(Case("opt", inv, 1, 5, W, W // 2 - 1, 3, R + 1, opts=o))
            if not inv:
                for c in (8, 24, 40):      # planes: a ragged first block, one and a half, two and a half (R = 16); whole blocks (R = 8)
                    out.append(Case("planes", inv, 1, 3, W, full, 2, c, opts=("planes",)))
                    out.append(Case("planes", inv, 1, 3, W, W // 2 - 1, 2, c, opts=("planes", "affine")))
                out.append(Case("planes", inv, 1, 8, W, full, 1, 24, opts=("planes", "absmax")))
        if not inv:
            out.append(Case("shift", inv, 1, 5, 360, 181, 3, 17, opts=("affine",), shift="large"))
            out.append(Case("shift", inv, 1, 5, 48, 25, 3, 17, opts=("affine",), shift="large"))
            # riders: launch-order branch (gx = 3, two rider blocks, one idle), XCD branch (gx = 8, four rider blocks, four idle),
            # one at W = 1440 (gx = 8, XCD branch), and W = 48, whose workgroup is too small to carry them
            out.append(Case("ride", inv, 1, 8, 360, 181, 1, 40, opts=("rider",), ride=(32, 32, 0)))
            out.append(Case("ride", inv, 1, 8, 360, 181, 1, 128, opts=("rider",), ride=(64, 32, 1)))
            out.append(Case("ride", inv, 1, 8, 360, 179, 2, 40, opts=("rider", "affine", "absmax", "mcut"), mcut="random", ride=(32, 32, 1)))
            out.append(Case("ride", inv, 1, 4, 1440, 721, 1, 64, opts=("rider",), ride=(64, 32, 0)))
            out.append(Case("ride", inv, 1, 8, 48, 25, 1, 40, opts=("rider",), ride=(32, 32, 0)))
        # ---------------- engine 0, the matrix form
        for W in (4, 6, 12, 128, 18, 90, 27, 256):     # W < 8; 16-byte loads of x; W % 4 != 0; odd; two m-tiles of 64 and a ragged third
            for c in (4, 5):
                out += _both("width", inv, 0, 5, W, W // 2 + 1, c)
        out += _both("w360", inv, 0, 5, 360, 181, 4)   # forced: three m-tiles forward, three w-tiles inverse
        out += _both("w360", inv, 0, 5, 360, 181, 5)
        # columns (H bt c) below, at and just above the 128 of a tile, with c % 4 == 0 and != 0
        for H, c in ((4, 28), (4, 32), (4, 36), (4, 31), (4, 33), (127, 1), (128, 1), (129, 1)):
            out.append(Case("cols", inv, 0, H, 24, 13, 1, c))
        out.append(Case("cols", inv, 0, 4, 24, 13, 3, 11, opts=("bias", "absmax") if inv else ("affine", "absmax")))
        for W, Mm in ((128, 64), (128, 65), (128, 1), (256, 64), (256, 65), (256, 1), (12, 1), (27, 13)):
            out += _both("mm", inv, 0, 5, W, Mm, 4)
        # the grid side off a 16-byte boundary: 4-byte loads of x (at W = 16 this is how a width with an FFT form reaches form 0; the
        # inverse form at W = 16 for a misaligned y); the spectral side off a 16-byte boundary: 4-byte stores / loads
        for W in (128, 16):
            out += _both("align", inv, 0, 5, W, W // 2 + 1, 4, mis_grid=True)
            out += _both("align", inv, 0, 5, W, W // 2 + 1, 4, mis_spec=True)
        out += _both("align", inv, 0, 5, 16, 9, 4)     # engine 0 named at a width with an FFT form, aligned: still the matrix form
        for o in (("bias",), ("absmax",)) if inv else (("affine",), ("absmax",)):
            out.append(Case("opt", inv, 0, 5, 128, 65, 3, 5, opts=o))
            out.append(Case("opt", inv, 0, 5, 128, 65, 3, 4, opts=o))
        if not inv:
            out.append(Case("shift", inv, 0, 5, 128, 65, 3, 5, opts=("affine",), shift="large"))
    assert len({c.id for c in out}) == len(out)
    assert all(takes(c) for c in out)
    return tuple(out)


# what an engine refuses (ACE_ERR_INVALID): (case, why); "scale_only" and "null" are built by the GPU test from the first case
REFUSALS = (
    Case("refuse", False, 1, 5, 18, 10, 1, 4),                          # no FFT form at W = 18
    Case("refuse", True, 1, 5, 18, 10, 1, 4),
    Case("refuse", False, 1, 5, 360, 181, 1, 4, mis_grid=True),         # a misaligned x
    Case("refuse", True, 1, 5, 360, 181, 1, 4, mis_grid=True),          # a misaligned y
    Case("refuse", False, 0, 3, 48, 25, 1, 8, opts=("planes",)),        # the matrix form takes no planes
    Case("refuse", False, 0, 5, 48, 25, 1, 4, opts=("mcut",)),          # ... and does not look at mcut
    Case("refuse", True, 0, 5, 48, 25, 1, 4, opts=("mcut",)),
    Case("refuse", False, 1, 3, 48, 25, 1, 12, opts=("planes",)),       # planes with c % 8 != 0
)


# --------------------------------------------------------------------------------------------- inputs
def mcut_values(case):
    """per-latitude cutoffs: every edge of the kernels' algebra - nothing stored, the DC alone, around the self-conjugate column,
    around the first wavenumber block, around Mm - or seeded uniform in [0, Mm + 5]"""
    if "mcut" not in case.opts:
        return None
    if case.mcut == "random":
        rng = np.random.default_rng(zlib.crc32(("mcut" + case.id).encode()))
        return rng.integers(0, case.Mm + 6, size=case.H).astype(np.int32)
    n1 = N1.get(case.W, 4)
    edges = [0, 1, n1 // 2, n1 // 2 + 1, n1 - 1, n1, n1 + 1, case.Mm - 1, case.Mm, case.Mm + 5]
    return np.array([max(0, edges[k % len(edges)]) for k in range(case.H)], dtype=np.int32)


def stored(case):
    """(Mm, H) bool: the entries the forward transform stores / the inverse one reads"""
    mc = mcut_values(case)
    lim = np.full(case.H, case.Mm) if mc is None else np.minimum(case.Mm, mc)
    return np.arange(case.Mm)[:, None] < lim[None, :]


def pow2_exponent_for(mx):
    """strip_common.h: the exponent e with max|x| 2^e in [2^11, 2^12)"""
    mx = np.float32(mx)
    e = 0
    if mx > 0 and mx < np.float32(3.0e38):
        e = 12 - int(np.frexp(mx)[1])
    return max(-100, min(100, e))


def planes_from(x):
    """x (bt, c, H, W) fp32, c % 8 == 0 -> (hi, lo, slot, values): the P-format fp16 planes [bt][c / 8][H W][8] exactly as a producer
    writes them (scale 2^e from the bound max|x| it publishes in word 0 of its 64-word slot; hi = fp16(x scale), lo = fp16(x scale -
    hi), both in fp32 arithmetic), and the fp64 values (hi + lo) / scale they represent, in x's layout"""
    bt, c, H, W = x.shape
    bound = np.float32(np.abs(x).max())
    scale = np.float32(2.0) ** pow2_exponent_for(bound)
    xs = x.astype(np.float32) * scale
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    values = (hi.astype(np.float64) + lo.astype(np.float64)) / np.float64(scale)
    slot = np.zeros(64, dtype=np.uint32)
    slot[0] = bound.view(np.uint32)

    def to_planes(a):      # (a channel count that is no multiple of 8 - the refusal case - is padded with zero channels)
        a = np.concatenate([a, np.zeros((bt, -c % 8, H, W), dtype=a.dtype)], axis=1)
        return np.ascontiguousarray(a.reshape(bt, -(-c // 8), 8, H * W).transpose(0, 1, 3, 2))
    return to_planes(hi), to_planes(lo), slot, values


def pack_frag_ref(w, order, scale):
    """pack_frag.h for one sample, a static scale, no fold: weight (O, I) -> (O / 32)(I / 16) blocks of 512 hi | 512 lo halves; block
    (T, J) at T (I / 16) + J (order 0) or J (O / 32) + T (order 1); element t = lane * 8 + e, lane = i + 32 g holds row 32 T + i,
    column 16 J + 8 g + e"""
    O, I = w.shape
    nT, nJ = O // 32, I // 16
    x = np.clip(w.astype(np.float32) * np.float32(scale), -65504.0, 65504.0).astype(np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    out = np.zeros((nT * nJ, 2, 512), dtype=np.float16)
    for T in range(nT):
        for J in range(nJ):
            b = T * nJ + J if order == 0 else J * nT + T
            for src, half in ((hi, 0), (lo, 1)):
                blk = src[32 * T:32 * T + 32, 16 * J:16 * J + 16].reshape(32, 2, 8)      # (i, g, e)
                out[b, half] = blk.transpose(1, 0, 2).reshape(512)                         # lane = i + 32 g
    return out.reshape(-1)


@functools.lru_cache(maxsize=4)
def inputs(case):
    """the case's operands, seeded by the case.  Forward: x ~ N(0, 1) white noise (with "planes": the planes made from it, and x is
    the values they represent, fp64), in_scale uniform in [0.5, 1.5], in_shift uniform in [-0.05, 0.05] ("large": 3 N(0, 1)).
    Inverse: spec ~ N(0, 1) in every entry (the GPU test overwrites the entries the kernels must not read), bias ~ N(0, 1)."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    d = {"mcut": mcut_values(case)}
    bt, c, H, W, Mm = case.bt, case.c, case.H, case.W, case.Mm
    if case.inverse:
        d["spec"] = rng.standard_normal((Mm, H, bt, 2, c)).astype(np.float32)
        d["bias"] = rng.standard_normal(c).astype(np.float32) if "bias" in case.opts else None
        return d
    x = rng.standard_normal((bt, c, H, W)).astype(np.float32)
    if "planes" in case.opts:
        d["xhi"], d["xlo"], d["xslot"], d["x"] = planes_from(x)
    else:
        d["x"] = x
    if "affine" in case.opts:
        d["in_scale"] = (0.5 + rng.random((bt, c))).astype(np.float32)
        d["in_shift"] = ((3.0 * rng.standard_normal((bt, c))) if case.shift == "large" else (0.1 * rng.random((bt, c)) - 0.05)).astype(np.float32)
    else:
        d["in_scale"] = d["in_shift"] = None
    if case.ride:
        O, I, _ = case.ride
        d["ride_weight"] = (rng.standard_normal((O, I)) / I ** 0.5).astype(np.float32)
        d["ride_scale"] = 2.0 ** 9
    return d


# --------------------------------------------------------------------------------------------- the truth and the plain fp32 forms
def to_spec_layout(F):
    """complex (bt, c, H, Mm) -> real X[m][lat][b][re | im][c]"""
    return np.ascontiguousarray(np.stack([F.real, F.imag], axis=0).transpose(4, 3, 1, 0, 2))


def from_spec_layout(S):
    """real X[m][lat][b][re | im][c] -> complex (bt, c, H, Mm)"""
    S = S.transpose(2, 4, 1, 0, 3)     # (b, c, lat, m, ri)
    return S[..., 0] + 1j * S[..., 1]


def inverse_spectrum(case, spec, dtype):
    """T of the inverse contract, complex (bt, c, H, W / 2 + 1): cut, Mm and the two real entries applied"""
    T = from_spec_layout(spec.astype(dtype)) * stored(case).T[None, None, :, :]
    T[..., 0] = T[..., 0].real
    if case.W % 2 == 0 and case.Mm == case.W // 2 + 1:
        T[..., -1] = T[..., -1].real
    full = np.zeros(T.shape[:-1] + (case.W // 2 + 1,), dtype=T.dtype)
    full[..., :case.Mm] = T
    return full


@functools.lru_cache(maxsize=4)
def truth(case):
    """the fp64 result of the case, computed once and only read afterwards"""
    return truth_of(case, inputs(case))


def truth_of(case, d):
    """the fp64 result for the operands d: forward (Mm, H, bt, 2, c) - every m < Mm, whatever mcut stores of it; inverse (bt, c, H, W)"""
    if case.inverse:
        y = np.fft.irfft(inverse_spectrum(case, d["spec"], np.float64), n=case.W, axis=-1, norm="forward")
        return y + d["bias"].astype(np.float64)[None, :, None, None] if d["bias"] is not None else y
    v = d["x"].astype(np.float64)
    if d["in_scale"] is not None:
        v = v * d["in_scale"].astype(np.float64)[:, :, None, None] + d["in_shift"].astype(np.float64)[:, :, None, None]
    return to_spec_layout(2.0 * np.pi * np.fft.rfft(v, axis=-1, norm="forward")[..., :case.Mm])


MATMUL_BLOCK = 32


def matmul_f32(a, b):
    """a (..., K) @ b (K, N) in fp32 with elementwise operations only - products rounded to fp32, summed in order within blocks of 32
    terms, the block sums summed in order - so that the figure is the same on every machine (a BLAS picks its blocking by processor
    and thread count)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    total = np.zeros(a.shape[:-1] + (b.shape[1],), dtype=np.float32)
    for k0 in range(0, a.shape[-1], MATMUL_BLOCK):
        part = np.zeros_like(total)
        for k in range(k0, min(k0 + MATMUL_BLOCK, a.shape[-1])):
            part += a[..., k:k + 1] * b[k]
        total += part
    return total


def plain_fp32(case):
    """the case evaluated in plain fp32, in the form of its kernel family: torch.fft in float32 for the FFT form, an fp32 matrix product
    with fp32 tables (tables.cpp: computed in fp64, rounded once) for the matrix form"""
    import torch
    d = inputs(case)
    W, Mm = case.W, case.Mm
    ang = 2.0 * np.pi * ((np.arange(Mm)[:, None] * np.arange(W)[None, :]) % W) / W
    if case.inverse:
        if case.engine == 1:
            T = torch.from_numpy(inverse_spectrum(case, d["spec"], np.float32).astype(np.complex64))
            y = torch.fft.irfft(T, n=W, dim=-1, norm="forward")
        else:
            g = np.where((np.arange(Mm) == 0) | (2 * np.arange(Mm) == W), 1.0, 2.0)[:, None]
            sn = np.sin(ang)
            sn[0] = 0.0
            if W % 2 == 0 and Mm == W // 2 + 1:
                sn[-1] = 0.0
            gc, gs = torch.from_numpy((g * np.cos(ang)).astype(np.float32)), torch.from_numpy((-g * sn).astype(np.float32))
            S = torch.from_numpy(d["spec"]).permute(2, 4, 1, 3, 0)     # (b, c, lat, ri, m)
            y = torch.from_numpy(matmul_f32(S[..., 0, :].numpy(), gc.numpy()) + matmul_f32(S[..., 1, :].numpy(), gs.numpy()))
        if d["bias"] is not None:
            y = y + torch.from_numpy(d["bias"])[None, :, None, None]
        assert y.dtype == torch.float32
        return y.numpy()
    v = torch.from_numpy(d["x"].astype(np.float32))     # (the planes' values are 22-bit: exact in fp32)
    if d["in_scale"] is not None:
        v = v * torch.from_numpy(d["in_scale"])[:, :, None, None] + torch.from_numpy(d["in_shift"])[:, :, None, None]
    if case.engine == 1:
        F = (torch.fft.rfft(v, dim=-1, norm="forward")[..., :Mm] * np.float32(2.0 * np.pi)).numpy()
    else:
        s = 2.0 * np.pi / W
        fc, fs = torch.from_numpy((s * np.cos(ang)).astype(np.float32)), torch.from_numpy((-s * np.sin(ang)).astype(np.float32))
        F = matmul_f32(v.numpy(), fc.numpy().T) + 1j * matmul_f32(v.numpy(), fs.numpy().T)
    assert F.dtype == np.complex64
    return to_spec_layout(F)


# --------------------------------------------------------------------------------------------- the norms
def whole_err(got, ref, mask=None):
    """max|err| / max|ref| over the compared entries (mask: (Mm, H) bool of a forward case, None = everything)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if mask is not None:
        got, ref = got[mask], ref[mask]
    if ref.size == 0:
        return 0.0
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def per_wavenumber_err(got, ref, mask=None):
    """forward results (Mm, H, bt, 2, c): the worst m of max|err| over that m / max|ref| over that m, over the compared latitudes;
    returns (error, m)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    worst, at = 0.0, -1
    for m in range(ref.shape[0]):
        g, r = (got[m], ref[m]) if mask is None else (got[m][mask[m]], ref[m][mask[m]])
        if r.size == 0:
            continue
        e = float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-300))
        if e > worst:
            worst, at = e, m
    return worst, at
