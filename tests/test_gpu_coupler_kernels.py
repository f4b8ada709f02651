"""ace_couple_ocean_to_atmosphere and ace_couple_atmosphere_to_ocean (csrc/coupler.hip) through the C ABI, at every shape and
layout their grid and their vector path branch on: a plane below a wave (5 x 7), hw % 4 != 0 (33 x 35), vector-eligible planes
(32 x 36), and planes past the launch's cap of 64 workgroups of 1024 pixels per (job, sample), hw > 65536, where the kernels
grid-stride: 257 x 257 on the scalar path and 264 x 250 on the 16-byte one.  Layouts of the vector-eligible shapes: a base one float
off, a sample stride = 1 (mod 4) that sends sample 0 down the 16-byte path and samples 1 and 2 down the scalar one in the same
launch, a mask plane one float off.

The reference is the reference's formulas in torch fp32 ops ON THE CPU (fme/coupled/stepper.py:1020-1101, fme/core/ocean_data.py:
194-218, fme/core/prescriber.py:54-117), not another kernel of this project.  Every buffer is compared whole - the gaps between
the samples and time levels of a strided field and the guard floats around it too - so a source comes back bitwise and nothing is
written outside a plane."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
GUARD = -777.0
SMALL = [(5, 7), (33, 35), (32, 36)]
LARGE = [(257, 257), (264, 250)]
SPECIALS = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000], dtype=np.uint32).view(np.int32)
MASK_VALUES = torch.tensor([0.0, -0.0, 0.5, 1.0, 1.0, 1.0, 2.0, float("nan")])
CARRIED, FROM_SIF, FROM_OCEAN_SIF = 0, 1, 2


def _layouts(hw):
    if (hw[0] * hw[1]) % 4:
        return [(hw, "window")]
    return [(hw, lay) for lay in ["window", "base_off", "stride_1mod4", "mask_off"]]


def _id(v):
    return "%dx%d-%s" % (v[0][0], v[0][1], v[1])


CASES = [c for hw in SMALL + LARGE for c in _layouts(hw)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _lib():
    from ace_amd import _lib as L
    return L.lib(), L.current_stream()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_numbers(got, want):
    """bitwise where ``want`` is a number, NaN where it is NaN"""
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(_bits(got)[~nan], _bits(want)[~nan])


def _special(v, g, specials=SPECIALS):
    """every special value in each sample of (B, T, HW) draws, one of them in the last element"""
    bits = v.view(torch.int32)
    n = v.shape[-1]
    for b in range(v.shape[0]):
        for t in range(v.shape[1]):
            pos = torch.randperm(n - 1, generator=g)[:min(n - 1, 2 * len(specials))]
            bits[b, t, pos] = torch.from_numpy(np.resize(specials, len(pos)))
            bits[b, t, n - 1] = int(specials[(b + t + 1) % len(specials)])
    return v


class Field:
    """(B, T, HW) values inside a flat buffer of guard floats: level t of sample b at offset + b * stride + t * step.  ``host`` is what
    the buffer held at the start (and, edited through ``expect``, what it should hold at the end), ``device`` its copy for the
    kernel."""

    def __init__(self, dev, values, HW, T, layout, off_base=False):
        self.HW, self.T = HW, T
        self.step = HW                                       # the levels of a sample are contiguous, as in a window
        self.stride = T * HW + (1 if layout == "stride_1mod4" else 4)
        self.offset = 4 + (1 if off_base else 0)
        self.host = torch.full((self.offset + (B - 1) * self.stride + T * HW + 4,), GUARD)
        if values is not None:
            self.expect().copy_(values)
        self.device = self.host.to(dev)
        assert self.device.data_ptr() % 16 == 0
        self.ptr = self.device.data_ptr() + 4 * self.offset

    def expect(self):
        return self.host.as_strided((B, self.T, self.HW), (self.stride, self.step, 1), self.offset)

    def level_ptr(self, t):
        return self.ptr + 4 * t * self.step

    def check(self, what, numbers_only=False):
        got = self.device.cpu()
        assert (_same_numbers if numbers_only else lambda a, b: torch.equal(_bits(a), _bits(b)))(got, self.host), what


def _i64(dev, values):
    return torch.tensor(values, dtype=torch.int64, device=dev)


def _masks(g, dev, HW, off):
    """two fp32 mask planes; ``off``: the table starts one float off"""
    masks = MASK_VALUES[torch.randint(0, len(MASK_VALUES), (2, HW), generator=g)].contiguous()
    start = 1 if off else 0
    buf = torch.full((2 * HW + 8,), GUARD)
    buf[start:start + 2 * HW] = masks.reshape(-1)
    d = buf.to(dev)
    assert d.data_ptr() % 16 == 0
    return masks, d, [d.data_ptr() + 4 * (start + k * HW) for k in range(2)]


def _keep(mask, v):
    return v if mask is None else v.where(mask.expand(v.shape) != 0, 0)          # stepper.py:1053-1058


def _reference_o2a(mode, interpolate, sst, ic, frac, sif, passed, masks):
    """the reference's formulas in its own torch ops, on the CPU.  ``masks``: slot -> mask plane or None.  Returns slot -> tensor."""
    out = {0: _keep(masks.get(0), sst)}
    if mode == CARRIED:
        out[2] = _keep(masks.get(2), frac)
    else:
        sea_ice = torch.nan_to_num(sif)                                          # stepper.py:178
        if mode == FROM_OCEAN_SIF:
            sea_ice = sea_ice * (1 - frac)                                       # ocean_data.py:201
        ocean_fraction = torch.clip(1 - frac - sea_ice, min=0)                   # ocean_data.py:218, stepper.py:1050
        out[2] = _keep(masks.get(2), ocean_fraction)
        out[3] = _keep(masks.get(3), sea_ice)
        out[4] = _keep(masks.get(4), sif)
    for k, p in enumerate(passed):
        slot = (3 if mode == CARRIED else 5) + k
        out[slot] = _keep(masks.get(slot), p)
    m, target = out[2][:, :1], out[0]
    if interpolate:                                                              # prescriber.py:95-101
        out[1] = m * target + (1 - m) * ic
    else:                                                                        # spatial_masking.py:11-30
        out[1] = torch.where(torch.round(m).to(int) == 1, target, ic)
    return out


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_ocean_to_atmosphere(dev, case):
    """every mode and both prescribers per shape and layout: bitwise on numbers, NaN on NaN"""
    (H, W), layout = case
    HW = H * W
    g = torch.Generator().manual_seed(HW)
    off = layout == "base_off"
    mask_values, mask_dev, mask_ptrs = _masks(g, dev, HW, layout == "mask_off")
    n_inner = {"window": 2, "base_off": 1, "stride_1mod4": 5, "mask_off": 2}[layout] if HW < 65536 else 1
    T = n_inner + 1
    npass = 3
    L, stream = _lib()
    runs = [(CARRIED, 0, True), (CARRIED, 1, False), (FROM_SIF, 0, True), (FROM_SIF, 1, False), (FROM_OCEAN_SIF, 1, True),
            (FROM_OCEAN_SIF, 0, False)]
    for mode, interpolate, optional in runs:      # optional: the destination the ABI allows to be NULL is there
        draw = lambda t, scale=3.0, shift=1.0: torch.randn(B, t, HW, generator=g) * scale + shift
        sst = Field(dev, _special(draw(1, 3.0, 285.0), g), HW, 1, layout, off)
        ic = Field(dev, draw(1, 5.0, 280.0), HW, 1, layout, off)
        sif = Field(dev, _special(torch.rand(B, 1, HW, generator=g) * 1.2 - 0.1, g), HW, 1, layout, off)
        frac_values = torch.rand(B, T, HW, generator=g) * (1.2 if mode == CARRIED else 1.0) - (0.1 if mode == CARRIED else 0.0)
        for value in (0.0, 0.5, 1.0, 1.5, 2.5) if mode == CARRIED else (0.0, 1.0):          # finite: round(NaN).to(int) is unspecified
            frac_values[torch.rand(B, T, HW, generator=g) < 0.1] = value
        frac = Field(dev, frac_values, HW, T, layout, off)
        passed = [Field(dev, _special(draw(1), g), HW, 1, layout, off) for _ in range(npass)]
        first = 3 if mode == CARRIED else 5
        # which slots carry a mask: the surface temperature, the ocean fraction, the sea ice, one pass-through field
        masked = {0: 0, 2: 1, 3: 0, first + 1: 1}
        if mode == CARRIED and not optional:
            del masked[2]                          # nothing to mask: no destination
        if mode == FROM_SIF:
            del masked[0]
        masks = {slot: mask_values[k] for slot, k in masked.items()}
        want = _reference_o2a(mode, interpolate, sst.expect(), ic.expect(), frac.expect(),
                              sif.expect(), [p.expect() for p in passed], masks)
        si_levels = T if mode == FROM_OCEAN_SIF else 1
        if mode == FROM_SIF:
            want[3] = want[3][:, :1]
        srcs = {0: sst, 1: ic, 2: frac}
        dsts = {0: Field(dev, None, HW, 1, layout), 1: Field(dev, None, HW, 1, layout),
                2: Field(dev, None, HW, T, layout) if (mode != CARRIED or optional) else None}
        if mode != CARRIED:
            srcs.update({3: sif, 4: sif})
            dsts.update({3: Field(dev, None, HW, si_levels, layout), 4: Field(dev, None, HW, 1, layout) if optional else None})
        for k, p in enumerate(passed):
            srcs[first + k] = p
            dsts[first + k] = Field(dev, None, HW, 1, layout)
        n = first + npass
        for slot in range(n):
            if dsts[slot] is not None:
                dsts[slot].expect().copy_(want[slot])
        tab = _i64(dev, [srcs[j].ptr for j in range(n)] + [x for j in range(n) for x in (srcs[j].stride, srcs[j].step)]
                   + [0 if dsts[j] is None else dsts[j].ptr for j in range(n)]
                   + [x for j in range(n) for x in ((0, 0) if dsts[j] is None else (dsts[j].stride, dsts[j].step))]
                   + [mask_ptrs[masked[j]] if j in masked else 0 for j in range(n)])
        a = tab.data_ptr()
        rc = L.ace_couple_ocean_to_atmosphere(a, a + 8 * n, a + 24 * n, a + 32 * n, a + 48 * n, npass, mode, interpolate, n_inner, B,
                                              HW, stream)
        assert rc == 0, L.ace_couple_last_error()
        torch.cuda.synchronize()
        what = (mode, interpolate, optional)
        for slot in range(n):
            if dsts[slot] is not None:
                dsts[slot].check(("destination", slot) + what, numbers_only=True)
        for f in (sst, ic, sif, frac, *passed):
            f.check(("source",) + what)
    assert _same_numbers(mask_dev.cpu()[(1 if layout == "mask_off" else 0):][:2 * HW], mask_values.reshape(-1))


def _mean_inputs(g, T, HW):
    """(B, T, HW) below 1e30 in magnitude with NaN, +-inf and +-0 (also +inf and -inf at one pixel: a NaN sum)"""
    v = torch.randn(B, T, HW, generator=g) * 3.0 + 1.0
    v[:, :, : HW // 3] *= 1e20
    bits = v.view(torch.int32)
    for b in range(B):                  # each special value at one time level of a pixel of its own, one of them in the last pixel
        pos = torch.randperm(HW - 3, generator=g)[:len(SPECIALS) - 1] + 2
        for k, p in enumerate([*pos.tolist(), HW - 1]):
            bits[b, int(torch.randint(0, T, (1,), generator=g)), p] = int(SPECIALS[(k + b) % len(SPECIALS)])
    if T > 1:
        v[0, 0, 1], v[0, 1, 1] = float("inf"), float("-inf")
    assert float(v[torch.isfinite(v)].abs().max()) < 1e30
    return v


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_atmosphere_to_ocean(dev, case):
    """The mean against m64, the fp64 mean of the fp32 inputs: |got - m64| <= 2^-23 |m64| + 2^-50 sum_t |x_t| - one fp32 rounding plus
    the fp64 accumulation, derived - the other slot all NaN, NaN and +-inf where the fp64 statement has them.  The reference's own fp32
    ``mean`` of the same inputs (torch on the CPU) is held against m64 at n_inner 2^-24 mean_t |x_t| in the same test: both sit inside
    that bound, which is the relation of the kernel's mean to the reference's.  Measured on an MI355X: the kernel's mean at most 0.500 of
    its bound (the one fp32 rounding), the reference's fp32 mean at most 0.61 of its own."""
    (H, W), layout = case
    HW = H * W
    g = torch.Generator().manual_seed(HW + 7)
    off = layout == "base_off"
    L, stream = _lib()
    combos = [(1, 1), (11, 2), (11, 5), (1, 20), (11, 20)] if HW < 65536 else [(11, 2), (1, 20)]
    for N, n_inner in combos:
        slots = [(j + 1) % 2 for j in range(N)]                 # both slot kinds in one launch (N = 1: [NaN, mean])
        ptrs, strides, fields, values = [], [], [], []
        for j in range(N):
            x = _mean_inputs(g, n_inner, HW)
            values.append(x)
            if j % 2 == 0:                                      # generated steps: separate tensors
                steps = [Field(dev, x[:, t:t + 1], HW, 1, layout, off) for t in range(n_inner)]
                fields += steps
                ptrs += [s.ptr for s in steps]
                strides += [s.stride for s in steps]
            else:                                               # a shared forcing: levels 1 .. n_inner of a record
                record = Field(dev, torch.cat([torch.full((B, 1, HW), 5.0), x], dim=1), HW, n_inner + 1, layout, off)
                fields.append(record)
                ptrs += [record.level_ptr(1 + t) for t in range(n_inner)]
                strides += [record.stride] * n_inner
        windows = [Field(dev, None, HW, 2, layout, off_base=(off and j % 2 == 1)) for j in range(N)]
        tab = _i64(dev, ptrs + strides + [w.ptr for w in windows] + [x for w in windows for x in (w.stride, w.step)])
        slot_dev = torch.tensor(slots, dtype=torch.int32, device=dev)
        a, n = tab.data_ptr(), N * n_inner
        rc = L.ace_couple_atmosphere_to_ocean(a, a + 8 * n, a + 16 * n, a + 16 * n + 8 * N, slot_dev.data_ptr(), N, n_inner, B, HW,
                                              stream)
        assert rc == 0, L.ace_couple_last_error()
        torch.cuda.synchronize()
        for j, (w, x) in enumerate(zip(windows, values)):
            got_buf = w.device.cpu()
            got = got_buf.as_strided((B, 2, HW), (w.stride, w.step, 1), w.offset)
            assert torch.isnan(got[:, 1 - slots[j]]).all(), ("the other slot", N, n_inner, j)
            mean = got[:, slots[j]].double()
            x64 = x.double()
            m64 = x64.sum(dim=1) / n_inner
            finite = torch.isfinite(m64)
            assert torch.equal(torch.isnan(mean), torch.isnan(m64)), (N, n_inner, j)
            assert torch.equal(mean[~finite & ~torch.isnan(m64)], m64[~finite & ~torch.isnan(m64)]), (N, n_inner, j)      # +-inf, signed
            bound = 2.0 ** -23 * m64.abs() + 2.0 ** -50 * x64.abs().sum(dim=1)
            err = (mean - m64).abs()
            worst = float((err[finite] / bound[finite].clamp_min(1e-300)).max())
            print(f"a2o {H}x{W} {layout} N={N} n_inner={n_inner} name {j}: worst |got - m64| / bound = {worst:.3f}")
            assert bool((err[finite] <= bound[finite]).all()), (N, n_inner, j, worst)
            # the reference's fp32 mean of the same inputs
            ref32 = x.mean(dim=1).double()
            ref_bound = n_inner * 2.0 ** -24 * x64.abs().mean(dim=1)
            ok = torch.isfinite(ref32) & finite
            ref_worst = float(((ref32 - m64).abs()[ok] / ref_bound[ok].clamp_min(1e-300)).max())
            print(f"    the reference's fp32 mean: worst |ref - m64| / bound = {ref_worst:.3f}")
            assert bool(((ref32 - m64).abs()[ok] <= ref_bound[ok]).all()), (N, n_inner, j, ref_worst)
            assert bool((err[ok] <= ref_bound[ok]).all()), (N, n_inner, j)
            # nothing outside the two planes of each sample
            expect = w.host.clone()
            expect.as_strided((B, 2, HW), (w.stride, w.step, 1), w.offset).copy_(got)
            assert torch.equal(_bits(got_buf), _bits(expect)), ("guards", N, n_inner, j)
        for f in fields:
            f.check(("source", N, n_inner))
