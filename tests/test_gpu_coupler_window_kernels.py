"""ace_couple_ocean_to_atmosphere_window (csrc/coupler.hip) through the C ABI, with the cases and helpers of
tests/test_gpu_coupler_kernels.py: the same shapes (below a wave, hw % 4 != 0, vector-eligible, past the 65536-pixel grid-stride
trip on the scalar and on the 16-byte path), all three modes, both prescribers, n_inner 1 and 3, B = 3, NULL and present masks,
NULL destinations of slots 2 and 4, that file's special values and mask values.

Every destination but slot 1's is a window of n_inner + 1 level rows inside a flat buffer of guard floats: the base one float off a
16-byte boundary, the step stride hw + 5 (hw + 6 where that is a multiple of 4: larger than hw and not a multiple of 4, so the rows of one window differ in alignment
and, where hw % 4 == 0, one row in four takes the 16-byte path), guard floats between and around the rows.  Every level is held,
bitwise where a number and NaN where NaN, against what the existing ace_couple_ocean_to_atmosphere stores for the same tables into
its own contiguous destinations AND against the reference's formulas in torch on the CPU (``_reference_o2a``); the buffers are
compared whole, so the guards must survive."""
import pytest
import torch

from test_gpu_coupler_kernels import (B, CARRIED, FROM_OCEAN_SIF, FROM_SIF, GUARD, LARGE, SMALL, Field, _i64, _lib, _masks,
                                      _reference_o2a, _same_numbers, _special, dev)  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu

NPASS = 3
RUNS = [(mode, interpolate, n_inner) for mode in (CARRIED, FROM_SIF, FROM_OCEAN_SIF) for interpolate in (0, 1) for n_inner in (1, 3)]


class Window:
    """(B, T, HW) level rows inside a flat buffer of guard floats: level t of sample b at offset + b * stride + t * step."""

    def __init__(self, dev, HW, T, values=None):
        self.HW, self.T = HW, T
        self.step = HW + 5 if (HW + 5) % 4 else HW + 6
        self.stride = T * self.step + 3
        self.offset = 5                                                       # one float off a 16-byte boundary
        assert self.step > HW and self.step % 4 != 0
        self.host = torch.full((self.offset + (B - 1) * self.stride + T * self.step + 4,), GUARD)
        if values is not None:
            self.expect().copy_(values)
        self.device = self.host.to(dev)
        assert self.device.data_ptr() % 16 == 0
        self.ptr = self.device.data_ptr() + 4 * self.offset

    def expect(self):
        return self.host.as_strided((B, self.T, self.HW), (self.stride, self.step, 1), self.offset)

    def check(self, what):
        assert _same_numbers(self.device.cpu(), self.host), what              # the guards are numbers: they must be there, bitwise


def _inputs(g, dev, HW, T, mode, off):
    draw = lambda t, scale=3.0, shift=1.0: torch.randn(B, t, HW, generator=g) * scale + shift
    sst = Field(dev, _special(draw(1, 3.0, 285.0), g), HW, 1, "window", off)
    ic = Field(dev, draw(1, 5.0, 280.0), HW, 1, "window", off)
    sif = Field(dev, _special(torch.rand(B, 1, HW, generator=g) * 1.2 - 0.1, g), HW, 1, "window", off)
    frac = torch.rand(B, T, HW, generator=g) * (1.2 if mode == CARRIED else 1.0) - (0.1 if mode == CARRIED else 0.0)
    for value in (0.0, 0.5, 1.0, 1.5, 2.5) if mode == CARRIED else (0.0, 1.0):              # finite: round(NaN).to(int) is unspecified
        frac[torch.rand(B, T, HW, generator=g) < 0.1] = value
    passed = [Field(dev, _special(draw(1), g), HW, 1, "window", off) for _ in range(NPASS)]
    return sst, ic, sif, frac, passed


def _table(dev, srcs, dsts, masked, mask_ptrs):
    n = len(srcs)
    tab = _i64(dev, [srcs[j].ptr for j in range(n)] + [x for j in range(n) for x in (srcs[j].stride, srcs[j].step)]
               + [0 if dsts[j] is None else dsts[j].ptr for j in range(n)]
               + [x for j in range(n) for x in ((0, 0) if dsts[j] is None else (dsts[j].stride, dsts[j].step))]
               + [mask_ptrs[masked[j]] if j in masked else 0 for j in range(n)])
    a = tab.data_ptr()
    return tab, (a, a + 8 * n, a + 24 * n, a + 32 * n, a + 48 * n)


def _levels(mode, slot, T):
    """time levels of a slot's destination in the existing entry"""
    return T if slot == 2 or (slot == 3 and mode == FROM_OCEAN_SIF) else 1


@pytest.mark.parametrize("hw", SMALL + LARGE, ids=lambda v: "%dx%d" % v)
def test_every_level_is_the_existing_entrys_value(dev, hw):
    H, W = hw
    HW = H * W
    g = torch.Generator().manual_seed(HW + 3)
    mask_values, mask_dev, mask_ptrs = _masks(g, dev, HW, False)
    L, stream = _lib()
    for k, (mode, interpolate, n_inner) in enumerate(RUNS):
        T = n_inner + 1
        optional = bool((interpolate + (n_inner == 3)) % 2)          # each mode runs with and without its NULL-able destination
        sst, ic, sif, frac_values, passed = _inputs(g, dev, HW, T, mode, off=bool(k % 2))
        frac = Field(dev, frac_values, HW, T, "window", bool(k % 2))
        first = 3 if mode == CARRIED else 5
        n = first + NPASS
        masked = {0: 0, 2: 1, 3: 0, first + 1: 1}
        if mode == CARRIED and not optional:
            del masked[2]                                            # nothing to mask: no destination
        if mode == FROM_SIF:
            del masked[0]
        masks = {slot: mask_values[m] for slot, m in masked.items()}
        want = _reference_o2a(mode, interpolate, sst.expect(), ic.expect(), frac.expect(), sif.expect(),
                              [p.expect() for p in passed], masks)
        srcs = {0: sst, 1: ic, 2: frac}
        if mode != CARRIED:
            srcs.update({3: sif, 4: sif})
        srcs.update({first + j: p for j, p in enumerate(passed)})
        absent = {2} if (mode == CARRIED and not optional) else {4} if (mode != CARRIED and not optional) else set()
        # ---- the existing entry on its own contiguous destinations
        old = {j: None if j in absent else Field(dev, None, HW, _levels(mode, j, T), "window") for j in range(n)}
        tab_old, addr = _table(dev, srcs, old, masked, mask_ptrs)
        assert L.ace_couple_ocean_to_atmosphere(*addr, NPASS, mode, interpolate, n_inner, B, HW, stream) == 0, L.ace_couple_last_error()
        # ---- the window entry
        new = {j: None if j in absent else (Field(dev, None, HW, 1, "window") if j == 1 else Window(dev, HW, T)) for j in range(n)}
        tab_new, addr = _table(dev, srcs, new, masked, mask_ptrs)
        rc = L.ace_couple_ocean_to_atmosphere_window(*addr, NPASS, mode, interpolate, n_inner, B, HW, stream)
        assert rc == 0, L.ace_couple_last_error()
        torch.cuda.synchronize()
        what = (mode, interpolate, n_inner, optional)
        for j in range(n):
            if new[j] is None:
                continue
            ref = want[j][:, :1] if (j == 3 and mode == FROM_SIF) else want[j]
            got_old = old[j].device.cpu().as_strided((B, old[j].T, HW), (old[j].stride, old[j].step, 1), old[j].offset)
            assert _same_numbers(got_old, ref.contiguous()), ("the existing entry against the reference", j) + what
            # against the existing entry: the whole buffer, guards included
            new[j].expect().copy_(got_old if got_old.shape[1] == new[j].T else got_old.expand(-1, new[j].T, -1))
            new[j].check(("against the existing entry", j) + what) if isinstance(new[j], Window) else \
                new[j].check(("against the existing entry", j) + what, numbers_only=True)
            # against the torch reference
            got = new[j].device.cpu().as_strided((B, new[j].T, HW), (new[j].stride, new[j].step, 1), new[j].offset)
            assert _same_numbers(got, ref.expand(-1, new[j].T, -1).contiguous()), ("against the reference", j) + what
        for f in (sst, ic, sif, frac, *passed):
            f.check(("source",) + what)                              # every source comes back bitwise
    assert _same_numbers(mask_dev.cpu()[:2 * HW], mask_values.reshape(-1))


@pytest.mark.parametrize("hw", [(32, 36), (33, 35), (264, 250)], ids=lambda v: "%dx%d" % v)
def test_carried_fraction_masked_in_place(dev, hw):
    """carried mode with slot 2's destination its own source: the window holds the masked fraction afterwards, level for level what
    the existing entry stores into a destination of its own, and the prescribed temperature is that of the masked level 0"""
    H, W = hw
    HW = H * W
    g = torch.Generator().manual_seed(HW + 5)
    mask_values, _, mask_ptrs = _masks(g, dev, HW, False)
    L, stream = _lib()
    for interpolate, n_inner in ((1, 3), (0, 1)):
        T = n_inner + 1
        sst, ic, sif, frac_values, passed = _inputs(g, dev, HW, T, CARRIED, off=False)
        n = 3 + NPASS
        masked = {0: 0, 2: 1, 4: 1}
        want = _reference_o2a(CARRIED, interpolate, sst.expect(), ic.expect(), frac_values, sif.expect(),
                              [p.expect() for p in passed], {slot: mask_values[m] for slot, m in masked.items()})
        frac = Field(dev, frac_values, HW, T, "window")
        srcs = {0: sst, 1: ic, 2: frac, **{3 + j: p for j, p in enumerate(passed)}}
        old = {j: Field(dev, None, HW, _levels(CARRIED, j, T), "window") for j in range(n)}
        tab_old, addr = _table(dev, srcs, old, masked, mask_ptrs)
        assert L.ace_couple_ocean_to_atmosphere(*addr, NPASS, CARRIED, interpolate, n_inner, B, HW, stream) == 0
        own = Window(dev, HW, T, frac_values)                        # source and destination
        srcs[2] = own
        new = {j: own if j == 2 else (Field(dev, None, HW, 1, "window") if j == 1 else Window(dev, HW, T)) for j in range(n)}
        tab_new, addr = _table(dev, srcs, new, masked, mask_ptrs)
        rc = L.ace_couple_ocean_to_atmosphere_window(*addr, NPASS, CARRIED, interpolate, n_inner, B, HW, stream)
        assert rc == 0, L.ace_couple_last_error()
        torch.cuda.synchronize()
        for j in range(n):
            got_old = old[j].device.cpu().as_strided((B, old[j].T, HW), (old[j].stride, old[j].step, 1), old[j].offset)
            assert _same_numbers(got_old, want[j].contiguous()), ("the existing entry against the reference", j, interpolate)
            new[j].expect().copy_(got_old if got_old.shape[1] == new[j].T else got_old.expand(-1, new[j].T, -1))
            if isinstance(new[j], Window):
                new[j].check(("in place" if j == 2 else "window", j, interpolate, n_inner))
            else:
                new[j].check(("prescribed", j, interpolate, n_inner), numbers_only=True)
