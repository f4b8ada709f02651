"""The four longitude DFT kernels - `dft_forward_fft_kernel` / `dft_inverse_fft_kernel` of ace_amd/csrc/fft.hip (the first and the last
kernel of every spectral block) and the matrix forms `dft_forward_kernel` / `dft_inverse_kernel` of kernels.hip - held to fp64 at every
branch they take, directly, through `ace_dft_stage` (include/ace_sfno.h):

    forward   X[m] = 2 pi * rfft(in_scale * x + in_shift, norm="forward")[m], m < min(Mm, mcut[lat]), laid out X[m][lat][b][re | im][c]
    inverse   y = irfft(T, n=W, norm="forward") + bias, T = the spectrum cut at min(Mm, mcut[lat]), Im of m = 0 and of a stored W / 2 zeroed

The cases, their inputs and the fp64 truth are tests/_dft_ref.py's (tests/test_dft_ref_cpu.py holds a plain fp32 evaluation of every case
to OP_TOL / 2 in every norm applied here, which is what makes OP_TOL = 2e-6 fair).  Sweeps, each shape once bare at batch 1 and once with
every option it takes at batch 3:
  engine 1 (FFT form), all six widths, both directions
    chan    c = 1, R - 1, R, R + 1, 2 R + 3 with R the rows per workgroup the route reports; H = 5 (launch-order unit mapping)
    unit    H = 8 (unit count a multiple of 8: XCD-contiguous mapping) and H = 7, asserted through the route's unit count
    mm      Mm = W/2, W/2 - 1, N1 + 1, N1, N1/2 + 1, N1/2, 1 (W/2 + 1 is every other sweep's)
    cut     mcut = 0, 1, N1/2, N1/2 + 1, N1 - 1, N1, N1 + 1, Mm - 1, Mm, Mm + 5 over the ten latitudes of ONE call, at Mm = W/2 + 1
            and W/2 - 1; seeded random at W = 360 and 1440
    opt     affine / bias / out_absmax alone;  planes  c = 8, 24, 40 alone and with the affine;  shift  a large in_shift
    ride    riders in the launch-order branch, in the XCD branch (four of eight rider slots idle), at W = 1440, and at W = 48 where the
            workgroup is too small to carry them
  engine 0 (matrix form)
    width   W = 4, 6 (< 8), 12, 128, 256 (16-byte loads of x), 18, 90 (W % 4 != 0), 27 (odd), with c % 4 == 0 and != 0
    w360    the forced matrix form at W = 360: three m-tiles forward, three w-tiles inverse (whole-tensor norm only)
    cols    H bt c = 112 .. 144 around the 128 columns of a tile;  mm  Mm = 64, 65, 1
    align   x / y and spec_out / spec off a 16-byte boundary (4-byte loads / stores; W = 16 reaches form 0 this way);  opt  as above
Every case (test_stage_vs_fp64)
  * asserts the route it means to check (form, rows per workgroup, workgroups, rode) as the entry reports it;
  * runs under poison.  Forward: x (or the planes) is a view inside a NaN-filled allocation with 64 elements in front and behind,
    spec_out a view inside a sentinel-filled buffer; afterwards every entry with m < min(Mm, mcut[lat]) is finite and compared with the
    truth, and EVERY other element of the buffer - the guards, the entries of the cut, the rows a ragged channel block does not
    have - is bitwise the sentinel.  Inverse: spec holds NaN at every entry from mcut[lat] on and a finite 7e3 in the imaginary
    parts of m = 0 and of the stored Nyquist entry; y is inside a sentinel buffer; afterwards y is finite, compared, the guards untouched;
  * is run twice, bitwise equal;
  * with out_absmax: the maximum over the 64 words equals max |stored value| exactly (forward with mcut: the value the same call
    publishes without mcut, which is that call's max |stored value|); the words around the slot are untouched;
  * with a rider: the DFT output is bitwise that of the same call without the rider, the ridden pack is bitwise the stand-alone
    pack, and both are tests/_dft_ref.py's restatement of the packer.
Errors: whole tensor max|err| / max|ref| on every case; per wavenumber (worst m of max|err| over m / max|ref| over m) on the centred
forward cases (not the matrix form at W >= 360).
test_refusals: what an engine does not take is a ValueError, never the other engine.

test_absmax_is_a_maximum_of_stored_values: a tone just beyond Mm, so that the largest value a truncated transform computes is one
it drops.

MEASURED on an MI355X (worst case of each form over all sweeps, against fp64; next to it the worst plain fp32 CPU evaluation of the
cases that take that form, tests/test_dft_ref_cpu.py; every case is within OP_TOL = 2e-6 in every norm that applies to it):
  forward, FFT form                whole 1.86e-7 at mm W720 Mm360 c9 bt3 affine+absmax+mcut          (CPU fp32 3.24e-7)
                                   per wavenumber 4.79e-7 at chan W1440 Mm721 c1 bt1 plain            (CPU fp32 5.43e-7)
  forward, matrix, 16-byte loads   whole 6.12e-7 at w360 W360 Mm181 c5 bt1 plain                      (CPU fp32 2.59e-7)
                                   per wavenumber 7.65e-7 at width W256 Mm129 c5 bt1 plain            (CPU fp32 3.07e-7)
  forward, matrix, 4-byte loads    whole 2.42e-7 at align W128 Mm65 c4 bt3 affine+absmax, x misaligned (CPU fp32 1.88e-7)
                                   per wavenumber 3.80e-7 at align W128 Mm65 c4 bt1, x misaligned     (CPU fp32 2.64e-7)
  inverse, FFT form                whole 2.23e-7 at opt W1440 Mm719 c9 bt3 absmax                     (CPU fp32 2.22e-7)
  inverse, matrix, 16-byte loads   whole 3.55e-7 at w360 W360 Mm181 c4 bt3 bias+absmax                (CPU fp32 2.23e-7)
  inverse, matrix, 4-byte loads    whole 4.09e-7 at w360 W360 Mm181 c5 bt3 bias+absmax                (CPU fp32 1.85e-7)
(The CPU matrix evaluation sums in blocks of 32 terms, the kernels in one k-ordered fma chain over W / 2 + 1 folded terms: the
matrix form's figures grow with W, 7.6e-7 per wavenumber at W = 256, which is why W >= 360 is held in the whole-tensor norm only.)
No case found a defect in a kernel: 661 pass, bitwise repeatable, nothing stored outside what a call stores, no poison reaches a
result.  One defect was found by reading, in the launch predicate: `lane_offsets_fit` did not bound the planes input's lane offset
((kg H W + w) 16 bytes with an ABSOLUTE k-group, up to 2 C H W bytes from the sample's base), so a planes launch past 2 GiB (C = 1040
on the 0.25-degree grid) would have had its loads answered with zeros by the descriptor's range check.  The term is added
(csrc/fft_units.h; the network keeps its fp32 stream for such a shape) and held at its boundary on the host by
tests/emul/fft_units_emul.cpp; no such shape is ever launched.
The file was also run once against five scratch libraries, each with ONE deliberate in-bounds mistake in fft.hip (645 sweep
cases and refusals at that time); cases that failed:
  the sign of the mirrored imaginary part (forward)                      233  (every forward FFT case with Mm > N1 / 2 + 1, i.e. that stores a mirrored column)
  the forward cut comparison off by one (direct column, one entry short) 106  (every forward FFT case with mcut)
  the forward affine without its per-sample stride                       123  (every forward FFT case with the affine at batch 2 or 3)
  the bias left out of the second of the inverse's paired outputs        102  (every inverse FFT case with the bias)
  the range maximum taken before the Mm check (truncated forward)         25  (of 49 truncated cases with out_absmax: white noise rarely
                                                                               peaks in the dropped wavenumbers)
which is what test_absmax_is_a_maximum_of_stored_values was then added for: all 12 of its FFT-form cases fail against the last library.
"""

import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import _dft_ref as R

pytestmark = pytest.mark.gpu

OP_TOL = R.OP_TOL
GUARD = 64                 # elements in front of and behind every operand
SENTINEL = -777.25         # what the output buffers hold before the call
SLOT_SENTINEL = 0x5A5A5A5A
HALF_SENTINEL = 0x5A5A     # the rider destinations (fp16 bit pattern)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


_PLANS = {}


def plan_for(case):
    """one fp32 plan per (H, W, Mm): it supplies the sizes and the matrix form's tables"""
    from ace_amd.sht import _Plan
    key = (case.H, case.W, case.Mm)
    if key not in _PLANS:
        _PLANS[key] = _Plan(case.H, case.W, None, case.Mm, "legendre-gauss", "fp32")
        assert (_PLANS[key].nlat, _PLANS[key].nlon, _PLANS[key].mmax) == key
    return _PLANS[key]


@pytest.fixture(scope="module", autouse=True)
def _plans_and_summary():
    yield
    _PLANS.clear()
    for key in sorted(WORST):
        err, cid = WORST[key]
        print(f"WORST {key[0]} form {key[1]} {key[2]}: {err:.3e} at {cid}")


def guarded(a, dev, fill, lead=GUARD):
    """numpy array `a` as a flat device view inside an allocation filled with `fill`: `lead` elements in front, GUARD behind.
    Returns (view, owner)."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).reshape(-1)
    buf = torch.full((lead + t.numel() + GUARD,), fill, dtype=t.dtype, device=dev)
    buf[lead:lead + t.numel()].copy_(t)
    return buf[lead:lead + t.numel()], buf


def poisoned_spectrum(case, spec):
    """the inverse input as the kernels must cope with it: NaN in every entry from mcut[lat] on, a finite 7e3 in the imaginary parts
    of m = 0 and of a stored Nyquist entry"""
    s = spec.copy()
    s[0, :, :, 1, :] = R.NYQ_POISON
    if case.W % 2 == 0 and case.Mm == case.W // 2 + 1:
        s[case.Mm - 1, :, :, 1, :] = R.NYQ_POISON
    s[~R.stored(case)] = np.nan
    return s


@dataclasses.dataclass
class Result:
    route: tuple
    out_buf: torch.Tensor      # the whole output allocation
    lead: int
    n: int
    slot: torch.Tensor = None
    ride: torch.Tensor = None
    ride_alone: torch.Tensor = None

    def out(self, shape):
        return self.out_buf[self.lead:self.lead + self.n].cpu().numpy().reshape(shape)


def run(case, dev, use_mcut=True, use_rider=True, d=None):
    """one call of ace_dft_stage on poisoned operands (the case's own inputs unless `d` gives others), whatever the two switches say"""
    from ace_amd import _lib
    d = d or R.inputs(case)
    nan = float("nan")
    keep, p = [], {}

    def put(name, a, fill=nan, lead=GUARD):
        if a is None:
            p[name] = None
            return
        view, buf = guarded(a, dev, fill, lead)
        keep.append(buf)
        p[name] = view.data_ptr()

    nspec = case.Mm * case.H * case.bt * 2 * case.c
    ngrid = case.bt * case.c * case.H * case.W
    desc = _lib.DftStageDesc(inverse=int(case.inverse), engine=case.engine, bt=case.bt, c=case.c)
    put("mcut", d["mcut"] if use_mcut else None, fill=-1)
    desc.mcut = p["mcut"]
    if case.inverse:
        put("spec", poisoned_spectrum(case, d["spec"]), lead=GUARD + (1 if case.mis_spec else 0))
        put("bias", d["bias"])
        lead, n = GUARD + (1 if case.mis_grid else 0), ngrid
        desc.spec, desc.bias = p["spec"], p["bias"]
    else:
        if "planes" in case.opts:
            put("xhi", d["xhi"])
            put("xlo", d["xlo"])
            put("xslot", d["xslot"], fill=0)
            desc.xhi, desc.xlo, desc.xslot, desc.sxp = p["xhi"], p["xlo"], p["xslot"], case.c * case.H * case.W
        else:
            put("x", d["x"], lead=GUARD + (1 if case.mis_grid else 0))
            desc.x = p["x"]
        put("in_scale", d["in_scale"])
        put("in_shift", d["in_shift"])
        desc.in_scale, desc.in_shift = p["in_scale"], p["in_shift"]
        lead, n = GUARD + (1 if case.mis_spec else 0), nspec
    out_buf = torch.full((lead + n + GUARD,), SENTINEL, device=dev)
    if case.inverse:
        desc.y = out_buf[lead:].data_ptr()
    else:
        desc.spec_out = out_buf[lead:].data_ptr()
    slot = None
    if "absmax" in case.opts:
        slot = torch.full((GUARD + 64 + GUARD,), SLOT_SENTINEL, dtype=torch.int32, device=dev)
        desc.out_absmax = slot[GUARD:].data_ptr()
    ride = ride_alone = None
    if case.ride and use_rider:
        O, I, order = case.ride
        nh = (O // 32) * (I // 16) * 1024
        put("ride_weight", d["ride_weight"])
        ride = torch.full((GUARD + nh + GUARD,), HALF_SENTINEL, dtype=torch.int16, device=dev)
        ride_alone = torch.full((GUARD + nh + GUARD,), HALF_SENTINEL, dtype=torch.int16, device=dev)
        desc.ride_weight, desc.ride_o, desc.ride_i, desc.ride_order, desc.ride_scale = p["ride_weight"], O, I, order, d["ride_scale"]
        desc.ride_dst, desc.ride_dst_alone = ride[GUARD:].data_ptr(), ride_alone[GUARD:].data_ptr()
    route = _lib.DftRoute(-9, -9, -9, -9)
    _lib.check(_lib.lib().ace_dft_stage(plan_for(case).handle, ctypes.byref(desc), ctypes.byref(route), _lib.current_stream()))
    torch.cuda.synchronize()
    del keep
    return Result((route.form, route.rows, route.units, route.rode), out_buf, lead, n, slot, ride, ride_alone)


def slot_max(slot):
    words = slot[GUARD:GUARD + 64]
    assert torch.all(slot[:GUARD] == SLOT_SENTINEL) and torch.all(slot[GUARD + 64:] == SLOT_SENTINEL), "a write around the slot"
    assert torch.all(words >= 0)   # bit patterns of non-negative floats
    return float(words.max().view(torch.float32))


WORST = {}


def note(case, form, norm, err):
    key = ("inverse" if case.inverse else "forward", form, norm)
    if err >= WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (err, case.id)


@pytest.mark.parametrize("case", R.cases(), ids=lambda c: c.id)
def test_stage_vs_fp64(dev, case):
    ref = R.truth(case)
    r1 = run(case, dev)
    r2 = run(case, dev)
    want = R.expected_route(case)
    assert r1.route == want == r2.route, (r1.route, r2.route, want)
    if case.engine == 1:
        assert r1.route[1] == R.rows(case)
    assert torch.equal(r1.out_buf.view(torch.int32), r2.out_buf.view(torch.int32)), "two calls differ"

    buf = r1.out_buf.cpu().numpy()
    sentinel = np.float32(SENTINEL).view(np.int32)
    inside = np.zeros(buf.shape, dtype=bool)
    if case.inverse:
        mask = None
        inside[r1.lead:r1.lead + r1.n] = True
        got = r1.out(ref.shape)
    else:
        mask = R.stored(case)      # (Mm, H)
        inside[r1.lead:r1.lead + r1.n] = np.broadcast_to(mask[:, :, None, None, None], ref.shape).reshape(-1)
        got = r1.out(ref.shape)
    assert np.array_equal(buf[~inside].view(np.int32), np.full((~inside).sum(), sentinel)), "a store outside what the call stores"
    assert np.isfinite(buf[inside]).all(), "a non-finite result, or an entry that was not written"
    assert not np.any(buf[inside].view(np.int32) == sentinel), "an entry the call should store was not written"

    whole = R.whole_err(got, ref, mask)
    note(case, r1.route[0], "whole", whole)
    line = f"{case.id}: route {r1.route}, whole {whole:.3e}"
    per = None
    if case.per_wavenumber:
        per, m = R.per_wavenumber_err(got, ref, mask)
        note(case, r1.route[0], "per-wavenumber", per)
        line += f", per wavenumber {per:.3e} (m = {m})"
    print(line)
    assert whole <= OP_TOL, (case.id, "whole tensor", whole)
    if per is not None:
        assert per <= OP_TOL, (case.id, "per wavenumber", per)

    if r1.slot is not None:
        assert torch.equal(r1.slot, r2.slot)
        published = slot_max(r1.slot)
        if not case.inverse and "mcut" in case.opts:
            # the bound deliberately covers the entries the cut drops: it is what the same call publishes without the cut
            r3 = run(case, dev, use_mcut=False)
            full = r3.out(ref.shape)
            assert slot_max(r3.slot) == float(np.abs(full).max())
            assert np.array_equal(full[np.broadcast_to(mask[:, :, None, None, None], ref.shape)], got[np.broadcast_to(mask[:, :, None, None, None], ref.shape)])
            assert published == slot_max(r3.slot), (published, slot_max(r3.slot))
        else:
            stored = np.abs(got).max() if mask is None else np.abs(buf[inside]).max()
            assert published == float(stored), (published, float(stored))

    if case.ride:
        O, I, order = case.ride
        d = R.inputs(case)
        packed = R.pack_frag_ref(d["ride_weight"], order, d["ride_scale"]).view(np.int16)
        nh = packed.size
        plain = run(case, dev, use_rider=False)
        assert plain.route[3] == 0 and plain.route[2] == -(-case.c // R.rows(case)) * case.H
        assert torch.equal(plain.out_buf.view(torch.int32), r1.out_buf.view(torch.int32)), "the riders changed the transform's output"
        for name, t in (("ridden", r1.ride), ("stand-alone", r1.ride_alone)):
            h = t.cpu().numpy()
            assert np.all(h[:GUARD] == HALF_SENTINEL) and np.all(h[GUARD + nh:] == HALF_SENTINEL), f"a write around the {name} pack"
            if name == "ridden" and not r1.route[3]:
                assert np.all(h == HALF_SENTINEL), "riders that did not ride wrote"
            else:
                assert np.array_equal(h[GUARD:GUARD + nh], packed), f"the {name} pack is not the packer's"
        if r1.route[3]:
            assert torch.equal(r1.ride, r1.ride_alone) and torch.equal(r1.ride, r2.ride)


PHANTOM = [(1, W, Mm) for W in R.FFT_WIDTHS for Mm in (W // 2, R.N1[W] + 1)] + [(0, 128, 64), (0, 128, 1), (0, 12, 6), (0, 27, 9)]


@pytest.mark.parametrize("engine,W,Mm", PHANTOM)
def test_absmax_is_a_maximum_of_stored_values(dev, engine, W, Mm):
    """A truncated transform computes wavenumbers it does not store: the whole last column block of the FFT form, the rest of the
    matrix form's 64-row tile.  Here the field carries a tone of amplitude 8 at a wavenumber just beyond Mm - the Nyquist entry when
    Mm = W / 2 - so the largest value the kernel computes (2 pi 8, or 2 pi 4) is one it drops, by a wide margin over everything it
    stores: a range maximum taken before the Mm check would show.  (Only the published maximum is held here: the tone's own
    rounding noise, 1e-7 of ITS amplitude, is above the bar relative to the small stored entries.)"""
    case = R.Case("phantom", False, engine, 5, W, Mm, 2, 5 if engine == 0 else R.ROWS[0][W] + 1, opts=("absmax",))
    d = dict(R.inputs(case))
    m0 = W // 2 if Mm == W // 2 else Mm + 1
    d["x"] = (d["x"] + 8.0 * np.cos(2.0 * np.pi * m0 * np.arange(W) / W)).astype(np.float32)
    full = R.truth_of(dataclasses.replace(case, Mm=W // 2 + 1), d)
    assert np.abs(full[:Mm]).max() < 0.5 * np.abs(full[m0]).max()      # the dropped tone dominates what is stored
    r = run(case, dev, d=d)
    assert r.route == R.expected_route(case)
    got = r.out((Mm, case.H, case.bt, 2, case.c))
    assert np.isfinite(got).all() and R.whole_err(got, full[:Mm]) <= 1e-4
    assert slot_max(r.slot) == float(np.abs(got).max()), (slot_max(r.slot), float(np.abs(got).max()))
    assert slot_max(r.slot) < 0.5 * np.abs(full[m0]).max()


def refusal_descs(dev):
    """descriptors the entry must refuse whatever the engine: a scale without a shift, null operands"""
    from ace_amd import _lib
    case = R.Case("refuse", False, 1, 5, 48, 25, 1, 4)
    x = torch.zeros(case.c * case.H * case.W, device=dev)
    sp = torch.zeros(case.Mm * case.H * 2 * case.c, device=dev)
    sc = torch.ones(case.c, device=dev)
    keep = (x, sp, sc)
    fwd = dict(inverse=0, bt=1, c=case.c)
    inv = dict(inverse=1, bt=1, c=case.c)
    out = []
    for e in (0, 1):
        out += [("scale without shift", _lib.DftStageDesc(engine=e, x=x.data_ptr(), spec_out=sp.data_ptr(), in_scale=sc.data_ptr(), **fwd)),
                ("shift without scale", _lib.DftStageDesc(engine=e, x=x.data_ptr(), spec_out=sp.data_ptr(), in_shift=sc.data_ptr(), **fwd)),
                ("no x", _lib.DftStageDesc(engine=e, spec_out=sp.data_ptr(), **fwd)),
                ("no spec_out", _lib.DftStageDesc(engine=e, x=x.data_ptr(), **fwd)),
                ("no spec", _lib.DftStageDesc(engine=e, y=x.data_ptr(), **inv)),
                ("no y", _lib.DftStageDesc(engine=e, spec=sp.data_ptr(), **inv)),
                ("no channels", _lib.DftStageDesc(engine=e, x=x.data_ptr(), spec_out=sp.data_ptr(), inverse=0, bt=1, c=0))]
    out.append(("engine 2", _lib.DftStageDesc(engine=2, x=x.data_ptr(), spec_out=sp.data_ptr(), **fwd)))
    return case, keep, out


@pytest.mark.parametrize("case", R.REFUSALS, ids=lambda c: c.id)
def test_refusals(dev, case):
    R.inputs(case)      # (built outside the expectation: only the entry's own refusal counts)
    with pytest.raises(ValueError, match="ace_dft_stage"):
        run(case, dev)
    # the same call is fine on the engine that takes it (where there is one): the refusal is the named engine's, and the call did not
    # silently run on the other
    other = dataclasses.replace(case, engine=1 - case.engine, sweep="refused")
    if R.takes(other):
        r = run(other, dev)
        assert r.route == R.expected_route(other)
        mask = None if other.inverse else R.stored(other)
        assert R.whole_err(r.out(R.truth(other).shape), R.truth(other), mask) <= OP_TOL


def test_refusals_of_the_descriptor(dev):
    from ace_amd import _lib
    case, keep, descs = refusal_descs(dev)
    plan = plan_for(case)
    for why, desc in descs:
        rc = _lib.lib().ace_dft_stage(plan.handle, ctypes.byref(desc), None, _lib.current_stream())
        assert rc == _lib.ACE_ERR_INVALID, (why, rc)
        assert _lib.lib().ace_last_error().decode().startswith("ace_dft_stage:"), why
    assert _lib.lib().ace_dft_stage(None, ctypes.byref(descs[0][1]), None, _lib.current_stream()) == _lib.ACE_ERR_INVALID
    assert _lib.lib().ace_dft_stage(plan.handle, None, None, _lib.current_stream()) == _lib.ACE_ERR_INVALID
    torch.cuda.synchronize()
    del keep
