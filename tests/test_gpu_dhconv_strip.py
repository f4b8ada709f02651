"""The spectral filter strip kernel (ace_amd/csrc/dhconv_strip.hip: hand-pipelined MFMA, filter streamed once into B fragments) held to
fp64 at every branch it takes, through `ace_dhconv_strip_op` (include/ace_sfno.h), which launches it as the network does.

The truth, the per-degree metric, the decaying inputs and the cases are tests/_dhconv_ref.py's (tests/test_dhconv_ref_cpu.py holds a
plain fp32 evaluation of every case to OP_TOL / 2 in the same metric, which is what makes OP_TOL = 2e-6 fair here; the kernel's index
algebra is restated on the host by tests/emul/dhconv_strip_emul.cpp).  Families:
  strips   n = 1, C = 128, L = 96: every row count 1 .. 96 once - the all-lanes-clamp-to-row-0 unit, both strip edges, a full chunk
  chunks   a second chunk of 3 .. 24 rows at row0 = 96, a third at row0 = 192, rows capped by Mm n
  cols     C = 128, 256, 384, 512 (4, 8, 12, 16 stages = 1 .. 4 trips of the stage loop, column groups 0 .. 3) at the two-chunk,
           three-strip ragged shape (5, 24, 25)
  xcd      L = 1, 5, 8, 9: empty per-XCD lists, rows = 0 padding units
  gdense   grouped filter as dense planes: (C, G) = (256, 4) (256, 2) (512, 2) skip the zero blocks, (384, 2) (384, 4) walk them
  gnative  the diagonal blocks alone: (256, 8) (256, 4) (512, 4) (512, 2); each grouped form at (5, 24, 25) and at (1, 5, 6)
  range    coefficients x 1e-12 and x 1e8, filter x 1e-6 and x 1e4, the bound in a single element, and max |coeffs| = 2^-95 and 2^115
Every case (test_strip_vs_fp64)
  * asserts the route it means to check (storage, kspan, units with 1 / 2 / 3 strips, chunks per group) as the entry reports it;
  * runs under poison: coefficients and filter are views inside NaN-filled allocations with 64 elements in front and behind, the
    coefficients with m > l are NaN as well (nothing may read them), `out` is a view inside a buffer of a sentinel; afterwards the
    guards are bitwise intact and the stored region is finite;
  * is run a second time with e_fill = a sentinel and without out_absmax: every entry with m > l comes back as the sentinel (the kernel
    stores no row beyond its unit's rows), every entry with m <= l bitwise as in the first run (which left the m > l entries zero);
  * the maximum over the 64 words of out_absmax equals max |out| over m <= l exactly, the words around the slot are untouched;
  * meets OP_TOL per degree against fp64.
test_grouped_forms_agree_bitwise: dense on the expanded filter, dense with groups = G and the diagonal blocks give the same bits
("skipping exact zeros changes no bit").  test_refusals: what the strip kernel does not take is a ValueError that names the constraint.

MEASURED (MI355X; worst per-degree error | whole-tensor max|err| / max|ref| of the same case, vs fp64; every case is within OP_TOL):
  dense C = 128 (strips, chunks, xcd, cols)   5.14e-7 | 3.75e-7   chunks-n5-C128-L40-Mm41 (l = 32)
  dense C = 256                               7.23e-7 | 5.36e-7   cols-n5-C256-L24-Mm25 (l = 23)
  dense C = 384                               8.56e-7 | 4.81e-7   cols-n5-C384-L24-Mm25 (l = 10)
  dense C = 512                               1.02e-6 | 5.71e-7   cols-n5-C512-L24-Mm25 (l = 9)
  grouped, dense planes                       7.04e-7 | 3.87e-7   gdense-n5-C512-L24-Mm25-G2-dense (l = 16)
  grouped, diagonal blocks                    7.04e-7 | 3.87e-7   gnative-n5-C512-L24-Mm25-G2-native (l = 16; the same bits as the line above)
  range                                       4.89e-7 | 2.11e-7   range-n3-C128-L24-Mm25-spike (l = 15); the two ends are refused
The error grows with C as an fp32 accumulation over 2 C terms does; the three grouped forms agree bitwise at all seven (C, G).
Found: no defect in the kernel.  One in its operator entry, as the issue supposed: `ace_dhconv_f16x3` scaled the coefficient planes by
the host's unclamped pow2_scale(max, 12) while the kernel undoes the clamped exponent of the same maximum - with the old line put back
range-...-xmax2^-95 comes out 64 times too large (per-degree error 63.0) and range-...-xmax2^115 16 times too small (0.9375).  Host
and kernels now take the exponent from csrc/range_exponent.h, and the entry refuses a maximum outside [2^-89, 2^112), where the clamp
acts and the planes no longer hold the precision of the bar.  The network path was never affected: the Legendre stage that writes the
planes there (strip.hip, strip_fold.hip) scales with the same clamped device function of the bound it publishes.
Sensitivity - the file run once against scratch libraries with one deliberate in-bounds mistake each (addresses and wait counts
untouched), failed tests of 45:
  the old host scale put back                            2   the two range ends, as above
  minus sign of the D_im Wi product dropped             42   every case that computes (all but the refused ends and test_refusals)
  lo x hi product of phase 2 dropped in the third strip 28   every case with a three-strip unit and all of test_grouped_forms_agree_bitwise;
                                                             per-degree error 1.0e-4 .. 1.2e-4 where the whole-tensor ratio stays at
                                                             2.1e-7 .. 5.7e-7 - the metric of the earlier operator test passes this mistake
  tb stepping by 4 stages instead of kspan / 32          5   (512, 2) only - the one kspan = 256 - dense and diagonal, both shapes, and its bitwise test
  live test one group too wide                           6   diagonal blocks with C / G = 32 and 64, both shapes, and their bitwise tests
  vmax taken before the row < rows mask                  0   not a mistake of this kernel: the A pieces of rows >= rows are fetched from row
                                                             rows - 1, so a phantom accumulator row is bitwise a stored row and cannot raise the maximum
  vmax over the real parts only (run in its place)      19   the exact-maximum check of every case whose largest stored value is an imaginary part
"""

import ctypes

import pytest
import torch

import _dhconv_ref as R

pytestmark = pytest.mark.gpu

OP_TOL = R.OP_TOL
GUARD = 64
SENTINEL = -777.25        # what out's buffer holds before the call
E_SENTINEL = 12345.0625   # e_fill of the second run
SLOT_SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def poisoned(t, dev):
    """`t` as a device view inside a NaN-filled allocation, GUARD NaNs in front and behind.  Returns (view, owner)."""
    buf = torch.full((GUARD + t.numel() + GUARD,), float("nan"), device=dev)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t.to(dev))
    return view, buf


def run(case, dev, x, w, groups=None, storage=None, e_fill=0.0, absmax=True):
    """one call of ace_dhconv_strip_op on poisoned operands; returns (out buffer, out view (n, C, L, Mm, 2), slot buffer or None, route)"""
    from ace_amd import _lib
    groups = case.groups if groups is None else groups
    storage = case.storage if storage is None else storage
    xv, xbuf = poisoned(x, dev)
    xv.masked_fill_(~R.triangle(case.L, case.Mm).to(dev)[None, None, :, :, None], float("nan"))   # m > l: never read
    wv, wbuf = poisoned(w, dev)
    numel = x.numel()
    obuf = torch.full((GUARD + numel + GUARD,), SENTINEL, device=dev)
    out = obuf[GUARD:GUARD + numel].view(x.shape)
    slot = torch.full((GUARD + 64 + GUARD,), SLOT_SENTINEL, dtype=torch.int32, device=dev) if absmax else None
    desc = _lib.DhconvDesc(coeffs=xv.data_ptr(), weight=wv.data_ptr(), out=out.data_ptr(),
                           out_absmax=(slot[GUARD:].data_ptr() if absmax else None),
                           n=case.n, c=case.C, L=case.L, Mm=case.Mm, groups=groups, storage=storage, e_fill=e_fill)
    route = _lib.DhconvRoute()
    _lib.check(_lib.lib().ace_dhconv_strip_op(ctypes.byref(desc), ctypes.byref(route), _lib.current_stream()))
    torch.cuda.synchronize()
    del xbuf, wbuf
    return obuf, out, slot, (route.storage, route.kspan, tuple(route.units), route.max_chunks), route.units_per_xcd


WORST = {}


def family_of(case):
    return f"cols C={case.C}" if case.family == "cols" else case.family


@pytest.mark.parametrize("case", R.cases(), ids=lambda c: c.id)
def test_strip_vs_fp64(dev, case):
    x, w = R.inputs(case)
    ref = R.truth(case)
    try:
        obuf, out, slot, route, per_xcd = run(case, dev, x, w)
    except ValueError as e:
        # the two ends of the range where host and kernel once took different exponents: correct to the bar, or refused by name
        assert case.variant in R.RANGE_ENDS and "max |coeffs|" in str(e), (case.id, str(e))
        print(f"{case.id}: refused: {e}")
        with pytest.raises(ValueError, match=r"max \|coeffs\|"):
            run(case, dev, x, w, e_fill=E_SENTINEL, absmax=False)
        return
    assert route == R.expected_route(case), (route, R.expected_route(case))
    assert 8 * per_xcd >= sum(route[2]) and per_xcd >= 1
    tri = R.triangle(case.L, case.Mm).to(dev)[None, None, :, :, None].expand_as(out)
    guard = torch.full((GUARD,), SENTINEL, device=dev).view(torch.int32)
    assert torch.equal(obuf[:GUARD].view(torch.int32), guard) and torch.equal(obuf[-GUARD:].view(torch.int32), guard), "a store outside out"
    assert torch.isfinite(out).all(), "a non-finite output: poison reached a result"
    assert torch.all(out[~tri] == 0.0), "an entry with m > l is not the scratch's zero"
    # second run: another fill of the scratch, no range maximum
    obuf2, out2, _, route2, _ = run(case, dev, x, w, e_fill=E_SENTINEL, absmax=False)
    assert route2 == route
    assert torch.all(out2[~tri] == E_SENTINEL), "the kernel stored a row beyond its unit's rows"
    assert torch.equal(out[tri].view(torch.int32), out2[tri].view(torch.int32)), "the two runs differ where m <= l"
    assert torch.equal(obuf2[:GUARD].view(torch.int32), guard) and torch.equal(obuf2[-GUARD:].view(torch.int32), guard)
    # the range maximum: exactly the maximum of what was stored
    assert torch.all(slot[:GUARD] == SLOT_SENTINEL) and torch.all(slot[GUARD + 64:] == SLOT_SENTINEL), "a write around the slot"
    words = slot[GUARD:GUARD + 64]
    assert torch.all(words >= 0)   # bit patterns of non-negative floats
    got_max = words.max().view(torch.float32)
    assert torch.equal(got_max, out[tri].abs().max()), (float(got_max), float(out[tri].abs().max()))
    # accuracy, per degree
    err, l, whole = R.degree_errors(torch.view_as_complex(out.cpu().double().contiguous()), ref)
    fam = family_of(case)
    if err > WORST.get(fam, (0.0,))[0]:
        WORST[fam] = (err, whole, case.id)
    print(f"{case.id}: route {route}, {per_xcd} per XCD, worst degree {err:.3e} (l = {l}), whole tensor {whole:.3e}; worst of {fam} so far {WORST[fam]}")
    assert err <= OP_TOL, (case.id, err, l)


GROUPED_T = sorted({(C, G) for C, G in R.GROUPS_DENSE + R.GROUPS_NATIVE})


@pytest.mark.parametrize("C,G", GROUPED_T, ids=lambda v: str(v))
def test_grouped_forms_agree_bitwise(dev, C, G):
    """dhconv_strip.hip: "Skipping exact zeros changes no bit" - the dense walk (groups = 1 on the expanded filter), the dense planes
    with groups = G (zero blocks skipped where C / G is a multiple or a divisor of 128) and, where the kernel takes it, the diagonal
    blocks alone (per-wave kbase, dead stages skipped, clamped fragment addresses), at the two-chunk, three-strip ragged shape."""
    n, L, Mm = R.T_SHAPE
    case = R.Case("gdense", n, C, L, Mm, G, R.DENSE)
    x, w = R.inputs(case)
    ref = R.truth(case)
    _, full, _, route_full, _ = run(case, dev, x, R.expand_grouped(w, C, G), groups=1, storage=R.DENSE)
    assert route_full[:2] == (R.DENSE, C)
    assert R.degree_errors(torch.view_as_complex(full.cpu().double().contiguous()), ref)[0] <= OP_TOL
    _, dense, _, route_dense, _ = run(case, dev, x, w)
    assert route_dense == R.expected_route(case)
    assert torch.equal(full.view(torch.int32), dense.view(torch.int32)), "dense planes: groups = G differs from groups = 1"
    if R.native_ok(C, G):
        ncase = R.Case("gnative", n, C, L, Mm, G, R.NATIVE)
        _, native, _, route_native, _ = run(ncase, dev, x, w)
        assert route_native == R.expected_route(ncase) and route_native[0] == R.NATIVE
        assert torch.equal(full.view(torch.int32), native.view(torch.int32)), "diagonal blocks differ from the dense form"
    else:
        with pytest.raises(ValueError, match="diagonal-block storage"):
            run(case, dev, x, w, storage=R.NATIVE)


def test_refusals(dev):
    """each constraint of the strip kernel is a ValueError that names it, never another engine"""
    def call(n=1, C=128, L=3, Mm=4, G=1, storage=R.DENSE, e_fill=0.0, wshape=None):
        case = R.Case("refusal", n, C, L, Mm, G, storage)
        x = torch.ones(n, C, L, Mm, 2)
        w = torch.ones(wshape or ((C, C, L, 2) if G == 1 else (G, L, max(C // G, 1), max(C // G, 1), 2)))
        return run(case, dev, x, w, e_fill=e_fill)
    call()   # the shape itself is fine
    for kwargs, msg in [
        (dict(C=192), r"channels % 128 == 0"),
        (dict(C=64), r"channels % 128 == 0"),
        (dict(C=256, G=3), r"groups must divide channels"),
        (dict(G=0, wshape=(1,)), r"groups must divide channels"),
        (dict(storage=2), r"storage is 0 \(dense planes\) or 1 \(diagonal blocks\)"),
        (dict(C=256, G=1, storage=R.NATIVE), r"diagonal-block storage needs groups > 1"),
        (dict(C=384, G=4, storage=R.NATIVE), r"diagonal-block storage needs"),    # C / G = 96
        (dict(C=256, G=16, storage=R.NATIVE), r"diagonal-block storage needs"),   # C / G = 16
        (dict(e_fill=float("nan")), r"bad argument"),
        (dict(L=0, wshape=(1,)), r"bad argument"),
    ]:
        with pytest.raises(ValueError, match="ace_dhconv_strip_op: .*" + msg):
            call(**kwargs)
    from ace_amd import _lib
    assert _lib.lib().ace_dhconv_strip_op(None, None, _lib.current_stream()) == _lib.ACE_ERR_INVALID
    # the earlier entry is the same call and refuses the same way
    t = torch.ones(1, 192, 3, 4, 2, device=dev)
    wt = torch.ones(192, 192, 3, 2, device=dev)
    with pytest.raises(ValueError, match=r"channels % 128 == 0"):
        _lib.check(_lib.lib().ace_dhconv_f16x3(_lib.ptr(t), _lib.ptr(wt), _lib.ptr(torch.empty_like(t)), 1, 192, 3, 4, _lib.current_stream()))
