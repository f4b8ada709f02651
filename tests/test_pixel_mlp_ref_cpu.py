"""The header's statement of ``ace_pixel_mlp_forward`` (tests/_pixel_mlp_ref.py, what the GPU tests hold the kernel to bit for bit)
against the reference LandNet itself: every golden case (tests/golden/gen_landnet_*.pt) within the project's per-step target of
1e-5 of the reference's fp64 output, NaN positions equal.  Measured (max |statement - fp64| / max |fp64|, beside the reference's
own fp32-against-fp64 figure): small_embed 1.6e-07 / 1.1e-07, shipped_embed 2.0e-07 / 2.3e-07, one_hidden 1.1e-07 / 8.2e-08,
no_hidden 0 / 0.  Plus the emulated fmaf against exact rational arithmetic."""
import fractions

import numpy as np
import pytest
import torch

import _landnet_cases as C
import _pixel_mlp_ref as R


@pytest.mark.parametrize("name", C.CASES)
def test_statement_matches_the_reference(name):
    c = C.case(name)
    got, ref64 = c["statement"], c["output64"]
    assert got.shape == ref64.shape and got.dtype == torch.float32
    assert torch.equal(torch.isnan(got), torch.isnan(ref64))
    err, ref_err = C.rel_err(got, ref64), C.rel_err(c["output"], ref64)
    print(f"{name}: statement vs fp64 {err:.3e}; reference fp32 vs fp64 {ref_err:.3e}")
    assert err <= C.TOL, (name, err, ref_err)


def test_k_order_is_a_permutation_in_the_headers_form():
    assert R.k_order(1) == [0] and R.k_order(5) == [0, 4, 1, 2, 3]
    assert R.k_order(16) == [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]
    for K in (1, 3, 16, 17, 30, 64, 65, 256):
        assert sorted(R.k_order(K)) == list(range(K))
    assert R.k_order(20)[:16] == R.k_order(16) and R.k_order(20)[16:] == [16, 17, 18, 19]


def test_fmaf_is_the_single_rounding():
    rng = np.random.default_rng(5)
    n = 2000
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    c = rng.standard_normal(n).astype(np.float32)
    c[::2] = (-(a[::2].astype(np.float64) * b[::2].astype(np.float64))).astype(np.float32)      # heavy cancellation
    a[5], b[5], c[5] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** 60)      # far apart: sticky bit only
    a[7], b[7], c[7] = np.float32(3.0), np.float32(2.0 ** -149), np.float32(2.0 ** -149)              # subnormals
    got = R.fmaf(a, b, c)
    for i in range(n):
        exact = fractions.Fraction(float(a[i])) * fractions.Fraction(float(b[i])) + fractions.Fraction(float(c[i]))
        want = _round_to_f32(exact)
        assert got[i] == want, (i, a[i], b[i], c[i])
    special = R.fmaf(np.array([np.inf, 0.0, np.nan, -0.0], np.float32), np.array([1.0, np.inf, 1.0, 0.0], np.float32),
                     np.array([1.0, 1.0, 1.0, -0.0], np.float32))
    assert special[0] == np.inf and np.isnan(special[1]) and np.isnan(special[2])
    assert special[3] == 0 and np.signbit(special[3])           # (-0)(+0) + (-0) = -0


def _round_to_f32(q: fractions.Fraction) -> np.float32:
    """round-to-nearest-even of an exact rational to fp32 (subnormals kept)"""
    if q == 0:
        return np.float32(0.0)
    sign = -1 if q < 0 else 1
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if fractions.Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)
    scaled = q / fractions.Fraction(2) ** (e - 23)             # the significand in units of the last place
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > fractions.Fraction(1, 2) or (rem == fractions.Fraction(1, 2) and n % 2 == 1):
        n += 1
    return np.float32(sign * float(fractions.Fraction(n) * fractions.Fraction(2) ** (e - 23)))


def test_relu_keeps_nan_and_negative_zero():
    v = R.relu(np.array([-1.0, -0.0, 0.0, 2.0, np.nan, -np.inf], np.float32))
    assert v[0] == 0 and not np.signbit(v[0]) and np.signbit(v[1]) and v[3] == 2 and np.isnan(v[4]) and v[5] == 0


def test_statement_isolates_pixels_and_ignores_nothing():
    rng = np.random.default_rng(6)
    w = [rng.standard_normal((20, 5)).astype(np.float32), rng.standard_normal((3, 20)).astype(np.float32)]
    b = [rng.standard_normal(20).astype(np.float32), None]
    x = rng.standard_normal((1, 5, 7)).astype(np.float32)
    e = rng.standard_normal((20, 7)).astype(np.float32)
    base = R.pixel_mlp(x, w, b, [1, 0], 0, e)
    x2 = x.copy()
    x2[0, :, 3] = np.nan
    y2 = R.pixel_mlp(x2, w, b, [1, 0], 0, e)
    assert np.isnan(y2[0, :, 3]).all()
    keep = [0, 1, 2, 4, 5, 6]
    assert np.array_equal(y2[0][:, keep].view(np.int32), base[0][:, keep].view(np.int32))
