"""tests/_dft_ref.py, the numpy statement of the longitude DFT stage that tests/test_gpu_dft_stage.py holds the four kernels to.

1. Conditioning (test_fp32_evaluation_is_within_half_the_bar): EVERY case of the lists, evaluated in plain fp32 in the form of its kernel
   family (torch.fft in float32 for the FFT form, an fp32 matrix product with fp32 tables for the matrix form), stays within
   OP_TOL / 2 = 1e-6 of the fp64 truth in every norm the GPU test applies to that case.  This is what makes OP_TOL = 2e-6 a fair bar: a
   correct fp32-class kernel has half the bar to spare.  A case that breaks it gets other inputs, not another bar.  Worst over the lists:
   FFT form 3.2e-7 whole tensor / 5.4e-7 per wavenumber (W = 1440); matrix form 2.6e-7 whole tensor / 3.1e-7 per wavenumber (W = 256).
   The matrix product is `matmul_f32`: elementwise fp32 operations in a fixed order, the same figure on every machine.
2. The truth against direct sums that share no code with it, the layout against the index formula of kernels.h, and the three
   zeroing rules of the inverse contract.
3. The producer restatement (`planes_from`) and the fragment packer (`pack_frag_ref`) against scalar loops.
4. The lists cover what they claim: every form in both directions, both unit-count parities, every mcut edge, operands below 2 MB."""

import numpy as np
import pytest

import _dft_ref as R


@pytest.mark.parametrize("case", R.cases(), ids=lambda c: c.id)
def test_fp32_evaluation_is_within_half_the_bar(case):
    ref, got = R.truth(case), R.plain_fp32(case)
    assert np.isfinite(ref).all() and got.shape == ref.shape
    mask = None if case.inverse else R.stored(case)
    whole = R.whole_err(got, ref, mask)
    line = f"{case.id}: plain fp32 vs fp64 whole {whole:.3e}"
    assert whole <= R.OP_TOL / 2, (case.id, whole)
    if case.per_wavenumber:
        per, m = R.per_wavenumber_err(got, ref, mask)
        line += f", per wavenumber {per:.3e} (m = {m})"
        assert per <= R.OP_TOL / 2, (case.id, per, m)
    print(line)


def test_forward_truth_is_the_direct_sum_in_the_layout_of_kernels_h():
    case = R.Case("direct", False, 0, 3, 10, 5, 2, 3, opts=("affine",))
    d, X = R.inputs(case), R.truth(case)
    flat = X.reshape(-1)
    H, W, Bt, C = case.H, case.W, case.bt, case.c
    for m in range(case.Mm):
        for k in range(H):
            for b in range(Bt):
                for c in range(C):
                    v = d["x"][b, c, k].astype(np.float64) * np.float64(d["in_scale"][b, c]) + np.float64(d["in_shift"][b, c])
                    s = (2.0 * np.pi / W) * sum(v[w] * np.exp(-2j * np.pi * m * w / W) for w in range(W))
                    base = ((m * H + k) * Bt + b) * 2 * C      # kernels.h: X[m][k][b][ri][c]
                    assert abs(flat[base + c] - s.real) <= 1e-13 and abs(flat[base + C + c] - s.imag) <= 1e-13, (m, k, b, c)


@pytest.mark.parametrize("W,Mm", [(10, 6), (10, 5), (10, 3), (9, 5), (9, 4)])
def test_inverse_truth_is_the_direct_hermitian_sum(W, Mm):
    case = R.Case("direct", True, 1, 4, W, Mm, 2, 3, opts=("bias", "mcut"), mcut="random")
    d, y = R.inputs(case), R.truth(case)
    S = d["spec"].astype(np.float64)
    mc = d["mcut"]
    assert y.shape == (2, 3, 4, W)
    for k in range(case.H):
        for b in range(case.bt):
            for c in range(case.c):
                want = np.full(W, np.float64(d["bias"][c]))
                for m in range(min(Mm, int(mc[k]))):
                    re, im = S[m, k, b, 0, c], S[m, k, b, 1, c]
                    if m == 0 or 2 * m == W:
                        want += re * np.cos(2.0 * np.pi * m * np.arange(W) / W)       # real entries: their imaginary part is ignored
                    else:
                        want += 2.0 * (re * np.cos(2.0 * np.pi * m * np.arange(W) / W) - im * np.sin(2.0 * np.pi * m * np.arange(W) / W))
                assert np.abs(y[b, c, k] - want).max() <= 1e-12, (k, b, c)


def test_inverse_truth_does_not_read_what_the_kernels_must_not():
    """the entries the GPU test poisons - everything from mcut[lat] on, the imaginary parts of m = 0 and of the stored m = W / 2 -
    do not enter the truth"""
    import dataclasses
    case = R.Case("poison", True, 1, 10, 16, 9, 2, 3, opts=("mcut",))
    d = R.inputs(case)
    spec = d["spec"].copy()
    spec[~R.stored(case)] = 1e30
    spec[0, :, :, 1, :] = R.NYQ_POISON
    spec[8, :, :, 1, :] = R.NYQ_POISON
    a = np.fft.irfft(R.inverse_spectrum(case, spec, np.float64), n=16, axis=-1, norm="forward")
    assert np.array_equal(a, R.truth(case))
    # a truncated spectrum stores no Nyquist entry: its last entry keeps its imaginary part
    short = dataclasses.replace(case, Mm=8, opts=())
    T = R.inverse_spectrum(short, R.inputs(short)["spec"], np.float64)
    assert np.abs(T[..., 7].imag).max() > 0.1 and np.all(T[..., 8] == 0.0) and np.all(T[..., 0].imag == 0.0)


def test_layout_round_trip():
    rng = np.random.default_rng(5)
    F = rng.standard_normal((2, 3, 4, 5)) + 1j * rng.standard_normal((2, 3, 4, 5))
    S = R.to_spec_layout(F)
    assert S.shape == (5, 4, 2, 2, 3) and S[3, 2, 1, 1, 0] == F[1, 0, 2, 3].imag
    assert np.array_equal(R.from_spec_layout(S), F)


def test_planes_are_what_a_producer_writes():
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((2, 16, 3, 24)) * 37.5).astype(np.float32)
    hi, lo, slot, values = R.planes_from(x)
    bound = np.abs(x).max()
    e = R.pow2_exponent_for(bound)
    assert 2.0 ** 11 <= float(bound) * 2.0 ** e < 2.0 ** 12
    assert slot[0] == np.float32(bound).view(np.uint32) and not slot[1:].any()
    assert hi.shape == lo.shape == (2, 2, 72, 8) and hi.dtype == lo.dtype == np.float16
    # entry (b, kg, pixel, e8) is channel 8 kg + e8 of that pixel
    for b, kg, pix, e8 in ((0, 0, 0, 0), (1, 1, 71, 7), (1, 0, 30, 3)):
        ch, k, w = 8 * kg + e8, pix // 24, pix % 24
        h = np.float16(np.float32(x[b, ch, k, w]) * np.float32(2.0 ** e))
        l = np.float16(np.float32(x[b, ch, k, w]) * np.float32(2.0 ** e) - np.float32(h))
        assert hi[b, kg, pix, e8] == h and lo[b, kg, pix, e8] == l
        assert values[b, ch, k, w] == (float(h) + float(l)) / 2.0 ** e
    # 22 bits: within 2^-22 of the bound, and exactly representable in fp32 (the kernel adds hi and lo in fp32)
    assert np.abs(values - x).max() <= float(bound) * 2.0 ** -21
    assert np.array_equal(values.astype(np.float32).astype(np.float64), values)
    assert [R.pow2_exponent_for(v) for v in (1.0, 0.75, 4096.0, 0.0)] == [11, 12, -1, 0]


def test_pack_frag_ref_against_a_scalar_restatement():
    rng = np.random.default_rng(11)
    w = rng.standard_normal((64, 32)).astype(np.float32)
    for order in (0, 1):
        got = R.pack_frag_ref(w, order, 512.0)
        assert got.shape == (2 * 2 * 1024,)
        for T, J, lane, e in ((0, 0, 0, 0), (1, 1, 63, 7), (1, 0, 33, 2), (0, 1, 31, 5)):
            i, g = lane & 31, lane >> 5
            x = np.float32(w[32 * T + i, 16 * J + 8 * g + e]) * np.float32(512.0)
            h = np.float16(x)
            blk = T * 2 + J if order == 0 else J * 2 + T
            assert got[blk * 1024 + lane * 8 + e] == h
            assert got[blk * 1024 + 512 + lane * 8 + e] == np.float16(x - np.float32(h))


def test_the_lists_cover_what_they_claim():
    cs = R.cases()
    routes = {(c.inverse, R.expected_route(c)[0]) for c in cs}
    assert routes == {(i, f) for i in (False, True) for f in (0, 1, 2)}, routes
    for W in R.FFT_WIDTHS:
        assert R.N1[W] * R.N2[W] == W
        for inv in (False, True):
            e1 = [c for c in cs if c.engine == 1 and c.W == W and c.inverse == inv]
            Rr = R.ROWS[1 if inv else 0][W]
            assert {c.c for c in e1} >= {1, Rr - 1, Rr, Rr + 1, 2 * Rr + 3}
            assert {R.expected_route(c)[2] % 8 == 0 for c in e1} == {True, False}      # both branches of the unit mapping
            assert {c.Mm for c in e1} >= set(R._mm_list(W)) and len(R._mm_list(W)) == 8
            cut = [c for c in e1 if c.sweep == "cut" and c.mcut == "edges"]
            assert {c.Mm for c in cut} == {W // 2 + 1, W // 2 - 1}
            for c in cut:
                n1 = R.N1[W]
                assert set(R.mcut_values(c).tolist()) == {0, 1, n1 // 2, n1 // 2 + 1, n1 - 1, n1, n1 + 1, c.Mm - 1, c.Mm, c.Mm + 5}
        pl = [c for c in cs if "planes" in c.opts and c.W == W]
        assert {c.c for c in pl} == {8, 24, 40} and any("affine" in c.opts for c in pl)
    rd = [c for c in cs if c.ride]
    assert [R.rides(c) for c in rd] == [True, True, True, True, False]
    assert R.expected_route(rd[0]) == (2, 16, 3 * 9, 1) and R.expected_route(rd[1]) == (2, 16, 8 * 9, 1)      # launch order; XCD, four idle
    assert R.expected_route(rd[3]) == (2, 8, 8 * 5, 1) and R.expected_route(rd[4]) == (2, 16, 3 * 8, 0)
    e0 = [c for c in cs if c.engine == 0]
    assert {c.W for c in e0} >= {4, 6, 12, 128, 18, 90, 27, 256, 360, 16}
    assert {c.H * c.bt * c.c for c in e0 if c.sweep == "cols"} >= {112, 124, 127, 128, 129, 132, 144}
    assert {c.Mm for c in e0 if c.W in (128, 256)} >= {1, 64, 65}
    assert {c.bt for c in cs} == {1, 2, 3}
    assert all(R.takes(c) for c in cs) and not any(R.takes(c) for c in R.REFUSALS)
    assert not any(c.per_wavenumber for c in cs if c.shift == "large" or c.inverse or (c.engine == 0 and c.W >= 360))
    for c in cs:      # tiny: every operand below 2 MB
        grid = c.bt * c.c * c.H * c.W * 4
        spec = c.Mm * c.H * c.bt * 2 * c.c * 4
        assert max(grid, spec) < 2 * 1024 * 1024, (c.id, grid, spec)
