"""tests/_regress_ref.py - the numpy statement of ace_diag_regress_window's header contract that the GPU tests hold the kernel to -
held three ways: to the reference's own functions through tests/golden/gen_regress.pt (tests/golden/make_golden_regress.py ran
``TrendEvaluatorAggregator._add_running_sums``, ``data_index_covariance`` and ``NearZeroFractionAggregator``), to chunking (one
window of T steps = two windows of T / 2), and to the fp32 floor the GPU evaluator test uses for the ENSO coefficients.

Bars.  u64 = 2^-53, u32 = 2^-24.
  trend sums (fp64 on both sides, different summation order, N = 16 terms): |a - b| <= 2 N u64 sum|c x| < 1e-14 sum|c x|.
  ENSO covariance (the reference in fp32: products rounded, a sum of T = 4 terms, one add per window; the statement in fp64):
      |a - b| <= (T + 2) u32 sum|c x|  (one rounding per product, T - 1 adds, one add across windows, rounded up by one).
  near-zero cell sums: small integers, exact in fp32: equal.
  near-zero fractions: each of the reference's fp32 weighted means of a 0/1 field over 162 cells is within
      (log2(162) + 3) u32 < 11 u32 of the exact ratio (a pairwise-or-better fp32 sum of the numerator and of the denominator, a
      product by the weight that is exact for 0/1, one division), and their fp32 running sum over K entries adds K u32 K at most:
      |a - b| <= K (11 + K) u32."""
import os

import numpy as np
import pytest
import torch

import _regress_cases as C
import _regress_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_regress.pt")
U32 = 2.0 ** -24
NAMES = ["t", "pr"]


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def run_statement(g, chunks):
    """the statement over the golden windows, each window cut into ``chunks`` calls along time"""
    gen, target = g["gen"], g["target"]
    B, T, H, W = gen[0]["t"].shape
    hw = H * W
    maps = np.zeros((2, 2, 2 + B, hw))
    count = np.zeros((2, 2, hw), np.int64)
    frac = np.zeros((2, 2))
    weights = g["weights"].reshape(1, hw).numpy()
    eps = np.array([g["eps"][n] for n in NAMES], np.float32)
    scale = np.zeros((2, 2, 2 + B, hw))
    for w in range(2):
        step = T // chunks
        for c in range(chunks):
            sl = slice(w * T + c * step, w * T + (c + 1) * step)
            cut = slice(c * step, (c + 1) * step)
            years, index = g["years"][:, sl].numpy(), g["index"][:, sl].double().numpy()
            planes = [[d[w][n][:, cut].reshape(B, step, hw).numpy() for n in NAMES] for d in (gen, target)]
            first = w == 0 and c == 0                                          # the step the trend and the fraction drop
            if first:                                                         # ... and the ENSO sums keep: a call of its own
                R.regress_window(planes[0], planes[1], [0, 1], 2, coef=index[None], slot=np.array([[2, 3]]), nmaps=2 + B, maps=maps)
            coef = np.stack([np.ones_like(years), years] + ([] if first else [index]))
            slot = np.array([[0] * B, [1] * B] + ([] if first else [[2, 3]]))
            R.regress_window(planes[0], planes[1], [0, 1], 2, coef=coef, slot=slot, nmaps=2 + B, maps=maps, eps=eps, weights=weights,
                             wrows=[0, 0], below_count=count, below_frac=frac, t_begin=1 if first else 0)
            for s in (0, 1):
                scale[s] += R.map_scale(planes[s], [0, 1], 2, np.stack([np.ones_like(years), years, index]), np.array([[0] * B, [1] * B, [2, 3]]), 2 + B)
    return maps, count, frac, scale


def test_statement_equals_the_reference(golden):
    maps, count, frac, scale = run_statement(golden, 1)
    H, W = golden["weights"].shape
    n, sum_t, sum_tt = golden["trend"]["n_sum_t_sum_tt"].tolist()
    denom = n * sum_tt - sum_t * sum_t
    for s, key in enumerate(("gen", "target")):
        for r, name in enumerate(NAMES):
            ref = golden["trend"][key]
            for m, sums in enumerate((ref["sum_y"], ref["sum_ty"])):
                err = np.abs(maps[s, r, m] - sums[name].reshape(-1).numpy())
                assert (err <= 1e-14 * scale[s, r, m]).all(), (key, name, m, float((err / scale[s, r, m]).max()))
            slope = (n * maps[s, r, 1] - sum_t * maps[s, r, 0]) / denom
            bar = 1e-13 * (n * scale[s, r, 1] + abs(sum_t) * scale[s, r, 0]) / denom
            assert (np.abs(slope - ref["slope"][name].reshape(-1).numpy()) <= bar).all(), (key, name)
            for b in range(2):
                cov = golden["enso"]["covariance"][key][b][name].reshape(-1).double().numpy()
                err = np.abs(maps[s, r, 2 + b] - cov)
                assert (err <= 6 * U32 * scale[s, r, 2 + b]).all(), (key, name, b, float((err / scale[s, r, 2 + b]).max()))
            cells = golden["nzf"][f"{key}_map_sum"][name]
            assert np.array_equal(count[s, r], cells.reshape(-1).numpy().astype(np.int64)), (key, name)
            K = golden["nzf"][f"{key}_count"][name]
            assert K == golden["nzf"]["map_count"][name] == 2 * 7
            assert abs(frac[s, r] - float(golden["nzf"][f"{key}_sum"][name])) <= K * (11 + K) * U32, (key, name)
    assert 0 < frac[0, 1] / 14 < 1 and count.max() <= 14 and count[:, 0].sum() > 0
    # the row of weight 0 is counted per cell and leaves the fraction: a field below eps only there has fraction 0
    hw = H * W
    x = np.ones((1, 1, hw), np.float32)
    x[0, 0, :W] = -1.0
    c1, f1 = np.zeros((2, 1, hw), np.int64), np.zeros((2, 1))
    R.regress_window([x], [None], [0], 1, eps=np.zeros(1, np.float32), weights=golden["weights"].reshape(1, hw).numpy(), wrows=[0],
                     below_count=c1, below_frac=f1)
    assert c1[0, 0].sum() == W and f1[0, 0] == 0.0 and c1[1].sum() == 0


def test_one_window_equals_two_half_windows(golden):
    whole, count1, frac1, scale = run_statement(golden, 1)
    halves, count2, frac2, _ = run_statement(golden, 2)
    assert np.array_equal(count1, count2)
    assert (np.abs(whole - halves) <= 8 * 2.0 ** -53 * scale).all()              # one more rounding per window boundary, 8 terms
    assert np.abs(frac1 - frac2).max() <= 16 * 2.0 ** -53 * 14


def test_order_nan_and_slots():
    """the stated order is k, then b, then t, each product rounded before it is added; a slot of -1 feeds nothing; 0 * NaN is NaN"""
    x = np.array([[[1.0, np.nan]], [[3.0, 5.0]]], np.float32)                  # (B = 2, T = 1, hw = 2)
    coef = np.array([[[1e16], [1.0]], [[-1e16], [0.0]]])                      # term 0 feeds map 0, term 1 map 0 too
    maps = np.zeros((2, 1, 2, 2))
    R.regress_window([x], [None], [0], 1, coef=coef, slot=np.array([[0, 0], [0, -1]]), nmaps=2, maps=maps)
    assert maps[0, 0, 0, 0] == (1e16 + 3.0) - 1e16 and np.isnan(maps[0, 0, 0, 1]) and not maps[0, 0, 1].any() and not maps[1].any()
    maps[:] = 0
    R.regress_window([x], [None], [5], 1, coef=coef, slot=np.array([[0, 0], [0, -1]]), nmaps=2, maps=maps)
    assert not maps.any()                                                     # a row out of range


@pytest.mark.parametrize("shape", sorted(C.SHAPES))
def test_the_fp32_floor_of_the_enso_coefficients(shape):
    """The GPU evaluator test compares the fused fp64 coefficients with the torch path's fp32 ones at 3 x this floor (the torch
    path's own error against the fp64 truth on the CPU; the factor covers another summation order on the GPU).  3 x floor must
    stay under 1e-5 max|coef|, the project's fp32 target: the seeds of _regress_cases.SHAPES are chosen so."""
    floors = C.enso_floor(C.case(*shape))
    for name, (floor, top) in floors.items():
        print(f"ENSOFLOOR {shape} {name}: floor {floor:.3e}, max|coef| {top:.3e}, 3 floor / (1e-5 max) = {3 * floor / (1e-5 * top):.3f}")
        assert 0 < 3 * floor < 1e-5 * top, (name, floor, top)
