"""tests/_hist_ref.py (the numpy statement of ace_diag_hist_window that the GPU kernel tests are judged by) against the reference's
own ComparedDynamicHistograms on tests/golden/gen_histogram.pt: counts and edges bitwise, the 99.9999th percentiles to 1e-12
relative (the same fp64 formula on the same integers; the bar leaves room for a different summation order only)."""
import os

import numpy as np
import pytest
import torch

import _hist_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_histogram.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def replay(golden, n_bins=200):
    """{source: {name: Hist}} after the golden windows, the target's NaN pattern of the first window masking both sides"""
    keep = {n: ~np.isnan(golden["target"][0][n][0, 0].numpy()) for n in golden["names"]}
    out = {}
    for source in ("target", "prediction"):
        out[source] = {n: R.Hist(n_bins) for n in golden["names"]}
        for win in golden[source]:
            for n in golden["names"]:
                assert out[source][n].add(win[n].numpy()[:, :, keep[n]])
    return out


def test_golden_covers_doublings_on_both_sides(golden):
    for n in golden["names"]:
        h = R.Hist(200)
        los, his = [], []
        for win in golden["prediction"]:
            h.add(win[n].numpy())
            los.append(h.lo)
            his.append(h.hi)
        assert min(los) < los[0] and max(his) > his[0], n
    assert bool(golden["target"][0]["ps"].isnan().any()) and not bool(golden["prediction"][0]["ps"].isnan().any())


def test_ref_equals_the_reference_bitwise(golden):
    got = replay(golden)
    for source in ("target", "prediction"):
        for n in golden["names"]:
            h = got[source][n]
            assert h.dropped == 0
            assert np.array_equal(h.counts, golden["counts"][source][n].numpy()), (source, n)
            assert np.array_equal(h.edges, golden["edges"][source][n].numpy()), (source, n)
            want = golden["logs"][f"{source}/99.9999th-percentile/{n}"]
            assert R.percentile(h) == pytest.approx(want, rel=1e-12), (source, n)


def test_ref_drops_and_edge_cases():
    h = R.Hist(8)
    assert h.add(np.linspace(0, 1, 50, dtype=np.float32))
    lo, hi, counts = h.lo, h.hi, h.counts.copy()
    assert not h.add(np.array([0.5, np.inf], dtype=np.float32)) and not h.add(np.array([np.nan], dtype=np.float32))
    assert not h.add(np.zeros(0, dtype=np.float32))
    assert h.dropped == 3 and (h.lo, h.hi) == (lo, hi) and np.array_equal(h.counts, counts)
    c = R.Hist(8)
    assert not c.add(np.full(10, 1e5, dtype=np.float32)) and c.dropped == 1 and np.isnan(c.lo)      # 1e5 +- 1e-6 is 1e5 in fp32
    assert c.add(np.array([1.0, 2.0], dtype=np.float32)) and c.counts.sum() == 2 and c.counts[0] == 1 and c.counts[-1] == 1
    assert c.add(np.array([100.0], dtype=np.float32)) and c.counts.sum() == 3                          # a x50 jump: repeated doublings
    assert c.hi >= 100.0 and c.lo == pytest.approx(1.0, abs=1e-5)
