"""``ace_amd.disco.disco_table`` against the reference's own tables (tests/golden/gen_ankur_tables.pt, emitted by
fme/core/disco/_convolution.py through make_golden_ankur.py) on every stored grid, 180 x 360 included: the index set is the
reference's exactly - row offsets and (hi, wi) in its order - and every value is within 1 ulp of fp32 of the reference's.  Both are
fp64 computations rounded once and can differ only in a last bit of libm; a larger gap means a missed rounding of the norm table
(held in fp32, its mean over rows and the eps in fp32).  Largest difference found: 0 ulp on every grid under the
suite's processor-independent MKL code path; 1 ulp, on one value of the 69048 of 180 x 360, outside it."""
import numpy as np
import pytest

from _util import load_golden
from ace_amd.disco import disco_table

GRIDS = [(6, 8, 3), (8, 16, 3), (9, 20, 2), (16, 36, 3), (24, 70, 4), (180, 360, 3)]


@pytest.fixture(scope="module")
def tables():
    return load_golden("gen_ankur_tables.pt")


def _ordered(v):
    """fp32 bit patterns mapped to integers that are ordered as the floats are (ulp distance = integer distance)"""
    i = v.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}k{g[2]}")
def test_table_is_the_references(tables, grid):
    H, W, ks = grid
    ref = tables[grid]
    t = disco_table((H, W), ks)
    assert np.array_equal(t.row_offsets, ref["row_offsets"].numpy())
    assert np.array_equal(t.hi.astype(np.int64) * W + t.wi, ref["col_idx"].numpy().astype(np.int64))
    want = np.ascontiguousarray(ref["vals"].numpy().T)                  # [points][K]
    assert t.vals.dtype == np.float32 and t.vals.shape == want.shape == (len(t.hi), ks * ks)
    ulp = np.abs(_ordered(t.vals) - _ordered(want))
    print(f"{grid}: {len(t.hi)} points, largest difference {int(ulp.max())} ulp, {int((ulp > 0).sum())} of {ulp.size} values differ, "
          f"{int((want == 0).sum())} exact zeros kept")
    assert ulp.max() <= 1
    assert np.array_equal(t.vals == 0, want == 0)                       # an exactly-zero entry stays a table entry
    # ascending (hi, wi) within a row, every row supported
    for ho in range(H):
        a, b = int(t.row_offsets[ho]), int(t.row_offsets[ho + 1])
        key = t.hi[a:b].astype(np.int64) * W + t.wi[a:b]
        assert b > a and (np.diff(key) > 0).all()


def test_support_sizes_of_the_issue(tables):
    """(6, 8): 19 / 15 points per row; (16, 36): 66 down to 21; (24, 70): 169 down to 31"""
    n = lambda g: np.diff(disco_table(g[:2], g[2]).row_offsets)     # noqa: E731
    assert sorted(set(n((6, 8, 3)))) == [15, 19]
    assert n((16, 36, 3)).max() == 66 and n((16, 36, 3)).min() == 21
    assert n((24, 70, 4)).max() == 169 and n((24, 70, 4)).min() == 31
