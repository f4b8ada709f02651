"""tests/_fill_ref.py, the fp64 numpy statement of the ``ace_diag_fill_planes`` contract, against the reference's own
SmoothFloodFill(num_steps=4) (tests/golden/gen_fill.pt, written by tests/golden/make_golden_fill.py), and ``ace_amd.fill`` - the
host tables and the torch path - against the statement.

The bar is measured, not derived: the reference runs in fp32 torch ops whose summation order is torch's, the statement in fp64.
With M = max |valid value| of a plane, the worst |statement - golden| / M measured when the golden was built was, in units of
2^-24: continent 4.55, single 2.62, seam 2.77, random 3.84, and 5.25 on a 180 x 360 blob mask with 14941 interior pixels (not
stored).  The test allows 4 x the worst of these, 21 x 2^-24 (torch's fp32 summation order may differ between builds; the allowance
may never pass 64 x 2^-24).  ``smooth_flood_fill`` on the CPU in fp32 is held to the statement at the same bar (measured: at most
4.13 x 2^-24).  The layer planes of ``fill_tables`` must equal the statement's exactly."""
import os

import numpy as np
import pytest
import torch

import _fill_ref as R
from ace_amd import fill as F

MEASURED = 5.25                                        # x 2^-24, the worst case above
BAR = 4 * MEASURED * 2.0 ** -24
assert BAR <= 64 * 2.0 ** -24
CASES = ("continent", "single", "seam", "random")


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_fill.pt"), weights_only=True)


def worst(got, want, M):
    return float((np.abs(np.asarray(got, np.float64) - want) / M).max())


def test_the_golden_masks_are_what_the_issue_describes(golden):
    counts = {n: np.bincount(R.layers(golden[n]["mask"].numpy() != 0).ravel(), minlength=6) for n in CASES}
    assert (counts["continent"] > 0).all()                                   # every layer 0..5
    assert counts["single"][0] == 1 and counts["single"][5] > 0
    seam = golden["seam"]["mask"]
    assert not seam[:, 0].any() and not seam[0].any() and counts["seam"][5] > 0
    assert counts["random"][5] == 0 and counts["random"][1] > 0
    for n in CASES:                                                          # NaN exactly where the mask is zero
        c = golden[n]
        assert torch.equal(torch.isnan(c["input"]), (c["mask"] == 0).expand_as(c["input"]))
        assert bool(torch.isfinite(c["output"]).all())


@pytest.mark.parametrize("name", CASES)
def test_the_statement_matches_the_reference(golden, name):
    c = golden[name]
    valid = c["mask"].numpy() != 0
    x = c["input"].numpy()
    got = R.fill_planes(x, valid)
    err = worst(got, c["output"].double().numpy(), R.scale(x, valid))
    print(f"FILLACC statement-vs-reference {name}: {err * 2 ** 24:.2f} x 2^-24")
    assert err <= BAR


@pytest.mark.parametrize("name", CASES)
def test_the_torch_path_matches_the_statement(golden, name):
    c = golden[name]
    valid = c["mask"].numpy() != 0
    x = c["input"]
    got = F.smooth_flood_fill(x, c["mask"])
    assert got.shape == x.shape and got.dtype == torch.float32
    err = worst(got.numpy(), R.fill_planes(x.numpy(), valid), R.scale(x.numpy(), valid))
    print(f"FILLACC torch-vs-statement {name}: {err * 2 ** 24:.2f} x 2^-24")
    assert err <= BAR
    # the values at masked pixels are never read
    junk = torch.where(torch.isnan(x), torch.full_like(x, 1e30), x)
    assert torch.equal(F.smooth_flood_fill(junk, c["mask"]), got)
    # the tables of a cache give the same result
    assert torch.equal(F.smooth_flood_fill(x, None, tables=F.FillTables().on(name, c["mask"], "cpu")), got)


@pytest.mark.parametrize("name", CASES)
def test_the_tables_match_the_statement(golden, name):
    mask = golden[name]["mask"]
    valid = mask.numpy() != 0
    layers, blurred = F.fill_tables(mask)
    assert layers.dtype == torch.uint8 and blurred.dtype == torch.float32 and layers.shape == blurred.shape == mask.shape
    assert np.array_equal(layers.numpy(), R.layers(valid))
    assert float(np.abs(blurred.numpy().astype(np.float64) - R.blurred_valid(valid)).max()) <= 2.0 ** -24
    assert np.array_equal(blurred.numpy() == 1.0, R.blurred_valid(valid) == 1.0)


def test_layers_from_the_first_simulation_alone_are_wrong(golden):
    """The trap of the contract: a pixel beside the interior is filled from the inside at step 1, so the layers are not the steps
    at which growing the valid set alone reaches a pixel."""
    c = golden["continent"]
    valid = c["mask"].numpy() != 0
    trap = R.layers_a_only(valid)
    assert np.array_equal(trap, F.fill_layers(valid, interior_first=False))
    lay = R.layers(valid)
    assert (trap != lay).sum() > 0 and np.array_equal(trap == 5, lay == 5) and np.array_equal(trap == 0, lay == 0)
    x = c["input"].numpy()[0, 0]
    M = float(R.scale(x, valid).max())
    wrong = worst(R.fill(x, valid, trap), c["output"].double().numpy()[0, 0], M)
    assert wrong > 100 * BAR                              # off by the field's own variability, not by roundings
    # without an interior the two agree
    rnd = golden["random"]["mask"].numpy() != 0
    assert np.array_equal(R.layers_a_only(rnd), R.layers(rnd))


def test_a_plane_without_a_valid_pixel_is_nan_and_an_unmasked_one_is_unchanged():
    x = torch.randn(1, 2, 6, 12)
    assert bool(torch.isnan(F.smooth_flood_fill(x, torch.zeros(6, 12))).all())
    assert np.isnan(R.fill(x[0, 0].numpy(), np.zeros((6, 12), bool))).all()
    layers, blurred = F.fill_tables(torch.ones(6, 12))
    assert not layers.any() and bool((blurred == 1).all())
    assert float((F.smooth_flood_fill(x, torch.ones(6, 12)) - x).abs().max()) <= 4 * 2.0 ** -24 * float(x.abs().max())


def test_the_cache_builds_and_uploads_once_per_key_and_device():
    cache, mask = F.FillTables(), torch.ones(6, 12)
    mask[2:4, 3:9] = 0
    other = torch.ones(6, 12)
    other[0] = 0
    a = cache.on("m", mask, "cpu")
    assert cache.on("m", mask, "cpu") is a and cache.uploads == 1
    assert cache.row("m", mask, "cpu") == 0 and cache.row("o", other, "cpu") == 1 and cache.row("m", mask, "cpu") == 0
    assert cache.uploads == 2
    layers, blurred, n = cache.stacks("cpu")
    assert n == 2 and layers.shape == blurred.shape == (2, 72)
    assert torch.equal(layers[1].reshape(6, 12), F.fill_tables(other)[0])
    assert cache.has_valid("m", mask) and not cache.has_valid("z", torch.zeros(6, 12))
    assert F.FillTables().stacks("cpu") == (None, None, 0)
    with pytest.raises(ValueError, match="fill tables"):
        F.smooth_flood_fill(torch.zeros(1, 1, 5, 12), mask)
