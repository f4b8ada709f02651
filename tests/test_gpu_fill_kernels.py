"""csrc/fill.hip through the C ABI (ace_diag_fill_planes) against tests/_fill_ref.py, the numpy statement of the header contract
that tests/test_fill_ref_cpu.py holds to the reference.  The tables handed to the kernel are the statement's own.

Bar, per pixel: |got - statement| <= 2^-21 x M, M = max |valid value| of the plane.  Derived: at most eight fp32 roundings lie on
the way to a pixel (the mean, four layers, two blur passes, the blend), every stage is a convex combination of values bounded by M,
so each rounding adds at most 2^-24 M and none is amplified.  Copied planes (tab = -1) must be bitwise equal.  dst and the scratch
lie between guards, which must come back intact; the input planes must come back unchanged; the scratch is pre-filled with NaN and
dst with a NaN pattern, so a pixel that is not written, or a mean that is read without having been written, shows."""
import os
import re

import numpy as np
import pytest
import torch

import _fill_ref as R
from test_gpu_diag_kernels import INVALID, Guarded, dev, lib  # noqa: F401
from test_gpu_regress_kernels import place

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ace_sfno.h")).read()
TILE_H, TILE_W, MIN_H, MIN_W = (int(re.search(rf"#define ACE_DIAG_FILL_{k} (\d+)", HEADER).group(1))
                                for k in ("TILE_H", "TILE_W", "MIN_NLAT", "MIN_NLON"))
BAR = 2.0 ** -21
UNWRITTEN = 0x7FC0DEAD                                  # dst pre-fill, an fp32 NaN
SCALES = [(290.0, 10.0), (1e5, 900.0), (-3.0, 2.0)]


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(ROOT, "tests", "golden", "gen_fill.pt"), weights_only=True)


def make_mask(H, W, seed):
    """random 30 % land, from 5 rows on with most of both pole rows; from 20 rows on instead sparse land, a block deep enough for
    an interior inside a clean rim (so that every layer 1..5 occurs), the seam column and the north pole row"""
    g = np.random.default_rng(seed)
    valid = g.random((H, W)) >= 0.3
    if 5 <= H < 20:
        valid[0, : W - 3] = valid[-1, 2:] = False
    if H >= 20:
        valid = g.random((H, W)) >= 0.05
        r0, r1, c0, c1 = H // 4, H // 4 + max(12, H // 3), W // 3, W // 3 + max(14, W // 3)
        valid[r0 - 2: r1 + 15, c0 - 2: c1 + 2] = True
        valid[r0: r1, c0: c1] = False
        valid[r1 + 6: r1 + 13, c0: c1] = False         # a strip 7 deep: no interior, layers up to 4
        valid[:, 0] = False
        valid[0] = False
    valid[H // 2, W // 2] = True
    return valid


def caps(H, W):
    """a second mask: both polar rows masked (on fewer than three rows: one column)"""
    valid = np.ones((H, W), bool)
    if H < 3:
        valid[:, 1] = False
    else:
        valid[0] = valid[-1] = False
    return valid


def fields(valids, tabs, B, T, seed, junk=float("nan")):
    """one (B, T, H, W) fp32 field per name, ``junk`` at the masked pixels of a filled name"""
    g = torch.Generator().manual_seed(seed)
    H, W = valids[0].shape
    out = []
    for i, t in enumerate(tabs):
        off, sc = SCALES[i % 3]
        x = (off + sc * torch.randn(B, T, H, W, generator=g)).float()
        if t >= 0:
            x = torch.where(torch.from_numpy(valids[t]), x, torch.tensor(junk))
        out.append(x)
    return out


def f32_guarded(n, dev):
    init = torch.full((n + (n & 1),), UNWRITTEN, dtype=torch.int32).view(torch.float64)
    return Guarded(init, dev)


def call(dev, xs, tabs, valids, layout="contiguous", seed=0, expect=0, change=None, tables=None):
    """one ace_diag_fill_planes on (B, T, H, W) CPU fields; returns dst as (n, B, T, H, W) fp32"""
    L = lib()
    n = len(xs)
    B, T, H, W = xs[0].shape
    g = torch.Generator().manual_seed(seed)
    placed = [place(x.reshape(B, T, H * W), layout, g) for x in xs]
    store = [p[0].to(dev) for p in placed]
    tab = [s.data_ptr() + 4 * p[1] for p, s in zip(placed, store)]
    for p in placed:
        tab += [p[2], p[3]]
    tab = torch.tensor(tab, dtype=torch.int64, device=dev)
    tabs_d = torch.tensor(tabs, dtype=torch.int32, device=dev)
    if tables is None:
        tables = [(R.layers(v), R.blurred_valid(v)) for v in valids]
    nmasks = len(tables)
    layers = torch.from_numpy(np.stack([t[0].ravel() for t in tables])).to(dev) if nmasks else None
    # the fp32 table one float past a 16-byte boundary
    blurred = torch.cat([torch.zeros(1), torch.from_numpy(np.stack([t[1].ravel() for t in tables])).reshape(-1)]).to(dev)[1:] \
        if nmasks else None
    a = dict(nmasks=nmasks, nnames=n, batch=B, steps=T, nlat=H, nlon=W, srcs=tab.data_ptr(), layers=layers.data_ptr() if nmasks else None)
    a.update(change or {})
    ndoubles = int(L.ace_diag_fill_scratch_doubles(a["nnames"], a["batch"], a["steps"], a["nlat"], a["nlon"]))
    by_shape = any(k in (change or {}) for k in ("nnames", "batch", "steps", "nlat", "nlon"))      # what the size query sees
    assert ndoubles == (-1 if by_shape else n * B * T)
    scratch = Guarded(torch.full((max(n * B * T, 1),), float("nan"), dtype=torch.float64), dev)
    total = n * B * T * H * W
    dst = f32_guarded(total, dev)
    rc = L.ace_diag_fill_planes(a["srcs"], tab.data_ptr() + 8 * n, tabs_d.data_ptr(), a["layers"],
                                blurred.data_ptr() if nmasks else None, a["nmasks"], scratch.ptr, dst.ptr, a["nnames"], a["batch"],
                                a["steps"], a["nlat"], a["nlon"], None)
    assert rc == expect, L.ace_diag_last_error().decode()
    torch.cuda.synchronize()
    scratch.read()
    out = dst.read().view(torch.float32)
    for p, s in zip(placed, store):
        assert torch.equal(s.cpu().view(torch.int32), p[0].view(torch.int32)), "an input plane changed"
    if rc != 0:
        assert bool((out.view(torch.int32) == UNWRITTEN).all()), "a refused call wrote to dst"
        assert "ace_diag_fill_planes" in L.ace_diag_last_error().decode()
        return None
    return out[:total].reshape(n, B, T, H, W)


def check(got, xs, tabs, valids, label=""):
    worst = 0.0
    for i, (x, t) in enumerate(zip(xs, tabs)):
        if t < 0:
            assert torch.equal(got[i].view(torch.int32), x.view(torch.int32)), f"copied name {i}"
            continue
        want = R.fill_planes(x.numpy(), valids[t])
        M = R.scale(x.numpy(), valids[t])
        err = np.abs(got[i].double().numpy() - want) / M
        assert not np.isnan(err).any(), f"name {i}: NaN in the output"
        worst = max(worst, float(err.max()))
    print(f"FILLACC kernel-vs-statement {label}: {worst / BAR:.3f} of the bar")
    assert worst <= BAR
    return worst


SHAPES = {"smallest": (MIN_H, MIN_W, 2, 1), "poles": (5, 18, 1, 2), "tiles": (2 * TILE_H + 5, 2 * TILE_W + 7, 1, 2),
          "one_degree": (180, 360, 1, 2)}
TABS = [0, -1, 1, 0]                                    # filled, copied, a second table, and a name sharing the first


@pytest.mark.parametrize("layout", ["contiguous", "odd"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_and_layouts(dev, shape, layout):
    H, W, B, T = SHAPES[shape]
    assert MIN_H <= 4 and MIN_W <= 16
    if shape == "tiles":
        assert H % TILE_H and W % TILE_W and -(-H // TILE_H) >= 3 and -(-W // TILE_W) >= 3
    valids = [make_mask(H, W, seed=H), caps(H, W)]
    xs = fields(valids, TABS, B, T, seed=W)
    got = call(dev, xs, TABS, valids, layout=layout)
    check(got, xs, TABS, valids, f"{shape} {layout}")
    if H >= 20:
        assert (R.layers(valids[0]) == 5).any() and (R.layers(valids[0]) == 4).any()


@pytest.mark.parametrize("layout", ["contiguous", "odd"])
@pytest.mark.parametrize("name", ["continent", "single", "seam", "random"])
def test_the_golden_masks(dev, golden, name, layout):
    c = golden[name]
    valid = c["mask"].numpy() != 0
    valids = [valid, caps(*valid.shape)]
    B, T = c["input"].shape[:2]
    xs = fields(valids, TABS, B, T, seed=3)
    xs[0] = c["input"].clone()
    got = call(dev, xs, TABS, valids, layout=layout)
    check(got, xs, TABS, valids, f"{name} {layout}")
    # and the reference's own output, at the bar of test_fill_ref_cpu.py plus the kernel's
    M = R.scale(c["input"].numpy(), valid)
    assert float((np.abs(got[0].double().numpy() - c["output"].double().numpy()) / M).max()) <= 21 * 2.0 ** -24 + BAR


def test_values_at_masked_pixels_are_never_read(dev):
    H, W = 2 * TILE_H + 5, 2 * TILE_W + 7
    valids = [make_mask(H, W, seed=5), caps(H, W)]
    a = call(dev, fields(valids, TABS, 1, 2, seed=1), TABS, valids)
    b = call(dev, fields(valids, TABS, 1, 2, seed=1, junk=1e30), TABS, valids)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(a.view(torch.int32), call(dev, fields(valids, TABS, 1, 2, seed=1), TABS, valids).view(torch.int32))


def test_a_table_without_a_valid_pixel_gives_nan(dev):
    H, W = 9, 18
    valids = [np.zeros((H, W), bool), make_mask(H, W, seed=2)]
    tabs = [0, 1, -1]
    xs = fields(valids, tabs, 2, 2, seed=4)
    got = call(dev, xs, tabs, valids)
    assert bool(torch.isnan(got[0]).all())
    check(got[1:], xs[1:], tabs[1:], valids, "beside an all-masked name")


def test_copies_alone_need_no_table(dev):
    xs = fields([np.ones((7, 20), bool)], [-1, -1], 2, 3, seed=6)
    got = call(dev, xs, [-1, -1], [], layout="odd")
    check(got, xs, [-1, -1], [])
    # a tab entry that names no table copies too
    valids = [make_mask(7, 20, seed=1)]
    got = call(dev, xs, [1, -7], valids)
    check(got, xs, [-1, -1], valids)


@pytest.mark.parametrize("change,word", [
    ({"nlat": MIN_H - 1}, "nlat"), ({"nlon": MIN_W - 1}, "nlon"), ({"batch": 0}, "batch"), ({"steps": 0}, "steps"),
    ({"nnames": -1}, "nnames"), ({"nmasks": -1}, "nmasks"), ({"nnames": 2 ** 31 - 1}, "2\\^31"), ({"srcs": None}, "null"),
    ({"layers": None}, "null")])
def test_refusals(dev, change, word):
    H, W = 6, 16
    valids = [make_mask(H, W, seed=1)]
    xs = fields(valids, [0, -1], 1, 2, seed=2)
    assert call(dev, xs, [0, -1], valids, expect=INVALID, change=change) is None
    assert re.search(word, lib().ace_diag_last_error().decode())


def test_no_names_is_a_no_op(dev):
    L = lib()
    assert L.ace_diag_fill_scratch_doubles(0, 1, 1, 4, 16) == 0
    assert L.ace_diag_fill_planes(None, None, None, None, None, 0, None, None, 0, 1, 1, 4, 16, None) == 0
