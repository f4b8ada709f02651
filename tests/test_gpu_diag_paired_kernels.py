"""csrc/diag.hip's paired pass through the C ABI (ace_diag_paired_window) against tests/_diag_paired_ref.py, on the raw fp64
accumulators, at every shape the kernel branches on: nlon 360 (4 rows per band), 1440 (one row per band), 1600 (the 12-pixel
variant), 27 and 90 (not multiples of 4, 27 below a wave), heights that do not divide the band, strided and offset planes, a null
target, zero-weight and NaN pixels on band edges and corners (the gradient's one-sided stencils), a fully masked row, out-of-range
rows and a zonal coarsening factor above 1.

Bars (``_diag_paired_ref.paired_series_errors``): each series entry within 1e-12 of its own natural scale; the zonal accumulator
within 1e-12 of the row mean of |x| it accumulated; the time sums bitwise.  Every output buffer sits between guards; inputs must
come back unchanged."""
import pytest
import torch

import _diag_paired_ref as P
import _diag_ref as R
from test_gpu_diag_kernels import INVALID, Guarded, dev, lib, nan_fill  # noqa: F401

pytestmark = pytest.mark.gpu


def area(H, W):
    return torch.cos(torch.linspace(-1.55, 1.55, H, dtype=torch.float64)).float()[:, None].expand(H, W).contiguous()


def masked(H, W, R_band, g):
    """zero weights (NaN data underneath) on the grid's corners, on both sides of the first band boundary, one whole row and
    scattered pixels"""
    w = area(H, W).clone()
    w[torch.rand(H, W, generator=g) < 0.05] = 0.0
    for r, c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        w[r, c] = 0.0
    b = min(R_band, H - 1)
    w[b - 1, W // 2] = 0.0
    w[b, W // 3] = 0.0
    w[b - 1, 0] = 0.0
    w[b, W - 1] = 0.0
    w[H // 2] = 0.0
    return w


def band_rows(H, W):
    k = 6 if W <= 1536 else 12
    return max(1, min(H, (256 * k) // W))


def layout(x, kind, g):
    """(storage, offset in floats, sample stride, step stride) holding x (B, T, H, W)"""
    B, T, H, W = x.shape
    hw = H * W
    if kind == "contiguous":
        return x.reshape(-1).clone(), 0, T * hw, hw
    if kind == "chanslice":
        s = torch.randn(B, T, 3, hw, generator=g)
        s[:, :, 1] = x.reshape(B, T, hw)
        return s.reshape(-1), hw, T * 3 * hw, 3 * hw
    if kind == "offset":                                  # 1 float past a 16-byte boundary, an odd sample stride
        s = torch.randn(B, T * hw + 3, generator=g)
        s[:, :T * hw] = x.reshape(B, -1)
        return torch.cat([torch.randn(1, generator=g), s.reshape(-1)]), 1, T * hw + 3, hw
    raise ValueError(kind)


def run_paired(dev, gen, tgt, weights, wrows, rows, nrows, n_time, t0, t_begin, do_maps, zt0, factor, nslots, kinds=None, init=None,
               expect=0):
    """gen / tgt: lists of (B, T, H, W) fp32 CPU tensors (tgt entries may be None); returns (series, tsum, zonal) CPU fp64"""
    L = lib()
    n = len(gen)
    B, T, H, W = gen[0].shape
    g = torch.Generator().manual_seed(99)
    kinds = kinds or ["contiguous"] * n
    store, ptrs, strides = [], [[], []], [[], []]
    for side, fields in enumerate((gen, tgt)):
        for x, kind in zip(fields, kinds):
            if x is None:
                ptrs[side].append(0)
                strides[side] += [0, 0]
                continue
            s, off, sb, st = layout(x, kind, g)
            d = s.to(dev)
            store.append((d, s))
            ptrs[side].append(d.data_ptr() + 4 * off)
            strides[side] += [sb, st]
    tab = torch.tensor(ptrs[0] + strides[0] + ptrs[1] + strides[1], dtype=torch.int64, device=dev)
    wdev = weights.reshape(weights.shape[0], -1).contiguous().to(dev)
    rows_d = torch.tensor(rows, dtype=torch.int32, device=dev)
    wrows_d = torch.tensor(wrows, dtype=torch.int32, device=dev)
    if init is None:
        init = (torch.zeros(6, nrows, n_time, dtype=torch.float64), torch.zeros(2, nrows, H * W, dtype=torch.float64),
                torch.zeros(2, nrows, nslots, H, dtype=torch.float64))
    series, tsum, zonal = (Guarded(x.clone(), dev) for x in init)
    npart = int(L.ace_diag_paired_partial_doubles(n, B, T, H, W))
    nband = (H + band_rows(H, W) - 1) // band_rows(H, W)
    assert npart == n * B * T * nband * 4 * 10
    partial = Guarded(nan_fill(npart), dev)
    base = tab.data_ptr()
    rc = L.ace_diag_paired_window(base, base + 8 * n, base + 24 * n, base + 32 * n, rows_d.data_ptr(), wrows_d.data_ptr(),
                                  wdev.data_ptr(), weights.shape[0], partial.ptr, tsum.ptr, zonal.ptr, series.ptr, nrows, n_time,
                                  t0, t_begin, do_maps, zt0, factor, nslots, n, B, T, H, W, None)
    assert rc == expect, L.ace_diag_last_error().decode()
    torch.cuda.synchronize()
    for d, s in store:
        assert torch.equal(d.cpu().view(torch.int32), s.view(torch.int32)), "an input plane changed"
    partial.read()
    return series.read(), tsum.read(), zonal.read()


def check_paired(dev, gen, tgt, weights, wrows, rows, nrows, n_time, t0, t_begin, do_maps, zt0, factor, nslots, what, kinds=None,
                 seed_init=None):
    B, T, H, W = gen[0].shape
    if seed_init is None:
        init = None
        ref = [torch.zeros(6, nrows, n_time, dtype=torch.float64), torch.zeros(2, nrows, H * W, dtype=torch.float64),
               torch.zeros(2, nrows, nslots, H, dtype=torch.float64)]
    else:
        gi = torch.Generator().manual_seed(seed_init)
        init = (torch.randn(6, nrows, n_time, dtype=torch.float64, generator=gi),
                torch.randn(2, nrows, H * W, dtype=torch.float64, generator=gi),
                torch.randn(2, nrows, nslots, H, dtype=torch.float64, generator=gi))
        ref = [x.clone() for x in init]
    start = [x.clone() for x in ref]
    got = run_paired(dev, gen, tgt, weights, wrows, rows, nrows, n_time, t0, t_begin, do_maps, zt0, factor, nslots, kinds, init)
    bar, zbar = ref[0].abs(), ref[2].abs()
    scale = P.paired_window_ref(gen, tgt, weights, wrows, rows, B, T, t0, t_begin, bool(do_maps), zt0, factor, ref[0], ref[1], ref[2],
                                zbar)
    P.add_paired_scale(bar, scale, rows, t0)
    errs = P.paired_series_errors(got[0], ref[0], bar)
    print(f"DIAGACC paired {what} {H}x{W} B={B} T={T} series={['%.2e' % e for e in errs]} (fractions of the bar)")
    assert max(errs) <= 1.0, (what, errs)
    assert R.bits_equal(got[1], ref[1]), f"{what}: the time sums are not the header's sequence of additions"
    assert torch.equal(torch.isnan(got[2]), torch.isnan(ref[2])), what
    ok = ~torch.isnan(ref[2])
    zerr = ((got[2] - ref[2]).abs()[ok] / (1e-12 * zbar[ok]).clamp_min(1e-320)).max() if bool(ok.any()) else torch.zeros(())
    print(f"DIAGACC paired {what} zonal={float(zerr):.2e}")
    assert float(zerr) <= 1.0, (what, float(zerr))
    named = {r for r, wr in zip(rows, wrows) if 0 <= r < nrows and 0 <= wr < weights.shape[0]}
    for r in set(range(nrows)) - named:                    # rows no plane names keep their bits
        for a, b in zip(got, start):
            assert R.bits_equal(a[:, r], b[:, r]), (what, r)
    return got


def make_pair(g, B, T, H, W, kind, w):
    base = torch.randn(B, T, H, W, generator=g)
    x = {"randn": base, "pressure": 1e5 + 1e2 * base}[kind].float()
    y = (x + 0.1 * (x - x.mean()).abs().mean() * torch.randn(B, T, H, W, generator=g)).float()
    x[:, :, w == 0] = float("nan")
    y[:, :, w == 0] = float("nan")
    return x, y


SHAPES = [(180, 360), (7, 1440), (3, 1600), (13, 27), (45, 90), (9, 360), (2, 2), (5, 64)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_paired_shapes(dev, H, W):
    """area weights, a masked weight row with NaN underneath (corners, band edges, a whole row), a surface-pressure-like pair, a
    name without a target; t0 > 0, the first step left out of the time sums"""
    B, T = (2, 3) if H * W <= 64800 else (1, 2)
    g = torch.Generator().manual_seed(H * 10000 + W)
    weights = torch.stack([area(H, W), masked(H, W, band_rows(H, W), g)])
    a = make_pair(g, B, T, H, W, "randn", weights[0])
    m = make_pair(g, B, T, H, W, "randn", weights[1])
    p = make_pair(g, B, T, H, W, "pressure", weights[0])
    lone = make_pair(g, B, T, H, W, "randn", weights[1])[0]
    series, _, zonal = check_paired(dev, [a[0], m[0], p[0], lone], [a[1], m[1], p[1], None], weights, [0, 1, 0, 1], [2, 0, 3, 1], 4,
                                    T + 2, 1, 1, 1, 0, 1, T, "shapes")
    assert bool(torch.isnan(series[2:, 1]).logical_not().all()) and bool((series[2:, 1] == 0).all())     # no target: untouched
    if H > 2:
        assert bool(torch.isnan(zonal[0, 0, :, H // 2]).all())                                           # the fully masked row
    assert not bool(torch.isnan(series[:, [2, 3], 1:T + 1]).any())          # the two names on the area weights


@pytest.mark.parametrize("H,W", [(45, 90), (180, 360), (5, 1440)])
@pytest.mark.parametrize("kind", ["chanslice", "offset"])
def test_paired_layouts_give_the_contiguous_bits(dev, H, W, kind):
    B, T = 2, 3
    g = torch.Generator().manual_seed(H + W)
    weights = torch.stack([area(H, W), masked(H, W, band_rows(H, W), g)])
    a, m = make_pair(g, B, T, H, W, "pressure", weights[0]), make_pair(g, B, T, H, W, "randn", weights[1])
    args = ([a[0], m[0]], [a[1], m[1]], weights, [0, 1], [1, 0], 2, T, 0, 0, 1, 0, 1, T)
    base = check_paired(dev, *args, "contiguous")
    got = check_paired(dev, *args, kind, kinds=[kind, kind])
    for x, y in zip(got, base):
        assert R.bits_equal(x, y), kind


@pytest.mark.parametrize("H,W", [(45, 90), (180, 360)])
@pytest.mark.parametrize("factor,zt0,nslots", [(2, 0, 3), (3, 1, 2), (2, 3, 2)])
def test_paired_coarsened_zonal_and_bookkeeping(dev, H, W, factor, zt0, nslots):
    """factor > 1, a window that starts inside a slot, slots past the end dropped, accumulators that are not zero, rows out of range
    (either table, either side) contributing to nothing"""
    B, T = 2, 5
    g = torch.Generator().manual_seed(H + factor)
    weights = torch.stack([area(H, W), masked(H, W, band_rows(H, W), g)])
    pairs = [make_pair(g, B, T, H, W, "randn", weights[i % 2]) for i in range(5)]
    rows, wrows = [3, INVALID, 0, 9, 1], [0, 1, 1, 0, 2]                 # planes 1, 3 and 4 do not count
    check_paired(dev, [p[0] for p in pairs], [p[1] for p in pairs], weights, wrows, rows, 5, T + 3, 2, 1, 1, zt0, factor, nslots,
                 f"factor {factor}", seed_init=factor)


@pytest.mark.parametrize("H,W", [(45, 90), (180, 360)])
def test_paired_nan_at_a_weighted_pixel_propagates(dev, H, W):
    """a NaN at a non-zero weight (generated side of one sample, target side of another step): the series entries it reaches are
    NaN, the gradient score of the other steps, the zonal nan-means and the time sums go on as the reference has them"""
    B, T = 2, 3
    g = torch.Generator().manual_seed(H + 77)
    weights = area(H, W)[None]
    x, y = make_pair(g, B, T, H, W, "randn", weights[0])
    x[1, 0, H // 3, W // 2] = float("nan")
    y[0, 2, H // 2, 0] = float("nan")
    series, tsum, zonal = check_paired(dev, [x], [y], weights, [0], [0], 1, T, 0, 0, 1, 0, 1, T, "weighted NaN")
    assert bool(torch.isnan(series[[0, 1, 3, 4], 0, 0]).all()) and not bool(torch.isnan(series[2, 0, 0]))
    assert bool(torch.isnan(series[2:5, 0, 2]).all()) and not bool(torch.isnan(series[:2, 0, 2]).any())
    assert not bool(torch.isnan(series[:, 0, 1]).any()) and not bool(torch.isnan(series[5]).any())       # the nan-mean skips them
    assert not bool(torch.isnan(zonal).any()) and int(torch.isnan(tsum).sum()) == 2


def test_paired_without_maps_and_repeatable(dev):
    H, W, B, T = 45, 90, 2, 2
    g = torch.Generator().manual_seed(5)
    weights = area(H, W)[None]
    a = make_pair(g, B, T, H, W, "randn", weights[0])
    got = check_paired(dev, [a[0]], [a[1]], weights, [0], [0], 1, T, 0, 0, 0, 0, 1, 1, "do_maps = 0", seed_init=1)
    gi = torch.Generator().manual_seed(1)
    torch.randn(6, 1, T, dtype=torch.float64, generator=gi)
    assert R.bits_equal(got[1], torch.randn(2, 1, H * W, dtype=torch.float64, generator=gi))
    runs = [run_paired(dev, [a[0]], [a[1]], weights, [0], [0], 1, T, 0, 0, 1, 0, 1, T) for _ in range(2)]
    for x, y in zip(*runs):
        assert R.bits_equal(x, y)
    # a pair that is its own target: zero bias and rmse bit for bit (d = 0 exactly), the gradient score within its bar
    same = run_paired(dev, [a[0]], [a[0]], weights, [0], [0], 1, T, 0, 0, 1, 0, 1, T)[0]
    assert bool((same[3:5, 0] == 0).all()) and float(same[5, 0].abs().max()) <= 1e-12 * 200.0


OK = dict(nw=1, nrows=1, n_time=4, t0=1, t_begin=0, do_maps=1, zt0=0, factor=1, nslots=3, nplanes=1, batch=2, steps=3, nlat=5, nlon=6)


@pytest.mark.parametrize("change,word", [
    (dict(t0=2), "n_time"), (dict(t0=-1), "t0"), (dict(t_begin=-1), "t_begin"), (dict(steps=0), "steps"), (dict(nplanes=-1), "nplanes"),
    (dict(nplanes=65536), "nplanes"), (dict(batch=0), "batch"), (dict(nw=0), "nw"), (dict(nrows=0), "nrows"), (dict(nlat=1), "nlat"),
    (dict(nlon=1), "nlon"), (dict(nlon=2731), "nlon"), (dict(factor=0), "factor"), (dict(nslots=0), "nslots"), (dict(zt0=-1), "zt0"),
    (dict(null=0), "null"), (dict(null=1), "null"), (dict(null=2), "null"), (dict(null=3), "null"), (dict(null=4), "null"),
    (dict(null=5), "null"), (dict(null=6), "null"), (dict(null=7), "null"), (dict(null=8), "null"), (dict(null=9), "null"),
    (dict(null=10), "null"),
])
def test_paired_refusals(dev, change, word):
    """every ACE_ERR_INVALID branch: the code, a message that names the constraint, and no buffer touched"""
    L = lib()
    a = dict(OK)
    a.update({k: v for k, v in change.items() if k != "null"})
    B, T, H, W = 2, 3, 5, 6
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(B, T, H, W, generator=g).to(dev), torch.randn(B, T, H, W, generator=g).to(dev)
    tab = torch.tensor([x.data_ptr(), T * H * W, H * W, y.data_ptr(), T * H * W, H * W], dtype=torch.int64, device=dev)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    weights = torch.ones(1, H * W, device=dev)
    init = [torch.randn(6, 1, 4, dtype=torch.float64, generator=g), torch.randn(2, 1, H * W, dtype=torch.float64, generator=g),
            torch.randn(2, 1, 3, H, dtype=torch.float64, generator=g)]
    series, tsum, zonal = (Guarded(v.clone(), dev) for v in init)
    partial = Guarded(nan_fill(int(L.ace_diag_paired_partial_doubles(1, B, T, H, W))), dev)
    b = tab.data_ptr()
    p = [b, b + 8, b + 24, b + 32, rows.data_ptr(), rows.data_ptr(), weights.data_ptr(), partial.ptr, tsum.ptr, zonal.ptr, series.ptr]
    if "null" in change:
        p[change["null"]] = None
    rc = L.ace_diag_paired_window(p[0], p[1], p[2], p[3], p[4], p[5], p[6], a["nw"], p[7], p[8], p[9], p[10], a["nrows"], a["n_time"],
                                  a["t0"], a["t_begin"], a["do_maps"], a["zt0"], a["factor"], a["nslots"], a["nplanes"], a["batch"],
                                  a["steps"], a["nlat"], a["nlon"], None)
    msg = L.ace_diag_last_error().decode()
    assert rc == INVALID and word in msg and msg.startswith("ace_diag_paired_window"), (rc, msg)
    torch.cuda.synchronize()
    for buf, v in zip((series, tsum, zonal), init):
        assert R.bits_equal(buf.read(), v)
    assert torch.equal(partial.read().view(torch.int64), nan_fill(partial.n).view(torch.int64))


def test_paired_no_planes_and_sizing(dev):
    L = lib()
    assert L.ace_diag_paired_window(None, None, None, None, None, None, None, 1, None, None, None, None, 1, 4, 0, 0, 1, 0, 1, 1, 0, 1,
                                    1, 5, 6, None) == 0
    assert L.ace_diag_paired_partial_doubles(0, 1, 1, 5, 6) == 0
    assert L.ace_diag_paired_partial_doubles(1, 1, 1, 1, 6) == -1 and L.ace_diag_paired_partial_doubles(1, 1, 1, 5, 2731) == -1
    assert L.ace_diag_paired_partial_doubles(2, 1, 40, 180, 360) == 2 * 40 * 45 * 4 * 10
    torch.cuda.synchronize()
