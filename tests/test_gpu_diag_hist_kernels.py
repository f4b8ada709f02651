"""csrc/hist.hip through the C ABI (ace_diag_hist_window) against tests/_hist_ref.py, which tests/test_hist_ref_cpu.py holds to the
reference bitwise.  Counts are integers and lo / hi exact fp64 formulas of exact fp32 minima and maxima, so every comparison is
``torch.equal`` / ``==``: there is no tolerance in this file.  Every output buffer (range, counts, dropped, scratch) lies between
guards, which must come back intact, and the input planes must come back unchanged."""
import os

import numpy as np
import pytest
import torch

import _hist_ref as R
from test_gpu_diag_kernels import INVALID, Guarded, dev, lib  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_histogram.pt")


class State:
    """the persistent device state of nrows rows, between guards, and its numpy twin"""

    def __init__(self, dev, nrows, n_bins):
        self.dev, self.nrows, self.n_bins = dev, nrows, n_bins
        self.range = Guarded(torch.full((2, nrows, 2), float("nan"), dtype=torch.float64), dev)
        self.counts = Guarded(torch.zeros(2, nrows, n_bins, dtype=torch.int64).view(torch.float64), dev)
        self.dropped = Guarded(torch.zeros(2 * nrows, dtype=torch.int32).view(torch.float64), dev)
        self.ref = [[R.Hist(n_bins) for _ in range(nrows)] for _ in range(2)]

    def read(self):
        return (self.range.read(), self.counts.read().view(torch.int64).reshape(2, self.nrows, self.n_bins),
                self.dropped.read().view(torch.int32).reshape(2, self.nrows))

    def check(self):
        rng, cnt, drop = self.read()
        for s in range(2):
            for r in range(self.nrows):
                h = self.ref[s][r]
                assert torch.equal(cnt[s, r], torch.from_numpy(h.counts)), (s, r)
                lo, hi = float(rng[s, r, 0]), float(rng[s, r, 1])
                assert (np.isnan(lo) and np.isnan(h.lo)) or (lo == h.lo and hi == h.hi), (s, r, lo, hi, h.lo, h.hi)
                assert int(drop[s, r]) == h.dropped, (s, r)
        return rng, cnt, drop


def place(data, layout, g):
    """(storage, offset in floats, sample stride, step stride) of a (B, T, hw) field"""
    B, T, hw = data.shape
    if layout == "contiguous":
        return data.reshape(-1).clone(), 0, T * hw, hw
    pitch = hw + 3                                      # "odd": one float past a 16-byte boundary, rows of a strided view
    s = torch.randn(1 + B * T * pitch, generator=g) * 1e30
    s[1:].view(B, T, pitch)[:, :, :hw] = data
    return s, 1, T * pitch, pitch


def window(st, gens, tgts, rows, masks=None, layout="contiguous", seed=0, expect=0, update_ref=True):
    """one ace_diag_hist_window on (B, T, hw) CPU fields; the numpy twin gets the same window"""
    L, dev = lib(), st.dev
    g = torch.Generator().manual_seed(seed)
    n = len(gens)
    B, T, hw = gens[0].shape
    placed = [[place(x, layout, g) if x is not None else None for x in side] for side in (gens, tgts)]
    store = [[p[0].to(dev) if p is not None else None for p in side] for side in placed]
    mdev = [m.to(dev) if m is not None else None for m in (masks or [None] * n)]
    tab = []
    for side, stores in zip(placed, store):
        tab += [s.data_ptr() + 4 * p[1] if p is not None else 0 for p, s in zip(side, stores)]
        for p in side:
            tab += [p[2], p[3]] if p is not None else [0, 0]
    tab += [m.data_ptr() if m is not None else 0 for m in mdev]
    tab = torch.tensor(tab, dtype=torch.int64, device=dev)
    rows_d = torch.tensor(rows, dtype=torch.int32, device=dev)
    nbytes = int(L.ace_diag_hist_scratch_bytes(n, B, T, hw))
    assert nbytes == 2 * n * (16 * ((hw + 1023) // 1024) + 16)
    scratch = Guarded(torch.full((nbytes // 8,), float("nan"), dtype=torch.float64), dev)
    base = tab.data_ptr()
    rc = L.ace_diag_hist_window(base, base + 8 * n, base + 24 * n, base + 32 * n, rows_d.data_ptr(),
                                base + 48 * n if masks is not None else None, scratch.ptr, st.range.ptr, st.counts.ptr,
                                st.dropped.ptr, st.nrows, st.n_bins, n, B, T, hw, None)
    assert rc == expect, L.ace_diag_last_error().decode()
    torch.cuda.synchronize()
    scratch.read()
    for side, stores in zip(placed, store):
        for p, s in zip(side, stores):
            if p is not None:
                assert torch.equal(s.cpu().view(torch.int32), p[0].view(torch.int32)), "an input plane changed"
    if update_ref:
        for s, side in enumerate((gens, tgts)):
            for j, x in enumerate(side):
                if x is not None and 0 <= rows[j] < st.nrows:
                    keep = np.ones(hw, bool) if not masks or masks[j] is None else masks[j].numpy() == 0
                    st.ref[s][rows[j]].add(x.numpy()[:, :, keep])


def three_names(B, T, hw, g, scale=1.0, shift=0.0):
    """unit Gaussian, a 3e-5 scale and a surface pressure: ranges eleven orders of magnitude apart"""
    r = lambda: torch.randn(B, T, hw, generator=g)                                # noqa: E731
    return [(scale * r() + shift).float(), (3e-5 * scale * r() + 3e-5 * shift).float(), (1e5 + 900 * scale * r() + 900 * shift).float()]


@pytest.mark.parametrize("layout", ["contiguous", "odd"])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 5)])
@pytest.mark.parametrize("hw", [5 * 7, 9 * 18, 33 * 65, 16 * 72])      # below a wave, ragged, three chunks, and hw % 4 == 0 (float4 loads)
def test_shapes_layouts_and_bins(dev, hw, B, T, layout):
    g = torch.Generator().manual_seed(hw + B)
    mask = (torch.rand(hw, generator=g) < 0.25).to(torch.uint8)
    for n_bins in (8, 200):
        st = State(dev, 4, n_bins)
        for w, (scale, shift) in enumerate([(1.0, 0.0), (2.5, 1.0), (0.5, -6.0)]):           # doublings right, then left
            gens, tgts = three_names(B, T, hw, g, scale, shift), three_names(B, T, hw, g, 1.1 * scale, shift)
            window(st, gens, tgts, rows=[2, 0, 3], masks=[None, mask, None], layout=layout, seed=w)
        rng, cnt, drop = st.check()
        assert int(cnt[0, 2].sum()) == 3 * B * T * hw and int(cnt[1, 0].sum()) == 3 * B * T * int((mask == 0).sum())
        assert int(cnt[:, 1].sum()) == 0 and bool(rng[:, 1].isnan().all())                    # row 1 belongs to no plane


def test_golden_windows(dev):
    golden = torch.load(GOLDEN, weights_only=False)
    names = golden["names"]
    st = State(dev, 3, 200)
    masks = [golden["target"][0][n][0, 0].isnan().reshape(-1).to(torch.uint8) for n in names]
    for t, p in zip(golden["target"], golden["prediction"]):
        window(st, [p[n].reshape(2, 3, -1) for n in names], [t[n].reshape(2, 3, -1) for n in names], rows=[0, 1, 2], masks=masks)
    rng, cnt, _ = st.check()
    for i, n in enumerate(names):
        for s, source in enumerate(("prediction", "target")):
            assert torch.equal(cnt[s, i], golden["counts"][source][n]), (source, n)
            edges = np.linspace(float(rng[s, i, 0]), float(rng[s, i, 1]), 201)
            assert np.array_equal(edges, golden["edges"][source][n].numpy()), (source, n)


def test_repeated_doublings_left_and_right(dev):
    g = torch.Generator().manual_seed(5)
    st = State(dev, 1, 200)
    for w, (scale, shift) in enumerate([(1.0, 0.0), (1.0, 50.0), (1.0, -50.0), (50.0, 0.0)]):     # x50 jumps: six doublings in one update
        x = (scale * torch.randn(2, 2, 9 * 18, generator=g) + shift).float()
        window(st, [x], [(-x).contiguous()], rows=[0])
        assert st.ref[0][0].dropped == 0
    rng, cnt, _ = st.check()
    assert float(rng[0, 0, 1] - rng[0, 0, 0]) > 50 and int(cnt.sum()) == 2 * 4 * 4 * 162


@pytest.mark.parametrize("n_bins", [8, 200])
def test_values_on_the_edges(dev, n_bins):
    """every edge of the current range rounded to fp32 - lo, hi and the interior ones - and its two fp32 neighbours; an edge that
    rounds to outside the range doubles it, which the numpy twin does alike"""
    st = State(dev, 1, n_bins)
    first = torch.linspace(-3.0, 5.0, 70).reshape(1, 2, 35)
    window(st, [first], [first + 100.0], rows=[0])
    for toward in (None, float("inf"), float("-inf")):
        planes = []
        for s in range(2):
            e = torch.from_numpy(st.ref[s][0].edges).float()
            if toward is not None:
                e = torch.nextafter(e, torch.full_like(e, toward))
            planes.append(e.reshape(1, 3, -1))                     # n_bins + 1 is 9 or 201: three steps
        window(st, [planes[0]], [planes[1]], rows=[0])
    _, cnt, drop = st.check()
    assert int(drop.sum()) == 0 and int(cnt[0].sum()) == 70 + 3 * (n_bins + 1)


def test_zero_inflated_plane(dev):
    g = torch.Generator().manual_seed(11)
    hw, B, T = 33 * 65, 2, 3
    wet = torch.rand(B, T, hw, generator=g) < 0.05
    x = torch.where(wet, 3e-4 * torch.randn(B, T, hw, generator=g).abs() ** 3, torch.zeros(B, T, hw)).float()
    y = torch.where(wet.roll(7, -1), 2e-4 * torch.randn(B, T, hw, generator=g).abs() ** 3, torch.zeros(B, T, hw)).float()
    assert float((x == 0).float().mean()) >= 0.94
    st = State(dev, 1, 200)
    window(st, [x], [y], rows=[0])
    window(st, [2 * x], [y * 0], rows=[0])
    _, cnt, _ = st.check()
    assert int(cnt[0, 0].max()) > 0.9 * 2 * B * T * hw


def test_null_target_and_out_of_range_rows(dev):
    g = torch.Generator().manual_seed(2)
    B, T, hw = 2, 2, 162
    st = State(dev, 2, 8)
    gens, tgts = three_names(B, T, hw, g), three_names(B, T, hw, g)
    window(st, gens, [tgts[0], None, tgts[2]], rows=[1, 0, 7])                 # plane 1: generated side only; plane 2: nowhere
    window(st, gens, [tgts[0], None, tgts[2]], rows=[1, 0, -1])
    rng, cnt, drop = st.check()
    assert int(cnt[1, 0].sum()) == 0 and bool(rng[1, 0].isnan().all()) and int(cnt[0, 0].sum()) == 2 * B * T * hw
    assert int(drop.sum()) == 0


def test_dropped_windows_leave_the_state(dev):
    g = torch.Generator().manual_seed(3)
    B, T, hw = 1, 2, 35
    st = State(dev, 3, 200)
    gens, tgts = three_names(B, T, hw, g), three_names(B, T, hw, g)
    window(st, gens, tgts, rows=[0, 1, 2])
    before = st.read()
    bad = [x.clone() for x in gens]
    bad[0][0, 1, 17] = float("nan")
    bad[1][0, 0, 3] = float("-inf")
    bad[2][:] = 1e5                                                            # 1e5 +- 1e-6 is 1e5 in fp32: a degenerate range
    fresh = State(dev, 3, 200)
    window(fresh, bad, [torch.full_like(x, 1e5) for x in bad], rows=[0, 1, 2])
    rng, cnt, drop = fresh.check()
    assert bool(rng.isnan().all()) and int(cnt.sum()) == 0 and torch.equal(drop, torch.ones(2, 3, dtype=torch.int32))
    window(st, bad, tgts, rows=[0, 1, 2])
    rng, cnt, drop = st.check()
    # the constant 1e5 lies inside row 2's existing range, so there it is recorded; the non-finite windows are not
    assert torch.equal(cnt[0, :2], before[1][0, :2]) and torch.equal(rng[0, :2], before[0][0, :2])
    assert drop[0].tolist() == [1, 1, 0] and drop[1].tolist() == [0, 0, 0]
    masked = State(dev, 1, 200)                                                # a NaN under the mask is no reason to drop
    m = torch.zeros(hw, dtype=torch.uint8)
    m[17] = 1
    window(masked, [bad[0]], [gens[0]], rows=[0], masks=[m])
    _, cnt, drop = masked.check()
    assert int(drop.sum()) == 0 and int(cnt.sum()) == 2 * B * T * (hw - 1)


def test_two_runs_are_bitwise_equal(dev):
    outs = []
    for _ in range(2):
        g = torch.Generator().manual_seed(8)
        st = State(dev, 3, 200)
        for w in range(3):
            window(st, three_names(3, 5, 2145, g, 1.0 + w, w), three_names(3, 5, 2145, g, 1.0 + w, -w), rows=[0, 1, 2], layout="odd")
        outs.append(st.read())
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.int32 else a.view(torch.int64),
                           b.view(torch.int32) if b.dtype == torch.int32 else b.view(torch.int64))


@pytest.mark.parametrize("change,word", [
    (dict(n_bins=7), "n_bins"), (dict(n_bins=0), "n_bins"), (dict(n_bins=1026), "n_bins"), (dict(nplanes=-1), "nplanes"),
    (dict(nplanes=65536), "nplanes"), (dict(batch=0), "batch"), (dict(steps=0), "steps"), (dict(batch=4096, steps=1024), "batch * steps"),
    (dict(hw=0), "hw"), (dict(nrows=0), "nrows"), (dict(null=4), "null"), (dict(null=6), "null"), (dict(null=8), "null"),
    (dict(misalign=True), "aligned")])
def test_refusals(dev, change, word):
    L = lib()
    st = State(dev, 1, 8)
    x = torch.zeros(64, dtype=torch.float64, device=dev)
    a = dict(nrows=1, n_bins=8, nplanes=1, batch=1, steps=1, hw=4)
    a.update({k: v for k, v in change.items() if k in a})
    p = [x.data_ptr()] * 5 + [None, x.data_ptr(), st.range.ptr, st.counts.ptr, st.dropped.ptr]
    if "null" in change:
        p[change["null"]] = None
    if "misalign" in change:
        p[6] += 8
    rc = L.ace_diag_hist_window(*p, a["nrows"], a["n_bins"], a["nplanes"], a["batch"], a["steps"], a["hw"], None)
    msg = L.ace_diag_last_error().decode()
    assert rc == INVALID and word in msg and msg.startswith("ace_diag_hist_window"), (rc, msg)
    torch.cuda.synchronize()
    rng, cnt, drop = st.check()
    assert bool(rng.isnan().all())


def test_no_planes_is_a_no_op(dev):
    L = lib()
    assert L.ace_diag_hist_window(None, None, None, None, None, None, None, None, None, None, 1, 200, 0, 1, 1, 64800, None) == 0
    assert L.ace_diag_hist_scratch_bytes(0, 1, 1, 64800) == 0
    assert L.ace_diag_hist_scratch_bytes(40, 1, 40, 64800) == 2 * 40 * (16 * 64 + 16)
    assert L.ace_diag_hist_scratch_bytes(1, 0, 1, 5) == -1 and L.ace_diag_hist_scratch_bytes(1, 4096, 1024, 5) == -1
