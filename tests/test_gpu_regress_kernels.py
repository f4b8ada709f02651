"""csrc/regress.hip through the C ABI (ace_diag_regress_window) against tests/_regress_ref.py, the numpy statement of the header
contract that tests/test_regress_ref_cpu.py holds to the reference.

Bars.  maps: |got - ref| <= 1e-12 x sum|c x| per (side, row, map, pixel), the bar of the other diag kernels (the kernel follows the
stated order without contraction, so the difference is in fact 0 or one rounding of the final +=).  counts: ``torch.equal``.
fractions: |got - ref| <= 1e-12 x the number of (b, t) entries (each entry a ratio in [0, 1] of fp64 sums in another order).
Every output buffer (maps, counts, fractions, scratch) lies between guards, which must come back intact; the input planes must come
back unchanged; the scratch is pre-filled with NaN, so a partial that is read without having been written shows."""
import numpy as np
import pytest
import torch

import _regress_ref as R
from test_gpu_diag_kernels import INVALID, Guarded, dev, lib  # noqa: F401

pytestmark = pytest.mark.gpu

MAX_MAPS = 8


class State:
    """the persistent device accumulators of nrows rows between guards, and their numpy twins"""

    def __init__(self, dev, nrows, nmaps, hw):
        self.dev, self.nrows, self.nmaps, self.hw = dev, nrows, nmaps, hw
        self.maps = Guarded(torch.zeros(2, nrows, max(nmaps, 1), hw, dtype=torch.float64), dev)
        self.count = Guarded(torch.zeros(2, nrows, hw, dtype=torch.int64).view(torch.float64), dev)
        self.frac = Guarded(torch.zeros(2, nrows, dtype=torch.float64), dev)
        self.ref_maps = np.zeros((2, nrows, max(nmaps, 1), hw))
        self.ref_count = np.zeros((2, nrows, hw), np.int64)
        self.ref_frac = np.zeros((2, nrows))
        self.scale = np.zeros((2, nrows, max(nmaps, 1), hw))
        self.entries = 0

    def read(self):
        return (self.maps.read(), self.count.read().view(torch.int64).reshape(2, self.nrows, self.hw), self.frac.read())

    def check(self):
        maps, count, frac = self.read()
        with np.errstate(invalid="ignore"):
            err = np.abs(maps.numpy() - self.ref_maps)
            bad = ~(err <= 1e-12 * self.scale) & ~(np.isnan(maps.numpy()) & np.isnan(self.ref_maps))
        assert not bad.any(), ("maps", float(np.nanmax(err / np.maximum(self.scale, 1e-300))))
        assert torch.equal(count, torch.from_numpy(self.ref_count)), "counts"
        with np.errstate(invalid="ignore"):
            ferr = np.abs(frac.numpy() - self.ref_frac)
            ok = (ferr <= 1e-12 * max(self.entries, 1)) | (np.isnan(frac.numpy()) & np.isnan(self.ref_frac))
        assert ok.all(), ("fractions", ferr)
        return maps, count, frac


def place(data, layout, g):
    """(storage, offset in floats, sample stride, step stride) of a (B, T, hw) field"""
    B, T, hw = data.shape
    if layout == "contiguous":
        return data.reshape(-1).clone(), 0, T * hw, hw
    pitch = hw + 3                                      # "odd": one float past a 16-byte boundary, rows of a strided view
    s = torch.randn(1 + B * T * pitch, generator=g) * 1e30
    s[1:].view(B, T, pitch)[:, :, :hw] = data
    return s, 1, T * pitch, pitch


def window(st, gens, tgts, rows, coef=None, slot=None, eps=None, weights=None, wrows=None, t_begin=0, layout="contiguous", seed=0,
           expect=0, nmaps=None, update_ref=True):
    """one ace_diag_regress_window on (B, T, hw) CPU fields; the numpy twin gets the same window"""
    L, dev = lib(), st.dev
    g = torch.Generator().manual_seed(seed)
    n = len(gens)
    B, T, hw = gens[0].shape
    nmaps = st.nmaps if nmaps is None else nmaps
    placed = [[place(x, layout, g) if x is not None else None for x in side] for side in (gens, tgts)]
    store = [[p[0].to(dev) if p is not None else None for p in side] for side in placed]
    tab = []
    for side, stores in zip(placed, store):
        tab += [s.data_ptr() + 4 * p[1] if p is not None else 0 for p, s in zip(side, stores)]
        for p in side:
            tab += [p[2], p[3]] if p is not None else [0, 0]
    tab = torch.tensor(tab, dtype=torch.int64, device=dev)
    rows_d = torch.tensor(rows, dtype=torch.int32, device=dev)
    nterms = 0 if coef is None else coef.shape[0]
    coef_d = torch.from_numpy(np.ascontiguousarray(coef)).to(dev) if nterms else None
    slot_d = torch.from_numpy(np.ascontiguousarray(slot, dtype=np.int32)).to(dev) if nterms else None
    ind = eps is not None
    eps_d = torch.tensor(eps, dtype=torch.float32, device=dev) if ind else None
    w_d = torch.cat([torch.zeros(1), torch.from_numpy(weights).reshape(-1)]).to(dev)[1:] if ind else None    # off a 16-byte boundary
    wrows_d = torch.tensor(wrows, dtype=torch.int32, device=dev) if ind else None
    ndoubles = int(L.ace_diag_regress_partial_doubles(n, B, T, hw))
    assert ndoubles == 2 * n * 4 * ((hw + 1023) // 1024) * (B * T + 1)
    scratch = Guarded(torch.full((ndoubles,), float("nan"), dtype=torch.float64), dev)
    base = tab.data_ptr()
    rc = L.ace_diag_regress_window(base, base + 8 * n, base + 24 * n, base + 32 * n, rows_d.data_ptr(),
                                   coef_d.data_ptr() if nterms else None, slot_d.data_ptr() if nterms else None, st.maps.ptr,
                                   eps_d.data_ptr() if ind else None, wrows_d.data_ptr() if ind else None,
                                   w_d.data_ptr() if ind else None, weights.shape[0] if ind else 0, scratch.ptr, st.count.ptr,
                                   st.frac.ptr, st.nrows, nterms, nmaps, t_begin, n, B, T, hw, None)
    assert rc == expect, L.ace_diag_last_error().decode()
    torch.cuda.synchronize()
    scratch.read()
    for side, stores in zip(placed, store):
        for p, s in zip(side, stores):
            if p is not None:
                assert torch.equal(s.cpu().view(torch.int32), p[0].view(torch.int32)), "an input plane changed"
    if update_ref and rc == 0:
        planes = [[x.numpy() if x is not None else None for x in side] for side in (gens, tgts)]
        R.regress_window(planes[0], planes[1], rows, st.nrows, coef=coef, slot=slot, nmaps=nmaps, maps=st.ref_maps, eps=eps,
                         weights=weights, wrows=wrows, below_count=st.ref_count, below_frac=st.ref_frac, t_begin=t_begin)
        if nterms:
            for s in (0, 1):
                st.scale[s, :, :nmaps] += R.map_scale(planes[s], rows, st.nrows, coef, np.asarray(slot), nmaps, t_begin)
        st.entries += B * max(T - t_begin, 0)


def fields(B, T, hw, g, n=3):
    """a unit Gaussian, a surface-pressure-like field and a zero-inflated one"""
    r = lambda: torch.randn(B, T, hw, generator=g)                                # noqa: E731
    wet = torch.rand(B, T, hw, generator=g) < 0.3
    return [r().float(), (1e5 + 900 * r()).float(), torch.where(wet, 3e-4 * r().abs() ** 3, torch.zeros(())).float()][:n]


def terms(B, T, g, with_index=True):
    """the evaluator's terms: 1 -> map 0, years -> map 1, an index -> map 2 + b"""
    years = 14.0 + 0.25 * np.arange(T)[None] + 3.5 * np.arange(B)[:, None]
    coef = [np.ones((B, T)), years]
    slot = [[0] * B, [1] * B]
    if with_index:
        coef.append(torch.randn(B, T, generator=g, dtype=torch.float64).numpy())
        slot.append([2 + b for b in range(B)])
    return np.stack(coef), np.array(slot)


def area(hw, zero=()):
    w = np.cos(np.linspace(-1.5, 1.5, hw)).astype(np.float32)
    for a, b in zero:
        w[a:b] = 0.0
    return w[None]


EPS3 = [0.25, 1e5, 0.0]


@pytest.mark.parametrize("layout", ["contiguous", "odd"])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 4)])
@pytest.mark.parametrize("hw", [5 * 13, 9 * 57, 33 * 65, 16 * 72])   # half a wave, a ragged workgroup, three tiles, hw % 4 == 0
def test_shapes_and_layouts(dev, hw, B, T, layout):
    g = torch.Generator().manual_seed(hw + B)
    st = State(dev, 4, 2 + B, hw)
    coef, slot = terms(B, T, g)
    w = area(hw, zero=[(3, 9)])
    for k in range(2):                                                          # a second call adds to the first
        window(st, fields(B, T, hw, g), fields(B, T, hw, g), [2, 0, 3], coef, slot, eps=EPS3, weights=w, wrows=[0, 0, 0],
               layout=layout, seed=k)
    maps, count, frac = st.check()
    assert not maps[:, 1].any() and not count[:, 1].any() and not frac[:, 1].any()            # row 1 belongs to no plane
    assert 0 < float(frac[0, 3]) < 2 * B * T and int(count[0, 3].max()) <= 2 * B * T and float(maps[0, 2, 0].abs().max()) > 0


def test_one_degree(dev):
    g = torch.Generator().manual_seed(1)
    B, T, hw = 1, 4, 180 * 360
    st = State(dev, 2, 3, hw)
    coef, slot = terms(B, T, g)
    window(st, fields(B, T, hw, g, 2), fields(B, T, hw, g, 2), [1, 0], coef, slot, eps=EPS3[:2], weights=area(hw), wrows=[0, 0], t_begin=1)
    _, count, frac = st.check()
    assert int(count.max()) == 3 and 0 < float(frac[0, 1]) < 3


def test_t_begin_past_the_window_changes_nothing(dev):
    g = torch.Generator().manual_seed(2)
    B, T, hw = 3, 1, 9 * 57
    st = State(dev, 3, 2 + B, hw)
    coef, slot = terms(B, T, g)
    window(st, fields(B, T, hw, g), fields(B, T, hw, g), [0, 1, 2], coef, slot, eps=EPS3, weights=area(hw), wrows=[0, 0, 0], t_begin=1)
    maps, count, frac = st.check()
    assert not maps.any() and not count.any() and not frac.any()
    assert torch.equal(maps.view(torch.int64), torch.zeros_like(maps).view(torch.int64))        # not even a -0


def test_null_target_bad_rows_and_idle_slots(dev):
    g = torch.Generator().manual_seed(3)
    B, T, hw = 3, 4, 9 * 57
    st = State(dev, 2, 2 + B, hw)
    coef, slot = terms(B, T, g)
    slot[2, 1] = -1                                                             # sample 1 has no index series
    slot[1, 2] = 99                                                             # any value outside [0, nmaps) is "none"
    gens, tgts = fields(B, T, hw, g), fields(B, T, hw, g)
    for rows in ([1, 0, 7], [1, 0, -1]):
        window(st, gens, [tgts[0], None, tgts[2]], rows, coef, slot, eps=EPS3, weights=area(hw), wrows=[0, 5, 0])
    maps, count, frac = st.check()
    assert not maps[1, 0].any() and not count[1, 0].any()                       # plane 1: the generated side only
    assert not maps[:, :, 3].any() and maps[0, 0, 2].any()
    assert not count[0, 0].any() and float(frac[0, 0]) == 0 and count[0, 1].any()            # a weight row out of range: no indicator
    assert maps[0, 0, 0].any()                                                  # ... its linear terms are still produced


def test_the_indicator_alone_and_the_terms_alone(dev):
    g = torch.Generator().manual_seed(4)
    B, T, hw = 1, 4, 33 * 65
    coef, slot = terms(B, T, g)
    gens, tgts = fields(B, T, hw, g), fields(B, T, hw, g)
    st = State(dev, 3, 0, hw)
    window(st, gens, tgts, [0, 1, 2], eps=EPS3, weights=area(hw), wrows=[0, 0, 0], nmaps=0)
    maps, count, _ = st.check()
    assert not maps.any() and count.any()
    st = State(dev, 3, 3, hw)
    window(st, gens, tgts, [0, 1, 2], coef, slot)
    maps, count, frac = st.check()
    assert maps.any() and not count.any() and not frac.any()
    st = State(dev, 3, 3, hw)                                                  # neither: nothing to do
    window(st, gens, tgts, [0, 1, 2])
    maps, count, frac = st.check()
    assert not maps.any() and not count.any()


def test_the_cap_on_maps(dev):
    g = torch.Generator().manual_seed(5)
    B, T, hw = 2, 4, 9 * 57
    gens, tgts = fields(B, T, hw, g, 1), fields(B, T, hw, g, 1)
    coef = torch.randn(MAX_MAPS // 2, B, T, generator=g, dtype=torch.float64).numpy()
    slot = np.arange(MAX_MAPS).reshape(MAX_MAPS // 2, B)                        # every map of the cap is fed
    st = State(dev, 1, MAX_MAPS, hw)
    window(st, gens, tgts, [0], coef, slot)
    maps, _, _ = st.check()
    assert all(maps[0, 0, m].any() for m in range(MAX_MAPS))
    st = State(dev, 1, MAX_MAPS + 1, hw)
    window(st, gens, tgts, [0], coef, slot, eps=[0.0], weights=area(hw), wrows=[0], expect=INVALID, nmaps=MAX_MAPS + 1)
    msg = lib().ace_diag_last_error().decode()
    assert msg.startswith("ace_diag_regress_window") and "nmaps" in msg
    maps, count, frac = st.check()
    assert not maps.any() and not count.any() and not frac.any()


def test_nan_planes_zero_weights_and_values_on_eps(dev):
    B, T, hw = 2, 2, 9 * 57
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, T, hw, generator=g).float()
    eps = float(x[0, 0, 200])                                                  # eps equal to field values: <= counts them
    x[1, 1, 300:320] = eps
    x[0, 1, 100:110] = float("nan")
    nan = torch.full((B, T, hw), float("nan"))
    w = area(hw, zero=[(0, 57)])                                               # a whole row of pixels of weight 0
    x[:, :, :57] = -50.0                                                       # ... all of them below eps
    st = State(dev, 2, 2, hw)
    coef = np.stack([np.ones((B, T)), np.zeros((B, T))])
    window(st, [x, nan], [nan, x], [0, 1], coef, np.array([[0, 0], [1, 1]]), eps=[eps, eps], weights=w, wrows=[0, 0])
    maps, count, frac = st.check()
    assert not count[0, 1].any() and not count[1, 0].any() and float(frac[0, 1]) == 0       # a plane of NaNs: counts stay 0
    assert bool(maps[0, 1].isnan().all()) and bool(maps[0, 0, 0, 100:110].isnan().all()) and bool(maps[0, 0, 1, 100:110].isnan().all())
    assert int(count[0, 0, 200]) >= 1 and int(count[0, 0, 300:320].min()) >= 1 and int(count[0, 0, 100:110].max()) <= 3
    assert count[0, 0, :57].eq(4).all()                                        # counted per cell ...
    live = torch.from_numpy(w[0]) != 0
    below = ((x <= eps) & live).double()
    want = float((below * torch.from_numpy(w[0]).double()).sum(-1).div(float(w[0].astype(np.float64).sum())).sum())
    assert abs(float(frac[0, 0]) - want) <= 1e-12 * 4 and 0 < want < 4          # ... and out of the fraction
    allzero = State(dev, 1, 0, hw)                                             # no pixel of non-zero weight: 0 / 0
    window(allzero, [x], [x], [0], eps=[eps], weights=np.zeros((1, hw), np.float32), wrows=[0], nmaps=0)
    assert bool(allzero.frac.read().isnan().all())


def test_two_runs_are_bitwise_equal(dev):
    outs = []
    for _ in range(2):
        g = torch.Generator().manual_seed(8)
        B, T, hw = 3, 4, 33 * 65
        st = State(dev, 3, 2 + B, hw)
        coef, slot = terms(B, T, g)
        for k in range(2):
            window(st, fields(B, T, hw, g), fields(B, T, hw, g), [0, 1, 2], coef, slot, eps=EPS3, weights=area(hw), wrows=[0, 0, 0],
                   layout="odd", t_begin=k)
        outs.append(st.read())
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("change,word", [
    (dict(nplanes=-1), "nplanes"), (dict(nplanes=65536), "nplanes"), (dict(nmaps=-1), "nmaps"), (dict(nmaps=9), "nmaps"),
    (dict(nterms=65), "nterms"), (dict(nterms=1, nmaps=0), "nterms"), (dict(batch=0), "batch"), (dict(steps=0), "steps"),
    (dict(hw=0), "hw"), (dict(nrows=0), "nrows"), (dict(t_begin=-1), "t_begin"), (dict(null=0), "null"), (dict(null=4), "null"),
    (dict(null=5), "null"), (dict(null=7), "null"), (dict(null=9), "null"), (dict(null=12), "null"), (dict(null=13), "null")])
def test_refusals(dev, change, word):
    L = lib()
    st = State(dev, 1, 2, 4)
    x = torch.zeros(64, dtype=torch.float64, device=dev)
    a = dict(nrows=1, nterms=1, nmaps=2, t_begin=0, nplanes=1, batch=1, steps=1, hw=4)
    a.update({k: v for k, v in change.items() if k in a})
    p = [x.data_ptr()] * 7 + [st.maps.ptr] + [x.data_ptr()] * 3 + [1, x.data_ptr(), st.count.ptr, st.frac.ptr]
    if "null" in change:
        p[change["null"]] = None
    rc = L.ace_diag_regress_window(*p, a["nrows"], a["nterms"], a["nmaps"], a["t_begin"], a["nplanes"], a["batch"], a["steps"], a["hw"], None)
    msg = L.ace_diag_last_error().decode()
    assert rc == INVALID and word in msg and msg.startswith("ace_diag_regress_window"), (rc, msg)
    torch.cuda.synchronize()
    maps, count, frac = st.check()
    assert not maps.any() and not count.any() and not frac.any()


def test_no_planes_is_a_no_op(dev):
    L = lib()
    assert L.ace_diag_regress_window(*([None] * 11), 0, None, None, None, 1, 3, 3, 0, 0, 1, 40, 64800, None) == 0
    assert L.ace_diag_regress_partial_doubles(0, 1, 1, 64800) == 0
    assert L.ace_diag_regress_partial_doubles(50, 1, 40, 64800) == 2 * 50 * 4 * 64 * 41
    assert L.ace_diag_regress_partial_doubles(1, 0, 1, 5) == -1 and L.ace_diag_regress_partial_doubles(65536, 1, 1, 5) == -1
