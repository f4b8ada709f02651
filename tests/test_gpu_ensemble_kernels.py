"""csrc/ensemble.hip through the C ABI (ace_diag_ensemble_step) against tests/_ensemble_ref.py, the numpy statement of the header
contract that tests/test_ensemble_ref_cpu.py holds to the reference.

Bar.  |got - ref| <= 1e-12 x the largest finite |ref| of each (slot, map, row), the bar of the other diag kernels: every sum is
fp64 in the stated order without contraction, so only the square root and the divisions can differ, by an ulp.  NaN and infinity
have to sit in the same places.  The maps and the ``seen`` flags lie between guards, which must come back intact; the input planes
must come back unchanged."""
import numpy as np
import pytest
import torch

import _ensemble_ref as R
from test_gpu_diag_kernels import INVALID, Guarded, dev, lib  # noqa: F401
from test_gpu_regress_kernels import place

pytestmark = pytest.mark.gpu

MAX_MEMBERS = 32


class State:
    """the persistent device maps and flags of nslots x nrows between guards, and their numpy twins"""

    def __init__(self, dev, nslots, nrows, hw):
        self.dev, self.nslots, self.nrows, self.hw = dev, nslots, nrows, hw
        self.maps = Guarded(torch.zeros(nslots, 4, nrows, hw, dtype=torch.float64), dev)
        self.nflags = nslots * nrows + (nslots * nrows) % 2
        self.seen = Guarded(torch.zeros(self.nflags, dtype=torch.int32).view(torch.float64), dev)
        self.ref_maps = np.zeros((nslots, 4, nrows, hw))
        self.ref_seen = np.zeros((nslots, nrows), np.int32)

    def read(self):
        seen = self.seen.read().view(torch.int32)[:self.nslots * self.nrows].reshape(self.nslots, self.nrows)
        return self.maps.read(), seen

    def check(self):
        maps, seen = self.read()
        got, ref = maps.numpy(), self.ref_maps
        assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN in other places"
        inf = np.isinf(ref)
        assert np.array_equal(got[inf], ref[inf]), "infinities differ"
        finite = np.where(np.isfinite(ref), ref, 0.0)
        scale = np.abs(finite).max(axis=-1, keepdims=True)
        with np.errstate(invalid="ignore"):
            err = np.where(np.isfinite(ref), np.abs(got - ref), 0.0)
        worst = float((err / np.maximum(scale, 1e-300)).max())
        print(f"ENSKERN worst |got - ref| / max|ref| = {worst:.3e}")
        assert (err <= 1e-12 * scale).all(), worst
        assert np.array_equal(seen.numpy(), self.ref_seen), "seen flags"
        return maps, seen


def step(st, gens, tgts, rows, slot, t, n_ic, E, layout="contiguous", seed=0, expect=0, steps=None, nslots=None, update_ref=True):
    """one ace_diag_ensemble_step on (n_ic * E, T, hw) CPU fields; the numpy twin gets the same call"""
    L, dev = lib(), st.dev
    g = torch.Generator().manual_seed(seed)
    n = len(gens)
    _, T, hw = gens[0].shape
    placed = [[place(x, layout, g) if x is not None else None for x in side] for side in (gens, tgts)]
    store = [[p[0].to(dev) if p is not None else None for p in side] for side in placed]
    tab = []
    for side, stores in zip(placed, store):
        tab += [s.data_ptr() + 4 * p[1] if p is not None else 0 for p, s in zip(side, stores)]
        for p in side:
            tab += [p[2], p[3]] if p is not None else [0, 0]
    tab = torch.tensor(tab, dtype=torch.int64, device=dev)
    rows_d = torch.tensor(rows, dtype=torch.int32, device=dev)
    base = tab.data_ptr()
    rc = L.ace_diag_ensemble_step(base, base + 8 * n, base + 24 * n, base + 32 * n, rows_d.data_ptr(), st.maps.ptr, st.seen.ptr,
                                  st.nrows, slot, st.nslots if nslots is None else nslots, R.PAIR_WEIGHT, t, n, n_ic, E,
                                  T if steps is None else steps, hw, None)
    assert rc == expect, L.ace_diag_last_error().decode()
    torch.cuda.synchronize()
    for side, stores in zip(placed, store):
        for p, s in zip(side, stores):
            if p is not None:
                assert torch.equal(s.cpu().view(torch.int32), p[0].view(torch.int32)), "an input plane changed"
    if update_ref and rc == 0:
        planes = [[x.numpy() if x is not None else None for x in side] for side in (gens, tgts)]
        R.ensemble_step(planes[0], planes[1], rows, st.ref_maps, st.ref_seen, slot, t, n_ic, E)


def fields(n_ic, E, T, hw, g, n=2):
    """per name a (gen, target) pair: members scattered round a value their initial condition shares, at two magnitudes"""
    gens, tgts = [], []
    for k in range(n):
        mean, spread = ((0.0, 1.0), (1e5, 900.0), (3e-4, 1e-4))[k % 3]
        shared = torch.randn(n_ic, 1, T, hw, generator=g)
        gens.append((mean + spread * (shared + 0.7 * torch.randn(n_ic, E, T, hw, generator=g))).float().reshape(n_ic * E, T, hw))
        tgts.append((mean + spread * (shared + 0.5 * torch.randn(n_ic, E, T, hw, generator=g))).float().reshape(n_ic * E, T, hw))
    return gens, tgts


@pytest.mark.parametrize("hw,E,n_ic,layout,T,t", [
    (35, 5, 3, "contiguous", 1, 0),                     # fewer pixels than one thread row, not a multiple of 4
    (1024 + 4 + 3, 3, 1, "odd", 3, 1),                  # two chunks, a ragged tail, a scalar tail; no 16-byte loads; the middle step
    (4 * 1024, 8, 1, "contiguous", 2, 1),               # aligned planes: 16-byte loads
    (35, 2, 3, "odd", 1, 0),                            # the fewest members
    (1024 + 4 + 3, 12, 1, "contiguous", 1, 0),          # the 16-member bucket
    (35, 17, 1, "contiguous", 1, 0),                    # the largest bucket, its first count
    (1026, 20, 2, "contiguous", 2, 1),                  # the largest bucket on even, 8-byte aligned planes: 8-byte loads
    (1024 + 4 + 3, MAX_MEMBERS, 3, "odd", 3, 1),        # the most members: 2 pixels per thread, three chunks of 512
])
def test_maps_follow_the_contract(dev, hw, E, n_ic, layout, T, t):
    g = torch.Generator().manual_seed(hw + E)
    gens, tgts = fields(n_ic, E, T, hw, g)
    st = State(dev, 1, 2, hw)
    step(st, gens, tgts, [1, 0], 0, t, n_ic, E, layout=layout)
    maps, seen = st.check()
    assert seen.tolist() == [[1, 1]]
    assert bool((maps[0, 3] > 0).all())


def test_null_target_row_out_of_range_two_calls_and_two_slots(dev):
    hw, E, n_ic = 35, 5, 3
    g = torch.Generator().manual_seed(3)
    gens, tgts = fields(n_ic, E, 2, hw, g, n=4)
    st = State(dev, 2, 3, hw)
    step(st, gens, [tgts[0], None, tgts[2], tgts[3]], [0, 1, -1, 3], 0, 0, n_ic, E)      # plane 1: no target; 2 and 3: no row
    maps, seen = st.check()
    assert bool((maps[0, :, 1:] == 0).all()) and bool((maps[1] == 0).all()) and seen.tolist() == [[1, 0, 0], [0, 0, 0]]
    step(st, gens, tgts, [0, 1, 2, 3], 0, 1, n_ic, E, seed=1)                             # a second record into slot 0
    step(st, gens[:2], tgts[:2], [2, 0], 1, 1, n_ic, E, seed=2)                           # and another entry's slot
    maps, seen = st.check()
    assert seen.tolist() == [[1, 1, 1], [1, 0, 1]] and bool((maps[1, :, 1] == 0).all())


def test_nan_infinity_identical_members_and_seen(dev):
    hw, E, n_ic = 1031, 5, 2
    g = torch.Generator().manual_seed(5)
    gens, tgts = fields(n_ic, E, 1, hw, g, n=3)
    gens[0][3, 0, 7] = float("nan")                     # one member at one pixel
    tgts[0][6, 0, 1030] = float("nan")
    gens[0][1, 0, 100] = float("inf")
    tgts[0][2, 0, 200] = float("-inf")
    gens[1] = gens[1].reshape(n_ic, E, 1, hw)[:, :1].expand(n_ic, E, 1, hw).reshape(n_ic * E, 1, hw).contiguous()      # identical members
    tgts[2][:] = float("nan")                           # a target that is NaN everywhere: never seen
    st = State(dev, 1, 3, hw)
    step(st, gens, tgts, [0, 1, 2], 0, 0, n_ic, E, layout="odd")
    maps, seen = st.check()
    assert seen.tolist() == [[1, 1, 0]]
    assert bool(maps[0, :, 0, 7].isnan().all()) and bool(maps[0, :, 0, 1030].isnan()[:3].all())
    assert torch.equal(maps[0, 3, 1].view(torch.int64), torch.zeros(hw, dtype=torch.int64))      # variance bitwise +0
    assert bool((maps[0, 2, 1] > 0).all())                                                       # so mse - var / E is the mse
    assert bool(maps[0, :3, 2].isnan().all()) and bool((maps[0, 3, 2] > 0).all())


def test_prescribed_pixels_have_zero_spread_and_zero_error(dev):
    hw, E, n_ic = 35, 8, 2
    g = torch.Generator().manual_seed(8)
    gens, tgts = fields(n_ic, E, 1, hw, g, n=2)
    base = tgts[1].reshape(n_ic, E, 1, hw)[:, :1, :, 10:20].expand(n_ic, E, 1, 10).reshape(n_ic * E, 1, 10).clone()
    gens[1][:, :, 10:20] = base                         # every member equals the target there
    tgts[1][:, :, 10:20] = base
    st = State(dev, 1, 2, hw)
    step(st, gens, tgts, [0, 1], 0, 0, n_ic, E)
    maps, _ = st.check()
    assert bool((maps[0, :, 1, 10:20] == 0).all())


@pytest.mark.parametrize("kw,message", [
    (dict(E=1), "2 <= n_members <= 32"), (dict(E=MAX_MEMBERS + 1), "2 <= n_members <= 32"),
    (dict(t=-1), "0 <= t < steps"), (dict(t=2), "0 <= t < steps"),
    (dict(slot=-1), "0 <= slot < nslots"), (dict(slot=2), "0 <= slot < nslots"),
    (dict(n_ic=0), "n_ic >= 1"),
])
def test_refusals(dev, kw, message):
    hw = 35
    g = torch.Generator().manual_seed(1)
    gens, tgts = fields(1, 2, 2, hw, g, n=1)
    st = State(dev, 2, 1, hw)
    args = dict(slot=0, t=0, n_ic=1, E=2)
    args.update(kw)
    step(st, gens, tgts, [0], args["slot"], args["t"], args["n_ic"], args["E"], expect=INVALID)
    assert message in lib().ace_diag_last_error().decode()
    maps, seen = st.check()
    assert bool((maps == 0).all()) and not seen.any()


def test_no_planes_is_a_no_op(dev):
    st = State(dev, 1, 1, 35)
    rc = lib().ace_diag_ensemble_step(None, None, None, None, None, st.maps.ptr, st.seen.ptr, 1, 0, 1, R.PAIR_WEIGHT, 0, 0, 1, 2, 1, 35, None)
    assert rc == 0
    torch.cuda.synchronize()
    st.check()


def test_bitwise_repeatable(dev):
    hw, E, n_ic = 1031, 8, 3
    runs = []
    for _ in range(2):
        g = torch.Generator().manual_seed(11)
        gens, tgts = fields(n_ic, E, 2, hw, g, n=3)
        st = State(dev, 1, 3, hw)
        step(st, gens, tgts, [2, 0, 1], 0, 1, n_ic, E, layout="odd", update_ref=False)
        step(st, gens, tgts, [2, 0, 1], 0, 0, n_ic, E, layout="odd", seed=1, update_ref=False)
        runs.append(st.read())
    assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64)) and torch.equal(runs[0][1], runs[1][1])
