"""csrc/video.hip through the C ABI (ace_diag_video_window) against tests/_video_ref.py, the numpy statement of the header contract
that tests/test_video_ref_cpu.py holds to the reference.

Bar: equality.  The kernel sums in fp64 in sample order with rounded products and divides in IEEE fp64, as the statement does:
the five fp64 channels agree bit for bit wherever they are not NaN and are NaN in the same places; the two extrema agree as
values (the sign of a zero and the payload of a NaN are not specified).  Every buffer lies between guards, which must come back
intact, and starts from a sentinel, so a slot that should have been written and was not shows, as does one that should have been
left alone; the input planes must come back unchanged."""
import numpy as np
import pytest
import torch

import _video_ref as R
from test_gpu_diag_kernels import INVALID, Guarded, dev, lib  # noqa: F401
from test_gpu_regress_kernels import place
from test_gpu_timeseg_kernels import Guarded32

pytestmark = pytest.mark.gpu

SENT = -12345.0                                      # pre-fill of the accumulators
DEPTH = 4                                            # csrc/video.hip: samples whose loads are in flight ahead of the adds


def lay(data, layout, g):
    """(storage, offset in floats, sample stride, step stride) of a (B, T, hw) field"""
    B, T, hw = data.shape
    if layout == "everysecond":                         # every second step of a (B, 2 T, hw) buffer
        s = torch.randn(B, 2 * T, hw, generator=g) * 1e30
        s[:, ::2] = data
        return s.reshape(-1), 0, 2 * T * hw, 2 * hw
    if layout == "permuted":                            # a (T, B, hw) buffer seen as (B, T, hw)
        return data.permute(1, 0, 2).contiguous().reshape(-1), 0, hw, B * hw
    return place(data, layout, g)


class State:
    """the three accumulators on the device between guards, and their numpy twins"""

    def __init__(self, dev, nrows, n_time, hw, extended=True, fill=SENT):
        self.dev, self.nrows, self.n_time, self.hw, self.extended = dev, nrows, n_time, hw, extended
        self.ref = [np.full((c, nrows, n_time, hw), fill, dt) for c, dt in ((2, np.float64), (3, np.float64), (2, np.float32))]
        self.bufs = [Guarded(torch.from_numpy(self.ref[0]), dev), Guarded(torch.from_numpy(self.ref[1]), dev),
                     Guarded32(torch.from_numpy(self.ref[2]), dev)]

    def window(self, gens, tgts, rows, t0, assign, layout="contiguous", expect=0, seed=0, **override):
        """one ace_diag_video_window on (B, T, hw) CPU fields (a target may be None); the twin gets the same window"""
        L, dev = lib(), self.dev
        g = torch.Generator().manual_seed(seed)
        B, T, hw = gens[0].shape
        placed = [[lay(x, layout, g) if x is not None else None for x in side] for side in (gens, tgts)]
        store = [[p[0].to(dev) if p is not None else None for p in side] for side in placed]
        tab = []
        for side, stores in zip(placed, store):
            tab += [s.data_ptr() + 4 * p[1] if p is not None else 0 for p, s in zip(side, stores)]
            for p in side:
                tab += [p[2], p[3]] if p is not None else [0, 0]
        tab = torch.tensor(tab, dtype=torch.int64, device=dev)
        rows_d = torch.tensor(rows, dtype=torch.int32, device=dev)
        n, base = len(gens), tab.data_ptr()
        a = dict(mean=self.bufs[0].ptr, sq=self.bufs[1].ptr if self.extended else None, err=self.bufs[2].ptr if self.extended else None,
                 nrows=self.nrows, n_time=self.n_time, t0=t0, assign=int(assign), nplanes=n, batch=B, steps=T, hw=hw)
        a.update(override)
        rc = L.ace_diag_video_window(base, base + 8 * n, base + 24 * n, base + 32 * n, rows_d.data_ptr(), a["mean"], a["sq"], a["err"],
                                     a["nrows"], a["n_time"], a["t0"], a["assign"], a["nplanes"], a["batch"], a["steps"], a["hw"], None)
        assert rc == expect, L.ace_diag_last_error().decode()
        torch.cuda.synchronize()
        for side, stores in zip(placed, store):
            for p, s in zip(side, stores):
                assert p is None or torch.equal(s.cpu().view(torch.int32), p[0].view(torch.int32)), "an input plane changed"
        if rc == 0 and a["nplanes"]:
            m = a["nplanes"]
            np_ = lambda side: [None if x is None else x.numpy() for x in side[:m]]      # noqa: E731
            R.video_window(np_(gens), np_(tgts), rows[:m], self.ref[0], self.ref[1] if self.extended else None,
                           self.ref[2] if self.extended else None, t0, assign=bool(assign))
        return self

    def read(self):
        return [b.read().numpy() for b in self.bufs]                           # the guards are checked here

    def check(self, what=""):
        got = self.read()
        for c, name in ((0, "mean"), (1, "sq")):
            nan = np.isnan(self.ref[c])
            assert np.array_equal(np.isnan(got[c]), nan), (what, name, "NaN pattern")
            assert np.array_equal(got[c][~nan].view(np.int64), self.ref[c][~nan].view(np.int64)), (what, name)
        assert np.array_equal(got[2], self.ref[2], equal_nan=True), (what, "err")
        return got


def fields(B, T, hw, g, n=2):
    """n generated planes (a unit Gaussian, a temperature-like field, ...) and their targets"""
    gens = [(torch.randn(B, T, hw, generator=g) if i % 2 == 0 else (280 + 15 * torch.randn(B, T, hw, generator=g)).float())
            for i in range(n)]
    return gens, [(x + 2 * torch.randn(B, T, hw, generator=g)).float() for x in gens]


@pytest.mark.parametrize("hw", [1, 3, 255, 1024, 1025, 2051])
@pytest.mark.parametrize("layout", ["contiguous", "odd"])
def test_sizes_and_base_offsets(dev, hw, layout):
    g = torch.Generator().manual_seed(hw)
    B, T, n_time = 3, 3, 5
    gens, tgts = fields(B, T, hw, g)
    st = State(dev, 2, n_time, hw).window(gens, tgts, [1, 0], 1, True, layout)
    st.window(*fields(B, T, hw, g), [0, 1], 1, False, layout).check((hw, layout))
    got = st.read()
    assert all(np.all(x[:, :, [0, 4]] == SENT) and not np.any(x[:, :, 1:4] == SENT) for x in got)


@pytest.mark.parametrize("B", [1, 2, 3, DEPTH - 1, DEPTH, DEPTH + 1, 2 * DEPTH + 1])
@pytest.mark.parametrize("T", [1, 3])
def test_batch_around_the_load_depth_and_both_ends_of_the_time_axis(dev, B, T):
    g = torch.Generator().manual_seed(10 * B + T)
    hw, n_time = 1025, 7
    st = State(dev, 2, n_time, hw)
    for t0 in (0, n_time - T):
        st.window(*fields(B, T, hw, g), [0, 1], t0, True, "odd" if B % 2 else "contiguous")
        st.window(*fields(B, T, hw, g), [1, 0], t0, False)
    st.check((B, T))


@pytest.mark.parametrize("layout", ["everysecond", "permuted"])
@pytest.mark.parametrize("hw", [1024, 1025])
def test_strided_views(dev, layout, hw):
    g = torch.Generator().manual_seed(3)
    B, T = 3, 3
    State(dev, 2, 4, hw).window(*fields(B, T, hw, g), [0, 1], 1, True, layout).window(*fields(B, T, hw, g), [0, 1], 0, False, layout).check(layout)


@pytest.mark.parametrize("extended", [True, False])
def test_null_target_rows_out_of_range_and_permuted_rows(dev, extended):
    g = torch.Generator().manual_seed(4)
    B, T, hw, nrows = 3, 2, 1030, 3
    gens, tgts = fields(B, T, hw, g, n=5)
    tgts[1] = None
    rows = [2, 0, -1, 1, nrows]                          # permuted, with one plane below and one above the range
    st = State(dev, nrows, 3, hw, extended).window(gens, tgts, rows, 1, True)
    got = st.window(gens, tgts, rows, 1, False).check(extended)
    # row 0 is the plane without a target: its target half, target square, squared error and extrema are untouched
    assert np.all(got[0][1, 0] == SENT) and not np.any(got[0][0, 0, 1:] == SENT)
    if extended:
        assert np.all(got[1][1:, 0] == SENT) and np.all(got[2][:, 0] == SENT) and not np.any(got[1][0, 0, 1:] == SENT)
        assert not np.any(got[1][:, 1:, 1:] == SENT) and not np.any(got[2][:, 1:, 1:] == SENT)
    else:
        assert np.all(got[1] == SENT) and np.all(got[2] == SENT)          # the basic call leaves sq and err alone


def test_assign_then_two_accumulations(dev):
    g = torch.Generator().manual_seed(5)
    B, T, hw = 3, 3, 1027
    st = State(dev, 2, 3, hw)
    for k, assign in enumerate((True, False, False)):
        st.window(*fields(B, T, hw, g), [0, 1], 0, assign)
        got = st.check(k)
    assert not any(np.any(x == SENT) for x in got)
    # from the family's initial state (zeros and the two infinities) an accumulation equals an assignment
    gens, tgts = fields(B, T, hw, g)
    a = State(dev, 2, 3, hw).window(gens, tgts, [0, 1], 0, True)
    b = State(dev, 2, 3, hw)
    b.ref[0][:], b.ref[1][:], b.ref[2][0], b.ref[2][1] = 0.0, 0.0, np.inf, -np.inf
    b.bufs = [Guarded(torch.from_numpy(b.ref[0]), dev), Guarded(torch.from_numpy(b.ref[1]), dev), Guarded32(torch.from_numpy(b.ref[2]), dev)]
    b.window(gens, tgts, [0, 1], 0, False)
    for x, y in zip(a.check(), b.check()):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("hw", [1024, 1027])
def test_nan_infinity_and_equal_fields(dev, hw):
    g = torch.Generator().manual_seed(6)
    B, T = 3, 2
    gens, tgts = fields(B, T, hw, g)
    gens[0][1, 0, 5] = float("nan")                     # one NaN in one sample of one pixel
    gens[0][0, 1, 9] = float("inf")
    tgts[1][2, 1, 11] = float("nan")                    # a NaN on the target side, in the last sample
    tgts[0][:, :, 20:24] = gens[0][:, :, 20:24]         # gen == target
    st = State(dev, 2, 2, hw).window(gens, tgts, [0, 1], 0, True)
    mean, sq, err = st.check("assign")
    assert np.isnan(mean[0, 0, 0, 5]) and np.isnan(sq[2, 0, 0, 5]) and np.isnan(err[:, 0, 0, 5]).all() and not np.isnan(mean[1, 0, 0, 5])
    assert mean[0, 0, 1, 9] == np.inf and err[1, 0, 1, 9] == np.inf and np.isfinite(err[0, 0, 1, 9])
    assert np.isnan(err[:, 1, 1, 11]).all() and np.isnan(mean[1, 1, 1, 11]) and not np.isnan(mean[0, 1, 1, 11])
    assert np.all(sq[2, 0, :, 20:24] == 0) and np.all(err[:, 0, :, 20:24] == 0)
    gens2, tgts2 = fields(B, T, hw, g)
    gens2[1][0, 0, 30] = float("nan")                   # a NaN arriving on a finite slot
    mean, sq, err = st.window(gens2, tgts2, [0, 1], 0, False).check("accumulate")
    assert np.isnan(err[:, 0, 0, 5]).all() and np.isnan(err[:, 1, 0, 30]).all()      # a stored NaN stays, a new one enters


def test_no_planes_is_a_no_op(dev):
    g = torch.Generator().manual_seed(7)
    gens, tgts = fields(2, 2, 1025, g)
    got = State(dev, 2, 2, 1025).window(gens, tgts, [0, 1], 0, True, nplanes=0).check()
    assert all(np.all(x == SENT) for x in got)


@pytest.mark.parametrize("override", [dict(t0=-1), dict(t0=2), dict(batch=0), dict(steps=0), dict(steps=-1), dict(nplanes=65536),
                                      dict(nplanes=-1), dict(mean=None), dict(sq=None), dict(err=None), dict(steps=65536, n_time=65537)])
def test_refused_calls_write_nothing(dev, override):
    g = torch.Generator().manual_seed(8)
    gens, tgts = fields(2, 2, 1025, g)
    st = State(dev, 2, 3, 1025)
    rest = {k: v for k, v in override.items() if k != "t0"}
    got = st.window(gens, tgts, [0, 1], override.get("t0", 0), True, expect=INVALID, **rest).check(override)
    assert all(np.all(x == SENT) for x in got)
    assert "ace_diag_video_window" in lib().ace_diag_last_error().decode()


def test_two_identical_calls_are_bitwise_equal(dev):
    runs = []
    for _ in range(2):
        g = torch.Generator().manual_seed(9)
        st = State(dev, 2, 3, 2051).window(*fields(5, 3, 2051, g), [1, 0], 0, True, "odd").window(*fields(5, 3, 2051, g), [0, 1], 0, False)
        runs.append(st.check())
    for x, y in zip(*runs):
        assert np.array_equal(x.view(np.int64 if x.dtype == np.float64 else np.int32), y.view(np.int64 if y.dtype == np.float64 else np.int32))


def test_accumulator_indices_past_two_to_the_31(dev):
    """nrows = 2, hw = 1024 and n_time = 524800: the last slot of the last row of the max channel of err is element 2 149 580 799
    of err, past 2^31 = 2 147 483 648, as it is of mean's target half and, further still, of sq.  All three accumulators are
    allocated at that shape (8.6 + 17.2 + 25.8 GB, not filled) when the device has the room; without it the case is skipped: no
    smaller arrangement can wrap.  One plane at the last row, assigned at the last slot; read back are that slot of every channel
    and, as guards, the slots a truncation of the element index to 31 bits would hit."""
    hw, nrows, n_time, B = 1024, 2, 524800, 2
    per = nrows * n_time * hw
    assert 2 * per > 2 ** 31 > per
    need = 2 * per * 8 + 3 * per * 8 + 2 * per * 4
    if torch.cuda.mem_get_info(dev)[0] < need + (4 << 30):
        pytest.skip(f"needs {need >> 30} GiB of free device memory")
    g = torch.Generator().manual_seed(10)
    (x,), (y,) = fields(B, 1, hw, g, n=1)
    mean = torch.empty((2, nrows, n_time, hw), dtype=torch.float64, device=dev)
    sq = torch.empty((3, nrows, n_time, hw), dtype=torch.float64, device=dev)
    err = torch.empty((2, nrows, n_time, hw), dtype=torch.float32, device=dev)
    last = (nrows - 1, n_time - 1)
    wrapped = [(c * per + (last[0] * n_time + last[1]) * hw) % 2 ** 31 for c in (1, 2)]          # element offsets, 31-bit truncation
    for buf in (mean, sq, err):
        flat = buf.view(-1)
        for o in wrapped:
            flat[o:o + hw] = SENT
    xd, yd = x.to(dev), y.to(dev)
    tab = torch.tensor([xd.data_ptr(), hw, hw, yd.data_ptr(), hw, hw], dtype=torch.int64, device=dev)
    rows_d = torch.tensor([nrows - 1], dtype=torch.int32, device=dev)
    base = tab.data_ptr()
    rc = lib().ace_diag_video_window(base, base + 8, base + 24, base + 32, rows_d.data_ptr(), mean.data_ptr(), sq.data_ptr(),
                                     err.data_ptr(), nrows, n_time, n_time - 1, 1, 1, B, 1, hw, None)
    assert rc == 0, lib().ace_diag_last_error().decode()
    torch.cuda.synchronize()
    ref = R.video_window([x.numpy()], [y.numpy()], [0], *R.new_buffers(1, 1, hw), 0, assign=True)
    for buf, want in zip((mean, sq, err), ref):
        assert np.array_equal(buf[:, last[0], last[1]].cpu().numpy(), want[:, 0, 0]), buf.dtype
        for o in wrapped:
            assert bool((buf.view(-1)[o:o + hw] == SENT).all()), "a truncated index was written"
    del mean, sq, err
    torch.cuda.empty_cache()
