"""csrc/timeseg.hip through the C ABI (ace_diag_time_segments) against tests/_timeseg_ref.py, the numpy statement of the header
contract that tests/test_timeseg_ref_cpu.py holds to the reference.

Bar: equality.  The kernel adds in fp64 in step order without reassociation and divides in IEEE fp64, as the statement does, so
``np.array_equal(..., equal_nan=True)`` on sums and means alike.  Both outputs lie between guards, which must come back intact, and
are pre-filled with a sentinel, so a slot that should have been written and was not shows, as does one that should have been left
alone (an out-of-range row) and was not; the input planes must come back unchanged."""
import numpy as np
import pytest
import torch

import _timeseg_ref as R
from test_gpu_diag_kernels import INVALID, Guarded, dev, lib  # noqa: F401
from test_gpu_regress_kernels import place

pytestmark = pytest.mark.gpu

SENT = -12345.0                                      # pre-fill of the outputs
G32 = 64
GUARD32 = 0x7FC5EED1                                 # guard pattern of the fp32 buffer (a NaN)


class Guarded32:
    """a device fp32 buffer between two guards, 16-byte aligned like the fp64 one"""

    def __init__(self, init: torch.Tensor, dev):
        self.shape, self.n = tuple(init.shape), init.numel()
        host = torch.full((self.n + 2 * G32,), GUARD32, dtype=torch.int32)
        host[G32:G32 + self.n] = init.reshape(-1).contiguous().view(torch.int32)
        self.buf = host.to(dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * G32

    def read(self) -> torch.Tensor:
        host = self.buf.cpu()
        assert bool((host[:G32] == GUARD32).all()) and bool((host[G32 + self.n:] == GUARD32).all()), "guard overwritten"
        return host[G32:G32 + self.n].view(torch.float32).reshape(self.shape).clone()


def lay(data, layout, g):
    """(storage, offset in floats, sample stride, step stride) of a (B, T, hw) field"""
    if layout != "timeoffset":
        return place(data, layout, g)
    B, T, hw = data.shape                               # steps 2 .. T + 1 of a window of T + 3
    s = torch.randn(B, T + 3, hw, generator=g) * 1e30
    s[:, 2:T + 2] = data
    return s.reshape(-1), 2 * hw, (T + 3) * hw, hw


def call(dev, planes, rows, nrows, edges, layout="contiguous", want=("sums", "means"), expect=0, seed=0, nplanes=None, nseg=None):
    """one ace_diag_time_segments on (B, T, hw) CPU fields; returns (sums, means) as numpy (``None`` when not asked for) and the
    statement's"""
    L = lib()
    g = torch.Generator().manual_seed(seed)
    B, T, hw = planes[0].shape
    edges = np.asarray(edges, dtype=np.int32)
    nseg = edges.shape[1] - 1 if nseg is None else nseg
    n = len(planes) if nplanes is None else nplanes
    placed = [lay(x, layout, g) for x in planes]
    store = [p[0].to(dev) for p in placed]
    tab = [s.data_ptr() + 4 * p[1] for p, s in zip(placed, store)]
    for p in placed:
        tab += [p[2], p[3]]
    tab = torch.tensor(tab, dtype=torch.int64, device=dev)
    rows_d = torch.tensor(rows, dtype=torch.int32, device=dev)
    edges_d = torch.from_numpy(np.ascontiguousarray(edges)).to(dev)
    shape = (nrows, B, max(nseg, 1), hw)
    sums = Guarded(torch.full(shape, SENT, dtype=torch.float64), dev)
    means = Guarded32(torch.full(shape, SENT, dtype=torch.float32), dev)
    base = tab.data_ptr()
    rc = L.ace_diag_time_segments(base, base + 8 * len(planes), rows_d.data_ptr(), edges_d.data_ptr(),
                                  sums.ptr if "sums" in want else None, means.ptr if "means" in want else None, nrows, nseg, n, B, T,
                                  hw, None)
    assert rc == expect, L.ace_diag_last_error().decode()
    torch.cuda.synchronize()
    got = (sums.read().numpy(), means.read().numpy())
    for p, s in zip(placed, store):
        assert torch.equal(s.cpu().view(torch.int32), p[0].view(torch.int32)), "an input plane changed"
    ref = (np.full(shape, SENT), np.full(shape, SENT, np.float32))
    if rc == 0 and n and nseg:
        R.time_segments([x.numpy() for x in planes[:n]], rows[:n], nrows, edges, sums=ref[0] if "sums" in want else None,
                        means=ref[1] if "means" in want else None)
    return got, ref


def same(got, ref, what=""):
    assert np.array_equal(got[0], ref[0], equal_nan=True), (what, "sums")
    assert np.array_equal(got[1], ref[1], equal_nan=True), (what, "means")


def fields(B, T, hw, g, n=2):
    """a unit Gaussian and a surface-pressure-like field"""
    return [torch.randn(B, T, hw, generator=g), (1e5 + 900 * torch.randn(B, T, hw, generator=g)).float()][:n]


def edge_table(B, T, nseg, g):
    """ascending cuts that differ per sample: sample 0 spans [0, T], the others start or end inside; small T gives empty and
    length-1 segments"""
    e = torch.randint(0, T + 1, (B, nseg + 1), generator=g).sort(dim=1).values
    e[0, 0], e[0, -1] = 0, T
    if B > 1:
        e[1, -1] = T                                     # an edge equal to steps
    return e.numpy()


@pytest.mark.parametrize("hw", [1, 3, 7, 1023, 1024, 1025, 2051])
@pytest.mark.parametrize("layout", ["contiguous", "odd", "timeoffset"])
def test_sizes_and_layouts(dev, hw, layout):
    g = torch.Generator().manual_seed(hw)
    B, T, nseg = 3, 9, 5
    same(*call(dev, fields(B, T, hw, g), [1, 0], 2, edge_table(B, T, nseg, g), layout=layout), what=(hw, layout))


def test_the_real_grid(dev):
    g = torch.Generator().manual_seed(1)
    B, T, hw = 1, 40, 64800
    same(*call(dev, fields(B, T, hw, g), [0, 1], 2, [[0, 4, 8, 12, 31, 40]]))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 9, 40])
@pytest.mark.parametrize("nseg", [1, 2, 5])
def test_batch_steps_and_segments(dev, B, T, nseg):
    g = torch.Generator().manual_seed(100 * B + 10 * T + nseg)
    hw = 1025
    edges = edge_table(B, T, nseg, g)
    if nseg == 1:
        edges[0] = [0, T]                                # the full window
    if nseg == 5 and T >= 2:
        edges[-1] = [0, 1, 1, 2, T, T]                   # length 1, empty, length 1, the rest, empty
    same(*call(dev, fields(B, T, hw, g), [0, 1], 2, edges, layout="odd"), what=(B, T, nseg))


def test_unroll_remainders(dev):
    g = torch.Generator().manual_seed(2)
    B, T, hw = 2, 40, 1030
    edges = [[0, 7, 15, 24, 24, 40], [1, 2, 4, 7, 11, 26]]       # lengths 7, 8, 9, 0, 16 and 1, 2, 3, 4, 15
    same(*call(dev, fields(B, T, hw, g), [0, 1], 2, edges))


@pytest.mark.parametrize("layout", ["contiguous", "odd"])
def test_edges_outside_the_window_are_clamped_and_falling_edges_are_empty(dev, layout):
    g = torch.Generator().manual_seed(3)
    B, T, hw = 3, 9, 1025
    edges = [[-5, 3, 2, 2000000000, 9, -2000000000], [9, 9, 0, 4, 12, 3], [-1, -1, 10, 10, 0, 9]]
    got, ref = call(dev, fields(B, T, hw, g), [0, 1], 2, edges, layout=layout)
    same(got, ref)
    assert np.all(got[0][:, 0, 1] == 0) and np.all(np.isnan(got[1][:, 0, 1]))          # 3 -> 2: empty, sums 0 and means NaN
    assert not np.any(got[0] == SENT)


def test_nan_and_infinities_propagate(dev):
    g = torch.Generator().manual_seed(4)
    B, T, hw = 2, 9, 1030
    x, y = fields(B, T, hw, g)
    x[:, :, 5:40] = float("nan")                        # a masked patch, every step
    x[0, 3, 100] = float("nan")
    y[0, 2, 7], y[0, 6, 8], y[1, 1, 9], y[1, 2, 9] = float("inf"), float("-inf"), float("inf"), float("-inf")
    got, ref = call(dev, [x, y], [0, 1], 2, [[0, 3, 9], [0, 5, 9]])
    same(got, ref)
    assert np.all(np.isnan(got[0][0, :, :, 5:40])) and np.isnan(got[0][0, 0, 1, 100]) and not np.isnan(got[0][0, 0, 0, 100])
    assert got[0][1, 0, 0, 7] == np.inf and got[1][1, 0, 1, 8] == -np.inf and np.isnan(got[0][1, 1, 0, 9])


def test_rows_out_of_range_write_nothing_and_rows_permute(dev):
    g = torch.Generator().manual_seed(5)
    B, T, hw = 2, 9, 1025
    x = fields(B, T, hw, g) + fields(B, T, hw, g)
    got, ref = call(dev, x, [2, -1, 0, 3], 3, edge_table(B, T, 2, g))
    same(got, ref)
    assert np.all(got[0][1] == SENT) and np.all(got[1][1] == SENT)                      # row 1: no plane names it
    assert not np.any(got[0][[0, 2]] == SENT)


@pytest.mark.parametrize("want", [("sums",), ("means",), ("sums", "means")])
def test_either_output_alone(dev, want):
    g = torch.Generator().manual_seed(6)
    B, T, hw = 2, 9, 1027
    got, ref = call(dev, fields(B, T, hw, g), [0, 1], 2, edge_table(B, T, 2, g), want=want)
    same(got, ref)
    if "sums" not in want:
        assert np.all(got[0] == SENT)
    if "means" not in want:
        assert np.all(got[1] == SENT)


def test_no_output_is_refused_and_no_planes_or_segments_are_ok(dev):
    g = torch.Generator().manual_seed(7)
    B, T, hw = 2, 9, 1027
    x = fields(B, T, hw, g)
    got, _ = call(dev, x, [0, 1], 2, edge_table(B, T, 2, g), want=(), expect=INVALID)
    assert np.all(got[0] == SENT) and np.all(got[1] == SENT)
    assert "sums and means" in lib().ace_diag_last_error().decode()
    for kw in (dict(nplanes=0), dict(nseg=0)):
        got, _ = call(dev, x, [0, 1], 2, edge_table(B, T, 2, g), **kw)
        assert np.all(got[0] == SENT) and np.all(got[1] == SENT)
    for kw in (dict(nplanes=-1), dict(nseg=-1), dict(nplanes=65536)):
        got, _ = call(dev, x, [0, 1], 2, edge_table(B, T, 2, g), expect=INVALID, **kw)
        assert np.all(got[0] == SENT) and np.all(got[1] == SENT)


def test_two_identical_calls_are_bitwise_equal(dev):
    B, T, hw = 3, 40, 2051
    runs = []
    for _ in range(2):
        g = torch.Generator().manual_seed(8)
        runs.append(call(dev, fields(B, T, hw, g), [1, 0], 2, edge_table(B, T, 5, g), layout="odd")[0])
    assert np.array_equal(runs[0][0].view(np.int64), runs[1][0].view(np.int64))
    assert np.array_equal(runs[0][1].view(np.int32), runs[1][1].view(np.int32))
