"""csrc/diag.hip through the C ABI (ace_diag_window, ace_diag_spectrum) against tests/_diag_ref.py, on the raw fp64 accumulators:
every shape the kernels branch on (planes smaller than a wave, ragged tails, hw % 4 != 0), every layout (channel slices, bases off a
16-byte boundary, odd sample strides, a step stride of 0), weights with whole waves, chunks and planes of zero, data whose mean
dwarfs its spread, and the bookkeeping of rows, t0, t_begin and repeated calls.

Bars (derived in the docstrings of ``_diag_ref.series_errors``; fp64 roundings along a summation tree about 100 deep, times 100):
  weighted mean   |got - ref| <= 1e-12 * (sum w|x| / sum w)
  weighted std    |got - ref| <= 1e-12 * ref + 1e-14 * |wmean|
  spectrum        |got - ref| <= 1e-12 * ref per (row, l)
  time sums       bitwise
Every output buffer has 64 guard doubles of a sentinel on each side; guards, input planes and weights must come back bitwise
unchanged.  ``partial`` is pre-filled with a NaN pattern, so a partial that is read without having been written shows.  Each test
prints its largest error as a fraction of the bar (``DIAGACC`` lines; profiles/diag_kernel_accuracy.txt keeps the maxima)."""

import pytest
import torch

import _diag_ref as R

pytestmark = pytest.mark.gpu

G = 64                                        # guard doubles on each side
SENT = 0x7FF85EEDC0DE0001                     # guard pattern (a NaN)
PART = 0x7FF8BAD0BAD0BAD1                     # pre-fill of the partial scratch (a NaN)
INVALID = -1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def lib():
    from ace_amd import _lib
    return _lib.lib()


class Guarded:
    """a device fp64 buffer between two guards"""

    def __init__(self, init: torch.Tensor, dev):
        self.shape, self.n = tuple(init.shape), init.numel()
        host = torch.full((self.n + 2 * G,), SENT, dtype=torch.int64)
        host[G:G + self.n] = init.reshape(-1).contiguous().view(torch.int64)
        self.buf = host.to(dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 8 * G

    def read(self) -> torch.Tensor:
        host = self.buf.cpu()
        assert bool((host[:G] == SENT).all()) and bool((host[G + self.n:] == SENT).all()), "guard overwritten"
        return host[G:G + self.n].view(torch.float64).reshape(self.shape).clone()


def nan_fill(n: int) -> torch.Tensor:
    return torch.full((n,), PART, dtype=torch.int64).view(torch.float64)


# ---- planes: a flat fp32 storage, an offset and two strides ----------------------------------------------------------------
class Plane:
    def __init__(self, storage, offset, sb, st, B, T, hw):
        self.storage, self.offset, self.sb, self.st = storage.contiguous(), offset, sb, st
        self.view = self.storage.as_strided((B, T, hw), (sb, st, 1), offset)


def make_plane(data: torch.Tensor, layout: str, g) -> Plane:
    """``data`` (B, T, hw) fp32 laid out as ``layout``; for "expand" only data[:, 0] is used"""
    B, T, hw = data.shape
    junk = lambda *s: torch.randn(*s, generator=g)                      # noqa: E731
    if layout == "contiguous":
        return Plane(data.reshape(-1).clone(), 0, T * hw, hw, B, T, hw)
    if layout == "chanslice":                                         # channel 1 of a packed (B, T, 3, hw)
        s = junk(B, T, 3, hw)
        s[:, :, 1] = data
        return Plane(s.reshape(-1), hw, T * 3 * hw, 3 * hw, B, T, hw)
    if layout.startswith("offset"):                                   # 1, 2 or 3 floats past a 16-byte boundary
        k = int(layout[-1])
        return Plane(torch.cat([junk(k), data.reshape(-1), junk(4 - k)]), k, T * hw, hw, B, T, hw)
    if layout == "oddstride":                                         # sample stride not a multiple of 4
        pad = 1 if (T * hw + 1) % 4 else 2
        s = junk(B, T * hw + pad)
        s[:, :T * hw] = data.reshape(B, -1)
        return Plane(s.reshape(-1), 0, T * hw + pad, hw, B, T, hw)
    if layout == "expand":                                            # one static field for every step
        return Plane(data[:, 0].reshape(-1).clone(), 0, hw, 0, B, T, hw)
    raise ValueError(layout)


def make_weights(kind: str, hw: int, g) -> torch.Tensor:
    if kind == "ones":
        return torch.ones(hw)
    area = torch.cos(torch.linspace(-1.55, 1.55, hw, dtype=torch.float64)).float()     # 1-degree-like: positive, 30x range
    if kind == "area":
        return area
    if kind == "zero":
        return torch.zeros(hw)
    if kind == "mask":            # one whole wave's 256 pixels, one whole 1024-pixel chunk and scattered pixels of zero weight
        w = area.clone()
        w[torch.rand(hw, generator=g) < 0.1] = 0.0
        if hw > 512:
            w[256:512] = 0.0
        if hw > 3072:
            w[2048:3072] = 0.0
        if not bool((w != 0).any()):
            w[hw // 2] = area[hw // 2]
        return w
    raise ValueError(kind)


def make_data(kind: str, B: int, T: int, hw: int, g) -> torch.Tensor:
    r = torch.randn(B, T, hw, generator=g)
    return {"randn": r, "pressure": 1e5 + 1e2 * r, "offset1e7": 1e7 + r, "constant": torch.full((B, T, hw), 101325.0),
            "tiny": 1e-30 * r}[kind].float()


def run_window(dev, planes, weights, wrows, rows, nrows, n_time, t0, t_begin, do_tsum, B, T, hw, series0=None, tsum0=None,
               calls=1, tsum_null=False, w_offset=0, expect=0):
    """``calls`` times ace_diag_window on device copies of the planes' storages; returns (series, tsum, partial) as CPU tensors
    after checking the guards and that planes and weights are bitwise unchanged."""
    L = lib()
    n = len(planes)
    store = [p.storage.to(dev) for p in planes]
    wstore = torch.cat([torch.zeros(w_offset), weights.reshape(-1)]).contiguous()
    wdev = wstore.to(dev)
    assert all(s.data_ptr() % 16 == 0 for s in store) and wdev.data_ptr() % 16 == 0
    tab = torch.tensor([s.data_ptr() + 4 * p.offset for s, p in zip(store, planes)]
                       + [v for p in planes for v in (p.sb, p.st)], dtype=torch.int64, device=dev)
    rows_d = torch.tensor(rows, dtype=torch.int32, device=dev)
    wrows_d = torch.tensor(wrows, dtype=torch.int32, device=dev)
    series = Guarded(torch.zeros(2, nrows, n_time, dtype=torch.float64) if series0 is None else series0, dev)
    tsum = Guarded(torch.zeros(nrows, hw, dtype=torch.float64) if tsum0 is None else tsum0, dev)
    npart = int(L.ace_diag_partial_doubles(n, B, T, hw))
    assert npart == n * B * T * ((hw + 1023) // 1024) * 4 * 3
    partial = Guarded(nan_fill(npart), dev)
    for _ in range(calls):
        rc = L.ace_diag_window(tab.data_ptr(), tab.data_ptr() + 8 * n, rows_d.data_ptr(), wrows_d.data_ptr(),
                               wdev.data_ptr() + 4 * w_offset, weights.shape[0], partial.ptr, None if tsum_null else tsum.ptr,
                               series.ptr, nrows, n_time, t0, t_begin, do_tsum, n, B, T, hw, None)
        assert rc == expect, L.ace_diag_last_error().decode()
    torch.cuda.synchronize()
    for s, p in zip(store, planes):
        assert torch.equal(s.cpu().view(torch.int32), p.storage.view(torch.int32)), "an input plane changed"
    assert torch.equal(wdev.cpu().view(torch.int32), wstore.view(torch.int32)), "the weights changed"
    return series.read(), tsum.read(), partial.read()


def check_window(dev, planes, weights, wrows, rows, nrows, n_time, t0, t_begin, do_tsum, B, T, hw, what, calls=1, seed_init=None,
                 tsum_null=False, w_offset=0):
    """one case against ``_diag_ref.window_ref``; returns (series, tsum, partial) of the device run"""
    if seed_init is None:
        series0 = torch.zeros(2, nrows, n_time, dtype=torch.float64)
        tsum0 = torch.zeros(nrows, hw, dtype=torch.float64)
    else:                                   # accumulators that are not zero: += must add, and untouched rows keep their bits
        gi = torch.Generator().manual_seed(seed_init)
        series0 = torch.randn(2, nrows, n_time, dtype=torch.float64, generator=gi)
        tsum0 = torch.randn(nrows, hw, dtype=torch.float64, generator=gi)
    got_s, got_t, part = run_window(dev, planes, weights, wrows, rows, nrows, n_time, t0, t_begin, do_tsum, B, T, hw,
                                    series0.clone(), tsum0.clone(), calls, tsum_null, w_offset)
    ref_s, ref_t = series0.clone(), tsum0.clone()
    bar = series0.abs()                     # the += onto an accumulator that is not zero rounds once more, relative to its value
    for _ in range(calls):
        scale = R.window_ref([p.view for p in planes], weights, wrows, rows, B, T, t0, t_begin, bool(do_tsum), ref_s,
                             None if not do_tsum else ref_t)
        R.add_scale(bar, scale, rows, t0)
    e_mean, e_std = R.series_errors(got_s, ref_s, bar)
    print(f"DIAGACC window {what} hw={hw} B={B} T={T} mean={e_mean:.3e} std={e_std:.3e} (fractions of the bar)")
    assert e_mean <= 1.0 and e_std <= 1.0, (what, e_mean, e_std)
    assert R.bits_equal(got_t, ref_t), f"{what}: the time sums are not the header's sequence of additions"
    # rows no plane names keep their bits
    named = {r for r, wr in zip(rows, wrows) if 0 <= r < nrows and 0 <= wr < weights.shape[0]}
    for r in set(range(nrows)) - named:
        assert R.bits_equal(got_s[:, r], series0[:, r]) and R.bits_equal(got_t[r], tsum0[r]), (what, r)
    return got_s, got_t, part


HWS = [1, 3, 13, 63, 64, 255, 256, 257, 1023, 1024, 1025, 351, 4050, 64800]
BTS = [(1, 1), (1, 7), (3, 1), (2, 5)]


@pytest.mark.parametrize("B,T", BTS)
@pytest.mark.parametrize("hw", HWS)
def test_window_sizes(dev, hw, B, T):
    """contiguous planes at every size: area weights, a masked row with NaN under the mask, a surface-pressure-like plane"""
    g = torch.Generator().manual_seed(1000 * hw + 10 * B + T)
    weights = torch.stack([make_weights("area", hw, g), make_weights("mask", hw, g)])
    data = [make_data("randn", B, T, hw, g), make_data("randn", B, T, hw, g), make_data("pressure", B, T, hw, g)]
    data[1][:, :, weights[1] == 0] = float("nan")
    planes = [make_plane(d, "contiguous", g) for d in data]
    check_window(dev, planes, weights, [0, 1, 0], [0, 1, 2], 3, T, 0, 0, 1, B, T, hw, "sizes")


def test_window_quarter_degree(dev):
    """721 x 1440: one plane set (the reference's sums are torch's pairwise fp64 sums here)"""
    hw, B, T = 721 * 1440, 1, 2
    g = torch.Generator().manual_seed(7)
    weights = torch.stack([make_weights("area", hw, g), make_weights("mask", hw, g)])
    data = [make_data("pressure", B, T, hw, g), make_data("randn", B, T, hw, g)]
    data[1][:, :, weights[1] == 0] = float("nan")
    planes = [make_plane(d, "contiguous", g) for d in data]
    check_window(dev, planes, weights, [0, 1], [1, 0], 2, T + 1, 1, 1, 1, B, T, hw, "quarter-degree")


LAYOUTS = [(hw, lay) for hw in (13, 64, 256, 1024, 4050, 64800) for lay in ("chanslice", "oddstride", "expand")]
# a base 1, 2 or 3 floats past a 16-byte boundary only changes the path where hw % 4 == 0
LAYOUTS += [(hw, f"offset{k}") for hw in (64, 256, 1024, 64800) for k in (1, 2, 3)]


@pytest.mark.parametrize("hw,layout", LAYOUTS)
def test_window_layouts(dev, hw, layout):
    """the same numbers whatever the layout: bitwise the contiguous run's, and right by the reference"""
    B, T = 2, 5
    g = torch.Generator().manual_seed(hw)
    weights = torch.stack([make_weights("area", hw, g), make_weights("mask", hw, g)])
    data = [make_data("pressure", B, T, hw, g), make_data("randn", B, T, hw, g)]
    data[1][:, :, weights[1] == 0] = float("nan")
    if layout == "expand":
        data = [d[:, :1].expand(B, T, hw).contiguous() for d in data]
    args = (weights, [0, 1], [0, 1], 2, T, 0, 1, 1, B, T, hw)
    base = check_window(dev, [make_plane(d, "contiguous", g) for d in data], *args, "contiguous")
    got = check_window(dev, [make_plane(d, layout, g) for d in data], *args, layout)
    for a, b, name in zip(got, base, ("series", "tsum", "partial")):
        assert R.bits_equal(a, b), (layout, name)


@pytest.mark.parametrize("hw", [64, 1024, 64800])
def test_window_weight_table_off_a_16_byte_boundary(dev, hw):
    """a weight table that starts 4 bytes past a 16-byte boundary with hw % 4 == 0 is read with scalar loads and gives the aligned
    run's bits"""
    B, T = 2, 3
    g = torch.Generator().manual_seed(hw + 1)
    weights = torch.stack([make_weights("mask", hw, g), make_weights("area", hw, g)])
    data = [make_data("randn", B, T, hw, g), make_data("pressure", B, T, hw, g)]
    data[0][:, :, weights[0] == 0] = float("nan")
    planes = [make_plane(d, "contiguous", g) for d in data]
    args = (planes, weights, [0, 1], [1, 0], 2, T, 0, 0, 1, B, T, hw)
    base = check_window(dev, *args, "aligned weights")
    got = check_window(dev, *args, "weights + 4 bytes", w_offset=1)
    for a, b in zip(got, base):
        assert R.bits_equal(a, b)


@pytest.mark.parametrize("kind", ["randn", "pressure", "offset1e7", "constant", "tiny"])
@pytest.mark.parametrize("wkind", ["ones", "area", "mask"])
@pytest.mark.parametrize("hw", [13, 1025, 64800])
def test_window_data_kinds(dev, hw, wkind, kind):
    """means up to 1e7 times the spread, a constant plane (the std of 101325 everywhere is at most 1e-14 * 101325: a one-pass
    E[x^2] - m^2 gives about 1e-8 * 101325 even in fp64), and values near fp32's smallest normal numbers"""
    B, T = 2, 2
    g = torch.Generator().manual_seed(hw + len(kind) + 7 * len(wkind))
    weights = make_weights(wkind, hw, g)[None]
    data = make_data(kind, B, T, hw, g)
    if wkind == "mask":
        data[:, :, weights[0] == 0] = float("nan")
    series, _, _ = check_window(dev, [make_plane(data, "contiguous", g)], weights, [0], [0], 1, T, 0, 0, 1, B, T, hw,
                                f"{kind}/{wkind}")
    if kind == "constant":
        assert bool((series[0, 0] == 101325.0).all()) or float((series[0, 0] - 101325.0).abs().max()) <= 1e-12 * 101325.0
        assert float(series[1, 0].max()) <= 1e-14 * 101325.0, float(series[1, 0].max())


@pytest.mark.parametrize("hw", [3, 257, 4050, 64800])
def test_window_zero_weight_plane_and_two_weight_rows(dev, hw):
    """a plane whose weights are all zero: series NaN, time sums still the plain sums; planes that share two weight rows"""
    B, T = 2, 3
    g = torch.Generator().manual_seed(hw + 2)
    weights = torch.stack([make_weights("zero", hw, g), make_weights("area", hw, g), make_weights("mask", hw, g)])
    data = [make_data("randn", B, T, hw, g) for _ in range(4)]
    data[3][:, :, weights[2] == 0] = float("nan")
    planes = [make_plane(d, "contiguous", g) for d in data]
    series, tsum, _ = check_window(dev, planes, weights, [0, 1, 1, 2], [0, 1, 2, 3], 4, T, 0, 0, 1, B, T, hw, "zero weights")
    assert bool(torch.isnan(series[:, 0]).all()) and not bool(torch.isnan(series[:, 1:]).any())
    assert not bool(torch.isnan(tsum[:3]).any())
    assert torch.equal(torch.isnan(tsum[3]), weights[2] == 0)


@pytest.mark.parametrize("t_begin", [0, 1, "T", "T+3"])
@pytest.mark.parametrize("hw", [13, 1025, 4050])
def test_window_bookkeeping(dev, hw, t_begin):
    """rows a permutation with nrows > nplanes and one -1, t0 > 0, accumulators that are not zero, the call made twice"""
    B, T = 2, 5
    t_begin = {"T": T, "T+3": T + 3}.get(t_begin, t_begin)
    g = torch.Generator().manual_seed(hw + 3)
    weights = torch.stack([make_weights("area", hw, g), make_weights("mask", hw, g)])
    data = [make_data("randn", B, T, hw, g) for _ in range(4)]
    planes = [make_plane(d, lay, g) for d, lay in zip(data, ("contiguous", "chanslice", "contiguous", "oddstride"))]
    rows, wrows = [4, INVALID, 0, 2], [0, 1, 1, 0]
    for calls in (1, 2):
        _, tsum, _ = check_window(dev, planes, weights, wrows, rows, 6, T + 4, 3, t_begin, 1, B, T, hw, f"rows, {calls} call(s)",
                                  calls=calls, seed_init=11)
    if t_begin >= T:                        # nothing to add: the sums keep their bits
        gi = torch.Generator().manual_seed(11)
        torch.randn(2, 6, T + 4, dtype=torch.float64, generator=gi)
        assert R.bits_equal(tsum, torch.randn(6, hw, dtype=torch.float64, generator=gi))


@pytest.mark.parametrize("hw", [13, 1024, 4050])
def test_window_out_of_range_rows_contribute_nothing(dev, hw):
    """a plane whose wrows[j] or rows[j] is out of range (either side) touches no accumulator, although ``partial`` holds NaN
    where that plane's partials would be"""
    B, T = 2, 3
    g = torch.Generator().manual_seed(hw + 4)
    weights = torch.stack([make_weights("area", hw, g), make_weights("mask", hw, g)])
    planes = [make_plane(make_data("randn", B, T, hw, g), "contiguous", g) for _ in range(5)]
    rows, wrows = [0, 1, 2, 7, INVALID], [INVALID, 2, 0, 0, 1]       # only plane 2 counts; nw = 2, nrows = 4
    series, tsum, part = check_window(dev, planes, weights, wrows, rows, 4, T + 1, 1, 0, 1, B, T, hw, "out of range", seed_init=5)
    per_plane = part.numel() // 5
    untouched = nan_fill(per_plane)
    for j in (0, 1):                        # no weight row: no partials are written either
        assert torch.equal(part[j * per_plane:(j + 1) * per_plane].view(torch.int64), untouched.view(torch.int64)), j


@pytest.mark.parametrize("hw", [257, 4050])
def test_window_without_time_sums_and_null_tsum(dev, hw):
    B, T = 2, 3
    g = torch.Generator().manual_seed(hw + 5)
    weights = make_weights("area", hw, g)[None]
    planes = [make_plane(make_data("pressure", B, T, hw, g), "contiguous", g) for _ in range(2)]
    a = check_window(dev, planes, weights, [0, 0], [1, 0], 2, T, 0, 0, 0, B, T, hw, "do_tsum = 0", seed_init=3)
    b = check_window(dev, planes, weights, [0, 0], [1, 0], 2, T, 0, 0, 0, B, T, hw, "tsum = NULL", seed_init=3, tsum_null=True)
    c = check_window(dev, planes, weights, [0, 0], [1, 0], 2, T, 0, 0, 1, B, T, hw, "do_tsum = 1", seed_init=3)
    assert R.bits_equal(a[0], b[0]) and R.bits_equal(a[0], c[0]) and R.bits_equal(a[1], b[1]) and not R.bits_equal(a[1], c[1])


def test_window_runs_are_bitwise_repeatable(dev):
    hw, B, T = 64800, 2, 5
    g = torch.Generator().manual_seed(6)
    weights = torch.stack([make_weights("area", hw, g), make_weights("mask", hw, g)])
    planes = [make_plane(make_data(k, B, T, hw, g), lay, g)
              for k, lay in (("randn", "contiguous"), ("pressure", "chanslice"), ("offset1e7", "offset1"))]
    runs = [run_window(dev, planes, weights, [0, 1, 0], [2, 0, 1], 3, T + 2, 2, 1, 1, B, T, hw, calls=2) for _ in range(2)]
    for a, b in zip(*runs):
        assert R.bits_equal(a, b)


# ---- ace_diag_spectrum ------------------------------------------------------------------------------------------------------
def run_spectrum(dev, coeffs, rows, spec0, calls=1, expect=0):
    L = lib()
    nnames, planes, Lm, M = coeffs.shape
    cdev = coeffs.contiguous().to(dev)
    rows_d = torch.tensor(rows, dtype=torch.int32, device=dev)
    spec = Guarded(spec0, dev)
    for _ in range(calls):
        rc = L.ace_diag_spectrum(cdev.data_ptr(), rows_d.data_ptr(), spec.ptr, spec0.shape[0], nnames, planes, Lm, M, None)
        assert rc == expect, L.ace_diag_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(cdev.cpu()).view(torch.int32), torch.view_as_real(coeffs.contiguous()).view(torch.int32))
    return spec.read()


@pytest.mark.parametrize("nnames,planes,L,M", [(1, 1, 1, 1), (1, 1, 5, 3), (3, 7, 12, 13), (2, 10, 180, 181), (1, 3, 721, 721),
                                               (5, 1, 45, 20)])
def test_spectrum(dev, nnames, planes, L, M):
    """coefficients whose amplitude falls by 12 orders of magnitude over the degrees (the power by 24), rows a permutation with
    one -1 and nrows > nnames, one call and two: each (row, l) within 1e-12 of the fp64 sum, relative to that degree's own power"""
    g = torch.Generator().manual_seed(nnames * 1000 + L)
    amp = 10.0 ** (-12.0 * torch.arange(L, dtype=torch.float64) / max(L - 1, 1))
    c = torch.complex(torch.randn(nnames, planes, L, M, generator=g, dtype=torch.float64),
                      torch.randn(nnames, planes, L, M, generator=g, dtype=torch.float64)) * amp[:, None]
    c = c.to(torch.complex64)
    nrows = nnames + 2
    rows = torch.randperm(nrows, generator=g)[:nnames].tolist()
    if nnames > 1:
        rows[1] = INVALID
    named = [r for r in rows if r >= 0]
    spec0 = torch.randn(nrows, L, dtype=torch.float64, generator=g)
    spec0[named] = 0.0
    runs = {}
    for calls in (1, 2):
        got = run_spectrum(dev, c, rows, spec0.clone(), calls)
        ref = spec0.clone()
        for _ in range(calls):
            R.spectrum_ref(c, rows, ref)
        assert bool((ref[named] > 0).all())
        err = float(((got[named] - ref[named]).abs() / ref[named]).max())
        print(f"DIAGACC spectrum nnames={nnames} planes={planes} L={L} M={M} calls={calls} rel={err:.3e}")
        assert err <= 1e-12, err
        for r in set(range(nrows)) - set(named):
            assert R.bits_equal(got[r], spec0[r]), r
        runs[calls] = got
    assert R.bits_equal(runs[2][named], 2 * runs[1][named])          # the second call adds the same fixed-order sums
    assert R.bits_equal(run_spectrum(dev, c, rows, spec0.clone(), 2), runs[2])


# ---- refusals ---------------------------------------------------------------------------------------------------------------
WINDOW_OK = dict(nw=1, nrows=2, n_time=4, t0=1, t_begin=0, do_tsum=1, nplanes=2, batch=2, steps=3, hw=13)


@pytest.mark.parametrize("change,word", [
    (dict(t0=2), "n_time"), (dict(t0=-1), "t0"), (dict(t_begin=-1), "t_begin"), (dict(steps=65536, n_time=70000), "steps"),
    (dict(steps=0), "steps"), (dict(nplanes=65536), "nplanes"), (dict(nplanes=-1), "nplanes"), (dict(hw=0), "hw"),
    (dict(hw=-5), "hw"), (dict(batch=0), "batch"), (dict(nw=0), "nw"), (dict(nrows=0), "nrows"),
    (dict(null="srcs"), "null"), (dict(null="strides"), "null"), (dict(null="rows"), "null"), (dict(null="wrows"), "null"),
    (dict(null="weights"), "null"), (dict(null="partial"), "null"), (dict(null="series"), "null"), (dict(null="tsum"), "null"),
])
def test_window_refusals(dev, change, word):
    """every ACE_ERR_INVALID branch: the code, a message that names the constraint, and no buffer touched"""
    L = lib()
    a = dict(WINDOW_OK)
    null = change.get("null")
    a.update({k: v for k, v in change.items() if k != "null"})
    B, T, hw, n = 2, 3, 13, 2
    g = torch.Generator().manual_seed(0)
    fields = torch.randn(n, B, T, hw, generator=g).to(dev)
    weights = torch.ones(1, hw, device=dev)
    tab = torch.tensor([fields[j].data_ptr() for j in range(n)] + [T * hw, hw] * n, dtype=torch.int64, device=dev)
    rows = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    wrows = torch.zeros(2, dtype=torch.int32, device=dev)
    series0, tsum0 = torch.randn(2, 2, 4, dtype=torch.float64, generator=g), torch.randn(2, hw, dtype=torch.float64, generator=g)
    series, tsum = Guarded(series0, dev), Guarded(tsum0, dev)
    partial = Guarded(nan_fill(int(L.ace_diag_partial_doubles(n, B, T, hw))), dev)
    p = dict(srcs=tab.data_ptr(), strides=tab.data_ptr() + 8 * n, rows=rows.data_ptr(), wrows=wrows.data_ptr(),
             weights=weights.data_ptr(), partial=partial.ptr, tsum=tsum.ptr, series=series.ptr)
    if null:
        p[null] = None
    rc = L.ace_diag_window(p["srcs"], p["strides"], p["rows"], p["wrows"], p["weights"], a["nw"], p["partial"], p["tsum"],
                           p["series"], a["nrows"], a["n_time"], a["t0"], a["t_begin"], a["do_tsum"], a["nplanes"], a["batch"],
                           a["steps"], a["hw"], None)
    msg = L.ace_diag_last_error().decode()
    assert rc == INVALID and word in msg and msg.startswith("ace_diag_window"), (rc, msg)
    torch.cuda.synchronize()
    assert R.bits_equal(series.read(), series0) and R.bits_equal(tsum.read(), tsum0)
    assert torch.equal(partial.read().view(torch.int64), nan_fill(partial.n).view(torch.int64))


def test_no_planes_and_no_names_are_ok(dev):
    L = lib()
    assert L.ace_diag_window(None, None, None, None, None, 1, None, None, None, 1, 4, 0, 0, 1, 0, 1, 1, 13, None) == 0
    assert L.ace_diag_spectrum(None, None, None, 1, 0, 1, 4, 3, None) == 0
    assert L.ace_diag_partial_doubles(2, 1, 1, 0) == -1 and L.ace_diag_partial_doubles(0, 1, 1, 5) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("change,word", [
    (dict(nnames=65536), "nnames"), (dict(nnames=-1), "nnames"), (dict(planes=0), "planes"), (dict(lmax=0), "lmax"),
    (dict(mmax=0), "mmax"), (dict(nrows=0), "nrows"), (dict(null="coeffs"), "null"), (dict(null="rows"), "null"),
    (dict(null="spec"), "null"),
])
def test_spectrum_refusals(dev, change, word):
    L = lib()
    a = dict(nrows=2, nnames=2, planes=3, lmax=4, mmax=5)
    null = change.get("null")
    a.update({k: v for k, v in change.items() if k != "null"})
    g = torch.Generator().manual_seed(0)
    c = torch.randn(2, 3, 4, 5, 2, generator=g).to(dev)
    rows = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    spec0 = torch.randn(2, 4, dtype=torch.float64, generator=g)
    spec = Guarded(spec0, dev)
    p = dict(coeffs=c.data_ptr(), rows=rows.data_ptr(), spec=spec.ptr)
    if null:
        p[null] = None
    rc = L.ace_diag_spectrum(p["coeffs"], p["rows"], p["spec"], a["nrows"], a["nnames"], a["planes"], a["lmax"], a["mmax"], None)
    msg = L.ace_diag_last_error().decode()
    assert rc == INVALID and word in msg and msg.startswith("ace_diag_spectrum"), (rc, msg)
    torch.cuda.synchronize()
    assert R.bits_equal(spec.read(), spec0)
