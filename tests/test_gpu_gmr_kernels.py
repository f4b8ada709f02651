"""ace_gmr_partials / ace_gmr_sample_means / ace_gmr_pack_normalize / ace_gmr_unpack_denormalize (csrc/gmr.hip) through the C ABI
against the numpy statement of their contract (tests/_gmr_ref.py; include/ace_sfno.h "Global-mean removal"), bit for bit: the shift
buffer, the packed tensor with its synthetic channels, and the unpacked planes - at plane sizes below a wave, not a multiple of 4,
of one and of many chunks; with planes one float off 16-byte alignment (the 4-byte load path has to give the bits of the 16-byte
one), planes that are time slices of (B, T, hw) buffers, K = 1 with 11 shifted channels of 20 ("shared") and K = 20 of 20 with 20
synthetic channels ("per_channel" over all inputs), a reduced plane that is not the first packed one, a NaN.  Every written
buffer carries guard floats in front and behind and is compared whole."""
import numpy as np
import pytest
import torch

import _gmr_ref as R

pytestmark = pytest.mark.gpu

GUARD = -777.0
T_SLICES = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _place(values, layout, dev):
    """values (B, hw) fp32 on the host -> (the device buffer, the (B, hw) view of it the tables name)
    dense: contiguous; offset: one float off a 16-byte boundary in every sample (hw % 4 == 0); sliced: [:, 1] of (B, T, hw)"""
    B, hw = values.shape
    if layout == "dense":
        buf = torch.full((4 + B * hw + 4,), GUARD, device=dev)
        view = buf[4:4 + B * hw].view(B, hw)
    elif layout == "offset":
        row = hw + 4
        buf = torch.full((B * row + 8,), GUARD, device=dev)
        view = torch.as_strided(buf, (B, hw), (row, 1), storage_offset=1 if hw % 4 == 0 else 5)
    else:
        buf = torch.full((B, T_SLICES, hw), GUARD, device=dev)
        view = buf[:, 1]
    view.copy_(values.to(dev))
    return buf, view


def _run(dev, B, hw, nin, reduced, shift_idx, extras, out_idx, layout="dense", scale="temperature", nan_at=None, seed=0):
    """One partials -> pack -> unpack round on the device and in the statement.  reduced: the channel of each of the K planes;
    shift_idx / out_idx: the k of every input / output channel (-1: none); extras: the k of every synthetic channel."""
    from ace_amd import _lib
    L, stream = _lib.lib(), _lib.current_stream()
    rng = np.random.default_rng(1000 * seed + hw + 7 * B + nin)
    K, nextra, nout = len(reduced), len(extras), len(out_idx)
    if scale == "temperature":
        src = (288.0 + rng.uniform(-30.0, 30.0, size=(B, nin, hw))).astype(np.float32)
        mean = (287.0 + rng.uniform(-5, 5, size=nin)).astype(np.float32)
        std = rng.uniform(2.0, 9.0, size=nin).astype(np.float32)
    else:
        src = (1e-3 * (1.0 + rng.uniform(-0.5, 0.5, size=(B, nin, hw)))).astype(np.float32)
        mean = (1e-3 * rng.uniform(0.8, 1.2, size=nin)).astype(np.float32)
        std = (1e-4 * rng.uniform(1.0, 3.0, size=nin)).astype(np.float32)
    if nan_at is not None:
        src[nan_at] = np.nan
    clim = np.array([mean[j] for j in reduced], dtype=np.float32) + np.float32(0.25) * std[reduced]
    extra_std = np.array([std[reduced[k]] for k in extras], dtype=np.float32)
    y = rng.standard_normal(size=(B, nout, hw)).astype(np.float32)
    out_mean = (287.0 + rng.uniform(-5, 5, size=nout)).astype(np.float32)
    out_std = rng.uniform(2.0, 9.0, size=nout).astype(np.float32)

    # ---- the statement
    want_shift = np.array([[R.shift_of(clim[k], src[b, reduced[k]]) for k in range(K)] for b in range(B)], dtype=np.float32)
    want_x = np.empty((B, nin + nextra, hw), dtype=np.float32)
    want_out = np.empty((B, nout, hw), dtype=np.float32)
    for b in range(B):
        for j in range(nin):
            want_x[b, j] = R.pack(src[b, j], want_shift[b, shift_idx[j]] if shift_idx[j] >= 0 else None, mean[j], std[j])
        for e, k in enumerate(extras):
            want_x[b, nin + e] = R.extra(want_shift[b, k], extra_std[e])
        for j in range(nout):
            want_out[b, j] = R.unpack(y[b, j], want_shift[b, out_idx[j]] if out_idx[j] >= 0 else None, out_mean[j], out_std[j])

    # ---- the device
    dt = lambda a, dtype: torch.tensor(np.asarray(a), dtype=dtype, device=dev)      # noqa: E731
    placed = [_place(torch.from_numpy(src[:, j]), layout, dev) for j in range(nin)]
    before = [buf.clone() for buf, _ in placed]
    table = dt([[v.data_ptr() for _, v in placed], [v.stride(0) for _, v in placed]], torch.int64)
    dsts = [_place(torch.full((B, hw), GUARD), layout, dev) for _ in range(nout)]
    dtable = dt([[v.data_ptr() for _, v in dsts], [v.stride(0) for _, v in dsts]], torch.int64)
    planes, in_idx, o_idx = dt(reduced, torch.int32), dt(shift_idx, torch.int32), dt(out_idx, torch.int32)
    ex_idx = dt(extras, torch.int32) if nextra else None
    ex_std = dt(extra_std, torch.float32) if nextra else None
    C = int(L.ace_gmr_chunks(hw))
    assert C == R.chunks(hw)
    partials = torch.full((B * K * C + 2,), GUARD, dtype=torch.float64, device=dev)
    shift = torch.full((B * K + 2,), GUARD, device=dev)
    xbuf = torch.full((4 + B * (nin + nextra) * hw + 4,), GUARD, device=dev)
    x = xbuf[4:-4]
    ydev = dt(y, torch.float32)
    d_mean, d_std, d_clim = dt(mean, torch.float32), dt(std, torch.float32), dt(clim, torch.float32)
    d_omean, d_ostd = dt(out_mean, torch.float32), dt(out_std, torch.float32)
    means = torch.full((B * K + 2,), GUARD, device=dev)
    part2 = torch.full_like(partials, GUARD)
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    got = []
    for _ in range(2):          # twice: identical bits
        _lib.check(L.ace_gmr_partials(table.data_ptr(), table.data_ptr() + 8 * nin, planes.data_ptr(), nin, partials.data_ptr() + 8,
                                      B, K, hw, stream))
        _lib.check(L.ace_gmr_pack_normalize(table.data_ptr(), table.data_ptr() + 8 * nin, d_mean.data_ptr(), d_std.data_ptr(),
                                            in_idx.data_ptr(), partials.data_ptr() + 8, d_clim.data_ptr(), p(ex_idx), p(ex_std),
                                            x.data_ptr(), shift.data_ptr() + 4, B, nin, nextra, K, hw, stream))
        _lib.check(L.ace_gmr_unpack_denormalize(ydev.data_ptr(), d_omean.data_ptr(), d_ostd.data_ptr(), dtable.data_ptr(),
                                                dtable.data_ptr() + 8 * nout, o_idx.data_ptr(), shift.data_ptr() + 4, B, nout, K, hw,
                                                stream))
        _lib.check(L.ace_gmr_sample_means(table.data_ptr(), table.data_ptr() + 8 * nin, planes.data_ptr(), nin, part2.data_ptr() + 8,
                                          means.data_ptr() + 4, B, K, hw, stream))
        torch.cuda.synchronize()
        got.append(dict(partials=partials.cpu().numpy().copy(), shift=shift.cpu().numpy().copy(), x=xbuf.cpu().numpy().copy(),
                        out=[buf.cpu().numpy().copy() for buf, _ in dsts], outs=np.stack([v.cpu().numpy() for _, v in dsts], axis=1),
                        means=means.cpu().numpy().copy(), part2=part2.cpu().numpy().copy()))
    for name in ("partials", "shift", "x", "means", "part2"):
        assert np.array_equal(got[0][name].view(np.int32), got[1][name].view(np.int32)), f"{name}: two runs differ"
    for a, b in zip(got[0]["out"], got[1]["out"]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "unpacked planes: two runs differ"
    for (buf, _), was in zip(placed, before):
        assert torch.equal(buf.view(torch.int32), was.view(torch.int32)), "a source was written"
    g = got[0]
    # guards: nothing written outside what the contract names
    assert g["partials"][0] == GUARD and g["partials"][-1] == GUARD and g["shift"][0] == GUARD and g["shift"][-1] == GUARD
    assert np.all(g["x"][:4] == GUARD) and np.all(g["x"][-4:] == GUARD) and g["means"][0] == GUARD and g["means"][-1] == GUARD
    for (buf, view), host in zip(dsts, g["out"]):
        mask = torch.ones_like(buf, dtype=torch.bool)
        torch.as_strided(mask, view.shape, view.stride(), view.storage_offset()).fill_(False)
        assert np.all(host[mask.cpu().numpy()] == GUARD), "unpack wrote outside its planes"
    want_part = np.array([[R.partials(src[b, reduced[k]]) for k in range(K)] for b in range(B)]).reshape(-1)
    want_mean = np.array([[R.sample_mean(src[b, reduced[k]]) for k in range(K)] for b in range(B)], dtype=np.float32).reshape(-1)
    return dict(src=src, got_part=g["partials"][1:-1], want_part=want_part, got_part2=g["part2"][1:-1],
                got_shift=g["shift"][1:-1].reshape(B, K), want_shift=want_shift,
                got_means=g["means"][1:-1], want_means=want_mean,
                got_x=g["x"][4:-4].reshape(B, nin + nextra, hw), want_x=want_x, got_out=g["outs"], want_out=want_out)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs differ"
    bits = np.int64 if got.dtype == np.float64 else np.int32
    bad = got.view(bits)[~nan] != want.view(bits)[~nan]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ in bits"


def _check(r):
    _same(r["got_part"], r["want_part"], "partials")
    _same(r["got_part2"], r["want_part"], "partials of ace_gmr_sample_means")
    _same(r["got_means"], r["want_means"], "sample means")
    _same(r["got_shift"], r["want_shift"], "shift buffer")
    _same(r["got_x"], r["want_x"], "packed tensor")
    _same(r["got_out"], r["want_out"], "unpacked planes")


def _shared(nin=20, nshift=11, ref=7):
    """K = 1: the reference field is channel `ref` (not the first one), every other channel up to nshift of them is listed;
    one synthetic channel; of the outputs every third is listed"""
    shift_idx = [0 if j % 2 == 1 or j == 0 else -1 for j in range(nin)]
    assert sum(1 for k in shift_idx if k == 0) == nshift and shift_idx[ref] == 0
    return dict(nin=nin, reduced=[ref], shift_idx=shift_idx, extras=[0], out_idx=[0 if j % 3 == 0 else -1 for j in range(9)])


def _per_channel(nin=20):
    """K = nin: every input has its own shift and its own synthetic channel, the reduced planes in another order than the packed
    ones; the outputs are the first (up to) 12 inputs plus two diagnostics"""
    reduced = list(range(nin - 1, -1, -1))
    k_of = {j: k for k, j in enumerate(reduced)}
    return dict(nin=nin, reduced=reduced, shift_idx=[k_of[j] for j in range(nin)], extras=list(range(nin)),
                out_idx=[k_of[j] for j in range(min(12, nin))] + [-1, -1])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [30, 128, 4050, 64800])
def test_shared_layout(dev, hw, B):
    _check(_run(dev, B, hw, **_shared()))


@pytest.mark.parametrize("hw,B", [(30, 3), (4050, 1), (64800, 3)])
def test_per_channel_layout(dev, hw, B):
    _check(_run(dev, B, hw, **_per_channel()))


@pytest.mark.parametrize("hw", [128, 64800])
def test_small_values(dev, hw):
    _check(_run(dev, 3, hw, scale="small", **_per_channel(6)))


@pytest.mark.parametrize("hw", [128, 4052, 64800])
def test_offset_planes_give_the_bits_of_aligned_ones(dev, hw):
    """the same values one float off a 16-byte boundary: the 4-byte paths of all three kernels"""
    aligned = _run(dev, 3, hw, **_shared())
    offset = _run(dev, 3, hw, layout="offset", **_shared())
    assert np.array_equal(aligned["src"], offset["src"])
    _check(offset)
    for name in ("got_part", "got_shift", "got_x", "got_out"):
        _same(offset[name], aligned[name], name + " (offset against aligned)")


@pytest.mark.parametrize("hw", [30, 64800])
def test_time_slices_of_window_buffers(dev, hw):
    """planes [:, s] of (B, T, hw) buffers: the per-sample stride is T hw"""
    _check(_run(dev, 3, hw, layout="sliced", **_shared()))
    _check(_run(dev, 1, hw, layout="sliced", **_per_channel(5)))


def test_a_nan_stays_in_its_sample_and_plane(dev):
    hw, B = 4200, 3
    case = dict(nin=6, reduced=[4, 1, 2], shift_idx=[0, 1, 2, 1, 0, -1], extras=[0, 1, 2], out_idx=[1, 2, -1, 0])
    r = _run(dev, B, hw, nan_at=(1, 1, 4100), **case)            # sample 1, channel 1 (k = 1), in the second chunk
    _check(r)
    nan_shift = np.isnan(r["got_shift"])
    assert nan_shift.sum() == 1 and nan_shift[1, 1]
    x_nan = np.isnan(r["got_x"]).all(axis=2)
    assert np.array_equal(np.isnan(r["got_x"]).any(axis=2), x_nan)            # a channel is NaN everywhere or nowhere
    want = np.zeros((B, 9), dtype=bool)
    want[1, [1, 3, 6 + 1]] = True                                           # the two channels with k = 1 and its synthetic channel
    assert np.array_equal(x_nan, want)
    out_nan = np.isnan(r["got_out"]).all(axis=2)
    assert out_nan.sum() == 1 and out_nan[1, 0]


def test_argument_checks(dev):
    from ace_amd import _lib
    L, stream = _lib.lib(), _lib.current_stream()
    t = torch.zeros(64, device=dev)
    a = t.data_ptr()
    assert L.ace_gmr_chunks(0) == 0 and L.ace_gmr_chunks(4096) == 1 and L.ace_gmr_chunks(4097) == 2
    assert L.ace_gmr_partials(a, a, a, 2, a, 0, 1, 16, stream) != 0                                   # batch < 1
    assert L.ace_gmr_partials(a, a, None, 2, a, 1, 1, 16, stream) != 0                                # null table
    assert L.ace_gmr_pack_normalize(a, a, a, a, a, a, a, None, None, a, a, 1, 2, 0, 3, 16, stream) != 0     # K > nin
    assert L.ace_gmr_pack_normalize(a, a, a, a, a, a, a, None, None, a, a, 1, 2, 1, 1, 16, stream) != 0     # extras without tables
    assert L.ace_gmr_unpack_denormalize(a, a, a, a, a, a, None, 1, 2, 1, 16, stream) != 0             # null shift
    with pytest.raises(ValueError, match="ace_gmr_sample_means"):
        _lib.check(L.ace_gmr_sample_means(a, a, a, 2, a, a, 1, 1, 0, stream))                        # hw < 1
