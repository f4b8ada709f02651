"""csrc/stepdiag.hip on the device against the numpy statement of its contract (tests/_stepdiag_ref.py, itself held to the real
reference in float64 by tests/test_stepdiag_ref_cpu.py): the snapshot and delta kernels bit for bit, the per-pixel sums of the
metric kernel bit for bit, its series to 1e-12 relative - the bar tests/test_gpu_diag_kernels.py holds for the same reduction scheme
(two-pass moments per wave, Chan's merge in a fixed order).

Shapes, the smallest at which each branch can go wrong: hw = 9 x 18 = 162 (under one chunk, under a wave's 256 pixels in its last
wave), 32 x 64 = 2048 (two full chunks, the 16-byte path), 45 x 90 = 4050 (a ragged fourth chunk, not a multiple of 4: the 4-byte
path)."""
import numpy as np
import pytest
import torch

import _stepdiag_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(9, 18), (32, 64), (45, 90)]
TOL = 1e-12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _lib():
    from ace_amd import _lib
    return _lib


def _check(rc):
    from ace_amd.aggregator import _check as check
    check(rc)


def _i64(values, dev):
    return torch.tensor(values, dtype=torch.int64, device=dev)


def _planes(g, K, B, T, hw, dev, offset=0, pad=0):
    """K fields of (B, T, hw) fp32 inside one allocation, each starting ``offset`` floats past a 16-byte boundary, with ``pad``
    extra floats between samples (a non-contiguous sample stride)"""
    per = B * (T * hw + pad)
    per_aligned = (per + offset + 3) // 4 * 4
    store = torch.zeros(K * per_aligned + 4, device=dev)
    views = []
    for k in range(K):
        flat = store[k * per_aligned + offset: k * per_aligned + offset + per]
        v = flat.as_strided((B, T, hw), (T * hw + pad, hw, 1))
        v.copy_(torch.randn(B, T, hw, generator=g).to(dev))
        views.append(v)
    return store, views


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("B,T,K", [(1, 1, 1), (3, 5, 5)])
@pytest.mark.parametrize("offset", [0, 1])
def test_snapshot_and_delta_are_bitwise(dev, H, W, B, T, K, offset):
    L, hw = _lib(), H * W
    g = torch.Generator().manual_seed(H * 1000 + B * 10 + offset)
    keep_o, outs = _planes(g, K, B, T, hw, dev, offset=offset, pad=4 if offset == 0 else 3)
    keep_s, snaps = _planes(g, K, B, T, hw, dev, offset=offset)
    for v in snaps:
        v.zero_()
    stream = L.current_stream()
    before = [o.cpu().numpy().copy() for o in outs]
    for s in range(T):                                                    # the planes of step s into time slot s
        src = _i64([o[:, s].data_ptr() for o in outs], dev)
        dst = _i64([q[:, s].data_ptr() for q in snaps], dev)
        sstr, dstr = _i64([o.stride(0) for o in outs], dev), _i64([q.stride(0) for q in snaps], dev)
        _check(L.lib().ace_stepdiag_snapshot(src.data_ptr(), sstr.data_ptr(), dst.data_ptr(), dstr.data_ptr(), K, B, hw, stream))
    torch.cuda.synchronize()
    for k in range(K):
        assert np.array_equal(snaps[k].cpu().numpy(), R.snapshot(before[k])), k
        assert np.array_equal(outs[k].cpu().numpy(), before[k]), k
    guard = keep_s.clone()
    for o in outs:                                                        # "the corrector" edits the outputs in place
        o.add_(torch.randn(B, T, hw, generator=g).to(dev) * 1e-3)
    after = [o.cpu().numpy().copy() for o in outs]
    optr, sptr = _i64([o.data_ptr() for o in outs], dev), _i64([q.data_ptr() for q in snaps], dev)
    ostr = _i64([v for o in outs for v in o.stride()[:2]], dev)
    sstr = _i64([v for q in snaps for v in q.stride()[:2]], dev)
    _check(L.lib().ace_stepdiag_delta_window(optr.data_ptr(), ostr.data_ptr(), sptr.data_ptr(), sstr.data_ptr(), K, B, T, hw, stream))
    torch.cuda.synchronize()
    for k in range(K):
        assert np.array_equal(snaps[k].cpu().numpy(), R.delta(after[k], before[k])), k
        assert np.array_equal(outs[k].cpu().numpy(), after[k]), k
    # nothing outside the planes was written: the floats between the fields and in front of an offset field
    mask = torch.ones_like(keep_s, dtype=torch.bool)
    per = B * T * hw
    per_aligned = (per + offset + 3) // 4 * 4
    for k in range(K):
        mask[k * per_aligned + offset: k * per_aligned + offset + per] = False
    assert torch.equal(keep_s[mask], guard[mask])


def _weights(H, W, dev, offset):
    lat = torch.tensor([-90 + (i + 0.5) * 180 / H for i in range(H)], dtype=torch.float64)
    area = torch.cos(torch.deg2rad(lat)).float()[:, None].expand(H, W).contiguous()
    masked = area.clone()
    masked[: H // 3] = 0.0                                                # rows of weight 0
    none = torch.zeros(H, W)                                              # a weight row with no weighted pixel
    table = torch.stack([area, masked, none]).reshape(3, -1)
    store = torch.zeros(table.numel() + 4, device=dev)
    view = store[offset: offset + table.numel()].view(3, -1)
    view.copy_(table.to(dev))
    return store, view, table.numpy()


def _run(dev, views, stds, rows, wrows, wview, nrows, n_time, t0, acc=None):
    L = _lib()
    K = len(views)
    B, T, hw = views[0].shape
    if acc is None:
        acc = (torch.zeros(nrows, hw, dtype=torch.float64, device=dev), torch.zeros(nrows, hw, dtype=torch.float64, device=dev),
               torch.zeros(2, nrows, n_time, dtype=torch.float64, device=dev))
    sgn, mag, series = acc
    ptrs = _i64([v.data_ptr() for v in views], dev)
    strides = _i64([s for v in views for s in v.stride()[:2]], dev)
    std_t = torch.tensor(stds, dtype=torch.float32, device=dev)
    rows_t = torch.tensor(rows, dtype=torch.int32, device=dev)
    wrows_t = torch.tensor(wrows, dtype=torch.int32, device=dev)
    partial = torch.empty(int(L.lib().ace_diag_correction_partial_doubles(K, B, T, hw)), dtype=torch.float64, device=dev)
    _check(L.lib().ace_diag_correction_window(ptrs.data_ptr(), strides.data_ptr(), std_t.data_ptr(), rows_t.data_ptr(),
                                              wrows_t.data_ptr(), wview.data_ptr(), wview.shape[0], partial.data_ptr(), sgn.data_ptr(),
                                              mag.data_ptr(), series.data_ptr(), nrows, n_time, t0, K, B, T, hw, L.current_stream()))
    torch.cuda.synchronize()
    return acc


def _statement(views, stds, rows, wrows, wtable, nrows, n_time, t0, acc=None):
    hw = views[0].shape[-1]
    if acc is None:
        acc = (np.zeros((nrows, hw)), np.zeros((nrows, hw)), np.zeros((2, nrows, n_time)))
    R.correction_window([v.cpu().numpy() for v in views], stds, rows, wrows, wtable, acc[0], acc[1], acc[2], t0)
    return acc


def _compare(got, want, what):
    for name, g, w in zip(("signed", "magnitude"), got[:2], want[:2]):
        assert np.array_equal(g.cpu().numpy(), w, equal_nan=True), (what, name)          # the per-pixel sums: bit for bit
    g, w = got[2].cpu().numpy(), want[2]
    assert np.array_equal(np.isnan(g), np.isnan(w)), what
    fin = np.isfinite(w)
    scale = np.abs(w[fin]).max() if fin.any() else 1.0
    print(what, "series: max |error| / scale", float(np.abs(g[fin] - w[fin]).max() / scale) if fin.any() else 0.0)
    assert np.abs(g[fin] - w[fin]).max(initial=0.0) <= TOL * scale, what


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("B,T,K", [(1, 1, 1), (3, 5, 5)])
@pytest.mark.parametrize("offset", [0, 1])
def test_correction_window_matches_the_statement(dev, H, W, B, T, K, offset):
    hw = H * W
    g = torch.Generator().manual_seed(H + 7 * B + offset)
    keep, views = _planes(g, K, B, T, hw, dev, offset=offset, pad=0 if offset else 8)       # pad: a non-contiguous sample stride
    wkeep, wview, wtable = _weights(H, W, dev, offset)
    stds = [0.3 + 0.7 * k for k in range(K)]
    nrows, n_time = K + 1, T + 3
    rows = [(k + 1) % (K + 1) for k in range(K)]                          # a permutation with a hole
    wrows = [k % 2 for k in range(K)]                                     # the area weights and the masked ones
    if K > 1:
        views[1][:, :, : (H // 3) * W] = float("nan")                     # NaN deltas under the zero-weight rows of weight row 1
    first = _run(dev, views, stds, rows, wrows, wview, nrows, n_time, 0)
    want = _statement(views, stds, rows, wrows, wtable, nrows, n_time, 0)
    _compare(first, want, "window 0")
    if K > 1:
        r = rows[1]
        assert torch.isfinite(first[2][:, r, :T]).all()                   # the series skip the zero-weight NaNs ...
        assert torch.isnan(first[0][r, : (H // 3) * W]).all() and torch.isnan(first[1][r, : (H // 3) * W]).all()      # ... the maps keep them
        assert torch.isfinite(first[0][r, (H // 3) * W:]).all()
    # a second window accumulates at t0 > 0
    for v in views:
        v.mul_(0.5)
    second = _run(dev, views, stds, rows, wrows, wview, nrows, n_time, 2, acc=first)
    want = _statement(views, stds, rows, wrows, wtable, nrows, n_time, 2, acc=want)
    _compare(second, want, "window 1")
    assert float(second[2][:, rows[0], T + 2].abs().sum()) == 0.0         # past the second window: untouched
    # a repeat run on fresh accumulators equals the first bit for bit
    for v in views:
        v.mul_(2.0)
    again = _run(dev, views, stds, rows, wrows, wview, nrows, n_time, 0)
    fresh = _statement(views, stds, rows, wrows, wtable, nrows, n_time, 0)
    _compare(again, fresh, "repeat")
    twice = _run(dev, views, stds, rows, wrows, wview, nrows, n_time, 0)
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(again, twice))


def test_nan_propagation_empty_samples_and_out_of_range_rows(dev):
    H, W, B, T, K = 9, 18, 2, 2, 4
    hw = H * W
    g = torch.Generator().manual_seed(3)
    keep, views = _planes(g, K, B, T, hw, dev)
    wkeep, wview, wtable = _weights(H, W, dev, 0)
    views[0][1, 0, hw - 1] = float("nan")                                 # a NaN at non-zero weight: that sample's step is NaN
    stds = [1.0, 2.0, 0.5, 3.0]
    rows, wrows = [0, 1, 7, 2], [0, 2, 0, 5]                              # plane 1: no weighted pixel; 2: row out of range; 3: weight row out of range
    nrows, n_time = 4, T
    acc = tuple(torch.full_like(a, 1.25) for a in _run(dev, views, stds, rows, wrows, wview, nrows, n_time, 0))
    got = _run(dev, views, stds, rows, wrows, wview, nrows, n_time, 0, acc=acc)
    want = _statement(views, stds, rows, wrows, wtable, nrows, n_time, 0,
                      acc=(np.full((nrows, hw), 1.25), np.full((nrows, hw), 1.25), np.full((2, nrows, n_time), 1.25)))
    _compare(got, want, "edge cases")
    series = got[2].cpu()
    assert torch.isnan(series[:, 0, 0]).all() and torch.isfinite(series[:, 0, 1]).all()           # the NaN propagates to its step only
    assert torch.isnan(series[:, 1]).all()                                                        # no weighted pixel: NaN
    assert torch.isfinite(got[0][1]).all()                                                        # ... but its maps are plain sums
    for a in got:                                                                                 # rows 2 and 3: bitwise untouched
        rows_of = a[2:] if a.dim() == 2 else a[:, 2:]
        assert torch.equal(rows_of, torch.full_like(rows_of, 1.25))


def test_refusals(dev):
    L = _lib()
    with pytest.raises(ValueError, match="ace_diag_correction_window"):
        _check(L.lib().ace_diag_correction_window(None, None, None, None, None, None, 1, None, None, None, None, 1, 4, 3, 1, 1, 2, 16,
                                                  L.current_stream()))      # t0 + steps > n_time
    with pytest.raises(ValueError, match="ace_stepdiag_delta_window"):
        _check(L.lib().ace_stepdiag_delta_window(None, None, None, None, 1, 70000, 1, 16, L.current_stream()))
    assert L.lib().ace_diag_correction_partial_doubles(2, 3, 5, 4050) == 2 * 3 * 5 * 4 * 4 * 4
