"""tests/_video_ref.py, the numpy statement of ``ace_diag_video_window``'s header contract, and ``video_frames`` against
tests/golden/gen_video.pt, which tests/golden/make_golden_video.py made with the reference's own ``VideoAggregator`` and
``_make_video`` (fme/ace/aggregator/inference/video.py).

Bars, derived: the reference takes fp32 means over the B samples and adds them into fp64; the statement sums in fp64.  With
u = 2^-24, N visits of a slot, m = max |x| and m_d = max |gen - target|, an fp32 mean of B values is within B u m of the exact
one, and squaring first adds one rounding, so the accumulators agree within
  N B u m (the means),   N (B + 1) u m^2 (the squares),   N (B + 1) u m_d^2 (the squared error).
The derived means divide both by N.  min_err and max_err subtract in fp32 on both sides: equal as values.  gen_var is a
cancelling difference and is not compared with the reference's value; it is held to the formula on the statement's accumulators.
The worst measured case of each bar is printed under the tag VIDEOACC."""
import os

import numpy as np
import pytest
import torch

import _video_ref as R
from ace_amd.evaluator import video_frames

U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_video.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def scales(golden, name):
    """(m of the generated side, m of the target side, m_d) over every visit"""
    mg = max(float(gen[name].abs().max()) for _, gen, _ in golden["visits"])
    mt = max(float(np.nanmax(tgt[name].abs().numpy())) for _, _, tgt in golden["visits"])
    md = max(float(np.nanmax((gen[name] - tgt[name]).abs().numpy())) for _, gen, tgt in golden["visits"])
    return mg, mt, md


def within(got, want, bar, what):
    """NaN and infinities in the same places, the rest within ``bar``; prints the measured worst case as a fraction of it"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite), what
    assert np.array_equal(got[~finite], want[~finite], equal_nan=True), what
    worst = float(np.abs(got[finite] - want[finite]).max()) if finite.any() else 0.0
    print(f"VIDEOACC {what}: worst {worst:.3e} bar {bar:.3e} ratio {worst / bar:.3f}")
    assert worst <= bar, (what, worst, bar)


def statement(golden, names=("a", "m")):
    """the statement's accumulators after every visit of the golden, and the visit counts"""
    n_time = golden["n_timesteps"]
    hw = golden["mask"].numel()
    mean, sq, err = R.new_buffers(len(names), n_time, hw)
    n = np.zeros(n_time, np.int64)
    for t0, gen, tgt in golden["visits"]:
        T = gen[names[0]].shape[1]
        flat = lambda d: [d[k].numpy().reshape(d[k].shape[0], T, hw) for k in names]      # noqa: E731
        R.video_window(flat(gen), flat(tgt), list(range(len(names))), mean, sq, err, t0, assign=not n[t0:t0 + T].any())
        n[t0:t0 + T] += 1
    return mean, sq, err, n


def test_visit_counts(golden):
    *_, n = statement(golden)
    assert np.array_equal(n, golden["n_batches"].numpy()) and n[0] == 0 and n.max() == 2


@pytest.mark.parametrize("row,name", [(0, "a"), (1, "m")])
def test_accumulators_within_the_derived_bars(golden, row, name):
    mean, sq, err, n = statement(golden)
    acc, B, N = golden["acc"], 3, int(n.max())
    mg, mt, md = scales(golden, name)
    flat = lambda t: t.numpy().reshape(t.shape[0], -1)      # noqa: E731
    within(mean[0, row], flat(acc["gen"][name]), N * B * U * mg, f"{name} gen mean")
    within(mean[1, row], flat(acc["target"][name]), N * B * U * mt, f"{name} target mean")
    within(mean[0, row], flat(acc["var_gen"][name]), N * B * U * mg, f"{name} gen mean (variance recorder)")
    within(mean[1, row], flat(acc["var_target"][name]), N * B * U * mt, f"{name} target mean (variance recorder)")
    within(sq[0, row], flat(acc["gen_sq"][name]), N * (B + 1) * U * mg ** 2, f"{name} gen square")
    within(sq[1, row], flat(acc["target_sq"][name]), N * (B + 1) * U * mt ** 2, f"{name} target square")
    within(sq[2, row], flat(acc["mse"][name]), N * (B + 1) * U * md ** 2, f"{name} squared error")
    for c, key in ((0, "min_err"), (1, "max_err")):
        assert np.array_equal(err[c, row].astype(np.float64), flat(acc[key][name]), equal_nan=True), key


@pytest.mark.parametrize("row,name", [(0, "a"), (1, "m")])
def test_derived_quantities(golden, row, name):
    mean, sq, err, n = statement(golden)
    d, B = R.derived(mean, sq, err, row, n), 3
    mg, mt, md = scales(golden, name)
    data = golden["data"]
    flat = lambda t: t.numpy().reshape(t.shape[0], -1)      # noqa: E731
    within(d["name"][0], flat(data[name][0]), B * U * mg, f"{name} prediction")
    within(d["name"][1], flat(data[name][1]), B * U * mt, f"{name} target")
    within(d["bias"], flat(data[f"bias/{name}"][0]), B * U * (mg + mt), f"{name} bias")
    within(d["rmse"] ** 2, flat(data[f"rmse/{name}"][0]) ** 2, (B + 1) * U * md ** 2, f"{name} rmse^2")
    assert np.array_equal(d["min_err"], flat(data[f"min_err/{name}"][0]), equal_nan=True)
    assert np.array_equal(d["max_err"], flat(data[f"max_err/{name}"][0]), equal_nan=True)
    # the unvisited slot: NaN, and the fills of the extrema
    assert np.isnan(d["name"][:, 0]).all() and np.isnan(d["bias"][0]).all() and np.isnan(d["rmse"][0]).all()
    assert np.isnan(d["gen_var"][0]).all()
    assert (d["min_err"][0] == np.inf).all() and (d["max_err"][0] == -np.inf).all()
    # gen_var: the formula on the statement's own accumulators
    with np.errstate(invalid="ignore", divide="ignore"):
        nn = n.astype(np.float64)[:, None]
        want = (sq[0, row] / nn - (mean[0, row] / nn) ** 2) / (sq[1, row] / nn - (mean[1, row] / nn) ** 2)
    assert np.array_equal(d["gen_var"], want, equal_nan=True)
    assert np.isfinite(d["gen_var"][1:][:, ~golden["mask"].reshape(-1).numpy()] if name == "m" else d["gen_var"][1:]).all()


def test_key_order_of_the_reference(golden):
    assert golden["keys"] == ["a", "bias/a", "m", "bias/m", "rmse/a", "rmse/m", "min_err/a", "min_err/m", "max_err/a", "max_err/m",
                              "gen_var/a", "gen_var/m"]


def test_a_plane_without_target_and_rows_out_of_range():
    g = np.random.default_rng(0)
    x, y = g.standard_normal((2, 3, 2, 5)).astype(np.float32)
    mean, sq, err = R.new_buffers(2, 4, 5)
    R.video_window([x, x, x, x], [None, y, y, y], [1, -1, 2, 0], mean, sq, err, 1)
    assert (mean[1, 1] == 0).all() and (sq[1:, 1] == 0).all() and (err[0, 1] == np.inf).all() and (err[1, 1] == -np.inf).all()
    assert (mean[0, 1, 1:3] != 0).all() and (sq[0, 1, 1:3] != 0).all() and (mean[:, :, 0] == 0).all() and (mean[:, :, 3] == 0).all()
    assert (sq[2, 0, 1:3] > 0).all()
    d = R.derived(mean, sq, err, 1, [0, 1, 1, 0], paired=False)
    assert list(d) == ["name"] and np.isnan(d["name"][1]).all() and np.isfinite(d["name"][0, 1:3]).all()


def test_nan_rule_and_assign():
    x = np.zeros((3, 1, 4), np.float32)
    y = np.zeros((3, 1, 4), np.float32)
    x[1, 0, 0] = np.nan                                       # a NaN in the middle sample
    x[0, 0, 1], x[2, 0, 1] = 3.0, -2.0
    x[0, 0, 2] = np.inf
    mean, sq, err = R.new_buffers(1, 1, 4)
    mean[:], sq[:], err[:] = 7.0, 7.0, 7.0
    R.video_window([x], [y], [0], mean, sq, err, 0, assign=True)
    assert np.isnan(err[:, 0, 0, 0]).all() and np.isnan(mean[0, 0, 0, 0]) and mean[1, 0, 0, 0] == 0.0
    assert err[0, 0, 0, 1] == -2.0 and err[1, 0, 0, 1] == 3.0 and mean[0, 0, 0, 1] == 1.0 / 3.0
    assert err[1, 0, 0, 2] == np.inf and err[0, 0, 0, 2] == 0.0 and mean[0, 0, 0, 2] == np.inf
    assert err[0, 0, 0, 3] == 0.0 and err[1, 0, 0, 3] == 0.0 and sq[2, 0, 0, 3] == 0.0
    x[1, 0, 0] = 1.0
    R.video_window([x], [y], [0], mean, sq, err, 0)             # a stored NaN stays, the sums add
    assert np.isnan(err[:, 0, 0, 0]).all() and mean[0, 0, 0, 1] == 2.0 / 3.0


@pytest.mark.parametrize("key", ["a", "m", "rmse/a"])
def test_video_frames_equal_the_reference(golden, key):
    gen, target = golden["data"][key]
    want, caption = golden["make_video"][key]
    frames, vmin, vmax = video_frames(gen, target)
    assert frames.dtype == np.float64 and np.array_equal(frames, want.numpy())
    assert frames.shape == (7, 3, 5, 9 if target is None else 28)
    scale = (gen if target is None else target).numpy()
    assert vmin == np.nanmin(scale) and vmax == np.nanmax(scale)
    assert caption.endswith(f"; vmin={vmin:.4g}, vmax={vmax:.4g}")
    again = video_frames(gen.numpy(), None if target is None else target.numpy())
    assert np.array_equal(again[0], frames) and again[1:] == (vmin, vmax)
