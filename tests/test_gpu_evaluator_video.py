"""The evaluator's video metric on the fused path (csrc/video.hip: one ace_diag_video_window per window) against the module's own
torch path on the same device tensors, against tests/_video_ref.py (exactly) and against tests/golden/gen_video.pt.

Bars, as tests/test_video_ref_cpu.py derives them: the torch path takes fp32 means over the B samples, the fused path fp64 sums
rounded once, so with u = 2^-24 the means agree within B u m, the bias within B u (m_gen + m_target) and rmse^2 within
(B + 1) u m_d^2 (every slot divides its N visits by N); the extrema subtract in fp32 on both paths and agree as values; gen_var,
a cancelling difference, is held to the formula on the path's own accumulators."""
import numpy as np
import pytest
import torch

import _video_ref as R
from ace_amd.evaluator import VideoMetricConfig
from ace_amd.normalizer import StandardNormalizer
from test_evaluator_video_cpu import B, N_TIME, check_against_golden, check_gen_var, config, golden, info  # noqa: F401
from test_gpu_diag_kernels import dev  # noqa: F401
from test_video_ref_cpu import U, within

pytestmark = pytest.mark.gpu

NAMES = ("a", "m", "c")
WINDOWS = ((1, 2), (3, 3))                             # slots 0 and 6 of 7 are never visited


def build(dev, video, grid, fused=True):
    norm = StandardNormalizer({n: 280.0 for n in NAMES}, {n: 15.0 for n in NAMES}, device=dev)
    agg = config(video).build(info(*grid), 1, N_TIME - 1, normalize=norm)
    agg.fused = fused
    return agg


def visits(grid, seed=0):
    """two windows, each visited twice with fresh data; the target of "m" is NaN at a fixed mask"""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(grid, generator=g) < 0.25
    out = []
    for _ in range(2):
        for t0, T in WINDOWS:
            gen = {n: (280.0 + 15.0 * torch.randn(B, T, *grid, generator=g)).float() for n in NAMES}
            tgt = {n: (gen[n] + 2.0 * torch.randn(B, T, *grid, generator=g)).float() for n in NAMES}
            tgt["m"][..., mask] = float("nan")
            out.append((t0, gen, tgt))
    return out


def replay(agg, vs, dev, view=lambda x: x):
    for t0, gen, tgt in vs:
        agg._n_seen = t0                                # the second pass over the same slots rewinds the step counter
        gen, tgt = {k: view(v.to(dev)) for k, v in gen.items()}, {k: view(v.to(dev)) for k, v in tgt.items()}
        assert agg.route(gen, tgt) == ("fused" if agg.fused else "torch")
        agg.record_batch(gen, tgt)
    return agg


def scales(vs, name):
    mg = max(float(gen[name].abs().max()) for _, gen, _ in vs)
    mt = max(float(np.nanmax(tgt[name].abs().numpy())) for _, _, tgt in vs)
    md = max(float(np.nanmax((gen[name] - tgt[name]).abs().numpy())) for _, gen, tgt in vs)
    return mg, mt, md


def same_bytes(a, b):
    assert list(a) == list(b)
    for k in a:
        assert np.array_equal(a[k].numpy().view(np.int64), b[k].numpy().view(np.int64)), k


@pytest.mark.parametrize("grid", [(5, 9), (6, 7), (4, 8)])          # H W = 45, 42 (no multiple of 4) and 32
@pytest.mark.parametrize("extended", [True, False])
def test_fused_against_the_torch_path_and_the_statement(dev, grid, extended):
    vs = visits(grid)
    cfg = VideoMetricConfig(enabled=True, enable_extended_videos=extended, variables=["m", "a"])
    fused, torch_ = replay(build(dev, cfg, grid), vs, dev), replay(build(dev, cfg, grid, fused=False), vs, dev)
    assert fused._path == "fused" and torch_._path == "torch"
    got, want = fused.get_dataset()["video"], torch_.get_dataset()["video"]
    assert list(got) == list(want) and "c" not in got and len(got) == (12 if extended else 2)
    for name in ("a", "m"):
        mg, mt, md = scales(vs, name)
        within(got[name][0], want[name][0], B * U * mg, f"{grid} {name} prediction")
        within(got[name][1], want[name][1], B * U * mt, f"{grid} {name} target")
        assert torch.isnan(got[name][:, [0, 6]]).all()
        if extended:
            within(got[f"bias_{name}"], want[f"bias_{name}"], B * U * (mg + mt), f"{grid} {name} bias")
            within(got[f"rmse_{name}"] ** 2, want[f"rmse_{name}"] ** 2, (B + 1) * U * md ** 2, f"{grid} {name} rmse^2")
            for key, fill in (("min_err", np.inf), ("max_err", -np.inf)):
                assert np.array_equal(got[f"{key}_{name}"].numpy(), want[f"{key}_{name}"].numpy(), equal_nan=True), key
                assert (got[f"{key}_{name}"][[0, 6]] == fill).all()
    if extended:
        check_gen_var(fused, got)
        check_gen_var(torch_, want)
    # the statement, exactly: the same windows into the same rows
    v, hw = fused._video, grid[0] * grid[1]
    assert sorted(v._rows) == ["a", "m"] and v._n.tolist() == [0, 2, 2, 2, 2, 2, 0]
    names = sorted(v._rows, key=v._rows.get)
    mean, sq, err = R.new_buffers(2, N_TIME, hw, extended)
    n = np.zeros(N_TIME, np.int64)
    for t0, gen, tgt in vs:
        T = gen["a"].shape[1]
        R.video_window([gen[k].numpy().reshape(B, T, hw) for k in names], [tgt[k].numpy().reshape(B, T, hw) for k in names], [0, 1],
                       mean, sq, err, t0, assign=not n[t0:t0 + T].any())
        n[t0:t0 + T] += 1
    for buf, ref in ((v._mean, mean), (v._sq, sq)):
        if ref is not None:
            mine = buf.cpu().numpy()
            nan = np.isnan(ref)
            assert np.array_equal(np.isnan(mine), nan) and np.array_equal(mine[~nan].view(np.int64), ref[~nan].view(np.int64))
    assert (v._sq is None and v._err is None) if not extended else np.array_equal(v._err.cpu().numpy(), err, equal_nan=True)


def test_launches_grow_by_one_per_window(dev):
    vs = visits((5, 9))
    on = build(dev, VideoMetricConfig(enabled=True, enable_extended_videos=True), (5, 9))
    off = build(dev, VideoMetricConfig(), (5, 9))
    counts = []
    for visit in vs:
        replay(on, [visit], dev), replay(off, [visit], dev)
        counts.append(on.launches() - off.launches())
    assert counts == [1, 2, 3, 4] and off._video is None


def test_a_transposed_window_and_two_fresh_aggregators(dev):
    grid, vs = (5, 9), visits((5, 9), seed=1)
    cfg = VideoMetricConfig(enabled=True, enable_extended_videos=True)
    plain = replay(build(dev, cfg, grid), vs, dev).get_dataset()["video"]
    again = replay(build(dev, cfg, grid), vs, dev).get_dataset()["video"]
    same_bytes(plain, again)                                                  # bitwise repeatable
    transposed = lambda x: x.transpose(-1, -2).contiguous().transpose(-1, -2)      # noqa: E731  (same values, planes not contiguous)
    assert not transposed(torch.zeros(1, 1, 5, 9)).is_contiguous()
    same_bytes(plain, replay(build(dev, cfg, grid), vs, dev, view=transposed).get_dataset()["video"])


def test_a_prediction_without_target(dev):
    grid, vs = (5, 9), visits((5, 9), seed=2)
    cfg = VideoMetricConfig(enabled=True, enable_extended_videos=True)
    full = replay(build(dev, cfg, grid), vs, dev).get_dataset()["video"]
    agg = build(dev, cfg, grid)
    for t0, gen, tgt in vs:
        agg._n_seen = t0
        agg.record_batch({k: v.to(dev) for k, v in gen.items()}, {k: v.to(dev) for k, v in tgt.items() if k != "c"})
    ds = agg.get_dataset()["video"]
    assert [k for k in full if k not in ds] == ["bias_c", "rmse_c", "min_err_c", "max_err_c", "gen_var_c"]
    assert torch.isnan(ds["c"][1]).all() and np.array_equal(ds["c"][0].numpy(), full["c"][0].numpy(), equal_nan=True)
    same_bytes({k: v for k, v in ds.items() if k != "c"}, {k: full[k] for k in ds if k != "c"})


def test_the_golden_through_the_fused_path(dev, golden):  # noqa: F811
    agg = build(dev, VideoMetricConfig(enabled=True, enable_extended_videos=True), (5, 9))
    replay(agg, golden["visits"], dev)
    ds = agg.get_dataset()["video"]
    assert list(ds) == [k.replace("/", "_") for k in golden["keys"]]
    check_against_golden(ds, golden)
    check_gen_var(agg, ds)
