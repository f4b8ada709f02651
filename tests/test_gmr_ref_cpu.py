"""The numpy statement of the global-mean-removal contract (tests/_gmr_ref.py; include/ace_sfno.h "Global-mean removal") held to
what it restates: its sample mean to the exactly rounded mean of the plane, its pack / synthetic channels / unpack to the torch
ops of the reference's formulas (fme/core/step/global_mean_removal.py, fme/core/normalizer.py:221, :236)."""
import math

import numpy as np
import pytest
import torch

import _gmr_ref as R

SIZES = [30, 128, 4050, 64800]


def _plane(hw, seed=0):
    rng = np.random.default_rng(seed + hw)
    return (288.0 + rng.uniform(-30.0, 30.0, size=hw)).astype(np.float32)


def _ulps(a: np.float32, b: np.float32) -> int:
    """distance of two positive finite fp32 values in units of the last place"""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def _exact_mean(x):
    return np.float32(math.fsum(float(v) for v in x) / x.size)


@pytest.mark.parametrize("hw", SIZES)
def test_sample_mean_within_one_ulp_of_the_exact_mean(hw):
    for seed in range(3):
        x = _plane(hw, seed)
        assert R.partials(x).shape == (R.chunks(hw),)
        assert _ulps(R.sample_mean(x), _exact_mean(x)) <= 1, (hw, seed, R.sample_mean(x), _exact_mean(x))


def test_a_running_fp32_sum_misses_that_bar_at_the_workload_plane():
    """the bar has teeth: the plain fp32 accumulation it rules out is off by many ulps at 64800 pixels"""
    x = _plane(64800)
    s = np.float32(0.0)
    for v in x:
        s = np.float32(s + v)
    naive = np.float32(s / np.float32(x.size))
    assert _ulps(naive, _exact_mean(x)) > 1, (naive, _exact_mean(x))
    assert _ulps(R.sample_mean(x), _exact_mean(x)) <= 1


def test_chunk_layout():
    assert [R.chunks(n) for n in (1, 4096, 4097, 64800)] == [1, 1, 2, 16]
    # a chunk's sum does not see what lies past the plane: padding the plane with zeros to whole chunks changes nothing
    x = _plane(4050)
    assert R.partials(x)[0] == R.partials(np.concatenate([x, np.zeros(46, np.float32)]))[0]
    # exactly representable data: the order cannot matter, the sum is exact
    ints = np.arange(1, 5001, dtype=np.float32)
    assert float(R.partials(ints).sum()) == 5000 * 5001 / 2


def test_nan_propagates():
    x = _plane(4200)
    x[4100] = np.nan
    p = R.partials(x)
    assert np.isfinite(p[0]) and np.isnan(p[1]) and np.isnan(R.sample_mean(x)) and np.isnan(R.shift_of(287.0, x))


@pytest.mark.parametrize("hw", [30, 4050])
def test_pack_extras_unpack_equal_the_torch_ops_of_the_reference(hw):
    x = _plane(hw, 5)
    t = torch.from_numpy(x.copy())[None]                    # [batch = 1, hw]
    clim, mean, std = np.float32(287.3), np.float32(286.9), np.float32(5.3)
    shift = R.shift_of(clim, x)
    ts = torch.tensor([float(shift)], dtype=torch.float32)
    # forward_transform (global_mean_removal.py:246-247 / :321-322), then normalizer.py:221
    want = ((t + ts.view(1, 1)) - torch.tensor(float(mean))) / torch.tensor(float(std))
    assert np.array_equal(R.pack(x, shift, mean, std), want[0].numpy())
    assert np.array_equal(R.pack(x, None, mean, std), ((t - torch.tensor(float(mean))) / torch.tensor(float(std)))[0].numpy())
    # the synthetic channel (global_mean_removal.py:236 / :329)
    assert R.extra(shift, std) == (-ts / torch.tensor(float(std))).numpy()[0]
    # normalizer.py:236, then inverse_transform (global_mean_removal.py:264-265 / :346-347)
    y = torch.from_numpy(np.random.default_rng(1).standard_normal(hw).astype(np.float32))[None]
    back = (y * torch.tensor(float(std)) + torch.tensor(float(mean))) - ts.view(1, 1)
    assert np.array_equal(R.unpack(y[0].numpy(), shift, mean, std), back[0].numpy())
    assert np.array_equal(R.unpack(y[0].numpy(), None, mean, std), (y * torch.tensor(float(std)) + torch.tensor(float(mean)))[0].numpy())
    # and the shift itself is the reference's fp32 subtraction from the stated mean
    assert shift == (torch.tensor(float(clim)) - torch.tensor(float(R.sample_mean(x)))).item()
