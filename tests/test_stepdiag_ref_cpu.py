"""The numpy statement of the correction-metric contract (tests/_stepdiag_ref.py) against the REAL reference's three correction
aggregators run in float64 on the fp32-formed ``delta / std`` (tests/golden/gen_step_diagnostics.pt, "aggregator"/"fp64"): 1e-12."""
import numpy as np
import torch

import _stepdiag_ref as R
from _util import load_golden
from ace_amd.dataset_info import DatasetInfo

TOL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    scale = np.nanmax(np.abs(want)) if np.isfinite(want).any() else 1.0
    assert np.nanmax(np.abs(got - want), initial=0.0) <= TOL * scale, (what, np.nanmax(np.abs(got - want)), scale)


def test_statement_equals_the_reference_in_float64():
    g = load_golden("gen_step_diagnostics.pt")
    delta, stds, agg = g["rollout"]["delta"], g["rollout"]["stds"], g["aggregator"]
    want = agg["fp64"]
    names = sorted(delta)
    B, T, H, W = delta[names[0]].shape
    info = DatasetInfo((H, W), lat=torch.linspace(-78.75, 78.75, H), lon=torch.arange(float(W)) * (360.0 / W))
    assert torch.equal(info.area_weights, agg["area_weights"])                  # the fp32 weights the reference's float64 run widened
    weights = info.area_weights.reshape(1, -1).numpy().astype(np.float32)
    n_time = agg["n_timesteps"]
    signed, magnitude = np.zeros((len(names), H * W)), np.zeros((len(names), H * W))
    series, counts = np.zeros((2, len(names), n_time)), np.zeros(n_time)
    rows, wrows = list(range(len(names))), [0] * len(names)
    for sl, t0 in zip((slice(0, 2), slice(2, T)), agg["i_time_start"]):
        planes = [delta[n][:, sl].reshape(B, -1, H * W).numpy() for n in names]
        R.correction_window(planes, [stds[n] for n in names], rows, wrows, weights, signed, magnitude, series, t0)
        counts[t0:t0 + planes[0].shape[1]] += 1
    denom = T * B
    with np.errstate(invalid="ignore", divide="ignore"):
        per_index = series / counts
    for r, n in enumerate(names):
        _close(signed[r], want["signed_sum"][n].reshape(-1), f"signed_sum {n}")
        _close(magnitude[r], want["magnitude_sum"][n].reshape(-1), f"magnitude_sum {n}")
        _close(signed[r] / denom, want["signed"][n].reshape(-1), f"signed {n}")
        w = weights[0].astype(np.float64)
        _close((w * magnitude[r] / denom).sum() / w.sum(), want["correction_magnitude"][n], f"correction_magnitude {n}")
        _close(per_index[0, r], want["series"]["weighted_correction_magnitude"][n], f"magnitude series {n}")
        _close(per_index[1, r], want["series"]["weighted_correction_std"][n], f"std series {n}")
    assert np.isnan(per_index[0, 0, 0]) and np.isnan(per_index[0, 0, 4])       # indices never recorded
