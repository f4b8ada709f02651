"""tests/_ensemble_ref.py, the numpy statement of the header contract of ``ace_diag_ensemble_step``, held to the reference's
``CRPSMetric``, ``EnsembleMeanRMSEMetric`` and ``SSRBiasMetric`` on tests/golden/gen_ensemble.pt ("f64": the reference's own classes
on the fp64 cast of the same fp32 fields, see tests/golden/make_golden_ensemble.py).  Both sides are fp64 sums of the same numbers
in different orders (torch's pairwise means against ascending sums): the CRPS and RMSE maps within 1e-12 of the magnitude the sums
are formed from (the field's values for the CRPS, their differences for the RMSE).  The spread-skill map divides by a clamped skill
that is 0 / 0-like wherever mse - var / E cancels, so it is compared where the reference's skill is well away from that: at cells
whose unbiased MSE exceeds 1e-3 of the field's largest, within 1e-9; the flags (0 at prescribed cells, -1 at zero skill) must agree
wherever the unbiased MSE is not within 1e-12 of the clamp.  The GPU tests hold the kernel to this statement."""
import os

import numpy as np
import pytest
import torch

import _ensemble_cases as C
import _ensemble_ref as R
from ace_amd.evaluator import ssr_bias

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_ensemble.pt")
HW = C.H * C.W


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)["f64"]


def through_the_contract(c, step):
    maps, seen = np.zeros((1, 4, len(C.NAMES), HW)), np.zeros((1, len(C.NAMES)), np.int32)
    for gen, tgt, i0 in c["windows"]:
        T = gen["a"].shape[1]
        if i0 <= step < i0 + T:
            flat = lambda d: [d[n].reshape(C.B, T, HW).numpy() for n in C.NAMES]      # noqa: E731
            R.ensemble_step(flat(gen), flat(tgt), [0, 1, 2], maps, seen, 0, step - i0, C.N_IC, C.E)
    return maps[0], seen[0]


@pytest.mark.parametrize("key,n_ic_steps,step,norm", [("en_2", 1, 2, False), ("en_5_norm", 1, 5, True), ("en_2_ic2", 2, 2, False)])
def test_the_contract_is_the_references_three_metrics(golden, key, n_ic_steps, step, norm):
    maps, seen = through_the_contract(C.case(n_ic_steps), step)
    assert seen.tolist() == [1, 1, 0]                                            # c's target is NaN everywhere
    for r, name in enumerate(C.NAMES):
        sigma = C.STDS[name] if norm else 1.0
        crps, rmse, umse, var = maps[0, r] / sigma, maps[1, r] / sigma, maps[2, r] / sigma ** 2, maps[3, r] / sigma ** 2
        want = {m: golden[key][f"x/{m}/mean_map/{name}"].reshape(-1).numpy() for m in ("crps", "ensemble_mean_rmse", "ssr_bias")}
        scale = (abs(C.MEANS[name]) + 3 * C.STDS[name]) / sigma
        for got, m in ((crps, "crps"), (rmse, "ensemble_mean_rmse")):
            assert np.array_equal(np.isnan(got), np.isnan(want[m])), (name, m)
            err = float(np.nanmax(np.abs(got - want[m]), initial=0.0))
            print(f"ENSREF {key} {m}/{name}: {err:.3e} of {scale:.3g}")
            assert err <= 1e-12 * scale, (name, m, err)
        ssr = ssr_bias(torch.from_numpy(umse), torch.from_numpy(var)).numpy()
        assert np.array_equal(np.isnan(ssr), np.isnan(want["ssr_bias"]))
        with np.errstate(invalid="ignore"):
            top = np.nanmax(np.maximum(umse, 0.0), initial=0.0)
            clear = umse > 1e-3 * top
            settled = np.abs(umse) > 1e-12 * max(top, 1e-300)
        assert float(np.max(np.abs(ssr - want["ssr_bias"])[clear], initial=0.0)) <= 1e-9
        flags = lambda x: np.stack([x == 0, x == -1])                             # noqa: E731
        assert np.array_equal(flags(ssr)[:, settled | (var == 0)], flags(want["ssr_bias"])[:, settled | (var == 0)])
    if key == "en_2":
        a = ssr_bias(torch.from_numpy(maps[2, 0]), torch.from_numpy(maps[3, 0])).reshape(C.H, C.W)
        assert bool((a[C.PRESCRIBED] == 0).all()) and bool((torch.from_numpy(maps[3, 0]).reshape(C.H, C.W)[C.PRESCRIBED] == 0).all())


def test_identical_members_give_a_variance_of_exactly_zero():
    """E g and its quotient by E are exact in fp64 for fp32 g and E <= 32, so m == g and every (g - m)^2 is +0"""
    rng = np.random.default_rng(0)
    for E in (2, 3, 7, 17, 32):
        g = (rng.standard_normal((1, 1, 64)) * 10.0 ** rng.integers(-20, 20, 64)).astype(np.float32)
        gen = np.repeat(g, E, axis=0)
        tgt = rng.standard_normal((E, 1, 64)).astype(np.float32)
        maps, seen = np.zeros((1, 4, 1, 64)), np.zeros((1, 1), np.int32)
        R.ensemble_step([gen], [tgt], [0], maps, seen, 0, 0, 1, E)
        assert np.array_equal(maps[0, 3, 0].view(np.int64), np.zeros(64, np.int64))
