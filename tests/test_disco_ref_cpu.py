"""The header's statement of ``ace_disco_forward`` (tests/_disco_ref.py, what the GPU tests hold the kernel to bit for bit) against
the fp64 truth of every golden case (tests/golden/gen_ankur_*.pt): the net evaluated through the statements (the module on the
emulation, tests/_fake_ankur.py; for ReLU also the composed numpy statement itself) errs no more than 2 x the reference's own fp32
forward does - both are fp32 sums of the same terms in different orders.  NaN positions of the statement equal those of a direct
fp64 sum over the table.

max |y - truth| / max |truth|, statement / reference: disco_gelu 2.5e-7 / 2.6e-7, disco_relu_embed 2.3e-7 / 2.9e-7,
disco_silu_embed 1.3e-7 / 1.2e-7, depthwise_relu 2.3e-7 / 2.6e-7, conv_gelu_embed 2.2e-7 / 3.3e-7, conv_relu_embed 2.0e-7 / 2.1e-7."""
import numpy as np
import pytest
import torch

import _ankur_cases as C
import _disco_cases as DC
import _disco_ref as R
from _fake_ankur import fake_ankur


@pytest.mark.parametrize("name", C.CASES)
def test_statement_within_twice_the_references_error(name):
    c = C.case(name)
    net = C.build(c)
    with fake_ankur(), torch.no_grad():
        y = net(c["input"])
    if "statement" in c:
        assert C.bits_equal(y, c["statement"])
    err = C.rel_err(y, c["output64"])
    print(f"{name}: statement vs fp64 {err:.3e}; reference fp32 vs fp64 {c['reference_error']:.3e}")
    assert err <= 2 * c["reference_error"]


def _direct64(x, t, w, groups):
    """z and the mix as plain fp64 sums over the table (no order, no fmaf)."""
    B, Cn, H, W = x.shape
    K = t.vals.shape[1]
    z = np.zeros((B, Cn, K, H, W))
    with np.errstate(all="ignore"):
        for ho in range(H):
            for e in range(int(t.row_offsets[ho]), int(t.row_offsets[ho + 1])):
                xr = np.roll(x[:, :, int(t.hi[e]), :].astype(np.float64), -int(t.wi[e]), axis=-1)
                z[:, :, :, ho, :] += t.vals[e].astype(np.float64)[None, None, :, None] * xr[:, :, None, :]
        O, gs, _ = w.shape
        return np.einsum("bgckxy,gock->bgoxy", z.reshape(B, groups, gs, K, H, W),
                         w.astype(np.float64).reshape(groups, O // groups, gs, K)).reshape(B, O, H, W)


@pytest.mark.parametrize("case", [((6, 8, 3), (6, 24)), ((9, 20, 2), (12, 32))], ids=DC.case_id)
def test_nan_and_inf_positions_equal_the_direct_sums(case):
    t, x, w, e, groups = DC.operands(case)
    x = np.array(x)
    x[0, 1, 2, 3] = np.nan
    x[-1, 4, 4, 1] = np.inf
    got = R.disco(x, t, w, groups)
    want = _direct64(x, t, w, groups)
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), ok)
    assert np.abs(got[ok] - want[ok]).max() <= 2e-6 * np.abs(want[ok]).max()


def test_statement_is_shift_equivariant_in_longitude():
    """the operator commutes with a rotation about the axis: bit for bit, since a pixel's chain only sees rolled operands"""
    case = ((8, 16, 3), (5, 24))
    t, x, w, e, groups = DC.operands(case)
    y = DC.statement_mix(case)
    y5 = R.disco_mix(R.disco_z(np.roll(x, 5, axis=-1), t), w, groups)
    assert np.array_equal(np.roll(y, 5, axis=-1).view(np.int32), y5.view(np.int32))
