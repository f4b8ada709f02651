"""tests/_gemm_ref.py, the torch statement of the fused GEMM contract that tests/test_gpu_gemm_engines.py holds the three tile
kernels to.

1. Conditioning (test_fp32_evaluation_is_within_half_the_bar): for EVERY case of the lists, as every engine runs it, a plain fp32
   evaluation of the formula stays within OP_TOL / 2 = 1e-6 of the fp64 one in the project's norm max|err| / max|ref|.  This is what
   makes OP_TOL = 2e-6 a fair bar for a kernel on these inputs: a correct fp32-class kernel has half the bar to spare.  A case that
   breaks it gets other inputs, not another bar.  Worst over the lists: 7.2e-7 (ReLU under the cap at 65 x 260, K = 30 + 6).
2. The formula against torch.nn.functional.conv1d on the plain bias case, and option by option against a restatement that shares no
   code with it.
3. The tile rule (128 x 128 iff M >= 128 and the rows wasted at 128 are no more than at 64), restated and checked on the row sweep's
   list, and the route each (case, engine) pair expects."""

import dataclasses
import math

import pytest
import torch

import _gemm_ref as R
from _util import rel_max


def unique_cases():
    seen = {}
    for c, _ in R.engine_cases():
        seen.setdefault(c.id, c)
    return list(seen.values())


@pytest.mark.parametrize("case", unique_cases(), ids=lambda c: c.id)
def test_fp32_evaluation_is_within_half_the_bar(case):
    d = R.inputs(case)
    err = rel_max(R.fused(d, case.act, case.cap, torch.float32), R.truth(case))
    print(f"{case.id}: fp32 formula vs fp64 {err:.3e}")
    assert torch.isfinite(R.truth(case)).all()
    assert err <= R.OP_TOL / 2, (case.id, err)


def test_formula_is_conv1d_on_the_plain_bias_case():
    case = R.Case("conv1d", 3, 30, 6, 65, 132, opts=("bias",))
    d = R.inputs(case)
    x = torch.cat([d["x"], d["x2"]], dim=1).double()
    want = torch.nn.functional.conv1d(x, d["weight"].double()[:, :, None], d["bias"].double())
    assert rel_max(R.truth(case), want) <= 1e-14


def test_formula_option_by_option():
    """each option against loops over samples and rows in fp64: the order of the operations is the contract's"""
    case = R.Case("loops", 2, 5, 3, 7, 12, opts=R.ALL, act=R.ACT_SILU, cap=0.75)
    d = {k: (v.double() if v is not None else None) for k, v in R.inputs(case).items()}
    got = R.truth(case)
    for b in range(case.n):
        xs = torch.cat([d["x"][b], d["x2"][b]], dim=0)
        xs = xs * d["in_scale"][b][:, None] + d["in_shift"][b][:, None]
        for o in range(case.cout):
            v = (d["weight"][o][:, None] * xs).sum(dim=0) + d["bias"][o]
            v = v + (d["res"][b, o] * d["res_scale"][b, o] + d["res_shift"][b, o])
            v = v / (1.0 + torch.exp(-v))
            v = v.clamp(max=0.75)
            v = v * d["out_scale"][o] + d["out_shift"][o]
            assert float((got[b, o] - v).abs().max()) <= 1e-13, (b, o)
    assert float((got - d["out_shift"][None, :, None]).div(d["out_scale"][None, :, None]).max()) <= 0.75 + 1e-12   # the cap bites before the affine
    assert float((got - d["out_shift"][None, :, None]).div(d["out_scale"][None, :, None]).max()) >= 0.75 - 1e-12


def test_tile_rule_on_the_row_sweep():
    def restated(M):   # the smallest numbers of 128- and of 64-row tiles that cover M rows, compared by the rows they cover
        return 1 if M >= 128 and math.ceil(M / 128) * 128 <= math.ceil(M / 64) * 64 else 0
    assert [m for m in R.ROWS_M if R.tile_rule(m) == 1] == list(R.ROWS_M_TILE128) == [128, 200, 250, 256]
    for m in range(1, 1100):
        assert R.tile_rule(m) == restated(m), m


def test_expected_routes_and_engine_eligibility():
    pairs = R.engine_cases()
    assert len({(c.id, e) for c, e in pairs}) == len(pairs)
    routes = {R.expected_route(c, e) for c, e in pairs}
    assert routes == {(f, t) for f in (0, 1, 2, 3) for t in (0, 1)}, routes          # every family on both tiles
    for c, e in pairs:
        assert R.takes(c, e)
        if e == 1:
            assert "in_affine" not in c.opts
    for c, e in R.REFUSALS:
        assert not R.takes(c, e), (c.id, e)
    # the scalar sizes reach engine 0 only, the 1024-row table's last entry reaches engine 2 with its affine
    assert all(e == 0 for c, e in pairs if c.hw in R.COLS_HW_SCALAR)
    assert any(e == 2 and c.K == 1024 and "in_affine" in c.opts for c, e in pairs)
    # both batch sizes, every activation under the cap, both larger pitches
    assert {c.n for c, _ in pairs} == {1, 3}
    assert {c.act for c, _ in pairs if c.cap == 1.5 and not c.opts} == {0, 1, 2, 3}
    assert {c.in_extra for c, _ in pairs} >= {0, 4, 36}
    one = R.Case("opt", 3, 30, 6, 65, 260, opts=("in_affine",))
    assert R.for_engine(one, 1) is None and R.for_engine(one, 2) == one
    assert R.for_engine(dataclasses.replace(one, opts=R.ALL), 1).opts == tuple(o for o in R.ALL if o != "in_affine")
