"""The three tile GEMM kernels of ace_amd/csrc/kernels.hip - `gemm_f32_kernel` (register-staged, 4- or 16-byte loads), `gemm2_f32_kernel`
(direct to LDS) and `gemm3_f16x3_kernel` (compensated fp16, loader waves) - held to the whole fused contract of `GemmArgs` at their
tile edges, against fp64, through `ace_conv1x1_fused` (include/ace_sfno.h):

    y = min(act(W . affine(x || x2) + bias + (res * res_scale + res_shift)), cap) * out_scale + out_shift

The cases, their inputs and the fp64 truth are tests/_gemm_ref.py's (tests/test_gemm_ref_cpu.py holds a plain fp32 evaluation of every
case to OP_TOL / 2, which is what makes OP_TOL = 2e-6, the operator bar of tests/test_gpu_parity.py, fair here).  Four sweeps, each
shape once with no option at batch 1 and once with every option at batch 3, on every engine that takes it:
  rows      cout 1 .. 257 across both tile shapes (N = 260, K = 36)
  cols      hw 4 .. 516 at cout 65 and 200; hw 1, 3, 13, 257 on engine 0 only (the 4-byte family)
  k         (cin, cin2) from (1, 0) to (68, 0) and five concatenations whose K1 falls on a stage edge, inside a stage and off a multiple
            of 4, with a one-row first and a one-row second source; (1020, 4) with the affine: the last entry of the f16x3 kernel's
            1024-row LDS table
  opt       at (65, 260, 30, 6) and (200, 132, 30, 6), batch 3: each option alone, the cap under each activation, pitches of hw + 4 and
            hw + 36, a y pitch of hw + 3 (4-byte stores on every engine) and an x off a 16-byte boundary (engine 0)
Every case (test_engine_vs_fp64)
  * asserts the route it means to check (family 0 / 1 / 2 / 3, tile 64 x 256 / 128 x 128) as the entry reports it;
  * runs under poison: each operand is a view inside a NaN-filled allocation with 64 elements in front and behind, pitch gaps are NaN,
    y is a view inside a buffer of a sentinel; afterwards everything outside the (n, cout, hw) region is bitwise the sentinel and
    everything inside is finite;
  * is run twice, bitwise equal;
  * where `out_absmax` is given: the maximum over its 64 words equals max |y| over the stored values exactly, and the words around
    the slot are untouched.
test_refusals: what an engine does not take is a ValueError, never another engine.

MEASURED (max|err| / max|ref| vs fp64, worst case of each engine over all sweeps; every case is within OP_TOL):
  engine 0 (gemm_f32_kernel)      9.98e-7  at (1020, 4) x 64 x 256 with every option; 7.2e-7 over the shapes with K <= 68
  engine 1 (gemm2_f32_kernel)     1.49e-6  at (1020, 4) x 64 x 256 with every option it takes; 6.0e-7 over the shapes with K <= 68
  engine 2 (gemm3_f16x3_kernel)   8.84e-7  at (1020, 4) x 64 x 256 with every option; 4.7e-7 over the shapes with K <= 68
No case found a defect in a kernel.  The uninitialised tail of the f16x3 kernel's LDS affine table (entries K .. roundup(K, 32), read by
the B stager and applied to the clamped row K - 1 in front of zero weight columns) is written as the zero affine now; the K % 32 != 0
cases with the affine on engine 2 hold it.  The file was also run once against a library with four deliberate in-bounds mistakes (a
residual affine and an input affine without their per-sample stride, the cap behind the output affine, a range maximum taken before
the bounds check): 173 of the sweep cases failed, each mistake in the cases that switch its option on, and the last one in
test_absmax_is_a_maximum_of_stored_values, which is built for it.
"""

import ctypes

import pytest
import torch

import _gemm_ref as R
from _util import rel_max

pytestmark = pytest.mark.gpu

OP_TOL = R.OP_TOL
GUARD = 64            # elements in front of and behind every operand
SENTINEL = -777.25    # what y's buffer holds before the call
SLOT_SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def poisoned(t, dev, pitch=None, lead=GUARD):
    """`t` (..., hw) as a device view of the same shape inside a NaN-filled allocation: `lead` NaNs in front, GUARD behind, rows at
    `pitch` with NaN gaps.  Returns (view, owner)."""
    hw = t.shape[-1]
    pitch = pitch or hw
    rows = t.numel() // hw
    buf = torch.full((lead + rows * pitch + GUARD,), float("nan"), device=dev)
    view = buf[lead:lead + rows * pitch].view(*t.shape[:-1], pitch)[..., :hw]
    view.copy_(t.to(dev))
    return view, buf


def run(case, engine, dev, d=None):
    """one call of ace_conv1x1_fused on poisoned operands (the case's own inputs unless `d` gives others); returns (y buffer, y view,
    slot buffer or None, (family, tile))"""
    from ace_amd import _lib
    d = d or R.inputs(case)
    in_pitch, out_pitch = case.hw + case.in_extra, case.hw + case.out_extra
    keep, ptr = [], {}
    for name, t in d.items():
        if t is None:
            ptr[name] = None
            continue
        pitched = name in ("x", "x2", "res")
        view, buf = poisoned(t, dev, in_pitch if pitched else None, GUARD + 1 if (name == "x" and case.misalign) else GUARD)
        keep.append(buf)
        ptr[name] = view.data_ptr()
    ybuf = torch.full((GUARD + case.n * case.cout * out_pitch + GUARD,), SENTINEL, device=dev)
    yview = ybuf[GUARD:GUARD + case.n * case.cout * out_pitch].view(case.n, case.cout, out_pitch)[..., :case.hw]
    slot = None
    if "absmax" in case.opts:
        slot = torch.full((GUARD + 64 + GUARD,), SLOT_SENTINEL, dtype=torch.int32, device=dev)
    desc = _lib.Conv1x1FusedDesc(
        x=ptr["x"], x2=ptr["x2"], weight=ptr["weight"], bias=ptr["bias"], in_scale=ptr["in_scale"], in_shift=ptr["in_shift"],
        res=ptr["res"], res_scale=ptr["res_scale"], res_shift=ptr["res_shift"], out_scale=ptr["out_scale"], out_shift=ptr["out_shift"],
        y=yview.data_ptr(), out_absmax=(slot[GUARD:].data_ptr() if slot is not None else None),
        n=case.n, cin=case.cin, cin2=case.cin2, cout=case.cout, hw=case.hw, in_pitch=in_pitch, out_pitch=out_pitch,
        act=case.act, cap=case.cap, engine=engine)
    route = _lib.GemmRoute(-9, -9)
    _lib.check(_lib.lib().ace_conv1x1_fused(ctypes.byref(desc), ctypes.byref(route), _lib.current_stream()))
    torch.cuda.synchronize()
    del keep
    return ybuf, yview, slot, (route.family, route.tile)


WORST = {}


@pytest.mark.parametrize("case,engine", R.engine_cases(), ids=lambda v: v.id if isinstance(v, R.Case) else f"engine{v}")
def test_engine_vs_fp64(dev, case, engine):
    ref = R.truth(case)
    ybuf, y, slot, route = run(case, engine, dev)
    ybuf2, y2, slot2, route2 = run(case, engine, dev)
    assert route == R.expected_route(case, engine) == route2, (route, route2, R.expected_route(case, engine))
    # outside the (n, cout, hw) region nothing was written; inside everything was, and is finite
    inside = torch.zeros_like(ybuf, dtype=torch.bool)
    out_pitch = case.hw + case.out_extra
    inside[GUARD:GUARD + case.n * case.cout * out_pitch].view(case.n, case.cout, out_pitch)[..., :case.hw] = True
    sentinel = torch.full_like(ybuf, SENTINEL)
    assert torch.equal(ybuf[~inside].view(torch.int32), sentinel[~inside].view(torch.int32)), "a store outside the output region"
    assert torch.isfinite(y).all(), "a non-finite output: poison reached a result"
    assert torch.equal(ybuf.view(torch.int32), ybuf2.view(torch.int32)), "two calls differ"
    err = rel_max(y, ref)
    WORST[engine] = max(WORST.get(engine, 0.0), err)
    print(f"{case.id} engine {engine}: route {route}, {err:.3e} vs fp64 (worst of engine {engine} so far {WORST[engine]:.3e})")
    assert err <= OP_TOL, (case.id, engine, err)
    if slot is not None:
        words = slot[GUARD:GUARD + 64]
        assert torch.all(slot[:GUARD] == SLOT_SENTINEL) and torch.all(slot[GUARD + 64:] == SLOT_SENTINEL), "a write around the slot"
        assert torch.all(words >= 0)   # bit patterns of non-negative floats
        got = slot_max(slot)
        assert torch.equal(got, y.abs().max()), (float(got), float(y.abs().max()))
        assert torch.equal(slot, slot2)


def slot_max(slot):
    return slot[GUARD:GUARD + 64].max().view(torch.float32)


@pytest.mark.parametrize("engine", R.ENGINES)
@pytest.mark.parametrize("cout,hw", [(65, 260), (200, 132)])
def test_absmax_is_a_maximum_of_stored_values(dev, cout, hw, engine):
    """A ragged tile computes rows and columns it does not store, from clamped addresses: the weight row of the last row, the row
    parameters of row 0.  Here row 0 has a zero weight row and a bias of 50, so y[:, 0] = 50 exactly and is the maximum of what is
    stored by a wide margin, while a phantom row (last weight row . x + 50) exceeds 50 at about every second pixel: a maximum
    taken before the bounds check would show."""
    case = R.Case("phantom", 3, 30, 6, cout, hw, opts=("bias", "absmax"))
    d = dict(R.inputs(case))
    d["weight"] = d["weight"].clone()
    d["weight"][0] = 0.0
    d["bias"] = d["bias"].clone()
    d["bias"][0] = 50.0
    ref = R.fused(d, case.act, case.cap, torch.float64)
    assert float(ref.abs().max()) == 50.0 and float(ref[:, 1:].abs().max()) < 25.0
    _, y, slot, route = run(case, engine, dev, d)
    assert route == R.expected_route(case, engine)
    assert rel_max(y, ref) <= OP_TOL
    assert float(y.abs().max()) == 50.0
    assert float(slot_max(slot)) == 50.0, float(slot_max(slot))


@pytest.mark.parametrize("case,engine", R.REFUSALS, ids=lambda v: v.id if isinstance(v, R.Case) else f"engine{v}")
def test_refusals(dev, case, engine):
    with pytest.raises(ValueError):
        run(case, engine, dev)
    if engine != 0 and R.takes(case, 0):   # the same call is fine where the engine takes it: the refusal is the engine's
        _, y, _, route = run(case, 0, dev)
        assert route == R.expected_route(case, 0)
        assert rel_max(y, R.truth(case)) <= OP_TOL
