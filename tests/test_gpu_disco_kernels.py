"""``ace_disco_*`` (csrc/disco.hip) through the C ABI against the header's statement in numpy (tests/_disco_ref.py): bit for bit with
activation none and ReLU, with and without the embedding, on every grid x channel case of tests/_disco_cases.py - NaN compared by
position, signs of zero included.  The grids are the smallest at which the kernel can go wrong: W below the 16-pixel run, W no
multiple of it, polar rows whose disk wraps every longitude next to windowed equatorial rows, K = 4 / 9 / 16; the channel cases
give 1, 3, 5 and 15 inputs and 1, 4, 8, 24 and 128 outputs per group (products no multiple of 4, outputs below and above one MFMA
tile, depthwise, one group).

GELU and SiLU are held to fp64: the kernel's output against the fp64 activation of the statement's bit-exact pre-activation may
err at most 2 x as much as torch's CPU fp32 F.gelu / F.silu of the same fp32 values does (another erf / exp of the same working
precision).  Measured on an MI355X, largest absolute error over the case below: GELU kernel 4.4e-7 against torch 1.1e-6; SiLU
kernel 7.1e-7 against torch 7.1e-7 (at 1 degree: profiles/ankur_bench.json)."""
import numpy as np
import pytest
import torch

import _disco_cases as C
import _disco_ref as R
from ace_amd import disco as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _dev(a, dev, off=0):
    """a numpy fp32 array on the device, `off` floats behind a 16-byte boundary"""
    buf = torch.zeros(a.size + off + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size]
    t.copy_(torch.from_numpy(np.array(a, dtype=np.float32).reshape(-1)))
    return t


def _same(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    bad = got.view(np.int32)[ok] != want.view(np.int32)[ok]
    assert not bad.any(), (int(bad.sum()), got[ok][bad][:4], want[ok][bad][:4])


def _run(dev, table, x, w, e, groups, act, embed, off=(0, 0)):
    B, cin, H, W = x.shape
    cout = w.shape[0]
    h = D.DiscoHandle(table, torch.from_numpy(np.array(w)).to(dev), cin, cout, groups, act, embed)
    try:
        xd, ed = _dev(x, dev, off[0]), _dev(e, dev)
        yd = _dev(np.full((B, cout, H, W), 7.5, np.float32), dev, off[1])
        h.forward(xd.data_ptr(), ed.data_ptr() if embed else None, yd.data_ptr(), B)
        torch.cuda.synchronize()
        return yd.cpu().numpy().reshape(B, cout, H, W)
    finally:
        h.close()


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_bit_for_bit(dev, case):
    t, x, w, e, groups = C.operands(case)
    for act in (R.ACT_NONE, R.ACT_RELU):
        for embed in (False, True):
            _same(_run(dev, t, x, w, e, groups, act, embed), C.statement(case, act, embed))


def test_one_degree_rows(dev):
    """180 x 360, 40 -> 256 in 8 groups of 5 (the shape tools/bench_ankur.py times): polar rows split over groups and short pixel
    runs, mid rows whose 40 channels take several staging passes, equatorial rows with every group in one unit.  The statement is
    formed on six output rows only; the kernel computes all."""
    from ace_amd.disco import disco_table
    rows = [0, 1, 5, 20, 89, 179]
    rng = np.random.default_rng(77)
    t = disco_table((180, 360), 3)
    x = rng.standard_normal((1, 40, 180, 360)).astype(np.float32)
    w = rng.standard_normal((256, 5, 9)).astype(np.float32)
    e = rng.standard_normal((256, 180, 360)).astype(np.float32)
    got = _run(dev, t, x, w, e, 8, R.ACT_RELU, True)
    _same(np.ascontiguousarray(got[:, :, rows]), R.disco(x, t, w, 8, R.ACT_RELU, e, rows=rows))


def test_nan_and_inf_reach_exactly_their_group_and_support(dev):
    """one NaN and one Inf in channel 4 (group 1 of 4) of (16, 36): the non-finite outputs are the statement's, and those are group
    1's outputs whose support holds the point - a zero-valued table entry included (0 * Inf)."""
    case = ((16, 36, 3), (12, 32))
    t, x, w, e, groups = C.operands(case)
    x = np.array(x)
    x[0, 4, 2, 5] = np.nan
    x[0, 4, 9, 30] = np.inf
    want = R.disco(x, t, w, groups, R.ACT_NONE, e)                 # no ReLU here: it would turn a -Inf into a finite 0
    got = _run(dev, t, x, w, e, groups, R.ACT_NONE, True)
    _same(got, want)
    bad = ~np.isfinite(want)
    assert bad.any() and not bad[:, :8].any() and not bad[:, 16:].any() and not bad[1:].any()
    H, W = 16, 36
    reach = np.zeros((H, W), bool)
    for ho in range(H):
        for k in range(int(t.row_offsets[ho]), int(t.row_offsets[ho + 1])):
            for (ph, pw) in ((2, 5), (9, 30)):
                if t.hi[k] == ph:
                    reach[ho, (pw - t.wi[k]) % W] = True
    assert np.array_equal(bad[0, 8:16].any(axis=0), reach) and bad[0, 8:16].all(axis=0)[reach].all()


def test_unaligned_x_and_y(dev):
    case = ((9, 20, 2), (5, 24))
    t, x, w, e, groups = C.operands(case)
    _same(_run(dev, t, x, w, e, groups, R.ACT_RELU, True, off=(1, 1)), C.statement(case, R.ACT_RELU, True))


def test_captured_replay_is_the_eager_call(dev):
    case = ((8, 16, 3), (12, 32))
    t, x, w, e, groups = C.operands(case)
    B, cin, H, W = x.shape
    h = D.DiscoHandle(t, torch.from_numpy(np.array(w)).to(dev), cin, 32, groups, R.ACT_RELU, True)
    try:
        xd, ed = _dev(x, dev), _dev(e, dev)
        y0, y1 = (_dev(np.zeros((B, 32, H, W), np.float32), dev) for _ in range(2))
        h.forward(xd.data_ptr(), ed.data_ptr(), y0.data_ptr(), B)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                h.forward(xd.data_ptr(), ed.data_ptr(), y1.data_ptr(), B)
        y1.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y0, y1)
        _same(y1.cpu().numpy().reshape(B, 32, H, W), C.statement(case, R.ACT_RELU, True))
    finally:
        h.close()


@pytest.mark.parametrize("name", ["gelu", "silu"])
def test_soft_activations_against_fp64(dev, name):
    case = ((16, 36, 3), (12, 32))
    t, x, w, e, groups = C.operands(case)
    act = {"gelu": R.ACT_GELU, "silu": R.ACT_SILU}[name]
    pre = C.statement(case, act, True, pre_activation=True)
    x = np.array(x)
    got = _run(dev, t, x, w, e, groups, act, True)
    truth = (R.gelu64 if name == "gelu" else R.silu64)(pre)
    fn = torch.nn.functional.gelu if name == "gelu" else torch.nn.functional.silu
    yard = float(np.abs(fn(torch.from_numpy(pre)).numpy().astype(np.float64) - truth).max())
    err = float(np.abs(got.astype(np.float64) - truth).max())
    print(f"{name}: kernel {err:.3e} torch-cpu-fp32 {yard:.3e}")
    assert err <= 2 * yard
    # NaN stays NaN
    x[0, 0, 3, 3] = np.nan
    got = _run(dev, t, x, w, e, groups, act, True)
    want = R.disco(x, t, w, groups, R.ACT_NONE, e)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any()


def test_refusals(dev):
    t, x, w, e, groups = C.operands(((6, 8, 3), (6, 24)))
    wd = torch.from_numpy(np.array(w)).to(dev)
    with pytest.raises(ValueError, match="groups"):
        D.DiscoHandle(t, torch.zeros(24, 1, 9, device=dev), 6, 24, 4)
    with pytest.raises(ValueError, match="ACE_DISCO_ACT"):
        D.DiscoHandle(t, wd, 6, 24, groups, act=9)
    with pytest.raises(ValueError, match="ACE_DISCO_MAX_PRODUCTS"):
        D.DiscoHandle(t, torch.zeros(1, 60, 9, device=dev), 60, 1, 1)
    h = D.DiscoHandle(t, wd, 6, 24, groups, R.ACT_NONE, True)
    try:
        xd = _dev(x, dev)
        yd = _dev(np.zeros((x.shape[0], 24, 6, 8), np.float32), dev)
        with pytest.raises(ValueError, match="embed must not be NULL"):
            h.forward(xd.data_ptr(), None, yd.data_ptr(), x.shape[0])
        with pytest.raises(ValueError, match="batch"):
            h.forward(xd.data_ptr(), xd.data_ptr(), yd.data_ptr(), 0)
    finally:
        h.close()
