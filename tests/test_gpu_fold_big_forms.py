"""The big form of the folded Legendre kernel (ace_amd/csrc/strip_fold.hip: `legendre_fold_big_kernel`, more than 96 folded latitudes
or degrees per parity) at every size it is instantiated for, and its polar cut, against fp64.

The kernel has bodies for 12, 18 and 24 k16-steps per unit (193-384, 385-576, 577-768 latitudes); the size also sets the launch's
dynamic LDS.  The 721 x 1440 tests reach the 24-step forward body only; a half-degree grid runs the 12-step one.  Every case here is an
f16x3 plan with 64 fields (128 columns of (re | im, field): the big form takes whole 128-column groups only) unless it says otherwise.

1. Oracle parity per instantiation (test_transforms_vs_oracle): forward and inverse against oracle.RealSHT / oracle.InverseRealSHT in
   fp64, the inverse fed independent random triangular coefficients (an error common to both directions cannot cancel), the route of
   both launches asserted (ace_sht_plan_route: 3 big form, 2 small form, 0 tile engine) and the cut asserted on (ace_sht_plan_cut)
   wherever the tables have dead rows.  The bar is SHT_TOL = 5e-6, the bar of the same kernel family at 721 x 1440; a shorter contraction has
   no reason to do worse.  MEASURED (max|err| / max|ref|, analysis / synthesis) - every case is also within OP_TOL = 2e-6:
       194 x 48 1.84e-7 / 1.74e-7;  384 x 48 1.95e-7 / 1.57e-7;  360 x 720 2.00e-7 / 2.15e-7;  385 x 48 2.01e-7 / 1.60e-7;
       576 x 24 2.16e-7 / 1.78e-7;  577 x 48 2.31e-7 / 1.79e-7;  768 x 48 2.13e-7 / 1.88e-7;  770 x 48 (tile engine) 6.08e-7 / 4.22e-7;
       192 x 48 (small form) 1.54e-7 / 1.59e-7;  361 x 720 equiangular 1.80e-7 / 2.22e-7;  361 x 48 lobatto 1.96e-7 / 1.52e-7;
       200 x 48 lmax 150 1.65e-7 / 1.46e-7;  194 x 720 1.73e-7 / 2.11e-7.
   This module found the 18-step forward body wrong: its strip load ran in chunks of four k16-steps, a ragged fifth chunk indexed
   the operand arrays at steps 18 and 19 and overwrote the first two steps of the odd operand - analysis at 385 x 48 1.50e-1 before
   the chunk was made to divide the unit, 2.01e-7 after.
2. The cut, poisoned (test_poisoned_cut_equals_the_plan_without_it): with ACE_POLAR_POISON=1 every X buffer starts as quiet NaNs and
   the cut leaves the dead entries unwritten, so a big-form kernel that still read one would turn the output into NaNs.  A fresh plan
   with the cut against a fresh plan with ACE_NO_POLAR_CUT=1: forward, inverse, then forward + inverse twice on one plan, bitwise
   equal and finite.  The cut plan's dead share is held to the value of the CPU walk over the packed tables
   (tests/emul/polar_cut_emul.cpp) within 1e-3, kdrop is 0 (the big form keeps its k16-steps), the other plan reports no cut.
3. Route alternation on one poisoned plan (test_route_alternation_on_one_plan): 64 fields (big form, cut), 3 fields (the fold is
   ineligible: tile engine, the FFT's cut switched off for that call), 64 fields again - bitwise equal to the same sequence on a plan
   without the cut, each call within SHT_TOL of the oracle, routes 3, 0, 3.  MEASURED: forward 2.00e-7, 6.23e-7, 2.00e-7; inverse
   2.15e-7, 3.73e-7, 2.15e-7.
4. In the network (test_network_on_the_mid_size_big_forms): one-block dhconv nets at C = 64, batch 1 (128 columns), whose forward
   Legendre launch writes fp16 hi / lo planes (`legendre_fold_big_kernel<1, 0>` at 12 and 18 steps), against SFNOOracle in fp64 at
   NET_TOL = 1e-5, route (3, 3), eager and graph replay bitwise equal, and under poison both bitwise equal to the build without the cut.
   MEASURED (eager = graph replay): 200 x 48 2.37e-7, 386 x 48 2.61e-7.

Every oracle result is computed once per module (`truth`) and only read afterwards."""

import ctypes
import functools

import pytest
import torch

from _util import assert_net_close, build_native_net, rel_max

pytestmark = pytest.mark.gpu

OP_TOL = 2e-6
SHT_TOL = 5e-6
NET_TOL = 1e-5
N_FIELDS = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def set_cut(monkeypatch, on, poison=True):
    if poison:
        monkeypatch.setenv("ACE_POLAR_POISON", "1")
    else:
        monkeypatch.delenv("ACE_POLAR_POISON", raising=False)
    if on:
        monkeypatch.delenv("ACE_NO_POLAR_CUT", raising=False)
    else:
        monkeypatch.setenv("ACE_NO_POLAR_CUT", "1")


def make_pair(nlat, nlon, lmax, mmax, grid):
    """forward and inverse modules on ONE f16x3 plan (the switches are read when the plan is built, at the first call)"""
    from ace_amd.sht import InverseRealSHT, RealSHT
    fwd = RealSHT(nlat, nlon, lmax, mmax, grid=grid, precision="f16x3")
    inv = InverseRealSHT(nlat, nlon, lmax, mmax, grid=grid, precision="f16x3")
    inv._plan = fwd._get_plan()
    return fwd, inv


def sht_route(pair):
    from ace_amd import _lib
    f, i = ctypes.c_int(-9), ctypes.c_int(-9)
    _lib.check(_lib.lib().ace_sht_plan_route(pair[0]._get_plan().handle, ctypes.byref(f), ctypes.byref(i)))
    return f.value, i.value


def sht_cut(pair):
    from ace_amd import _lib
    share, kdrop = ctypes.c_double(-1.0), ctypes.c_int(-9)
    _lib.check(_lib.lib().ace_sht_plan_cut(pair[0]._get_plan().handle, ctypes.byref(share), ctypes.byref(kdrop)))
    return share.value, kdrop.value


@functools.lru_cache(maxsize=None)
def truth(nlat, nlon, lmax, mmax, grid):
    """(fields, coefficients, fp64 analysis of the fields, fp64 synthesis of the coefficients), N_FIELDS of each, built once and only
    read afterwards.  The coefficients are independent of the fields: triangular (l >= m), a decaying, large-scale dominated spectrum."""
    import oracle
    fo = oracle.RealSHT(nlat, nlon, lmax, mmax, grid, dtype=torch.float64)
    io = oracle.InverseRealSHT(nlat, nlon, lmax, mmax, grid, dtype=torch.float64)
    L, M = fo.lmax, fo.mmax
    g = torch.Generator().manual_seed(1000 * nlat + nlon)
    x = torch.randn(N_FIELDS, nlat, nlon, generator=g)
    coef = torch.complex(torch.randn(N_FIELDS, L, M, generator=g), torch.randn(N_FIELDS, L, M, generator=g))
    coef = coef * (torch.arange(L)[:, None] >= torch.arange(M)[None, :])
    coef = coef / (1.0 + torch.arange(L, dtype=torch.float32)[:, None]) ** 0.5
    return x, coef, fo(x.double()), io(coef.to(torch.complex128))


LG, EQ, LOB = "legendre-gauss", "equiangular", "lobatto"
# (nlat, nlon, lmax, mmax, grid, routes (forward, inverse), the plan has a polar cut).  The last is what the CPU walk over the packed
# tables finds (tests/emul/polar_cut_emul.cpp's derivation on the real tables): every folded grid of 25 wavenumbers or more has dead
# rows; at 576 x 24 (m <= 12) P_l^12 of the degrees near 575 is still ~1e-7 at the first latitude, above the fp16 lo fragment's
# smallest subnormal once scaled, so no row is dead and the plan rightly reports no cut; 770 latitudes are not folded at all.
PARITY_CASES = {
    "12steps-194x48": (194, 48, None, None, LG, (3, 3), True),           # first big form
    "12steps-384x48": (384, 48, None, None, LG, (3, 3), True),           # last 12-step size
    "12steps-360x720": (360, 720, None, None, LG, (3, 3), True),         # the half-degree grid
    "18steps-385x48-odd": (385, 48, None, None, LG, (3, 3), True),       # first 18-step size, self-mirrored middle row
    "18steps-576x24": (576, 24, None, None, LG, (3, 3), False),          # last 18-step size
    "24steps-577x48": (577, 48, None, None, LG, (3, 3), True),           # first 24-step size
    "24steps-768x48": (768, 48, None, None, LG, (3, 3), True),           # the last foldable size
    "beyond-770x48": (770, 48, None, None, LG, (0, 0), False),           # 385 folded latitudes: tile engine
    "small-192x48": (192, 48, None, None, LG, (2, 2), True),             # the small form's last size
    "equiangular-361x720": (361, 720, None, None, EQ, (3, 3), True),
    "lobatto-361x48": (361, 48, None, None, LOB, (3, 3), True),
    "truncated-200x48-l150-m25": (200, 48, 150, 25, LG, (3, 2), True),   # forward big form, inverse small form with 4 tile pairs
    "mmax-gt-lmax-194x720": (194, 720, None, None, LG, (3, 3), True),    # wavenumbers 194 .. 360 have no degree: wholly dead
}


@pytest.mark.parametrize("case", list(PARITY_CASES))
def test_transforms_vs_oracle(dev, monkeypatch, case):
    nlat, nlon, lmax, mmax, grid, routes, has_cut = PARITY_CASES[case]
    set_cut(monkeypatch, True, poison=False)   # the library as it runs by default
    x, coef, oc, oy = truth(nlat, nlon, lmax, mmax, grid)
    pair = make_pair(nlat, nlon, lmax, mmax, grid)
    c = pair[0](x.to(dev))
    y = pair[1](coef.to(dev))
    torch.cuda.synchronize()
    share, kdrop = sht_cut(pair)
    ec, ey = rel_max(c, oc), rel_max(y, oy)
    print(f"{case}: analysis {ec:.3e}, synthesis {ey:.3e} vs fp64; routes {sht_route(pair)}, dead share {share:.4f}, kdrop {kdrop}")
    assert sht_route(pair) == routes, sht_route(pair)
    if has_cut:
        assert share > 0.0, "the plan has no polar cut"
        assert kdrop == (1 if routes[0] == 2 else 0), kdrop
    else:
        assert (share, kdrop) == (0.0, 0), (share, kdrop)
    assert torch.isfinite(torch.view_as_real(c)).all() and torch.isfinite(y).all()
    assert ec <= SHT_TOL and ey <= SHT_TOL, (case, ec, ey)


# dead share of X from the CPU walk over the packed tables (tests/emul/polar_cut_emul.cpp)
POISON_CASES = {
    "360x720": (360, 720, LG, 0.2850),
    "361x720-equiangular": (361, 720, EQ, 0.2860),
    "385x720": (385, 720, LG, 0.2586),
    "194x720": (194, 720, LG, 0.5955),
}


@pytest.mark.parametrize("case", list(POISON_CASES))
def test_poisoned_cut_equals_the_plan_without_it(dev, monkeypatch, case):
    nlat, nlon, grid, want_share = POISON_CASES[case]
    x, coef, _, _ = truth(nlat, nlon, None, None, grid)
    x, coef = x.to(dev), coef.to(dev)
    got = {}
    for on in (False, True):
        set_cut(monkeypatch, on)
        # a fresh plan: the poison is applied when X is allocated, and no call on a plan with the cut ever writes a dead entry, so they
        # stay NaN in front of every call below
        pair = make_pair(nlat, nlon, None, None, grid)
        c = pair[0](x).clone()
        y = pair[1](coef).clone()
        rt = [pair[1](pair[0](x)).clone() for _ in range(2)]   # the inverse leaves its own dead entries in X in front of the next forward
        torch.cuda.synchronize()
        assert sht_route(pair) == (3, 3), sht_route(pair)
        got[on] = (c, y, rt, sht_cut(pair))
        del pair
    assert got[False][3] == (0.0, 0), got[False][3]
    share, kdrop = got[True][3]
    print(f"{case}: dead share {share:.4f} (CPU walk {want_share:.4f}), kdrop {kdrop}")
    assert abs(share - want_share) <= 1e-3, (share, want_share)
    assert kdrop == 0, kdrop
    assert torch.isfinite(torch.view_as_real(got[False][0])).all() and torch.isfinite(got[False][1]).all()
    assert torch.isfinite(torch.view_as_real(got[True][0])).all() and torch.isfinite(got[True][1]).all()
    assert torch.equal(torch.view_as_real(got[True][0]), torch.view_as_real(got[False][0])), "forward differs"
    assert torch.equal(got[True][1], got[False][1]), "inverse differs"
    for rep in range(2):
        assert torch.isfinite(got[True][2][rep]).all()
        assert torch.equal(got[True][2][rep], got[False][2][rep]), f"forward + inverse on one plan, pass {rep}"


@pytest.mark.parametrize("direction", ["forward", "inverse"])
def test_route_alternation_on_one_plan(dev, monkeypatch, direction):
    """64 fields, 3 fields, 64 fields on ONE poisoned plan at 360 x 720: the middle call runs the tile engine (a field count that is
    no multiple of 64 makes the fold ineligible) with the FFT's cut off, behind and in front of calls that leave dead entries unwritten"""
    nlat, nlon = 360, 720
    x, coef, oc, oy = truth(nlat, nlon, None, None, LG)
    src, ref = (x, oc) if direction == "forward" else (coef, oy)
    src = src.to(dev)
    which = 0 if direction == "forward" else 1
    got = {}
    for on in (False, True):
        set_cut(monkeypatch, on)
        pair = make_pair(nlat, nlon, None, None, LG)
        outs, routes = [], []
        for n in (N_FIELDS, 3, N_FIELDS):
            outs.append(pair[which](src[:n]).clone())
            torch.cuda.synchronize()
            routes.append(sht_route(pair)[which])
        got[on] = outs
        assert routes == [3, 0, 3], routes
        share, kdrop = sht_cut(pair)
        assert (share > 0.0) == on and kdrop == 0, (on, share, kdrop)
        del pair
    for k, n in enumerate((N_FIELDS, 3, N_FIELDS)):
        a, b = got[True][k], got[False][k]
        if a.is_complex():
            a, b = torch.view_as_real(a), torch.view_as_real(b)
        assert torch.isfinite(a).all(), (direction, k)
        assert torch.equal(a, b), f"{direction} call {k} (n = {n}) differs from the plan without the cut"
        err = rel_max(got[True][k], ref[:n])
        print(f"{direction} call {k} (n = {n}): {err:.3e} vs fp64")
        assert err <= SHT_TOL, (direction, k, n, err)


def net_query(net):
    from ace_amd import _lib
    f, i, share, kdrop = ctypes.c_int(-9), ctypes.c_int(-9), ctypes.c_double(-1.0), ctypes.c_int(-9)
    _lib.check(_lib.lib().ace_sfno_sht_route(net._native, ctypes.byref(f), ctypes.byref(i)))
    _lib.check(_lib.lib().ace_sfno_sht_cut(net._native, ctypes.byref(share), ctypes.byref(kdrop)))
    return (f.value, i.value), share.value, kdrop.value


@pytest.mark.parametrize("hw", [(200, 48), (386, 48)], ids=["12steps-200x48", "18steps-386x48"])
def test_network_on_the_mid_size_big_forms(dev, monkeypatch, hw):
    from oracle.sfno import SFNOConfig, SFNOOracle, init_state
    cfg = SFNOConfig(in_chans=3, out_chans=2, img_shape=hw, embed_dim=64, num_layers=1, operator_type="dhconv")
    state = init_state(cfg, seed=5)
    xin = torch.randn(1, 3, *hw, generator=torch.Generator().manual_seed(6))
    ref = SFNOOracle(cfg, state, dtype=torch.float64).forward(xin)
    x = xin.to(dev)
    outs = {}
    for on in (False, True):
        set_cut(monkeypatch, on)
        net = build_native_net(cfg, state, dev, "f16x3")
        with torch.no_grad():
            eager = net(x).clone()
            out = torch.empty_like(eager)
            net.forward_graph(x, out)
            net.forward_graph(x, out)   # the second call replays the captured graph
        torch.cuda.synchronize()
        routes, share, kdrop = net_query(net)
        assert routes == (3, 3), routes
        assert (share > 0.0) == on and kdrop == 0, (on, share, kdrop)
        outs[on] = (eager, out.clone())
        del net
    print(f"{hw}: eager {rel_max(outs[True][0], ref):.3e}, graph replay {rel_max(outs[True][1], ref):.3e} vs fp64")
    assert torch.isfinite(outs[True][0]).all() and torch.isfinite(outs[False][0]).all()
    assert torch.equal(outs[True][1], outs[True][0]), "graph replay differs from the eager forward"
    assert torch.equal(outs[True][0], outs[False][0]), "eager forward differs from the build without the cut"
    assert torch.equal(outs[True][1], outs[False][1]), "graph replay differs from the build without the cut"
    assert_net_close(outs[True][0], ref, NET_TOL)
    assert_net_close(outs[True][1], ref, NET_TOL)
