"""The polar cut of the spherical transform on the GPU: results bitwise equal to the same library with ACE_NO_POLAR_CUT=1.

Near the poles the folded Legendre tables of a high wavenumber pack to exact zeros (ace_amd/csrc/strip_pack.h, PolarCut); the
forward FFT does not store those entries of X, the folded Legendre kernels neither load, multiply, compute nor store them and the
inverse FFT does not load them.  Every run here sets ACE_POLAR_POISON=1: every X buffer starts as quiet NaNs, the cut leaves the
dead entries unwritten, so a kernel that still read one would turn the output into NaNs.

Shapes: width 48 has the two-level FFT (both halves of either pair take the cut), 23 x 48 the self-mirrored middle row, width 92
only the matrix DFT (pairing rule: Legendre window on, FFT cut off, the inverse Legendre kernel keeps writing its zeros), 180 x 360
is the benchmark grid.  The reference of every comparison is the library itself without the cut, so equality is exact.  That the cut
was on at all is asserted through ace_sht_plan_cut: a dead share above zero on the plan with the cut (with the forward table's dead
k16-steps dropped at 180 x 360), none on the other."""

import ctypes

import pytest
import torch

from _util import build_native_net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def set_cut(monkeypatch, on):
    monkeypatch.setenv("ACE_POLAR_POISON", "1")
    if on:
        monkeypatch.delenv("ACE_NO_POLAR_CUT", raising=False)
    else:
        monkeypatch.setenv("ACE_NO_POLAR_CUT", "1")


def make_pair(nlat, nlon):
    """forward and inverse modules on ONE f16x3 plan (the switches are read when the plan is built, at the first call)"""
    from ace_amd.sht import InverseRealSHT, RealSHT
    fwd = RealSHT(nlat, nlon, grid="legendre-gauss", precision="f16x3")
    inv = InverseRealSHT(nlat, nlon, grid="legendre-gauss", precision="f16x3")
    inv._plan = fwd._get_plan()
    return fwd, inv


def plan_cut(module):
    from ace_amd import _lib
    share, kdrop = ctypes.c_double(-1.0), ctypes.c_int(-9)
    _lib.check(_lib.lib().ace_sht_plan_cut(module._get_plan().handle, ctypes.byref(share), ctypes.byref(kdrop)))
    return share.value, kdrop.value


def fields(n, nlat, nlon, dev, seed):
    return torch.randn(n, nlat, nlon, generator=torch.Generator().manual_seed(seed)).to(dev)


def coefficients(n, lmax, mmax, dev, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.complex(torch.randn(n, lmax, mmax, generator=g), torch.randn(n, lmax, mmax, generator=g))
    return (c * torch.tril(torch.ones(lmax, mmax))).to(dev)   # degrees l >= m only


@pytest.mark.parametrize("n,nlat,nlon", [(16, 24, 48), (16, 23, 48), (16, 46, 92), (8, 180, 360)], ids=["24x48", "23x48", "46x92", "180x360"])
def test_public_transforms_equal_the_plan_without_the_cut(dev, monkeypatch, n, nlat, nlon):
    """ace_sht_forward / ace_sht_inverse; then forward followed by inverse on one plan, twice in a row"""
    x = fields(n, nlat, nlon, dev, 11)
    set_cut(monkeypatch, False)
    f0, i0 = make_pair(nlat, nlon)
    c = coefficients(n, f0.lmax, f0.mmax, dev, 12)
    want_c, want_x = f0(x).clone(), i0(c).clone()
    want_rt = i0(f0(x)).clone()
    set_cut(monkeypatch, True)
    f1, i1 = make_pair(nlat, nlon)
    got_c, got_x = f1(x).clone(), i1(c).clone()
    assert plan_cut(f0) == (0.0, 0), plan_cut(f0)
    share, kdrop = plan_cut(f1)
    assert share > 0.0, "the plan has no polar cut: the comparison below would pass vacuously"
    if (nlat, nlon) == (180, 360):
        assert kdrop == 1, kdrop
    assert torch.isfinite(torch.view_as_real(want_c)).all() and torch.isfinite(want_x).all()
    assert torch.equal(torch.view_as_real(got_c), torch.view_as_real(want_c)), "forward differs"
    assert torch.equal(got_x, want_x), "inverse differs"
    for rep in range(2):   # the inverse leaves its own dead entries in the plan's X in front of the next forward
        assert torch.equal(i1(f1(x)), want_rt), f"forward + inverse on one plan, pass {rep}"
    torch.cuda.synchronize()


@pytest.mark.parametrize("hw,layers,batch", [((24, 48), 2, 2), ((180, 360), 1, 1)], ids=["24x48-2blocks", "180x360-1block"])
def test_network_equals_the_library_without_the_cut(dev, monkeypatch, hw, layers, batch):
    """the SFNO forward through the C ABI, eager and replayed from the library's graph"""
    from oracle.sfno import SFNOConfig, init_state
    cfg = SFNOConfig(in_chans=5, out_chans=4, img_shape=hw, embed_dim=128, num_layers=layers, operator_type="dhconv")
    state = init_state(cfg, seed=3)
    x = torch.randn(batch, 5, *hw, generator=torch.Generator().manual_seed(4)).to(dev)
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
        outs[on] = (eager, out.clone())
        del net
    assert torch.isfinite(outs[False][0]).all()
    assert torch.equal(outs[True][0], outs[False][0]), "eager forward differs"
    assert torch.equal(outs[True][1], outs[False][1]), "graph replay differs"
    assert torch.equal(outs[True][1], outs[True][0]), "graph replay differs from the eager forward"
