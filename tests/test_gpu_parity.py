"""HIP path vs the CPU oracle / golden fixtures, through the C ABI (libace_sfno.so).

Tolerances (fp32 everywhere, stated per test):
  * single operators        max|err|/max|ref| <= 2e-6   (a handful of fp32 ulps over K<=768 sums)
  * SHT at 180x360          <= 5e-6
  * whole-network step      <= 1e-5  (BASELINE.json north_star: "per-step output within 1e-5 rel-err")
Size-independent properties (round-trip idempotence, linearity, constant field) are
checked at the full 1-degree size where the oracle would be slow.
"""

import ctypes

import pytest
import torch

from _util import (assert_net_close, build_native_net, checkpoint_case, checkpoint_override, conditioning_floor, load_golden,
                   rel_l2, rel_max)

pytestmark = pytest.mark.gpu

OP_TOL = 2e-6
SHT_TOL = 5e-6
NET_TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


# every network-level parity test runs in both arithmetic modes of the contractions:
#   "fp32"  exact-fp32 MFMA everywhere; "f16x3" error-compensated fp16 MFMA (the default)
@pytest.fixture(params=["f16x3", "fp32"])
def precision(request):
    return request.param


# ---------------------------------------------------------------------------------- building blocks
@pytest.mark.parametrize("n,cin,cout,hw,act", [
    (1, 44, 384, 64800, 1), (2, 16, 16, 162, 1), (1, 2, 3, 162, 0), (3, 18, 16, 288, 2),
    (1, 428, 50, 4096 + 36, 3), (1, 7, 5, 13, 1), (1, 384, 768, 8000, 1),
])
def test_conv1x1(dev, n, cin, cout, hw, act):
    from ace_amd import _lib
    g = torch.Generator().manual_seed(n * 1000 + cin)
    x = torch.randn(n, cin, hw, generator=g)
    w = torch.randn(cout, cin, generator=g) / cin**0.5
    b = torch.randn(cout, generator=g)
    ref = torch.nn.functional.conv1d(x.double(), w.double()[:, :, None], b.double())
    ref = [ref, torch.nn.functional.gelu(ref), torch.relu(ref), torch.nn.functional.silu(ref)][act]
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    y = torch.empty(n, cout, hw, device=dev)
    _lib.check(_lib.lib().ace_conv1x1(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(y), n, cin, cout, hw, act,
                                      _lib.current_stream()))
    assert rel_max(y, ref) <= OP_TOL


@pytest.mark.parametrize("n,c,hw", [(1, 384, 64800), (2, 16, 162), (3, 5, 77)])
def test_instance_norm(dev, n, c, hw):
    from ace_amd import _lib
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, c, hw, generator=g) * 3 + 1.5
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    ref = torch.nn.functional.instance_norm(x.double(), weight=gamma.double(), bias=beta.double(), eps=1e-6)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    y = torch.empty_like(xd)
    _lib.check(_lib.lib().ace_instance_norm(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(bd), 1e-6,
                                            _lib.ptr(y), n, c, hw, _lib.current_stream()))
    assert rel_max(y, ref) <= OP_TOL


@pytest.mark.parametrize("mean_over_std", [0, 30, 300, 1e4])
@pytest.mark.parametrize("n,c,hw", [(2, 16, 162), (3, 5, 77), (2, 16, 164), (1, 3, 2052)])   # H W % 4 != 0: the scalar branch; the float4 one, a row per thread and four
def test_instance_norm_under_a_large_mean(dev, n, c, hw, mean_over_std):
    """The stand-alone ace_instance_norm (instnorm_stats_kernel: fp64 sums of x and x^2) when every channel carries a constant of
    mean_over_std standard deviations, random sign per channel.  Truth: F.instance_norm in fp64; bar max(OP_TOL, 4 floor) with the
    floor F.instance_norm in fp32 gives on the same data (2 for another rounding order x 2 for the fp32 affine the kernel applies)."""
    from ace_amd import _lib
    g = torch.Generator().manual_seed(7)
    sign = torch.randint(0, 2, (c,), generator=g).float() * 2 - 1
    x = torch.randn(n, c, hw, generator=g) * 3 + (3 * mean_over_std * sign)[None, :, None]
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    ref = torch.nn.functional.instance_norm(x.double(), weight=gamma.double(), bias=beta.double(), eps=1e-6)
    floor = rel_max(torch.nn.functional.instance_norm(x, weight=gamma, bias=beta, eps=1e-6), ref)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    y = torch.empty_like(xd)
    _lib.check(_lib.lib().ace_instance_norm(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(bd), 1e-6,
                                            _lib.ptr(y), n, c, hw, _lib.current_stream()))
    err = rel_max(y, ref)
    print(f"instance norm ({n}, {c}, {hw}) mean/std {mean_over_std:g}: err {err:.3e}, fp32 reference floor {floor:.3e}")
    assert err <= max(OP_TOL, 4 * floor), (err, floor)


# ---------------------------------------------------------------------------------- SHT
@pytest.mark.parametrize("n,c,j,hw,affine,cond", [(2, 16, 8, 288, True, True), (1, 384, 32, 4132, True, True),
                                                   (3, 5, 4, 64, False, True), (2, 24, 0, 100, True, False),
                                                   (4, 16, 12, 162, False, True), (1, 7, 3, 13, True, True)])   # H W % 4 != 0: 4-byte path
def test_conditional_layer_norm(dev, n, c, j, hw, affine, cond):
    """ConditionalLayerNorm with noise conditioning (conditional_sfno/layers.py:95-141, 245-318) against the reference's
    torch formula in fp64."""
    from ace_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(c + hw)
    x = torch.randn(n, c, hw, generator=g) * 3.0 + 1.5
    noise = torch.randn(n, max(j, 1), hw, generator=g)
    gamma = 1.0 + 0.3 * torch.randn(c, generator=g)
    beta = 0.2 * torch.randn(c, generator=g)
    ws = 0.3 * torch.randn(c, max(j, 1), generator=g)
    wb = 0.3 * torch.randn(c, max(j, 1), generator=g)
    xd = x.double()
    mean = xd.mean(dim=1, keepdim=True)
    var = xd.var(dim=1, keepdim=True, unbiased=False)
    ref = (xd - mean) * torch.rsqrt(var + 1e-5)
    if affine:
        ref = ref * gamma.double()[None, :, None] + beta.double()[None, :, None]
    if cond:
        scale = 1.0 + torch.einsum("cj,njp->ncp", ws.double(), noise.double())
        bias = torch.einsum("cj,njp->ncp", wb.double(), noise.double())
        ref = ref * scale + bias
    t = [v.to(dev) for v in (x, noise, gamma, beta, ws, wb)]
    y = torch.empty(n, c, hw, device=dev)
    null = ctypes.c_void_p(0)
    _lib.check(L.ace_conditional_layer_norm(_lib.ptr(t[0]), _lib.ptr(t[1]) if cond else null,
                                            _lib.ptr(t[2]) if affine else null, _lib.ptr(t[3]) if affine else null,
                                            _lib.ptr(t[4]) if cond else null, _lib.ptr(t[5]) if cond else null,
                                            1e-5, _lib.ptr(y), n, c, j, hw, _lib.current_stream()))
    assert rel_max(y, ref) <= OP_TOL


@pytest.mark.parametrize("n,c,j,hw,affine,cond", [(2, 256, 33, 64, True, True), (1, 512, 33, 4096, True, True),
                                                   (1, 512, 16, 32, True, True), (3, 256, 5, 160, False, True),
                                                   (1, 768, 33, 96, True, True), (1, 1024, 40, 64, True, True),
                                                   (2, 256, 128, 32, True, True), (2, 512, 0, 96, True, False),
                                                   (1, 512, 33, 4100, True, True), (2, 256, 8, 36, True, True),     # ragged last 128-pixel tile
                                                   (1, 512, 33, 516, False, True), (1, 768, 8, 64, False, False)])
def test_conditional_layer_norm_single_pass_mfma(dev, n, c, j, hw, affine, cond):
    """The single-pass form of the same operator (csrc/cln_mfma.hip: the two conditioning convolutions on the matrix cores with
    error-compensated fp16 operands), which the f16x3 NoiseConditionedSFNO uses when C % 256 == 0: same fp64 formula, same bar."""
    from ace_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(c + hw + j)
    x = torch.randn(n, c, hw, generator=g) * 3.0 + 1.5
    noise = torch.randn(n, max(j, 1), hw, generator=g) * 1.7
    gamma = 1.0 + 0.3 * torch.randn(c, generator=g)
    beta = 0.2 * torch.randn(c, generator=g)
    ws = 0.3 * torch.randn(c, max(j, 1), generator=g)
    wb = 0.02 * torch.randn(c, max(j, 1), generator=g)       # different magnitudes: each weight has its own power-of-two scale
    xd = x.double()
    ref = (xd - xd.mean(dim=1, keepdim=True)) * torch.rsqrt(xd.var(dim=1, keepdim=True, unbiased=False) + 1e-5)
    if affine:
        ref = ref * gamma.double()[None, :, None] + beta.double()[None, :, None]
    if cond:
        ref = ref * (1.0 + torch.einsum("cj,njp->ncp", ws.double(), noise.double())) + torch.einsum("cj,njp->ncp", wb.double(), noise.double())
    t = [v.to(dev) for v in (x, noise, gamma, beta, ws, wb)]
    null = ctypes.c_void_p(0)
    args = lambda y: (_lib.ptr(t[0]), _lib.ptr(t[1]) if cond else null, _lib.ptr(t[2]) if affine else null,
                      _lib.ptr(t[3]) if affine else null, _lib.ptr(t[4]) if cond else null, _lib.ptr(t[5]) if cond else null,
                      1e-5, _lib.ptr(y))
    y = torch.empty(n, c, hw, device=dev)
    _lib.check(L.ace_conditional_layer_norm_f16x3(*args(y), n, c, j, hw, _lib.current_stream()))
    assert rel_max(y, ref) <= OP_TOL, rel_max(y, ref)
    two_pass = torch.empty(n, c, hw, device=dev)
    _lib.check(L.ace_conditional_layer_norm(*args(two_pass), n, c, j, hw, _lib.current_stream()))
    assert rel_max(y, two_pass) <= OP_TOL
    inplace = t[0].clone()                                   # the network normalises in place
    _lib.check(L.ace_conditional_layer_norm_f16x3(_lib.ptr(inplace), *args(inplace)[1:], n, c, j, hw, _lib.current_stream()))
    assert torch.equal(inplace, y)


def test_conditional_layer_norm_single_pass_refuses_other_shapes(dev):
    """No silent fallback at the op level: shapes outside the single-pass kernel's reach are an error naming the constraint."""
    from ace_amd import _lib
    L = _lib.lib()
    x = torch.randn(1, 40, 64, device=dev)
    y = torch.empty_like(x)
    null = ctypes.c_void_p(0)
    for c, hw in ((40, 64), (256, 10)):
        with pytest.raises(ValueError, match="c % 256"):
            _lib.check(L.ace_conditional_layer_norm_f16x3(_lib.ptr(x), null, null, null, null, null, 1e-5, _lib.ptr(y), 1, c, 0, hw,
                                                          _lib.current_stream()))


def test_sht_golden_regression(dev):
    """fme/core/benchmark/testdata/{sht,inverse_sht}-regression.pt (lobatto 9x18)."""
    import ace_amd
    x = load_golden("gen_sht_input.pt")["x"]
    g = load_golden("ref_sht-regression.pt")["output"]
    gi = load_golden("ref_inverse_sht-regression.pt")["output"]
    sht, isht = ace_amd.RealSHT(9, 18), ace_amd.InverseRealSHT(9, 18)
    c = sht(x.to(dev))
    assert c.shape == (1, 8, 10) and c.dtype == torch.complex64
    torch.testing.assert_close(c.cpu(), g)            # the reference's own bar (rtol 1.3e-6, atol 1e-5)
    torch.testing.assert_close(isht(c).cpu(), gi)
    assert rel_max(c, g) <= OP_TOL


@pytest.mark.parametrize("nlat,nlon,lmax,mmax,grid,n", [
    (9, 18, None, None, "lobatto", 1), (9, 18, None, None, "equiangular", 5), (6, 12, None, None, "legendre-gauss", 3),
    (12, 24, 8, 9, "legendre-gauss", 4), (45, 90, None, None, "legendre-gauss", 16), (13, 27, None, None, "equiangular", 2),
    (13, 27, None, None, "legendre-gauss", 2),
    (64, 128, 40, 50, "legendre-gauss", 7),
    # widths with an instantiated two-level FFT (csrc/fft.hip: 16, 24, 48, 360, 720, 1440), truncated mmax, channel counts that
    # leave the last 8 / 16 / 32-row channel block ragged
    (8, 16, None, None, "equiangular", 3), (24, 48, 20, 17, "legendre-gauss", 33), (180, 360, 120, 100, "legendre-gauss", 17),
    (30, 720, 24, 15, "equiangular", 9), (20, 1440, 16, 12, "legendre-gauss", 5),
])
@pytest.mark.parametrize("precision", ["fp32", "f16x3", "f16x3-nofold"])
def test_sht_vs_oracle(dev, nlat, nlon, lmax, mmax, grid, n, precision, monkeypatch):
    """f16x3: the Legendre stages run the equatorially folded strip kernel (csrc/strip_fold.hip) wherever the tables are
    mirror-symmetric (all three quadratures; odd nlat has a self-mirrored middle row); f16x3-nofold: csrc/strip.hip, all latitudes."""
    import ace_amd
    import oracle
    if precision == "f16x3-nofold":
        monkeypatch.setenv("ACE_NO_FOLD", "1")   # read when the plan is built
        precision = "f16x3"
    x = torch.randn(n, nlat, nlon, generator=torch.Generator().manual_seed(nlat))
    o_f = oracle.RealSHT(nlat, nlon, lmax, mmax, grid, dtype=torch.float64)
    o_i = oracle.InverseRealSHT(nlat, nlon, lmax, mmax, grid, dtype=torch.float64)
    c_ref = o_f(x)
    sht = ace_amd.RealSHT(nlat, nlon, lmax, mmax, grid, precision=precision)
    isht = ace_amd.InverseRealSHT(nlat, nlon, lmax, mmax, grid, precision=precision)
    c = sht(x.to(dev))
    assert rel_max(c, c_ref) <= OP_TOL
    # arbitrary (non band-limited, l<m populated) coefficients through the inverse
    cz = torch.randn(n, o_i.lmax, o_i.mmax, dtype=torch.complex64, generator=torch.Generator().manual_seed(3))
    assert rel_max(isht(cz.to(dev)), o_i(cz)) <= OP_TOL


def test_sht_leading_dims_and_empty(dev):
    import ace_amd
    import oracle
    sht = ace_amd.RealSHT(12, 24, grid="legendre-gauss")
    x = torch.randn(2, 3, 12, 24, generator=torch.Generator().manual_seed(0))
    c = sht(x.to(dev))
    assert c.shape == (2, 3, 12, 13)
    assert rel_max(c, oracle.RealSHT(12, 24, grid="legendre-gauss", dtype=torch.float64)(x)) <= OP_TOL
    assert sht(torch.empty(0, 12, 24, device=dev)).shape == (0, 12, 13)
    with pytest.raises(AssertionError):
        sht(torch.zeros(1, 12, 25, device=dev))
    with pytest.raises(ValueError):
        ace_amd.RealSHT(12, 24, grid="nonsense")
    with pytest.raises(NotImplementedError):
        ace_amd.RealSHT(12, 24, grid="healpix")


@pytest.mark.parametrize("precision", ["fp32", "f16x3", "f16x3-nofold"])
def test_sht_180x360_vs_reference(dev, precision, monkeypatch):
    """coefficients and round trip emitted by the reference itself (tests/golden/make_golden.py)."""
    import ace_amd
    if precision == "f16x3-nofold":
        monkeypatch.setenv("ACE_NO_FOLD", "1")
        precision = "f16x3"
    d = load_golden("gen_sht_180x360.pt")
    x = torch.randn(3, 180, 360, generator=torch.Generator().manual_seed(d["seed"]))
    sht = ace_amd.RealSHT(180, 360, lmax=180, mmax=181, grid="legendre-gauss", precision=precision)
    isht = ace_amd.InverseRealSHT(180, 360, lmax=180, mmax=181, grid="legendre-gauss", precision=precision)
    c = sht(x.to(dev))
    assert rel_max(c, d["coeffs"]) <= SHT_TOL
    assert rel_max(isht(c), d["roundtrip"]) <= SHT_TOL
    assert rel_max(isht(d["coeffs"].to(dev)), d["roundtrip"]) <= SHT_TOL


@pytest.mark.parametrize("grid", ["equiangular", "legendre-gauss"])
@pytest.mark.parametrize("constant", [1.0, 0.42])
def test_constant_field(dev, grid, constant):
    """fme/test_harmonics.py:10-25."""
    import ace_amd
    coeffs = ace_amd.RealSHT(6, 12, grid=grid).to(dev)(torch.full((6, 12), constant, device=dev)).ravel().cpu()
    assert abs(coeffs[0]) > 1e-3
    assert torch.all(coeffs[1:].abs() < 1e-6)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_full_size_properties(dev, precision):
    """ACE2 shape (384 fields of 180x360): round-trip idempotence (fme/test_harmonics.py:35-42), linearity and
    the triangular zero pattern, where the CPU oracle would take minutes."""
    import ace_amd
    sht = ace_amd.RealSHT(180, 360, lmax=180, mmax=181, grid="legendre-gauss", precision=precision)
    isht = ace_amd.InverseRealSHT(180, 360, lmax=180, mmax=181, grid="legendre-gauss", precision=precision)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(384, 180, 360, device=dev, generator=g)
    y = torch.randn(384, 180, 360, device=dev, generator=g)
    cx, cy = sht(x), sht(y)
    p = isht(cx)
    assert rel_max(isht(sht(p)), p) <= SHT_TOL                       # projection is idempotent
    assert rel_max(sht(2.5 * x - 0.5 * y), 2.5 * cx - 0.5 * cy) <= SHT_TOL   # linear
    l = torch.arange(180, device=dev)[:, None]
    m = torch.arange(181, device=dev)[None, :]
    assert torch.all(cx[:, (m > l)] == 0)                            # l < m coefficients are exactly zero


# ---------------------------------------------------------------------------------- network
def _oracle_and_native(cfg, state, x, dev, precision):
    from oracle.sfno import SFNOOracle
    net = build_native_net(cfg, state, dev, precision)
    with torch.no_grad():
        y = net(x.to(dev))
    ref64 = SFNOOracle(cfg, state, dtype=torch.float64)(x)
    ref32 = SFNOOracle(cfg, state, dtype=torch.float32)(x)
    return y, ref32, ref64, net


def test_modulus_sfnonet_golden(dev, precision):
    """fme/ace/models/modulus/testdata/test_sfnonet_output_is_unchanged.pt ('diagonal' operator,
    equiangular outer grid => residual round-trips through spectral space)."""
    from oracle.sfno import SFNOConfig
    d = load_golden("gen_modulus_sfnonet_case.pt")
    g = load_golden("ref_modulus_sfnonet_output.pt")
    cfg = SFNOConfig(**d["cfg"])
    net = build_native_net(cfg, d["state"], dev, precision)
    with torch.no_grad():
        y = net(d["x"].to(dev))
    torch.testing.assert_close(y.cpu(), g)
    assert_net_close(y, g, NET_TOL)


@pytest.mark.parametrize("name", ["gen_sfno_dhconv_12x24.pt", "gen_sfno_dhconv_equiangular_9x18.pt",
                                  "gen_sfno_dhconv_180x360_c8.pt",
                                  # the "layer_norm" normalisation (sfnonet.py:584-592), make_golden_layer_norm.py
                                  "gen_sfno_layer_norm_12x24.pt", "gen_sfno_layer_norm_equiangular_9x18.pt"])
def test_dhconv_nets_vs_reference(dev, name, precision):
    from oracle.sfno import SFNOConfig, init_state
    d = load_golden(name)
    cfg = SFNOConfig(**{**d["cfg"], "img_shape": tuple(d["cfg"]["img_shape"])})
    state = init_state(cfg, seed=d["seed"])
    x = torch.randn(d["batch"], cfg.in_chans, *cfg.img_shape, generator=torch.Generator().manual_seed(d["seed"] + 1000))
    net = build_native_net(cfg, state, dev, precision)
    with torch.no_grad():
        y = net(x.to(dev))
    assert_net_close(y, d["y"], NET_TOL)


@pytest.mark.parametrize("C,hw", [(128, (24, 48)), (40, (16, 32))])
def test_layer_norm_nets_vs_oracle(dev, C, hw, precision):
    """normalization_layer = "layer_norm" (sfnonet.py:584-592: nn.LayerNorm over (H, W), an (H, W) affine shared by the channels, in
    front of the filter and of the MLP): materialised in place by spatial_layer_norm_kernel, the convolutions on the packed-operand
    engine (C = 128) or the tile engines (C = 40) - 3 blocks, batch 2, random affines, against the fp64 oracle; graph replay = eager."""
    from oracle.sfno import SFNOConfig, SFNOOracle, init_state
    cfg = SFNOConfig(in_chans=5, out_chans=4, img_shape=hw, embed_dim=C, num_layers=3, operator_type="dhconv", normalization_layer="layer_norm")
    st = init_state(cfg, seed=41)
    x = torch.randn(2, 5, *hw, generator=torch.Generator().manual_seed(42))
    ref = SFNOOracle(cfg, st, dtype=torch.float64).forward(x)
    net = build_native_net(cfg, st, dev, precision)
    out = torch.empty(2, 4, *hw, device=dev)
    with torch.no_grad():
        y = net(x.to(dev)).clone()
        net.forward_graph(x.to(dev), out)
        torch.cuda.synchronize()
    assert_net_close(y, ref, NET_TOL)
    assert torch.equal(out, y)


@pytest.mark.parametrize("case", ["sf2_3blocks", "sf2_2blocks", "sf2_1block", "sf3_equiangular", "sf2_layer_norm", "sf2_diagonal_no_norm",
                                  "rff2", "rff2_sf2", "rff3_sf3_equiangular"])
def test_scale_factor_nets_vs_reference(dev, case, precision):
    """scale_factor != 1 (sfnonet.py:467-515; the filter's residual round trip, s2convolutions.py:165-172) against outputs of the REAL
    reference net (tests/golden/make_golden_scale_factor.py): the first block goes from the data grid to the inner Gauss-Legendre grid,
    the last one back, one to three blocks, instance / layer / no norm, dhconv and diagonal filters."""
    from oracle.sfno import SFNOConfig, init_state
    d = load_golden("gen_sfno_scale_factor.pt")[case]
    cfg = SFNOConfig(**{**d["cfg"], "img_shape": tuple(d["cfg"]["img_shape"])})
    state = init_state(cfg, seed=d["seed"])
    x = torch.randn(d["batch"], cfg.in_chans, *cfg.img_shape, generator=torch.Generator().manual_seed(d["seed"] + 1000))
    net = build_native_net(cfg, state, dev, precision)
    with torch.no_grad():
        y = net(x.to(dev))
    assert_net_close(y, d["y"], NET_TOL)


@pytest.mark.parametrize("kw", [dict(), dict(num_layers=2), dict(normalization_layer="layer_norm"), dict(data_grid="equiangular", scale_factor=3),
                                dict(residual_filter_factor=2), dict(residual_filter_factor=3, scale_factor=1)])
def test_scale_factor_wide_nets_vs_oracle(dev, kw, precision):
    """scale_factor 2 / 3 at C = 128 on 48 x 96 (inner grid 24 x 48 / 16 x 32): the middle blocks run the fused packed-operand path with
    its fast kernels on the inner grid, the first and the last block the mixed-grid path - batch 2, four blocks, against the fp64
    oracle (itself exact against the real reference: test_oracle_golden.py::test_scale_factor_nets_vs_reference); graph = eager."""
    from oracle.sfno import SFNOConfig, SFNOOracle, init_state
    cfg = SFNOConfig(**{**dict(in_chans=5, out_chans=4, img_shape=(48, 96), embed_dim=128, num_layers=4, operator_type="dhconv", scale_factor=2), **kw})
    st = init_state(cfg, seed=71)
    x = torch.randn(2, 5, 48, 96, generator=torch.Generator().manual_seed(72))
    ref = SFNOOracle(cfg, st, dtype=torch.float64).forward(x)
    net = build_native_net(cfg, st, dev, precision)
    out = torch.empty(2, 4, 48, 96, device=dev)
    with torch.no_grad():
        y = net(x.to(dev)).clone()
        net.forward_graph(x.to(dev), out)
        torch.cuda.synchronize()
    assert_net_close(y, ref, NET_TOL)
    assert torch.equal(out, y)


@pytest.mark.parametrize("kw", [
    dict(normalization_layer="none"), dict(use_mlp=False), dict(big_skip=False, pos_embed=False),
    dict(activation_function="silu", encoder_layers=2), dict(hard_thresholding_fraction=0.6),
    dict(operator_type="diagonal", data_grid="equiangular"), dict(num_layers=1, data_grid="equiangular"),
])
def test_config_variants_vs_oracle(dev, kw, precision):
    from oracle.sfno import SFNOConfig, init_state
    base = dict(in_chans=5, out_chans=4, img_shape=(16, 32), embed_dim=12, num_layers=2, operator_type="dhconv")
    cfg = SFNOConfig(**{**base, **kw})
    state = init_state(cfg, seed=3)
    x = torch.randn(2, 5, 16, 32, generator=torch.Generator().manual_seed(9))
    y, ref32, ref64, _ = _oracle_and_native(cfg, state, x, dev, precision)
    assert_net_close(y, ref64, NET_TOL)


def test_block_taps_vs_oracle(dev, precision):
    """teacher-forced per-block error at a mid size (C=64, 45x90), against the fp64 oracle."""
    from oracle.sfno import SFNOConfig, SFNOOracle, init_state
    cfg = SFNOConfig(in_chans=6, out_chans=5, img_shape=(45, 90), embed_dim=64, num_layers=3, operator_type="dhconv")
    state = init_state(cfg, seed=4)
    x = torch.randn(2, 6, 45, 90, generator=torch.Generator().manual_seed(10))
    net = build_native_net(cfg, state, dev, precision)
    with torch.no_grad():
        y, taps = net.forward_with_taps(x.to(dev))
    ref, rtaps = SFNOOracle(cfg, state, dtype=torch.float64).forward(x, return_blocks=True)
    for i, rt in enumerate(rtaps):
        assert rel_max(taps[i + 1], rt) <= NET_TOL, f"block {i}"
    assert_net_close(y, ref, NET_TOL)


@pytest.mark.parametrize("offset", [0.0, 4.0])
def test_packed_fused_path_vs_oracle(dev, precision, offset):
    """The packed-operand path with fused instance norms (P-format planes from the producers' epilogues, norm affine
    folded into tiled fp16 weights, statistics from the epilogue partials): C % 8 == 0 and H*W % 4 == 0, batch 3,
    4 blocks (blocks 1.. take h in P format from the previous fc2), random norm gains/offsets, and an input with a
    large mean (the folded affine then cancels a big constant) - per-block taps against the fp64 oracle."""
    from oracle.sfno import SFNOConfig, SFNOOracle, init_state
    cfg = SFNOConfig(in_chans=5, out_chans=4, img_shape=(24, 48), embed_dim=32, num_layers=4, operator_type="dhconv")
    state = init_state(cfg, seed=11)
    g = torch.Generator().manual_seed(12)
    for k in state:
        if ".norm" in k and k.endswith("weight"):
            state[k] = 1.0 + 0.3 * torch.randn(state[k].shape, generator=g)
        if ".norm" in k and k.endswith("bias"):
            state[k] = 0.2 * torch.randn(state[k].shape, generator=g)
    x = torch.randn(3, 5, 24, 48, generator=g) * 0.7 + offset
    net = build_native_net(cfg, state, dev, precision)
    with torch.no_grad():
        y, taps = net.forward_with_taps(x.to(dev))
        y2 = net(x.to(dev))
    assert torch.equal(y, y2)
    ref, rtaps = SFNOOracle(cfg, state, dtype=torch.float64).forward(x, return_blocks=True)
    for i, rt in enumerate(rtaps):
        assert rel_max(taps[i + 1], rt) <= NET_TOL, f"block {i}: {rel_max(taps[i + 1], rt)}"
    assert_net_close(y, ref, NET_TOL)


@pytest.mark.parametrize("kw", [
    dict(activation_function="silu"), dict(activation_function="relu", encoder_layers=2), dict(use_mlp=False),
    dict(normalization_layer="none"), dict(num_layers=10), dict(mlp_ratio=1.0), dict(big_skip=False, pos_embed=False),
    dict(hard_thresholding_fraction=0.6), dict(data_grid="equiangular", num_layers=3),
    dict(embed_dim=128, num_layers=2),       # C % 128 == 0: the compact complex-structured filter operand
    dict(embed_dim=128, num_layers=3, data_grid="equiangular"),   # ... mixed with expanded operands on the edge blocks
])
def test_packed_path_config_variants(dev, kw):
    """every branch around the packed-operand path (C % 8 == 0, H*W % 4 == 0), f16x3 against the fp64 oracle: activations,
    no MLP, no norm (pack passes instead of folds), > 8 blocks (slot recycling), mixed grids (fp32 D on the edge blocks),
    truncated spectra, and the compact filter operand."""
    from oracle.sfno import SFNOConfig, SFNOOracle, init_state
    base = dict(in_chans=5, out_chans=4, img_shape=(24, 48), embed_dim=32, num_layers=3, operator_type="dhconv")
    cfg = SFNOConfig(**{**base, **kw})
    state = init_state(cfg, seed=5)
    x = torch.randn(2, 5, 24, 48, generator=torch.Generator().manual_seed(6))
    net = build_native_net(cfg, state, dev, "f16x3")
    with torch.no_grad():
        y = net(x.to(dev))
    ref = SFNOOracle(cfg, state, dtype=torch.float64).forward(x)
    assert_net_close(y, ref, NET_TOL)


def test_corrector_and_ocean_on_device(dev):
    """the post-step hooks are plain torch ops on the device the state lives on: the ACE2-like corrector configuration
    (fp64 global means on the GPU) and the prescribed-SST ocean against the reference's golden vectors."""
    import datetime
    import ace_amd
    from ace_amd.corrector import AtmosphereCorrectorConfig
    from ace_amd.ocean import OceanConfig
    g = load_golden("gen_corrector.pt")
    to = lambda d: {k: v.to(dev) for k, v in d.items()}
    info = ace_amd.DatasetInfo((8, 16), timestep=datetime.timedelta(seconds=g["timestep_seconds"]), lat=g["lat"],
                               lon=g["lon"], ak=g["ak"], bk=g["bk"])
    cfg = AtmosphereCorrectorConfig(conserve_dry_air=True, moisture_budget_correction="advection_and_precipitation",
                                    force_positive_names=["PRATEsfc", "specific_total_water_0", "specific_total_water_1"],
                                    total_energy_budget_correction={"method": "constant_temperature"},
                                    clip_frozen_precipitation=True)
    c = cfg.get_corrector(info)
    out0, st = c(to(g["input0"]), to(g["gen0"]), to(g["forcing"]), None)
    out1, _ = c({**out0, **to(g["forcing"])}, to(g["gen1"]), to(g["forcing"]), st)
    exp = g["expected"]["ace2_like"]
    for k in exp["step0"]:   # budget residuals are differences of nearly cancelling terms: tolerance relative to the field
        for got, want in ((out0[k], exp["step0"][k]), (out1[k], exp["step1"][k])):
            torch.testing.assert_close(got.cpu(), want, rtol=2e-6, atol=2e-6 * float(want.abs().max()))
    o = g["ocean"]
    oc = OceanConfig("sst", "frac").build(["sst", "frac", "q"], ["sst", "q"])(to(o["input"]), to(o["gen"]), to(o["target"]))
    assert torch.equal(oc["sst"].cpu(), o["expected"][False]["sst"])


def test_graph_replay_packed_path_batch2(dev):
    """hipGraph replay == eager on the packed path with batch 2 (per-sample folded weights, statistics partials) and
    fresh inputs on every replay."""
    from oracle.sfno import SFNOConfig, init_state
    cfg = SFNOConfig(in_chans=4, out_chans=4, img_shape=(24, 48), embed_dim=32, num_layers=3, operator_type="dhconv")
    net = build_native_net(cfg, init_state(cfg, seed=8), dev, "f16x3")
    x = torch.randn(2, 4, 24, 48, device=dev)
    out = torch.empty(2, 4, 24, 48, device=dev)
    with torch.no_grad():
        for _ in range(6):
            x.normal_()
            ref = net(x).clone()
            net.forward_graph(x, out)
            torch.cuda.synchronize()
            assert torch.equal(out, ref)


def _csfno_noise(cfg, batch, seed):
    """the conditioning noise exactly as the reference forward draws it after torch.manual_seed(seed) (CPU)"""
    from oracle.csfno import isotropic_noise
    from oracle.sht import InverseRealSHT as OInv
    torch.manual_seed(seed)
    h, w = cfg.img_shape
    if cfg.noise_type == "isotropic":
        isht = OInv(h, w, lmax=h, mmax=w // 2 + 1, grid=cfg.data_grid, dtype=torch.float32)
        return isotropic_noise((batch, cfg.noise_embed_dim), h, w // 2 + 1, isht, torch.float32)
    return torch.randn(torch.Size([batch, cfg.noise_embed_dim, h, w]), dtype=torch.float32)


@pytest.mark.parametrize("name", ["isotropic_affine_bigskipnorm", "gaussian_groups2", "equiangular_nomlp"])
def test_noise_conditioned_sfno_vs_reference(dev, name, precision):
    """NoiseConditionedSFNO through the registry and the C ABI against the outputs of the real
    reference module (tests/golden/gen_csfno.pt) and the fp64 oracle, with the reference's own noise draw."""
    import ace_amd
    from oracle.csfno import CSFNOConfig, CSFNOOracle
    case = load_golden("gen_csfno.pt")[name]
    cfg = CSFNOConfig(in_chans=5, out_chans=4, img_shape=(12, 24), **case["kwargs"])
    noise = _csfno_noise(cfg, 2, case["forward_seed"])
    sel = ace_amd.ModuleSelector(type="NoiseConditionedSFNO", config=dict(case["kwargs"]))
    mod = sel.build(5, 4, ace_amd.DatasetInfo((12, 24)))
    net = mod.torch_module
    assert list(net.state_dict()) == list(case["state"])          # the reference's names, in its order
    net.load_state_dict(case["state"], strict=True)
    net.to(dev).set_precision(precision)
    with torch.no_grad():
        y = net(case["x"].to(dev), noise=noise.to(dev))
        y2 = net(case["x"].to(dev), noise=noise.to(dev))
    assert torch.equal(y, y2)
    assert_net_close(y, case["y"], NET_TOL)
    ref64 = CSFNOOracle(cfg, case["state"], dtype=torch.float64).forward(case["x"], noise=noise)
    assert_net_close(y, ref64, NET_TOL)
    with torch.no_grad():                                         # own noise draw: runs, finite, differs per call
        a, b = net(case["x"].to(dev)), net(case["x"].to(dev))
    assert torch.isfinite(a).all() and not torch.equal(a, b)


@pytest.mark.parametrize("embed,noise_dim,groups", [(128, 8, 1), (256, 8, 1), (512, 33, 1), (256, 8, 4), (256, 8, 2), (512, 8, 2), (384, 8, 2),
                                                    (512, 8, 8), (256, 8, 8)])
def test_noise_conditioned_sfno_wide_vs_oracle(dev, embed, noise_dim, groups):
    """Channel widths at which the noise-conditioned net's fc1 runs on csrc/conv_wl.hip (weights in LDS; K = 128 / 256 here,
    512 at the ERA5 configuration), the other convolutions on the packed-operand engine and - C % 256 == 0 - the conditional
    layer norms on the single-pass MFMA kernel (csrc/cln_mfma.hip): against the fp64 oracle with the module's own
    (reference-order) initial weights.  The small reference-emitted goldens stay on the tile engines.  groups > 1: the block-diagonal
    spectral filter (s2convolutions.py:119-135) on csrc/dhconv_strip.hip, which skips the zero blocks where the group size divides or
    is a multiple of its 128-channel column groups (64, 128, 256 here; 192 = the dense walk)."""
    import ace_amd
    from oracle.csfno import CSFNOConfig, CSFNOOracle
    kwargs = dict(embed_dim=embed, noise_embed_dim=noise_dim, noise_type="gaussian", num_layers=2, use_mlp=True, mlp_ratio=2.0,
                  affine_norms=True, normalize_big_skip=True, filter_num_groups=groups)
    cfg = CSFNOConfig(in_chans=5, out_chans=4, img_shape=(16, 32), **kwargs)
    torch.manual_seed(11)
    net = ace_amd.ModuleSelector(type="NoiseConditionedSFNO", config=dict(kwargs)).build(5, 4, ace_amd.DatasetInfo((16, 32))).torch_module
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    for k, v in state.items():                      # biases / norm affines / noise projections away from their trivial initial values
        if v.ndim <= 1 or "W_scale" in k or "W_bias" in k:
            state[k] = v + 0.1 * torch.randn(v.shape, generator=g)
    net.load_state_dict(state, strict=True)
    net.to(dev).set_precision("f16x3")
    x = torch.randn(2, 5, 16, 32, generator=g)
    noise = _csfno_noise(cfg, 2, 17)
    with torch.no_grad():
        y = net(x.to(dev), noise=noise.to(dev))
    ref64 = CSFNOOracle(cfg, state, dtype=torch.float64).forward(x, noise=noise)
    assert_net_close(y, ref64, NET_TOL)
    if groups > 1:
        # The grouped filter is stored as the reference stores it - (G, L, C/G, C/G, 2), diagonal blocks only - wherever the strip
        # kernel reads that form (C / G a multiple of 32 that divides or is a multiple of 128); ACE_DENSE_GROUPED_FILTER=1 expands
        # it to the dense (C x C) form of round 4.  Skipping exact zeros changes no bit; the memory is 1 / G.
        import os
        from ace_amd import _lib
        native_bytes = _lib.lib().ace_sfno_workspace_size(net._native, 2)
        os.environ["ACE_DENSE_GROUPED_FILTER"] = "1"
        try:
            dense = ace_amd.ModuleSelector(type="NoiseConditionedSFNO", config=dict(kwargs)).build(5, 4, ace_amd.DatasetInfo((16, 32))).torch_module
            dense.load_state_dict(state, strict=True)
            dense.to(dev).set_precision("f16x3")
            with torch.no_grad():
                yd = dense(x.to(dev), noise=noise.to(dev))
            dense_bytes = _lib.lib().ace_sfno_workspace_size(dense._native, 2)
        finally:
            del os.environ["ACE_DENSE_GROUPED_FILTER"]
        assert torch.equal(y, yd)
        cg = embed // groups
        if cg % 32 == 0 and (cg % 128 == 0 or 128 % cg == 0):
            L = 16
            saved = 2 * (embed * embed * L * 2 * 4) * (1 - 1 / groups) * 2          # 2 layers x (fp32 copy + hi / lo planes) x the off-diagonal share
            assert dense_bytes - native_bytes >= 0.95 * saved, (dense_bytes, native_bytes, saved)
        else:
            assert dense_bytes == native_bytes


@pytest.mark.parametrize("name", ["labels3_pos4", "labels3_embed2_pos2_isotropic", "labels2_nopos"])
def test_noise_conditioned_sfno_with_labels_and_positional_context(dev, name, precision):
    """label and positional conditioning (stochastic_sfno.py:88-175, conditional_sfno/layers.py:160-318) through the registry
    with conditional=True: BatchLabels conformed to the module's encoding, positional context pos_embed + labels . label_pos_embed,
    every conditional norm's label / positional weights merged into the one conditioning field the native kernel reads -
    against the REAL reference's output (tests/golden/gen_csfno_context.pt) and the fp64 oracle, with the reference's own noise
    draw."""
    import ace_amd
    from ace_amd.labels import BatchLabels
    from oracle.csfno import CSFNOConfig, CSFNOOracle
    case = load_golden("gen_csfno_context.pt")[name]
    cfg = CSFNOConfig(in_chans=5, out_chans=4, img_shape=(12, 24), **case["kwargs"])
    noise = _csfno_noise(cfg, 3, case["forward_seed"])

    class Info:
        img_shape = (12, 24)
        all_labels = set(case["all_labels"])

    mod = ace_amd.ModuleSelector(type="NoiseConditionedSFNO", config=dict(case["kwargs"]), conditional=True).build(5, 4, Info())
    mod.load_state({**case["state"], "label_encoding": {"labels": case["all_labels"]}})
    net = mod.torch_module.to(dev).set_precision(precision)
    labels = case["labels"].to(dev)
    with torch.no_grad():
        y = net(case["x"].to(dev), labels=labels, noise=noise.to(dev))
    assert_net_close(y, case["y"], NET_TOL)
    ref64 = CSFNOOracle(cfg, case["state"], dtype=torch.float64).forward(case["x"], noise=noise, labels=case["labels"])
    assert_net_close(y, ref64, NET_TOL)
    with torch.no_grad():                                         # through the registry wrapper, columns in another order
        perm = list(reversed(range(len(case["all_labels"]))))
        bl = BatchLabels(labels[:, perm], [case["all_labels"][i] for i in perm])
        torch.manual_seed(7)
        a = ace_amd.registry.Module(net, mod._label_encoding)(case["x"].to(dev), labels=bl)
        torch.manual_seed(7)
        b = net(case["x"].to(dev), labels=labels)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    with pytest.raises(ValueError):
        net(case["x"].to(dev))                                    # labels must be provided


def test_conditional_stepper_rollout_with_labels(dev):
    """A conditional module behind the SAME stepper API: SingleModuleStepConfig with ModuleSelector(conditional=True) on a
    dataset with labels; Stepper.predict(..., labels=BatchLabels) hands the labels to every step (single_module.py:420-428).
    Same seed -> same rollout; other labels -> another rollout; missing labels -> TypeError (module.py:80-82)."""
    import ace_amd
    from ace_amd.labels import BatchLabels
    from ace_amd.step import NormalizationConfig
    in_names, out_names = ["f0", "p0"], ["p0", "d0"]
    names = sorted(set(in_names + out_names))
    cfg = ace_amd.SingleModuleStepConfig(
        builder=ace_amd.ModuleSelector(type="NoiseConditionedSFNO", conditional=True,
                                       config={"embed_dim": 16, "noise_embed_dim": 4, "num_layers": 2, "pos_embed": False,
                                               "context_pos_embed_dim": 2}),
        in_names=in_names, out_names=out_names,
        normalization=NormalizationConfig(means={k: 0.0 for k in names}, stds={k: 1.0 for k in names}))
    torch.manual_seed(0)
    stepper = ace_amd.Stepper.from_config(cfg, ace_amd.DatasetInfo((12, 24), all_labels={"era5", "shield"}), device=dev)
    stepper.set_eval()
    net = stepper.modules[0]
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if ".W_scale_" in k or ".W_bias_" in k or k in ("label_pos_embed",):
                p.copy_((0.3 * torch.randn(p.shape, generator=g)).to(dev))
    B, T = 2, 3
    ic = {"p0": torch.randn(B, 1, 12, 24, generator=g).to(dev)}
    forcing = {"f0": torch.randn(B, T + 1, 12, 24, generator=g).to(dev)}
    enc = stepper._step_obj.module._label_encoding
    assert enc.names == ["era5", "shield"]
    la = enc.encode([{"era5"}, {"shield"}], dev)
    lb = enc.encode([{"shield"}, {"shield"}], dev)
    assert isinstance(la, BatchLabels)
    torch.manual_seed(3)
    a, _ = stepper.predict(ic, forcing, labels=la)
    torch.manual_seed(3)
    a2, _ = stepper.predict(ic, forcing, labels=la)
    torch.manual_seed(3)
    b, _ = stepper.predict(ic, forcing, labels=lb)
    assert all(torch.equal(a[k], a2[k]) and torch.isfinite(a[k]).all() and a[k].shape == (B, T, 12, 24) for k in out_names)
    assert not torch.equal(a["p0"][0], b["p0"][0])                 # sample 0 changed its label
    assert rel_max(a["p0"][1, 0], b["p0"][1, 0]) <= 2e-6           # sample 1 did not (first step: same noise draw, same label;
                                                                   #  the range bounds span the batch, so not bitwise)
    with pytest.raises(TypeError):
        stepper.predict(ic, forcing)
    # the static-buffer engine: labels set once per window series, merged into the conditioning field of every step
    from ace_amd.rollout import RolloutEngine
    eng = RolloutEngine(stepper, batch=B, n_forward_steps=T, graph=None)
    eng.set_labels(la)
    torch.manual_seed(3)
    e, _ = eng.predict(ic, forcing)
    torch.cuda.synchronize()
    for k in out_names:
        assert rel_max(e[k], a[k]) <= 2e-6, k
    eng.set_labels(None)
    with pytest.raises(ValueError):
        eng.predict(ic, forcing)                                   # labels must be provided


def test_noise_conditioned_sfno_reference_held_checkpoint_golden(dev, precision):
    """The reference-HELD, RNG-free golden of the conditional family (conditional_sfno/test_sfnonet.py:162-191,
    testdata/test_sfnonet_checkpoint_{input,output}.pt) through the registry and the C ABI: legacy spectral-filter layout on load,
    scalar embedding + labels as one label vector (tests/_util.py), 16-channel noise context, equiangular 9 x 18, big skip - at the
    reference's own assert_close bar (rtol 1.3e-6, atol 1e-5)."""
    import ace_amd
    from _util import csfno_reference_checkpoint_case
    c = csfno_reference_checkpoint_case()

    class Info:
        img_shape = (9, 18)
        all_labels = set(c["labels"])

    net = ace_amd.ModuleSelector(type="NoiseConditionedSFNO", config=dict(c["kwargs"]), conditional=True).build(2, 3, Info()).torch_module
    net.load_state_dict(c["state"], strict=True)
    net.to(dev).set_precision(precision)
    with torch.no_grad():
        y = net(c["x"].to(dev), labels=c["label_vector"].to(dev), noise=c["noise"].to(dev))
    torch.testing.assert_close(y.cpu(), c["y"])
    assert_net_close(y, c["y"], NET_TOL)


@pytest.mark.parametrize("name", ["csfno_block", "csfno_block_8_groups"])
def test_noise_conditioned_sfno_reference_held_block_goldens(dev, name, precision):
    """The reference's block-level regression goldens (fme/core/benchmark/testdata/csfno_block{,_8_groups}-regression.pt,
    conditional_sfno/benchmark.py:100-119: dense and 8-group spectral filter, lobatto 9 x 18, noise + label + positional context)
    through the C ABI: a one-block network with identity encoder / decoder (tests/_util.py: csfno_block_case) minus norm0(x) - the
    identity outer skip the stand-alone block does not have - at the reference's own assert_close bar."""
    import ace_amd
    from _util import csfno_block_case, csfno_block_norm0
    c = csfno_block_case(name)

    class Info:
        img_shape = (9, 18)
        all_labels = set(c["labels"])

    net = ace_amd.ModuleSelector(type="NoiseConditionedSFNO", config=dict(c["kwargs"]), conditional=True).build(16, 16, Info()).torch_module
    net.load_state_dict(c["state"], strict=True)
    net.to(dev).set_precision(precision)
    with torch.no_grad():
        y = net(c["x"].to(dev), labels=c["label_vector"].to(dev), noise=c["noise"].to(dev))
    block = (y.cpu().double() - csfno_block_norm0(c)).float()
    torch.testing.assert_close(block, c["y"])
    assert_net_close(block, c["y"], NET_TOL)


def test_noise_conditioned_sfno_errors(dev):
    import ace_amd
    sel = ace_amd.ModuleSelector(type="NoiseConditionedSFNO", config={"embed_dim": 8, "noise_embed_dim": 4, "num_layers": 1})
    net = sel.build(2, 2, ace_amd.DatasetInfo((8, 16))).torch_module.to(dev)
    with pytest.raises(ValueError):
        net(torch.zeros(1, 2, 8, 16, device=dev), noise=torch.zeros(1, 3, 8, 16, device=dev))
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 2, 8, 16))
    with pytest.raises(NotImplementedError):
        ace_amd.ModuleSelector(type="NoiseConditionedSFNO", config={"lora_rank": 2}).build(2, 2, ace_amd.DatasetInfo((8, 16)))
    with pytest.raises(ValueError):
        ace_amd.ModuleSelector(type="NoiseConditionedSFNO", config={"separable": True})


def test_quarter_degree_grid(dev):
    """BASELINE configs[3] geometry (0.25 degree: 721 x 1440, L = M = 721): the SHT pair and a small dhconv net against
    the fp64 oracle - index arithmetic, odd nlat, table sizes (1.5 GB per transform) and ragged tiles at the large grid."""
    import ace_amd
    from oracle.sht import RealSHT as ORealSHT, InverseRealSHT as OInverseRealSHT
    from oracle.sfno import SFNOConfig, SFNOOracle, init_state
    H, W = 721, 1440
    f = ace_amd.RealSHT(H, W, H, W // 2 + 1, "legendre-gauss")
    i = ace_amd.InverseRealSHT(H, W, H, W // 2 + 1, "legendre-gauss")
    x = torch.randn(2, H, W, generator=torch.Generator().manual_seed(0))
    c = f(x.to(dev))
    y = i(c)
    oc = ORealSHT(H, W, H, W // 2 + 1, "legendre-gauss")(x.double())
    oy = OInverseRealSHT(H, W, H, W // 2 + 1, "legendre-gauss")(oc)
    assert rel_max(c, oc) <= SHT_TOL and rel_max(y, oy) <= SHT_TOL
    cfg = SFNOConfig(in_chans=3, out_chans=2, img_shape=(H, W), embed_dim=16, num_layers=1, operator_type="dhconv")
    st = init_state(cfg, seed=1)
    xin = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(2))
    ref = SFNOOracle(cfg, st, dtype=torch.float64).forward(xin)
    for prec in ("f16x3", "fp32"):
        net = build_native_net(cfg, st, dev, prec)
        with torch.no_grad():
            out = net(xin.to(dev))
        assert_net_close(out, ref, NET_TOL)


def _sht_route(plan_handle):
    import ctypes
    from ace_amd import _lib
    f, i = ctypes.c_int(-9), ctypes.c_int(-9)
    _lib.check(_lib.lib().ace_sht_plan_route(plan_handle, ctypes.byref(f), ctypes.byref(i)))
    return f.value, i.value


def test_quarter_degree_big_fold_kernel_vs_oracle(dev):
    """The kernel that carries BASELINE configs[3]: `legendre_fold_big_kernel` (strip_fold.hip; more than 96 folded latitudes, whole
    128-column groups) against the fp64 oracle - fme/sht_fix.py:119-139 (analysis) and :202-226 (synthesis) at 721 x 1440,
    lmax = mmax = 721, 64 fields = 128 columns of (re | im, field).  The synthesis operand is NOT band-limited data from the analysis
    but independent random coefficients, so an error common to both directions cannot cancel.  The route query asserts that both
    launches really took the big form (route 3), and that the exact-fp32 plan (which has no strip kernels) did not."""
    import ace_amd
    from oracle.sht import RealSHT as ORealSHT, InverseRealSHT as OInverseRealSHT
    H, W, n = 721, 1440, 64
    L, M = H, W // 2 + 1
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, H, W, generator=g)
    coef = torch.complex(torch.randn(n, L, M, generator=g), torch.randn(n, L, M, generator=g))
    coef = coef * (torch.arange(L)[:, None] >= torch.arange(M)[None, :])      # l >= m, as every SHT output has it
    coef = coef / (1.0 + torch.arange(L, dtype=torch.float32)[:, None]) ** 0.5   # a decaying spectrum, large-scale dominated
    oc = ORealSHT(H, W, L, M, "legendre-gauss", dtype=torch.float64)(x.double())
    oy = OInverseRealSHT(H, W, L, M, "legendre-gauss", dtype=torch.float64)(coef.to(torch.complex128))
    for prec, want_route in (("f16x3", 3), ("fp32", 0)):
        f = ace_amd.RealSHT(H, W, L, M, "legendre-gauss", precision=prec)
        i = ace_amd.InverseRealSHT(H, W, L, M, "legendre-gauss", precision=prec)
        c = f(x.to(dev))
        y = i(coef.to(dev))
        torch.cuda.synchronize()
        assert _sht_route(f._get_plan().handle)[0] == want_route, (prec, _sht_route(f._get_plan().handle))
        assert _sht_route(i._get_plan().handle)[1] == want_route, (prec, _sht_route(i._get_plan().handle))
        ec, ey = rel_max(c, oc), rel_max(y, oy)
        print(f"0.25 degree SHT pair, 64 fields, {prec}: analysis {ec:.3e}, synthesis {ey:.3e} vs fp64")
        assert ec <= SHT_TOL and ey <= SHT_TOL, (prec, ec, ey)
        # per field as well: no single column group may hide behind the tensor's maximum
        for k in (0, 31, 32, 63):
            assert rel_max(c[k], oc[k]) <= 2 * SHT_TOL and rel_max(y[k], oy[k]) <= 2 * SHT_TOL, (prec, k)


def test_quarter_degree_net_on_the_big_fold_kernel_vs_oracle(dev):
    """The in-network instantiations of the big folded Legendre kernel at 0.25 degree - the forward one writes the coefficients as
    fp16 hi / lo planes for the filter (`legendre_fold_big_kernel<1, 0>`), which the stand-alone transform never does: a C = 64
    (128 columns), one-block dhconv net against the fp64 oracle (sfnonet.py:217-252), with the route asserted."""
    import ctypes
    from ace_amd import _lib
    from oracle.sfno import SFNOConfig, SFNOOracle, init_state
    H, W = 721, 1440
    cfg = SFNOConfig(in_chans=3, out_chans=2, img_shape=(H, W), embed_dim=64, num_layers=1, operator_type="dhconv")
    st = init_state(cfg, seed=5)
    xin = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(6))
    ref = SFNOOracle(cfg, st, dtype=torch.float64).forward(xin)
    net = build_native_net(cfg, st, dev, "f16x3")
    with torch.no_grad():
        out = net(xin.to(dev))
    torch.cuda.synchronize()
    f, i = ctypes.c_int(-9), ctypes.c_int(-9)
    _lib.check(_lib.lib().ace_sfno_sht_route(net._native, ctypes.byref(f), ctypes.byref(i)))
    assert (f.value, i.value) == (3, 3), (f.value, i.value)
    assert_net_close(out, ref, NET_TOL)


ROUTING_SWITCHES = [   # (environment, value): every run-time routing switch of DESIGN section 5 that no other test sets
    ("ACE_NO_STRIP", "1"), ("ACE_NO_FOLD", "1"), ("ACE_NO_FFT", "1"), ("ACE_NO_DHCONV_STRIP", "1"), ("ACE_NO_ENC_WS", "1"), ("ACE_NO_ENC_PK", "1"),
    ("ACE_FUSED_PACK", "0"), ("ACE_PLANES_STREAM", "0"), ("ACE_CONV_WS", "none"), ("ACE_CONV_WS", "skip,fc2"), ("ACE_CONV_WL", "0"),
]


@pytest.mark.parametrize("env,value", ROUTING_SWITCHES, ids=[f"{e}={v}" for e, v in ROUTING_SWITCHES])
def test_every_routing_switch_against_the_oracle(dev, env, value, monkeypatch):
    """The routing switches are read once per handle and select between gfx950 kernels that all have to give the reference's answer
    (sfnonet.py:217-252 per block): a 3-block C = 128 net at 24 x 48 - a shape at which EVERY fast kernel is eligible (conv_ws /
    conv_wl at K = 128, the 8 x 6 longitude FFT, the folded strip Legendre kernels, dhconv_strip, the planes-only residual stream,
    rider workgroups, the encoder on conv_ws) - under each switch in turn against the fp64 oracle, batch 2, random norm gains."""
    from oracle.sfno import SFNOConfig, SFNOOracle, init_state
    cfg = SFNOConfig(in_chans=5, out_chans=4, img_shape=(24, 48), embed_dim=128, num_layers=3, operator_type="dhconv")
    st = init_state(cfg, seed=21)
    g = torch.Generator().manual_seed(22)
    for k in st:
        if "norm" in k:
            st[k] = st[k] + 0.2 * torch.randn(st[k].shape, generator=g)
    x = torch.randn(2, 5, 24, 48, generator=g)
    ref = SFNOOracle(cfg, st, dtype=torch.float64).forward(x)
    base = build_native_net(cfg, st, dev, "f16x3")
    with torch.no_grad():
        y0 = base(x.to(dev)).clone()
    assert_net_close(y0, ref, NET_TOL)
    monkeypatch.setenv(env, value)
    net = build_native_net(cfg, st, dev, "f16x3")
    out = torch.empty_like(y0)
    with torch.no_grad():
        y = net(x.to(dev)).clone()
        net.forward_graph(x.to(dev), out)
        torch.cuda.synchronize()
    assert_net_close(y, ref, NET_TOL)
    assert torch.equal(out, y)
    assert rel_max(y, y0) <= 2e-6       # two routings of one arithmetic: rounding apart


@pytest.mark.parametrize("env", ["ACE_NO_CLN_MFMA", "ACE_NO_CLN_PLANES"])
def test_conditional_norm_routing_switches_against_the_oracle(dev, env, monkeypatch):
    """ACE_NO_CLN_MFMA (statistics + apply passes) and ACE_NO_CLN_PLANES (single pass, fp32 out + a pack pass) at embed 256, where the
    single-pass MFMA norm writing planes is the default (conditional_sfno/layers.py:245-318)."""
    import ace_amd
    from oracle.csfno import CSFNOConfig, CSFNOOracle
    kwargs = dict(embed_dim=256, noise_embed_dim=8, noise_type="gaussian", num_layers=2, use_mlp=True, mlp_ratio=2.0, affine_norms=True,
                  normalize_big_skip=True, filter_num_groups=1)
    cfg = CSFNOConfig(in_chans=5, out_chans=4, img_shape=(16, 32), **kwargs)
    monkeypatch.setenv(env, "1")
    torch.manual_seed(11)
    net = ace_amd.ModuleSelector(type="NoiseConditionedSFNO", config=dict(kwargs)).build(5, 4, ace_amd.DatasetInfo((16, 32))).torch_module
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    for k, v in state.items():
        if v.ndim <= 1 or "W_scale" in k or "W_bias" in k:
            state[k] = v + 0.1 * torch.randn(v.shape, generator=g)
    net.load_state_dict(state, strict=True)
    net.to(dev).set_precision("f16x3")
    x = torch.randn(2, 5, 16, 32, generator=g)
    noise = _csfno_noise(cfg, 2, 17)
    with torch.no_grad():
        y = net(x.to(dev), noise=noise.to(dev))
    assert_net_close(y, CSFNOOracle(cfg, state, dtype=torch.float64).forward(x, noise=noise), NET_TOL)


def test_graph_replay_matches_eager(dev, precision):
    from oracle.sfno import SFNOConfig, init_state
    cfg = SFNOConfig(in_chans=4, out_chans=4, img_shape=(24, 48), embed_dim=16, num_layers=2, operator_type="dhconv")
    net = build_native_net(cfg, init_state(cfg, seed=6), dev, precision)
    x = torch.randn(1, 4, 24, 48, device=dev)
    out = torch.empty(1, 4, 24, 48, device=dev)
    with torch.no_grad():
        ref = net(x).clone()
        for _ in range(3):
            net.forward_graph(x, out)
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        for _ in range(8):               # same storage, new contents: every replay must see them (and must reset the
            x.normal_()                  # dynamic-range slots itself: a stale bound only shows with fresh inputs)
            ref2 = net(x).clone()
            net.forward_graph(x, out)
            torch.cuda.synchronize()
            assert torch.equal(out, ref2)


def _rescaled_state(state):
    """every tensor times a factor that is no power of two, one per kind of parameter: every stored scale, bound and fragment changes"""
    out = {}
    for k, v in state.items():
        f = 0.11 if k.endswith("filter.filter.weight") else 5.0 if (v.ndim <= 1 or k.endswith("pos_embed")) else 3.7
        out[k] = v * f
    return out


REUPLOAD_NETS = {   # the smallest nets at which each stored operand form of ace_sfno_set_weight exists
    # fused body, static fragments of skip / fc2 / last encoder convolution, pos_embed slot, compact filter planes
    "dhconv_f16x3": (dict(img_shape=(24, 48), embed_dim=128, num_layers=3, operator_type="dhconv"), "f16x3"),
    # library copies only + the expanded fp32 filter
    "dhconv_fp32": (dict(img_shape=(24, 48), embed_dim=128, num_layers=3, operator_type="dhconv"), "fp32"),
    # mixed-grid first and last blocks (expanded f16 operand there), inner blocks on the inner grid
    "scale_factor_2": (dict(img_shape=(48, 96), embed_dim=128, num_layers=4, operator_type="dhconv", scale_factor=2), "f16x3"),
    "diagonal": (dict(img_shape=(24, 48), embed_dim=32, num_layers=3, operator_type="diagonal"), "f16x3"),
    # conditional-norm fragments, the inner skip's and fc1's static fragments; 2 groups: the native grouped filter
    "csfno_groups_1": (1, "f16x3"),
    "csfno_groups_2": (2, "f16x3"),
}


@pytest.mark.parametrize("name", list(REUPLOAD_NETS))
def test_second_upload_into_a_live_handle_equals_a_fresh_handle(dev, name):
    """ace_sfno_set_weight into a handle that already holds values and captured graphs: every derived buffer is reused in place and
    the graphs are marked stale.  A handle loaded with A, run, then loaded with B must give - eager and replayed - bit for bit what a
    fresh handle loaded with B gives, and every upload must advance ace_sfno_weights_generation.  (The conditioned forward has no
    graph entry: the cSFNO cases run eager only.)"""
    import ace_amd
    from ace_amd import _lib
    from oracle.sfno import SFNOConfig, init_state
    spec, precision = REUPLOAD_NETS[name]
    g = torch.Generator().manual_seed(31)
    csfno = isinstance(spec, int)
    if csfno:   # the net of test_conditional_norm_routing_switches_against_the_oracle
        kwargs = dict(embed_dim=256, noise_embed_dim=8, noise_type="gaussian", num_layers=2, use_mlp=True, mlp_ratio=2.0, affine_norms=True,
                      normalize_big_skip=True, filter_num_groups=spec)
        hw = (16, 32)

        def make(state=None):
            net = ace_amd.ModuleSelector(type="NoiseConditionedSFNO", config=dict(kwargs)).build(5, 4, ace_amd.DatasetInfo(hw)).torch_module
            if state is not None:
                net.load_state_dict(state, strict=True)
            return net.to(dev).set_precision(precision)
        torch.manual_seed(11)
        state_a = {k: v.detach().clone() for k, v in make().state_dict().items()}
        noise = torch.randn(2, 8, *hw, generator=g).to(dev)
    else:
        cfg = SFNOConfig(in_chans=5, out_chans=4, **spec)
        hw = cfg.img_shape
        state_a = init_state(cfg, seed=41)
        noise = None

        def make(state):
            return build_native_net(cfg, state, dev, precision)
    for k, v in state_a.items():   # biases and norm affines away from their 0 / 1 initialisation
        if v.ndim <= 1:
            state_a[k] = v.cpu() + 0.1 * torch.randn(v.shape, generator=g)
    state_b = _rescaled_state(state_a)
    x = torch.randn(2, 5, *hw, generator=g).to(dev)

    def run(net):
        with torch.no_grad():
            if csfno:
                return net(x, noise=noise).clone(), None
            y = net(x).clone()
            out = torch.empty_like(y)
            net.forward_graph(x, out)
            torch.cuda.synchronize()
            return y, out

    def generation(net):
        return int(_lib.lib().ace_sfno_weights_generation(net._native))

    live = make(state_a)
    ya, ga = run(live)
    nparams = int(_lib.lib().ace_sfno_num_weights(live._native))
    assert generation(live) == nparams
    live.load_state_dict({k: v.to(dev) for k, v in state_b.items()}, strict=True)
    yb, gb = run(live)
    assert generation(live) == 2 * nparams          # every parameter went up again, each upload counted
    fresh = make(state_b)
    yf, gf = run(fresh)
    assert generation(fresh) == nparams
    assert torch.isfinite(yb).all() and not torch.equal(ya, yb)
    assert torch.equal(yb, yf)
    if not csfno:
        assert torch.equal(ga, ya) and torch.equal(gb, yb) and torch.equal(gf, yf)


@pytest.mark.parametrize("scale", [1e-4, 1.0, 3e3])
def test_f16x3_dynamic_range(dev, scale):
    """the compensated engine derives its power-of-two operand scales from the data: inputs and weights far from
    O(1) (trained nets, unnormalised fields) must not cost accuracy."""
    from oracle.sfno import SFNOConfig, SFNOOracle, init_state
    cfg = SFNOConfig(in_chans=4, out_chans=3, img_shape=(24, 48), embed_dim=32, num_layers=2, operator_type="dhconv")
    state = init_state(cfg, seed=8)
    for k in state:  # rescale weights so intermediate activations drift far from O(1)
        if k.endswith("filter.filter.weight") or k.startswith("encoder.0.weight"):
            state[k] = state[k] * scale
    x = torch.randn(2, 4, 24, 48, generator=torch.Generator().manual_seed(2)) * scale
    net = build_native_net(cfg, state, dev, "f16x3")
    with torch.no_grad():
        y = net(x.to(dev))
    ref = SFNOOracle(cfg, state, dtype=torch.float64)(x)
    assert torch.isfinite(y).all()
    assert_net_close(y, ref, NET_TOL)


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
def test_shrinking_batch_after_large_magnitudes(dev, prec):
    """A handle sized by a batch of 3 at magnitude 1e4, then reused for a batch of 1 at magnitude 1e-3 (lmax = 24 is not a
    multiple of 16: the strip Legendre kernels read contraction rows past K, which now fall INSIDE stale data of the larger
    call - round-2 advisor finding: stale * scale could overflow fp16 and poison the MFMA with 0 * inf).  Also the
    standalone f16x3 transform plan with a smaller n after a larger one."""
    from oracle.sfno import SFNOConfig, SFNOOracle, init_state
    cfg = SFNOConfig(in_chans=4, out_chans=3, img_shape=(24, 48), embed_dim=128, num_layers=2, operator_type="dhconv")
    state = init_state(cfg, seed=8)
    g = torch.Generator().manual_seed(9)
    big = torch.randn(3, 4, 24, 48, generator=g) * 1e4
    small = torch.randn(1, 4, 24, 48, generator=g) * 1e-3
    net = build_native_net(cfg, state, dev, prec)
    with torch.no_grad():
        yb = net(big.to(dev))
        ys = net(small.to(dev))
    assert torch.isfinite(yb).all() and torch.isfinite(ys).all()
    assert_net_close(ys, SFNOOracle(cfg, state, dtype=torch.float64)(small), NET_TOL)
    if prec == "f16x3":
        import ace_amd
        f = ace_amd.RealSHT(24, 48, 24, 25, "legendre-gauss", precision="f16x3").to(dev)
        i = ace_amd.InverseRealSHT(24, 48, 24, 25, "legendre-gauss", precision="f16x3").to(dev)
        xb = torch.randn(40, 24, 48, generator=g) * 1e4
        xs = torch.randn(3, 24, 48, generator=g) * 1e-3
        cb = f(xb.to(dev)); _ = i(cb)
        cs = f(xs.to(dev)); rs = i(cs)
        cs1 = f(xs[:1].to(dev))
        assert torch.isfinite(cs).all() and torch.isfinite(rs).all()
        assert rel_max(torch.view_as_real(cs[:1]), torch.view_as_real(cs1)) <= 1e-6


def test_f16x3_conv_vs_fp64(dev):
    """the f16x3 building block against fp64 (and against the exact-fp32 engine's own error)."""
    from ace_amd import _lib
    L = _lib.lib()
    for (n, cin, cout, hw, act, xs) in [(1, 384, 768, 8192, 1, 1.0), (2, 48, 40, 164, 1, 50.0), (1, 428, 50, 4132, 0, 1e-3)]:
        g = torch.Generator().manual_seed(cin)
        x = torch.randn(n, cin, hw, generator=g) * xs
        w = torch.nn.init.trunc_normal_(torch.empty(cout, cin), std=0.02, generator=g)
        b = torch.randn(cout, generator=g) * 0.01 * xs
        ref = torch.nn.functional.conv1d(x.double(), w.double()[:, :, None], b.double())
        if act:
            ref = torch.nn.functional.gelu(ref)
        xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
        y = torch.empty(n, cout, hw, device=dev)
        _lib.check(L.ace_conv1x1_f16x3(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(y), n, cin, cout, hw, act,
                                       _lib.current_stream()))
        assert rel_max(y, ref) <= OP_TOL


def test_f16x3_packed_mlp_vs_fp64(dev):
    """MLP (layers.py:97-137) on the packed-operand engine: P-format input, bound-scaled P-format hidden activation,
    against fp64; includes ragged tiles (hw not a multiple of the tile), batch > 1 and wide dynamic range."""
    from ace_amd import _lib
    L = _lib.lib()
    cases = [(1, 384, 768, 384, 8192, 1, 1.0), (2, 48, 40, 56, 164, 1, 50.0), (1, 136, 264, 72, 4132, 3, 1e-3),
             (3, 8, 8, 8, 4, 2, 1.0), (1, 64, 128, 64, 1000, 1, 1e8), (1, 64, 128, 64, 1000, 1, 1e-12)]
    for (n, cin, hid, cout, hw, act, xs) in cases:
        g = torch.Generator().manual_seed(cin + hw)
        x = torch.randn(n, cin, hw, generator=g) * xs
        w1 = torch.nn.init.trunc_normal_(torch.empty(hid, cin), std=0.05, generator=g)
        b1 = torch.randn(hid, generator=g) * 0.1 * xs
        w2 = torch.nn.init.trunc_normal_(torch.empty(cout, hid), std=0.05, generator=g)
        b2 = torch.randn(cout, generator=g) * 0.1 * xs
        u = torch.nn.functional.conv1d(x.double(), w1.double()[:, :, None], b1.double())
        u = {1: torch.nn.functional.gelu, 2: torch.relu, 3: torch.nn.functional.silu}[act](u)
        ref = torch.nn.functional.conv1d(u, w2.double()[:, :, None], b2.double())
        t = [v.to(dev) for v in (x, w1, b1, w2, b2)]
        y = torch.empty(n, cout, hw, device=dev)
        _lib.check(L.ace_mlp_f16x3(*[_lib.ptr(v) for v in t], _lib.ptr(y), n, cin, hid, cout, hw, act,
                                   _lib.current_stream()))
        assert rel_max(y, ref) <= OP_TOL, (n, cin, hid, cout, hw, act, xs, rel_max(y, ref))
    with pytest.raises(ValueError):
        _lib.check(L.ace_mlp_f16x3(*[_lib.ptr(v) for v in t], _lib.ptr(y), 1, 7, 8, 8, 4, 0, _lib.current_stream()))


def test_race_screen(dev, precision):
    """repeated eager / graph-replayed forwards are bitwise identical (LDS-DMA pipelines, counted vmcnt, wave roles)."""
    from oracle.sfno import SFNOConfig, init_state
    for (C, hw, L, B) in [(32, (45, 90), 2, 2), (64, (24, 48), 2, 1)]:
        cfg = SFNOConfig(in_chans=4, out_chans=4, img_shape=hw, embed_dim=C, num_layers=L, operator_type="dhconv")
        net = build_native_net(cfg, init_state(cfg, seed=6), dev, precision)
        x = torch.randn(B, 4, *hw, device=dev)
        out = torch.empty(B, 4, *hw, device=dev)
        with torch.no_grad():
            ref = net(x).clone()
            for _ in range(15):
                y = net(x)
                net.forward_graph(x, out)
                torch.cuda.synchronize()
                assert torch.equal(y, ref) and torch.equal(out, ref)


def test_errors(dev):
    """Module / builder error behaviour (module.py:77-82, sfno.py:50-53, registry.py:58)."""
    import ace_amd
    sel = ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet", config={"embed_dim": 8, "num_layers": 1})
    mod = sel.build(2, 2, ace_amd.DatasetInfo((8, 16))).to(dev)
    with pytest.raises(TypeError):
        mod(torch.zeros(1, 2, 8, 16, device=dev), labels=object())
    with pytest.raises(AssertionError):
        mod(torch.zeros(1, 2, 8, 17, device=dev))
    with pytest.raises(ValueError):
        sel.build(2, 2, ace_amd.DatasetInfo((8, 16), all_labels={"a"}))
    with pytest.raises(KeyError):
        ace_amd.ModuleSelector(type="NoSuchNet", config={})
    with pytest.raises(ValueError):
        ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet", config={"no_such_field": 1})


# ---------------------------------------------------------------------------------- stepper
def test_stepper_predict_golden(dev):
    """fme/ace/stepper/testdata/stepper_predict_regression.pt through the registry + Stepper mirror."""
    import ace_amd
    from ace_amd.step import NormalizationConfig
    d = load_golden("gen_stepper_case.pt")
    g = load_golden("ref_stepper_predict_regression.pt")
    names = ["a", "b", "c"]
    config = ace_amd.SingleModuleStepConfig(
        builder=ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet",
                                       config={"embed_dim": 16, "num_layers": 2}),
        in_names=d["in_names"], out_names=d["out_names"],
        normalization=NormalizationConfig(means={k: d["mean"] for k in names}, stds={k: d["std"] for k in names}),
    )
    stepper = ace_amd.Stepper.from_config(config, ace_amd.DatasetInfo((9, 18)), device=dev)
    stepper.load_state({"step": {"module": {**d["state"], "label_encoding": None}}})
    stepper.set_eval()
    out, nxt = stepper.predict({"b": d["b"][:, :1].to(dev)}, {"a": d["a"].to(dev)})
    torch.testing.assert_close(out["b"].cpu(), g["output.b"])
    torch.testing.assert_close(out["c"].cpu(), g["output.c"])
    torch.testing.assert_close(nxt["b"].cpu(), g["next_state.b"])


@pytest.mark.parametrize("graph", [None, "step", "window"])
def test_rollout_engine_with_hooks_matches_stepper(dev, graph):
    """post-step hooks inside the static-buffer engine (force-positive + zero-mean moisture advection corrector with
    area weights, prescribed-SST ocean whose target is a prognostic name) == the dict-of-tensors Stepper; a second
    window continued from the first keeps the corrector state."""
    import ace_amd
    from ace_amd.rollout import RolloutEngine
    from ace_amd.step import NormalizationConfig
    adv = "tendency_of_total_water_path_due_to_advection"
    in_names = ["f0", "sst", adv, "frac"]
    out_names = ["sst", adv, "d0"]
    names = sorted(set(in_names + out_names))
    config = ace_amd.SingleModuleStepConfig(
        builder=ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet",
                                       config={"embed_dim": 16, "num_layers": 2, "operator_type": "dhconv"}),
        in_names=in_names, out_names=out_names,
        normalization=NormalizationConfig(means={k: 0.1 * (i + 1) for i, k in enumerate(names)},
                                          stds={k: 1.0 + 0.1 * i for i, k in enumerate(names)}),
        ocean={"surface_temperature_name": "sst", "ocean_fraction_name": "frac"},
        corrector={"force_positive_names": ["d0"], "zero_global_mean_moisture_advection": True})
    torch.manual_seed(0)
    info = ace_amd.DatasetInfo((12, 24), lat=torch.linspace(-82.5, 82.5, 12), lon=torch.arange(24.0) * 15.0)
    stepper = ace_amd.Stepper.from_config(config, info, device=dev)
    stepper.set_eval()
    B, T = 2, 4
    ic = {k: torch.randn(B, 1, 12, 24, device=dev) for k in ["sst", adv]}
    forcing = {k: torch.randn(B, T + 1, 12, 24, device=dev) for k in ["f0", "sst"]}
    forcing["frac"] = torch.rand(B, T + 1, 12, 24, device=dev)
    ref, _ = stepper.predict(ic, forcing)
    eng = RolloutEngine(stepper, batch=B, n_forward_steps=T, graph=graph)
    assert eng.target_names == ["sst"]
    out, state = eng.predict(ic, forcing)
    torch.cuda.synchronize()
    for k in out_names:   # the mean-removed advection field is small against the field it was computed from
        assert rel_max(out[k], ref[k]) <= (1e-5 if k == adv else 2e-6), k
    assert float(out["d0"].min()) >= 0.0
    w = info.area_weights.to(dev)
    assert float((out[adv] * w).sum(dim=(-2, -1)).abs().max()) <= 1e-6
    ocean_cells = torch.round(forcing["frac"][:, 1:]) == 1
    assert torch.equal(out["sst"][ocean_cells], forcing["sst"][:, 1:][ocean_cells])


@pytest.mark.parametrize("graph", [None, "window"])
def test_rollout_engine_with_slab_ocean_matches_stepper(dev, graph):
    """slab ocean (fme/core/ocean.py:64-92) in the static-buffer engine: the fused physics kernels know the prescribed SST only,
    so the engine applies the slab update as the same torch ops the Stepper runs (captured in the graph modes) - engine ==
    Stepper == the formula applied by hand to the Stepper's own output of the first step."""
    import datetime
    import ace_amd
    from ace_amd.rollout import RolloutEngine
    from ace_amd.step import NormalizationConfig
    flux = ["DLWRFsfc", "ULWRFsfc", "DSWRFsfc", "USWRFsfc", "LHTFLsfc", "SHTFLsfc"]
    in_names = ["f0", "sst", "frac"]
    out_names = ["sst"] + flux
    names = sorted(set(in_names + out_names))
    config = ace_amd.SingleModuleStepConfig(
        builder=ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet",
                                       config={"embed_dim": 16, "num_layers": 2, "operator_type": "dhconv"}),
        in_names=in_names, out_names=out_names,
        normalization=NormalizationConfig(means={k: 0.1 * (i + 1) for i, k in enumerate(names)},
                                          stds={k: 1.0 + 0.1 * i for i, k in enumerate(names)}),
        ocean={"surface_temperature_name": "sst", "ocean_fraction_name": "frac",
               "slab": {"mixed_layer_depth_name": "mld", "q_flux_name": "qflux"}})
    torch.manual_seed(0)
    info = ace_amd.DatasetInfo((12, 24), timestep=datetime.timedelta(hours=6))
    stepper = ace_amd.Stepper.from_config(config, info, device=dev)
    stepper.set_eval()
    B, T = 2, 3
    ic = {"sst": 290.0 + torch.randn(B, 1, 12, 24, device=dev)}
    forcing = {"f0": torch.randn(B, T + 1, 12, 24, device=dev), "frac": torch.rand(B, T + 1, 12, 24, device=dev),
               "mld": 20.0 + 60.0 * torch.rand(B, T + 1, 12, 24, device=dev), "qflux": 15.0 * torch.randn(B, T + 1, 12, 24, device=dev)}
    ref, _ = stepper.predict(ic, forcing)
    eng = RolloutEngine(stepper, batch=B, n_forward_steps=T, graph=graph)
    assert eng._physics is None                                   # torch-op hooks, not the fused kernels
    out, _ = eng.predict(ic, forcing)
    torch.cuda.synchronize()
    for k in out_names:
        assert rel_max(out[k], ref[k]) <= 2e-6, k
    # first step by hand: over ocean, SST = SST_in + (F_net + Q) / (rho c_p depth) * dt
    f_net = (ref["DSWRFsfc"][:, 0] - ref["USWRFsfc"][:, 0] + ref["DLWRFsfc"][:, 0] - ref["ULWRFsfc"][:, 0]) + (-ref["LHTFLsfc"][:, 0] - ref["SHTFLsfc"][:, 0])
    want = ic["sst"][:, 0] + (f_net + forcing["qflux"][:, 1]) / (1000.0 * forcing["mld"][:, 1] * 4000.0) * 21600.0
    ocean_cells = torch.round(forcing["frac"][:, 1]) == 1
    assert rel_max(ref["sst"][:, 0][ocean_cells], want[ocean_cells]) <= 1e-6


@pytest.mark.parametrize("graph", [None, "step", "window"])
def test_rollout_engine_matches_stepper(dev, graph):
    """hipGraph rollout with static buffers vs the dict-of-tensors Stepper loop (which normalises with torch
    elementwise kernels: its fp32 division may differ from the engine's correctly rounded one by an ulp) and vs
    the CPU oracle loop."""
    from oracle import stepper as ostep
    from oracle.sfno import SFNOConfig, SFNOOracle
    import ace_amd
    from ace_amd.rollout import RolloutEngine
    from ace_amd.step import NormalizationConfig
    in_names = ["f0", "p0", "p1", "f1"]
    out_names = ["p1", "d0", "p0"]
    names = sorted(set(in_names + out_names))
    config = ace_amd.SingleModuleStepConfig(
        builder=ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet",
                                       config={"embed_dim": 16, "num_layers": 2, "operator_type": "dhconv"}),
        in_names=in_names, out_names=out_names, next_step_forcing_names=["f1"],
        normalization=NormalizationConfig(means={k: 0.1 * (i + 1) for i, k in enumerate(names)},
                                          stds={k: 1.0 + 0.1 * i for i, k in enumerate(names)}),
    )
    torch.manual_seed(0)
    stepper = ace_amd.Stepper.from_config(config, ace_amd.DatasetInfo((12, 24)), device=dev)
    stepper.set_eval()
    B, T = 2, 5
    ic = {k: torch.randn(B, 1, 12, 24, device=dev) for k in ["p0", "p1"]}
    forcing = {k: torch.randn(B, T + 1, 12, 24, device=dev) for k in ["f0", "f1"]}
    ref, ref_state = stepper.predict(ic, forcing)
    eng = RolloutEngine(stepper, batch=B, n_forward_steps=T, graph=graph)
    out, state = eng.predict(ic, forcing)
    out2, _ = eng.predict(ic, forcing)   # replay is deterministic
    torch.cuda.synchronize()
    cfg = SFNOConfig(in_chans=4, out_chans=3, img_shape=(12, 24), embed_dim=16, num_layers=2, operator_type="dhconv")
    net = SFNOOracle(cfg, stepper.modules[0].state_dict(), dtype=torch.float64)
    means = {k: torch.tensor(0.1 * (i + 1), dtype=torch.float64) for i, k in enumerate(names)}
    stds = {k: torch.tensor(1.0 + 0.1 * i, dtype=torch.float64) for i, k in enumerate(names)}
    oref = ostep.predict(net, {k: v.cpu().double() for k, v in ic.items()}, {k: v.cpu().double() for k, v in forcing.items()},
                         T, in_names, out_names, means, stds, next_step_forcing_names=["f1"])
    for k in out_names:
        assert rel_max(out[k], ref[k]) <= 2e-6, k
        assert rel_max(out[k], torch.stack([o[k] for o in oref], 1)) <= NET_TOL, k   # 5 free-running steps
        assert torch.equal(out[k], out2[k])
    for k in ["p0", "p1"]:
        assert rel_max(state[k], ref_state[k]) <= 2e-6


def test_s80_state_at_180x360_matches_the_oracle_stepper(dev):
    """SURVEY 8(d) "S80" on the device at the FULL 1-degree grid and embed width: 80 distinct variables, 8 forcing-only + 36
    prognostic in = 44 channels, 36 prognostic + 36 diagnostic out = 72 (the headline state is ACE2's 44 / 50), mu = 0.1 /
    sigma = 1.1 for every name (test_single_module.py:2331-2333), embed 384 on the weight-stationary kernels, 2 layers so that the
    fp32 CPU oracle (the reference's torch-CPU op sequence) finishes in seconds.  Two free-running steps of the per-step-hipGraph
    engine against the oracle's stepper loop: every one of the 72 output fields within 1e-5 of its own maximum per step."""
    from oracle import stepper as ostep
    from oracle.sfno import SFNOConfig, SFNOOracle
    import ace_amd
    from ace_amd.rollout import RolloutEngine
    from ace_amd.step import NormalizationConfig
    H, W, T = 180, 360, 2
    forcing_names = [f"forcing_{i}" for i in range(8)]
    prog = [f"prog_{i}" for i in range(36)]
    diag = [f"diag_{i}" for i in range(36)]
    in_names, out_names = forcing_names + prog, prog + diag
    names = forcing_names + prog + diag
    assert len(set(names)) == 80 and len(in_names) == 44 and len(out_names) == 72
    config = ace_amd.SingleModuleStepConfig(
        builder=ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet",
                                       config={"embed_dim": 384, "num_layers": 2, "operator_type": "dhconv", "scale_factor": 1}),
        in_names=in_names, out_names=out_names,
        normalization=NormalizationConfig(means={k: 0.1 for k in names}, stds={k: 1.1 for k in names}))
    torch.manual_seed(0)
    stepper = ace_amd.Stepper.from_config(config, ace_amd.DatasetInfo((H, W)), device=dev)
    stepper.set_eval()
    g = torch.Generator().manual_seed(1)
    ic = {k: torch.randn(1, 1, H, W, generator=g) * 1.1 + 0.1 for k in prog}
    forcing = {k: torch.randn(1, T + 1, H, W, generator=g) * 1.1 + 0.1 for k in forcing_names}
    eng = RolloutEngine(stepper, batch=1, n_forward_steps=T, graph="step")
    out, state = eng.predict({k: v.to(dev) for k, v in ic.items()}, {k: v.to(dev) for k, v in forcing.items()})
    torch.cuda.synchronize()
    assert set(out) == set(out_names)
    cfg = SFNOConfig(in_chans=44, out_chans=72, img_shape=(H, W), embed_dim=384, num_layers=2, operator_type="dhconv")
    net = SFNOOracle(cfg, {k: v.detach().cpu() for k, v in stepper.modules[0].state_dict().items()}, dtype=torch.float32)
    means, stds = {k: torch.tensor(0.1) for k in names}, {k: torch.tensor(1.1) for k in names}
    oref = ostep.predict(net, ic, forcing, T, in_names, out_names, means, stds)
    worst = 0.0
    for s in range(T):
        for k in out_names:
            want = oref[s][k]
            err = float((out[k][:, s].cpu() - want).abs().max() / want.abs().max())
            worst = max(worst, err / (s + 1))
            assert err <= NET_TOL * (s + 1), (k, s, err)
    print(f"S80 at 180x360: worst per-field error / step {worst:.2e}")


@pytest.mark.parametrize("case,engine", [("ace2_like", "stepper"), ("ace2_like", None), ("ace2_like", "step"),
                                         ("ace2_like", "window"), ("ace2_like_override", "window"),
                                         ("residual_prescribed", "stepper"), ("residual_prescribed", None),
                                         ("residual_prescribed", "step"), ("residual_prescribed", "window"),
                                         ("ace2_like_override", "stepper"), ("ace2_like_override", "step")])
def test_reference_checkpoint_rollout_matches_reference_stepper(dev, precision, case, engine):
    """End-to-end drop-in check against the REAL reference stepper (tests/golden/gen_checkpoint.pt, emitted by
    fme.ace.stepper.Stepper on CPU): load its get_state() with ace_amd.load_stepper, roll 3 steps with the ACE2-style
    corrector (dry air, moisture and energy budgets, positivity), the prescribed-SST ocean and a next-step forcing,
    and compare every output of every step with the reference's own predict_generator.  Tolerance: 1e-5 of the
    field's maximum per step (north_star), 3e-5 by step 3 (the error of step s is carried through s more networks),
    or - for an ill-conditioned field - 3x the distance of the reference's own fp32 result from exact arithmetic
    (conditioning_floor: from step 2 on the advective moisture tendency is a residual of nearly cancelling terms and
    the reference's fp32 value is itself 3e-4 / 8e-4 of the field maximum away from the fp64 evaluation).
    Second case: residual_prediction with a prescribed prognostic (equiangular grid, no big skip / position embedding).
    Third case: the first checkpoint loaded with StepperOverrideConfig(ocean=None, prescribed_prognostic_names=[SST]).
    engine: "stepper" = the dict-of-tensors Stepper.predict, otherwise the static-buffer RolloutEngine's graph mode."""
    import ace_amd
    from ace_amd.rollout import RolloutEngine
    g = checkpoint_case(load_golden("gen_checkpoint.pt"), case)
    loaded = ace_amd.load_stepper(g["state"], override_config=checkpoint_override(g), device=dev)
    assert loaded.ignored == []
    stepper = loaded.stepper
    stepper._step_obj.module.torch_module.set_precision(precision)
    ic = {k: v.to(dev) for k, v in g["ic"].items()}
    forcing = {k: v.to(dev) for k, v in g["forcing"].items()}
    T = len(g["steps"])
    if engine == "stepper":
        out, state = stepper.predict(ic, forcing)
    else:
        out, state = RolloutEngine(stepper, batch=2, n_forward_steps=T, graph=engine).predict(ic, forcing)
    torch.cuda.synchronize()
    assert set(out) == set(g["steps"][0])
    if case in ("residual_prescribed", "ace2_like_override"):
        assert torch.equal(out["surface_temperature"], forcing["surface_temperature"][:, 1:])
    floor = conditioning_floor(g)
    worst = []
    for s, want_all in enumerate(g["steps"]):
        for k, want in want_all.items():
            got = out[k][:, s].cpu()
            err = float((got - want).abs().max()) / float(want.abs().max())
            tol = max(NET_TOL * (s + 1), 3.0 * floor[s][k])
            worst.append((err / tol, err, tol, k, s))
    worst.sort(reverse=True)
    print("worst (err/tol, err, tol, field, step):", worst[:3])
    assert worst[0][0] <= 1.0, worst[:5]
    for k, v in state.items():
        assert torch.equal(v[:, 0], out[k][:, -1])


@pytest.mark.parametrize("engine", ["stepper", None, "step", "window"])
@pytest.mark.parametrize("case", ["isotropic", "gaussian_groups2"])
def test_seeded_stochastic_rollout_matches_reference_stepper(dev, precision, case, engine):
    """The reference's RNG contract (fme/core/rand.py:39-104, fme/ace/stepper/single_module.py:1063-1068):
    a NoiseConditionedSFNO stepper rolled 3 steps from ``StepperState(random_state=RandomState.from_seed(seed))`` reproduces the
    REAL reference stepper's seeded rollout (tests/golden/gen_rng.pt: isotropic noise through the inverse SHT, and gaussian noise
    with a grouped filter) - the draw comes from the rollout's CPU generator whatever the device's global RNG holds, through
    Stepper.predict and through the static-buffer RolloutEngine (eager / per-step hipGraph / the whole window captured, its
    conditioning fields drawn in front of the replay into a static buffer).  Bar: 1e-5 of the field maximum
    per step (carried through s + 1 networks), per channel."""
    import ace_amd
    from ace_amd.rand import RandomState
    from ace_amd.rollout import RolloutEngine
    from ace_amd.step import StepperState
    from ace_amd.stepper import PrognosticState
    g = load_golden("gen_rng.pt")[case]
    stepper = ace_amd.load_stepper(g["state"], device=dev).stepper
    stepper._step_obj.module.torch_module.set_precision(precision)
    T = len(g["steps"])
    forcing = {k: v.to(dev) for k, v in g["forcing"].items()}

    def run():
        ic = PrognosticState({k: v.to(dev) for k, v in g["ic"].items()})
        ic.stepper_state = StepperState(random_state=RandomState.from_seed(g["seed"]))
        torch.manual_seed(int(torch.randint(0, 1 << 30, (1,))))          # the global RNGs (host and device) must not matter
        if engine == "stepper":
            return stepper.predict(ic, forcing)
        return RolloutEngine(stepper, batch=2, n_forward_steps=T, graph=engine).predict(ic, forcing)

    out, state = run()
    out = {k: v.clone() for k, v in out.items()}
    torch.cuda.synchronize()
    for s, want_all in enumerate(g["steps"]):
        for k, want in want_all.items():
            err = float((out[k][:, s].cpu() - want).abs().max() / want.abs().max())
            assert err <= NET_TOL * (s + 1), (case, engine, s, k, err)
    rs = state.stepper_state.random_state
    assert torch.equal(rs.generator.get_state(), g["generator_state_after"])     # consumed exactly what the reference consumed
    again, _ = run()
    for k in out:
        assert torch.equal(out[k], again[k]), k                                   # a seeded rollout is reproducible to the bit
    with torch.no_grad():      # without a random state: the device's RNG, a different rollout every time
        a, _ = stepper.predict({k: v.to(dev) for k, v in g["ic"].items()}, forcing)
    assert not torch.equal(a["p0"], out["p0"])


@pytest.mark.parametrize("how", ["stepper", "engine"])
def test_windowed_inference_matches_reference_continuous_rollout(dev, how, tmp_path):
    """run_inference over forcing windows of 2 + 1 steps (ace_amd/inference.py: window feeder with the one-ahead upload,
    Looper, restart dump) == the REAL reference stepper's continuous 3-step rollout of tests/golden/gen_checkpoint.pt: the
    dry-air reference mass of the corrector has to ride on the prognostic state from window to window, as the reference's
    stepper_state does (fme/ace/data_loading/batch_data.py:214-235)."""
    import ace_amd
    from ace_amd.inference import EnginePredict, ForcingWindows, InferenceData, TensorFileWriter, run_inference
    g = load_golden("gen_checkpoint.pt")["ace2_like"]
    stepper = ace_amd.load_stepper(g["state"], device=dev).stepper
    ic = {k: v.to(dev) for k, v in g["ic"].items()}
    T = len(g["steps"])
    loader = ForcingWindows(g["forcing"], total_forward_steps=T, forward_steps_in_memory=2, device=dev)
    assert len(loader) == 2
    predict = stepper.predict if how == "stepper" else EnginePredict(stepper, batch=2, graph="step")
    writer = TensorFileWriter(str(tmp_path))
    state = run_inference(predict, InferenceData(ic, loader), writer=writer)
    torch.cuda.synchronize()
    series = torch.load(tmp_path / "autoregressive_predictions.pt", weights_only=True)
    floor = conditioning_floor(g)
    for s, want_all in enumerate(g["steps"]):
        for k, want in want_all.items():
            err = float((series[k][:, s] - want).abs().max()) / float(want.abs().max())
            assert err <= max(NET_TOL * (s + 1), 3.0 * floor[s][k]), (k, s, err)
    restart = torch.load(tmp_path / "restart.pt", weights_only=True)
    assert set(restart) == set(stepper.prognostic_names)
    for k, v in restart.items():
        assert torch.equal(v, series[k][:, -1:]) and torch.equal(v, state[k].cpu())
    # the dry-air reference seeded by the first window is still the one on the final state (carried, not re-seeded)
    cs = state.stepper_state.corrector_state
    assert cs is not None and cs.global_dry_air_mass is not None
    first = run_inference(predict, InferenceData(ic, ForcingWindows(g["forcing"], 1, 1, device=dev)))
    assert torch.equal(cs.global_dry_air_mass, first.stepper_state.corrector_state.global_dry_air_mass)


# ---- fused post-step physics (csrc/physics.hip) against the reference corrector's own vectors ----------------------------
def _physics_case(dev, g, corr_cfg, ocean=None, prescribed=()):
    """Static buffers laid out as the RolloutEngine lays them out (two steps) + a FusedPhysics over them."""
    import datetime

    import ace_amd
    from ace_amd.corrector import AtmosphereCorrectorConfig
    from ace_amd.physics import FusedPhysics
    info = ace_amd.DatasetInfo((8, 16), timestep=datetime.timedelta(seconds=g["timestep_seconds"]), lat=g["lat"], lon=g["lon"],
                               ak=g["ak"], bk=g["bk"])
    corrector = AtmosphereCorrectorConfig.from_state(corr_cfg).get_corrector(info) if corr_cfg is not None else None
    prog = sorted(g["gen0"])
    B, T, H, W = 2, 2, 8, 16
    HW = H * W
    out = {n: torch.zeros(B, T, H, W, device=dev) for n in prog}
    ic = {n: g["input0"][n].reshape(B, 1, H, W).to(dev).contiguous() for n in prog}
    forcing = {n: torch.stack([g["forcing"][n]] * (T + 1), dim=1).to(dev).contiguous() for n in g["forcing"]}

    def locate_gen(name, s):
        return (out[name].data_ptr() + 4 * s * HW, T * HW) if name in out else None

    def locate_in(name, s):
        if name in ic:
            return (ic[name].data_ptr(), HW) if s == 0 else (out[name].data_ptr() + 4 * (s - 1) * HW, T * HW)
        return (forcing[name].data_ptr() + 4 * s * HW, (T + 1) * HW) if name in forcing else None

    def locate_next(name, s):
        return (forcing[name].data_ptr() + 4 * (s + 1) * HW, (T + 1) * HW) if name in forcing else None

    phys = FusedPhysics(corrector, ocean, list(prescribed), B, (H, W), T, gen_names=prog, in_names=prog + list(forcing),
                        next_names=list(forcing), locate_gen=locate_gen, locate_in=locate_in, locate_next=locate_next, device=dev)
    return phys, out, (ic, forcing)


@pytest.mark.parametrize("name", ["force_positive", "dry_air", "zero_advection", "moisture_precipitation", "moisture_evaporation",
                                  "moisture_advection_and_precipitation", "moisture_advection_and_evaporation", "energy", "ace2_like"])
def test_fused_physics_vs_reference_corrector(dev, name):
    """The four physics kernels on the golden vectors the REFERENCE corrector emitted (tests/golden/make_golden_corrector.py):
    every option of AtmosphereCorrectorConfig (fme/core/corrector/atmosphere.py:223-398), two consecutive steps (the dry-air
    reference mass is seeded on the first, carried to the second).  fp32 per-column arithmetic in the reference's operation
    order, fp64 global sums: each field within 2e-6 of its maximum (the torch restatement is held to 1e-6 on the CPU)."""
    from ace_amd import _lib
    from test_corrector_cpu import CONFIGS
    g = load_golden("gen_corrector.pt")
    phys, out, keep = _physics_case(dev, g, CONFIGS[name])
    exp = g["expected"][name]
    st = _lib.current_stream()
    phys.reset(st)
    for s, gen in enumerate((g["gen0"], g["gen1"])):
        for n, v in gen.items():
            out[n][:, s].copy_(v.to(dev))
        phys.apply(s, st)
        torch.cuda.synchronize()
        for k, want in exp[f"step{s}"].items():
            got = out[k][:, s].cpu()
            scale = float(want.abs().max()) or 1.0
            assert float((got - want).abs().max()) / scale <= 2e-6, (name, s, k, float((got - want).abs().max()) / scale)
        for k, v in gen.items():          # fields the reference leaves alone are untouched, bit for bit
            if k not in exp[f"step{s}"]:
                assert torch.equal(out[k][:, s].cpu(), v), (name, s, k)
    mass = phys.get_reference(st)
    if exp["global_dry_air_mass"] is None:
        assert mass is None
    else:
        torch.testing.assert_close(mass.cpu().reshape(-1), exp["global_dry_air_mass"].reshape(-1), rtol=1e-6, atol=0.0)
    # determinism: the same two steps again give the same bits
    first = {k: v.clone() for k, v in out.items()}
    phys.reset(st)
    for s, gen in enumerate((g["gen0"], g["gen1"])):
        for n, v in gen.items():
            out[n][:, s].copy_(v.to(dev))
        phys.apply(s, st)
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], first[k]) for k in out)


@pytest.mark.parametrize("interpolate", [False, True])
def test_fused_physics_ocean_and_prescribed(dev, interpolate):
    """prescribed SST (fme/core/ocean.py:167-215; half-to-even rounding of the mask) and prescribed prognostics
    (single_module.py:700-716) in the fused kernel: bitwise against the reference's vectors."""
    from ace_amd import _lib
    from ace_amd.ocean import OceanConfig
    from ace_amd.physics import FusedPhysics
    o = load_golden("gen_corrector.pt")["ocean"]
    ocean = OceanConfig(surface_temperature_name="sst", ocean_fraction_name="frac", interpolate=interpolate).build(
        ["sst", "frac", "q"], ["sst", "q"])
    B, H, W = o["gen"]["sst"].shape
    HW = H * W
    out = {k: v.reshape(B, 1, H, W).to(dev).contiguous().clone() for k, v in o["gen"].items()}
    nxt = {k: torch.stack([v, v], dim=1).to(dev).contiguous() for k, v in o["target"].items()}
    nxt["q"] = torch.stack([o["gen"]["q"] - 2.0, o["gen"]["q"] + 1.0], dim=1).to(dev).contiguous()   # a prescribed prognostic: step s + 1's data
    phys = FusedPhysics(None, ocean, ["q"], B, (H, W), 1, gen_names=list(out), in_names=list(out),
                        next_names=list(nxt), locate_gen=lambda n, s: (out[n].data_ptr(), HW) if n in out else None,
                        locate_in=lambda n, s: None,
                        locate_next=lambda n, s: (nxt[n].data_ptr() + 4 * HW, 2 * HW) if n in nxt else None, device=dev)
    phys.apply(0, _lib.current_stream())
    torch.cuda.synchronize()
    assert torch.equal(out["sst"][:, 0].cpu(), o["expected"][interpolate]["sst"])
    assert torch.equal(out["q"][:, 0].cpu(), o["gen"]["q"] + 1.0)


# ---- HEALPix variant (csrc/healpix.hip, ace_amd/healpix.py) ---------------------------------------------------------------
def test_healpix_padding_kernel_vs_reference(dev):
    """ace_hpx_pad on the device against the reference's HEALPixPadding outputs (bitwise), reading a source with a row pitch
    larger than the face and writing into a channel window of a wider padded tensor (how concatenations are formed)."""
    import numpy as np
    from ace_amd import _lib
    L = _lib.lib()
    gold = load_golden("gen_healpix.pt")
    for (nside, p), d in gold["padding"].items():
        m = nside + 2 * p
        ia = np.zeros(12 * m * m, dtype=np.int32)
        ib = np.zeros_like(ia)
        assert L.ace_hpx_pad_table_host(nside, p, ia.ctypes.data, ib.ctypes.data) == 0
        iad, ibd = torch.from_numpy(ia).to(dev), torch.from_numpy(ib).to(dev)
        pitch = nside + 3
        src = torch.full((24, 3, nside, pitch), float("nan"), device=dev)
        src[..., :nside] = d["x"].to(dev)
        mp = (m + 3) // 4 * 4 + 4                      # a pitch wider than the padded face: gap columns must come out zero
        flat = torch.full((24 * 5 * m * mp + 16,), -7.0, device=dev)
        y = flat[: 24 * 5 * m * mp].view(24, 5, m, mp)
        amax = torch.zeros(64, dtype=torch.int32, device=dev)
        assert L.ace_hpx_pad(src.data_ptr(), src.stride(0), src.stride(1), pitch, flat.data_ptr(), 5, 1, 3, iad.data_ptr(), ibd.data_ptr(),
                             2, nside, p, mp, amax.data_ptr(), _lib.current_stream()) == 0, L.ace_hpx_last_error()
        torch.cuda.synchronize()
        assert torch.equal(y[:, 1:4, :, :m].cpu(), d["padded"]), (nside, p)
        assert bool((y[:, 1:4, :, m:] == 0).all())
        assert bool((y[:, 0] == -7.0).all()) and bool((y[:, 4] == -7.0).all())
        assert bool((flat[-16:] == -7.0).all())        # the slack is zeroed only by the call that writes the last channels
        assert float(amax.view(torch.float32).max()) == float(d["padded"].abs().max())
        assert L.ace_hpx_pad(src.data_ptr(), src.stride(0), src.stride(1), pitch, flat.data_ptr(), 5, 2, 3, iad.data_ptr(), ibd.data_ptr(),
                             2, nside, p, mp, None, _lib.current_stream()) == 0, L.ace_hpx_last_error()
        torch.cuda.synchronize()
        assert bool((flat[-16:] == 0).all())


@pytest.mark.parametrize("name", ["convnext_avgpool_tconv", "basic_maxpool"])
def test_healpix_unet_vs_reference(dev, name):
    """The HEALPix UNet through the registry (ModuleSelector type "HEALPixUNet") with the REFERENCE's weights against the
    reference's own output (tests/golden/make_golden_healpix.py): ConvNeXt blocks with capped GELU, dilated 3 x 3 convolutions
    on padded faces (dilations 1 / 2 / 4), average / max pooling, transposed-convolution upsampling, skip concatenations.
    Compensated-fp16 MFMA arithmetic (fp32-class, as the SFNO path): 1e-5 of the output's maximum."""
    import ace_amd
    g = load_golden("gen_healpix.pt")["unet"][name]
    case = g["case"]
    mod = ace_amd.ModuleSelector(type="HEALPixUNet", config=case["config"]).build(case["n_in"], case["n_out"],
                                                                                 ace_amd.DatasetInfo((case["nside"], case["nside"])))
    net = mod.torch_module.to(dev)
    net.load_state_dict(g["state_dict"], strict=True)
    with torch.no_grad():
        y = net(g["x"].to(dev))
        y2 = net(g["x"].to(dev))
    assert y.shape == g["y"].shape
    assert torch.equal(y, y2)
    assert_net_close(y, g["y"], NET_TOL)


def test_healpix_isolatitude_padding_and_unet_vs_reference(dev):
    """hpx_padding_mode="isolatitude" (healpix_paddings.py:613-1140): the same gather kernel with the table
    ace_amd.healpix.isolatitude_pad_table builds - padded faces against the reference's HEALPixPaddingIsolatitude, and a UNet
    built with that padding (nside per level) against the reference's output (tests/golden/gen_healpix_isolatitude.pt)."""
    import ace_amd
    from ace_amd import _lib
    from ace_amd.healpix import isolatitude_pad_table
    L = _lib.lib()
    gold = load_golden("gen_healpix_isolatitude.pt")
    for (nside, p), d in gold["padding"].items():
        m = nside + 2 * p
        mp = (m + 3) // 4 * 4
        ia, ib = isolatitude_pad_table(nside, p)
        iad, ibd = torch.from_numpy(ia).to(dev), torch.from_numpy(ib).to(dev)
        src = d["x"].to(dev).contiguous()
        flat = torch.zeros(24 * 3 * m * mp + 16, device=dev)
        assert L.ace_hpx_pad(src.data_ptr(), src.stride(0), src.stride(1), nside, flat.data_ptr(), 3, 0, 3, iad.data_ptr(), ibd.data_ptr(),
                             2, nside, p, mp, None, _lib.current_stream()) == 0, L.ace_hpx_last_error()
        torch.cuda.synchronize()
        y = flat[: 24 * 3 * m * mp].view(24, 3, m, mp)[..., :m]
        assert float((y.cpu() - d["padded"]).abs().max()) <= 2.5e-7, (nside, p)
    g = gold["unet"]["isolatitude"]
    case = g["case"]
    net = ace_amd.ModuleSelector(type="HEALPixUNet", config=case["config"]).build(
        case["n_in"], case["n_out"], ace_amd.DatasetInfo((case["nside"], case["nside"]))).torch_module.to(dev)
    net.load_state_dict(g["state_dict"], strict=True)
    with torch.no_grad():
        out = net(g["x"].to(dev))
    assert_net_close(out, g["y"], NET_TOL)


def test_healpix_interpolate_upsample_unet_vs_reference(dev):
    """the "Interpolate" upsampling block (nn.Upsample(scale_factor=2, mode="nearest"), healpix_blocks.py:229-253) on ace_hpx_upsample2
    (round 5: a transposed convolution with identity taps), in a ConvNeXt UNet with max pooling, against the reference's output"""
    import ace_amd
    g = load_golden("gen_healpix_isolatitude.pt")["unet"]["interpolate_upsample"]
    case = g["case"]
    net = ace_amd.ModuleSelector(type="HEALPixUNet", config=case["config"]).build(
        case["n_in"], case["n_out"], ace_amd.DatasetInfo((case["nside"], case["nside"]))).torch_module.to(dev)
    assert list(net.state_dict()) == list(g["state_dict"])
    net.load_state_dict(g["state_dict"], strict=True)
    with torch.no_grad():
        y = net(g["x"].to(dev))
    assert_net_close(y, g["y"], NET_TOL)
    dec = dict(case["config"]["decoder"])
    dec["up_sampling_block"] = {"block_type": "Interpolate", "upsample_mode": "bilinear"}       # built since round 6 (ace_hpx_upsample2)
    bil = ace_amd.ModuleSelector(type="HEALPixUNet", config={**case["config"], "decoder": dec}).build(
        case["n_in"], case["n_out"], ace_amd.DatasetInfo((case["nside"], case["nside"]))).torch_module.to(dev)
    bil.load_state_dict(g["state_dict"], strict=True)
    with torch.no_grad():
        yb = bil(g["x"].to(dev))
    assert yb.shape == y.shape and bool(torch.isfinite(yb).all()) and not torch.equal(yb, y)
    with pytest.raises(NotImplementedError):
        dec["up_sampling_block"] = {"block_type": "Interpolate", "upsample_mode": "bicubic"}
        ace_amd.ModuleSelector(type="HEALPixUNet", config={**case["config"], "decoder": dec}).build(3, 2, ace_amd.DatasetInfo((8, 8)))


def test_healpix_symmetric_convnext_unet_vs_reference(dev):
    """SymmetricConvNeXtBlock (encoder) and Multi_SymmetricConvNeXtBlock (decoder, two blocks per level, concatenated skip inputs):
    skip(x) + act(conv(...)) with the residual added after the last activation - here by an identity contraction that carries the
    residual - against the reference's output."""
    import ace_amd
    g = load_golden("gen_healpix_isolatitude.pt")["unet"]["symmetric"]
    case = g["case"]
    net = ace_amd.ModuleSelector(type="HEALPixUNet", config=case["config"]).build(
        case["n_in"], case["n_out"], ace_amd.DatasetInfo((case["nside"], case["nside"]))).torch_module.to(dev)
    net.load_state_dict(g["state_dict"], strict=True)
    with torch.no_grad():
        y = net(g["x"].to(dev))
        assert torch.equal(y, net(g["x"].to(dev)))
    assert_net_close(y, g["y"], NET_TOL)


@pytest.mark.parametrize("nside,cin,cin2,cout,k,dil,act,cap", [(8, 12, 0, 24, 3, 1, 1, 10.0), (8, 5, 6, 136, 3, 2, 1, 0.7), (16, 16, 0, 20, 3, 4, 0, float("inf")),
                                                              (8, 9, 0, 7, 3, 1, 2, 2.0), (8, 24, 8, 544, 3, 1, 1, 10.0)])
def test_healpix_packed_operators_vs_torch(dev, nside, cin, cin2, cout, k, dil, act, cap):
    """ace_hpx_pad_planes + ace_hpx_conv_packed (+ ace_hpx_conv1_packed on the planes it writes) against torch in fp64 on the
    reference-padded tensor: channel counts that are not multiples of 8, two sources (the skip concatenation), dilations 1 / 2 / 4,
    capped GELU / ReLU / no activation, cout below and above the 128-row tile rule; and equal to rounding to ace_hpx_pad + ace_hpx_conv."""
    import numpy as np
    from ace_amd import _lib
    L = _lib.lib()
    st = _lib.current_stream()
    g = torch.Generator().manual_seed(nside + cin + cout)
    p = (k - 1) * dil // 2
    m = nside + 2 * p
    mp = (m + 3) // 4 * 4
    imgs = 12
    x = torch.randn(imgs, cin, nside, nside, generator=g) * 2.0
    x2 = torch.randn(imgs, cin2, nside, nside, generator=g) * 0.5 if cin2 else None
    w = torch.randn(cout, cin + cin2, k, k, generator=g) / (3.0 * (cin + cin2)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    ia, ib = np.zeros(12 * m * m, dtype=np.int32), np.zeros(12 * m * m, dtype=np.int32)
    assert L.ace_hpx_pad_table_host(nside, p, ia.ctypes.data, ib.ctypes.data) == 0
    iad, ibd = torch.from_numpy(ia).to(dev), torch.from_numpy(ib).to(dev)

    def host_pad(t):          # the same gather on the host, in fp64
        a = torch.from_numpy(ia).long().view(12, m, m)
        bb = torch.from_numpy(ib).long().view(12, m, m)
        td = t.double().view(1, 12, t.shape[1], nside, nside)
        ga = td[0, a >> 24, :, (a >> 12) & 4095, a & 4095]
        gb = td[0, bb >> 24, :, (bb >> 12) & 4095, bb & 4095]
        return (0.5 * ga + 0.5 * gb).permute(0, 3, 1, 2)        # [12][c][m][m]  (a == b: 0.5 a + 0.5 a = a exactly)

    xs = [t for t in (x, x2) if t is not None]
    padded = torch.cat([host_pad(t) for t in xs], dim=1)
    ref = torch.nn.functional.conv2d(padded, w.double(), b.double(), dilation=dil)
    # the arithmetic's error scales with the contraction's magnitude; a low cap shrinks max|ref| (the norm's denominator) below it
    tol = OP_TOL * max(1.0, float(ref.abs().max()) / min(cap, float(ref.abs().max())))
    if act == 1:
        ref = torch.nn.functional.gelu(ref)
    elif act == 2:
        ref = torch.relu(ref)
    ref = torch.clamp(ref, max=cap)

    def slot_of(t):
        s_ = torch.zeros(64, dtype=torch.int32, device=dev)
        assert L.ace_hpx_absmax(t.data_ptr(), t.numel(), s_.data_ptr(), st) == 0
        return s_

    xd, x2d = x.to(dev).contiguous(), (x2.to(dev).contiguous() if x2 is not None else None)
    sx, sx2 = slot_of(xd), (slot_of(x2d) if x2d is not None else None)
    ctot = cin + cin2
    cpad = (ctot + 7) // 8 * 8
    planes = torch.full((2, imgs * cpad * m * mp + 16 * 8), float("nan"), dtype=torch.float16, device=dev)
    pmax = torch.zeros(64, dtype=torch.int32, device=dev)
    assert L.ace_hpx_pad_planes(xd.data_ptr(), xd.stride(0), xd.stride(1), nside, x2d.data_ptr() if x2d is not None else None,
                                x2d.stride(0) if x2d is not None else 0, x2d.stride(1) if x2d is not None else 0, nside if x2d is not None else 0,
                                cin, cin2, planes[0].data_ptr(), planes[1].data_ptr(), iad.data_ptr(), ibd.data_ptr(), 1, nside, p, mp,
                                sx.data_ptr(), sx2.data_ptr() if sx2 is not None else None, pmax.data_ptr(), st) == 0, L.ace_hpx_last_error()
    assert bool(torch.isfinite(planes.float()).all())
    wp = torch.zeros(cout, k * k, cpad)
    wp[:, :, :ctot] = w.permute(0, 2, 3, 1).reshape(cout, k * k, ctot)
    wp = wp.reshape(cout, k * k * cpad).contiguous().to(dev)
    hw = ctypes.c_void_p()
    assert L.ace_hpx_weight_create(wp.data_ptr(), cout, k * k * cpad, st, ctypes.byref(hw)) == 0
    bd = b.to(dev)
    y = torch.empty(imgs, cout, nside, mp, device=dev)
    ymax = torch.zeros(64, dtype=torch.int32, device=dev)
    null = ctypes.c_void_p(0)
    assert L.ace_hpx_conv_packed(planes[0].data_ptr(), planes[1].data_ptr(), cpad, 0, hw, bd.data_ptr(), 0.0, y.data_ptr(), null, null, 0, imgs, cout,
                                 nside, nside, mp, k, dil, act, cap, pmax.data_ptr(), ymax.data_ptr(), st) == 0, L.ace_hpx_last_error()
    torch.cuda.synchronize()
    assert rel_max(y[..., :nside], ref) <= tol, rel_max(y[..., :nside], ref)
    assert abs(float(ymax.view(torch.float32).max()) - float(y.abs().max())) == 0.0
    if cout % 8 == 0:          # the same result handed to a 1 x 1 convolution as planes (with a residual)
        c3 = 10
        w3 = torch.randn(c3, cout, generator=g) / cout ** 0.5
        b3 = torch.randn(c3, generator=g) * 0.1
        r3 = torch.randn(imgs, c3, nside, mp, generator=g)
        oplanes = torch.empty(2, imgs * cout * nside * mp, dtype=torch.float16, device=dev)
        oslot = torch.zeros(64, dtype=torch.int32, device=dev)
        assert L.ace_hpx_conv_packed(planes[0].data_ptr(), planes[1].data_ptr(), cpad, 0, hw, bd.data_ptr(), float(b.abs().max()), null,
                                     oplanes[0].data_ptr(), oplanes[1].data_ptr(), 0, imgs, cout, nside, nside, mp, k, dil, act, cap, pmax.data_ptr(),
                                     oslot.data_ptr(), st) == 0, L.ace_hpx_last_error()
        assert float(oslot.view(torch.float32).max()) >= float(ref.abs().max()) * (1.0 - 1e-6)   # a bound (fp32), not the maximum
        h3 = ctypes.c_void_p()
        w3d = w3.to(dev).contiguous()
        assert L.ace_hpx_weight_create(w3d.data_ptr(), c3, cout, st, ctypes.byref(h3)) == 0
        y3 = torch.empty(imgs, c3, nside, mp, device=dev)
        y3max = torch.zeros(64, dtype=torch.int32, device=dev)
        r3d, b3d = r3.to(dev), b3.to(dev)
        assert L.ace_hpx_conv1_packed(oplanes[0].data_ptr(), oplanes[1].data_ptr(), cout, h3, b3d.data_ptr(), r3d.data_ptr(), y3.data_ptr(), imgs, c3,
                                      nside, nside, mp, 0, oslot.data_ptr(), y3max.data_ptr(), st) == 0, L.ace_hpx_last_error()
        torch.cuda.synchronize()
        ref3 = torch.einsum("oc,nchw->nohw", w3.double(), ref) + b3.double().view(1, c3, 1, 1) + r3.double()[..., :nside]
        assert rel_max(y3[..., :nside], ref3) <= tol, rel_max(y3[..., :nside], ref3)
        L.ace_hpx_weight_destroy(h3)
        # ... and written into the interior of the padded planes of a second (k, dil) convolution, halo gathered in place
        c2 = 9
        w2 = torch.randn(c2, cout, k, k, generator=g) / (3.0 * cout) ** 0.5
        pp2 = torch.full((2, imgs * cout * m * mp + 16 * 8), float("nan"), dtype=torch.float16, device=dev)
        slot2 = torch.zeros(64, dtype=torch.int32, device=dev)
        yo = (p * mp + p) * 16
        assert L.ace_hpx_conv_packed(planes[0].data_ptr(), planes[1].data_ptr(), cpad, 0, hw, bd.data_ptr(), float(b.abs().max()), null,
                                     pp2[0].data_ptr() + yo, pp2[1].data_ptr() + yo, m * mp, imgs, cout, nside, nside, mp, k, dil, act, cap,
                                     pmax.data_ptr(), slot2.data_ptr(), st) == 0, L.ace_hpx_last_error()
        assert L.ace_hpx_halo_planes(pp2[0].data_ptr(), pp2[1].data_ptr(), cout, iad.data_ptr(), ibd.data_ptr(), 1, nside, p, mp, st) == 0, L.ace_hpx_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(pp2.float()).all())                  # every cell defined: interior, halo, gap columns, slack
        w2p = w2.permute(0, 2, 3, 1).reshape(c2, k * k * cout).contiguous().to(dev)
        h2 = ctypes.c_void_p()
        assert L.ace_hpx_weight_create(w2p.data_ptr(), c2, k * k * cout, st, ctypes.byref(h2)) == 0
        y2 = torch.empty(imgs, c2, nside, mp, device=dev)
        y2max = torch.zeros(64, dtype=torch.int32, device=dev)
        assert L.ace_hpx_conv_packed(pp2[0].data_ptr(), pp2[1].data_ptr(), cout, 0, h2, null, 0.0, y2.data_ptr(), null, null, 0, imgs, c2, nside, nside,
                                     mp, k, dil, 0, float("inf"), slot2.data_ptr(), y2max.data_ptr(), st) == 0, L.ace_hpx_last_error()
        torch.cuda.synchronize()
        ref2 = torch.nn.functional.conv2d(host_pad(ref), w2.double(), None, dilation=dil)
        assert rel_max(y2[..., :nside], ref2) <= tol, rel_max(y2[..., :nside], ref2)
        L.ace_hpx_weight_destroy(h2)
    # a 1 x 1 convolution (the ConvNeXt skip branch) on the INTERIOR of the same padded planes
    c1 = 11
    w1 = torch.randn(c1, ctot, generator=g) / ctot ** 0.5
    w1p = torch.zeros(c1, cpad)
    w1p[:, :ctot] = w1
    w1p = w1p.contiguous().to(dev)
    h1 = ctypes.c_void_p()
    assert L.ace_hpx_weight_create(w1p.data_ptr(), c1, cpad, st, ctypes.byref(h1)) == 0
    y1 = torch.empty(imgs, c1, nside, mp, device=dev)
    y1max = torch.zeros(64, dtype=torch.int32, device=dev)
    xo = (p * mp + p) * 16
    assert L.ace_hpx_conv_packed(planes[0].data_ptr() + xo, planes[1].data_ptr() + xo, cpad, m * mp, h1, null, 0.0, y1.data_ptr(), null, null, 0, imgs,
                                 c1, nside, nside, mp, 1, 1, 0, float("inf"), pmax.data_ptr(), y1max.data_ptr(), st) == 0, L.ace_hpx_last_error()
    torch.cuda.synchronize()
    ref1 = torch.einsum("oc,nchw->nohw", w1.double(), torch.cat([t.double() for t in xs], dim=1))
    assert rel_max(y1[..., :nside], ref1) <= OP_TOL, rel_max(y1[..., :nside], ref1)
    L.ace_hpx_weight_destroy(h1)
    L.ace_hpx_weight_destroy(hw)


def test_healpix_forward_captured_in_a_graph(dev):
    """ace_amd.CapturedHEALPixForward: the whole forward replayed from a hipGraph (no Python between the launches) gives the eager
    forward's bits on the captured input and on fresh inputs, and stays within the bar of the reference's output."""
    import ace_amd
    g = load_golden("gen_healpix.pt")["unet"]["convnext_avgpool_tconv"]
    case = g["case"]
    net = ace_amd.ModuleSelector(type="HEALPixUNet", config=case["config"]).build(
        case["n_in"], case["n_out"], ace_amd.DatasetInfo((case["nside"], case["nside"]))).torch_module.to(dev)
    net.load_state_dict(g["state_dict"], strict=True)
    x = g["x"].to(dev)
    cap = ace_amd.CapturedHEALPixForward(net, x)
    with torch.no_grad():
        y = cap(x).clone()
        assert torch.equal(y, net(x))
        assert_net_close(y, g["y"], NET_TOL)
        x2 = torch.randn_like(x) * 2.0 + 0.5                  # another range: the bound slots are recomputed inside the graph
        assert torch.equal(cap(x2), net(x2))
        assert torch.equal(cap(x), y)
    with pytest.raises(ValueError, match="captured for inputs of shape"):
        cap(x[:, :, :1])


def test_healpix_weight_update_is_seen(dev):
    """The prepared (fp16 hi / lo) copy of a convolution weight is re-made when the parameter changes in place: doubling the
    output layer's weight and bias (a 1 x 1 convolution without activation) doubles the output."""
    import ace_amd
    g = load_golden("gen_healpix.pt")["unet"]["convnext_avgpool_tconv"]
    case = g["case"]
    net = ace_amd.ModuleSelector(type="HEALPixUNet", config=case["config"]).build(
        case["n_in"], case["n_out"], ace_amd.DatasetInfo((case["nside"], case["nside"]))).torch_module.to(dev)
    net.load_state_dict(g["state_dict"], strict=True)
    x = g["x"].to(dev)
    with torch.no_grad():
        y0 = net(x)
        out_conv = [m for m in net.decoder.output_layer.modules() if isinstance(m, torch.nn.Conv2d)]
        assert len(out_conv) == 1 and out_conv[0].kernel_size == (1, 1)
        out_conv[0].weight.mul_(2.0)
        if out_conv[0].bias is not None:
            out_conv[0].bias.mul_(2.0)
        y1 = net(x)
    assert rel_max(y1, 2.0 * y0) <= 1e-6
    assert_net_close(y0, g["y"], NET_TOL)


def test_healpix_stepper_rollout(dev):
    """configs[4]: the HEALPix variant behind the SAME stepper API - SingleModuleStepConfig with builder type "HEALPixUNet", data
    laid out [sample, face = 12, nside, nside] per variable (the packer stacks channels at dim -3, fme/core/packer.py:45-52) - a
    3-step rollout through Stepper.predict equals the hand-written loop normalise -> network -> denormalise -> feed back."""
    import ace_amd
    from ace_amd.step import NormalizationConfig
    g = load_golden("gen_healpix.pt")["unet"]["basic_maxpool"]
    case = g["case"]
    in_names, out_names = ["f0", "p0", "p1"], ["p0", "p1"]
    names = sorted(set(in_names + out_names))
    cfg = ace_amd.SingleModuleStepConfig(
        builder=ace_amd.ModuleSelector(type="HEALPixUNet", config=case["config"]), in_names=in_names, out_names=out_names,
        normalization=NormalizationConfig(means={k: 0.1 * (i + 1) for i, k in enumerate(names)},
                                          stds={k: 1.0 + 0.2 * i for i, k in enumerate(names)}))
    torch.manual_seed(0)
    ns = case["nside"]
    stepper = ace_amd.Stepper.from_config(cfg, ace_amd.DatasetInfo((ns, ns)), device=dev)
    stepper.set_eval()
    B, T = 2, 3
    gen = torch.Generator().manual_seed(5)
    ic = {k: torch.randn(B, 1, 12, ns, ns, generator=gen).to(dev) for k in ["p0", "p1"]}
    forcing = {"f0": torch.randn(B, T + 1, 12, ns, ns, generator=gen).to(dev)}
    out, _ = stepper.predict(ic, forcing)
    net = stepper.modules[0]
    norm = stepper._step_obj.normalizer
    state = {k: v[:, 0] for k, v in ic.items()}
    with torch.no_grad():
        for s in range(T):
            x = torch.stack([(forcing["f0"][:, s] if n == "f0" else state[n]) for n in in_names], dim=-3)
            mean = torch.tensor([float(norm.means[n]) for n in in_names], device=dev).reshape(-1, 1, 1)
            std = torch.tensor([float(norm.stds[n]) for n in in_names], device=dev).reshape(-1, 1, 1)
            y = net((x - mean) / std)
            for j, n in enumerate(out_names):
                state[n] = y[:, :, j] * float(norm.stds[n]) + float(norm.means[n])
                assert rel_max(out[n][:, s], state[n]) <= 2e-6, (s, n)
    assert all(out[n].shape == (B, T, 12, ns, ns) for n in out_names)


def test_async_ensemble_mean_side_stream_on_the_device(dev):
    """ace_amd/distributed.py AsyncEnsembleMean on CUDA tensors (one process: the all-reduce itself is the identity, the stream and
    event choreography is what runs): fields produced on the step stream are stacked and reduced on the side stream after an event,
    the step stream keeps running, result() synchronises on the reduction only, last_allreduce_ms() times it."""
    from ace_amd.distributed import AsyncEnsembleMean, Distributed
    Distributed.reset()
    d = Distributed.get_instance()
    ens = AsyncEnsembleMean((5, 18, 36), dev, d)
    g = torch.Generator().manual_seed(2)
    base = torch.randn(5, 18, 36, generator=g).to(dev)
    fields = [(base[i] * 2.0 + 1.0) for i in range(5)]          # produced by kernels on the current (step) stream
    ens.submit(fields)
    busy = torch.randn(2048, 2048, device=dev) @ torch.randn(2048, 2048, device=dev)   # the step stream goes on meanwhile
    out = ens.result()
    assert torch.equal(out, torch.stack(fields))
    ms = ens.last_allreduce_ms()
    assert ms is not None and ms >= 0.0
    ens.submit(3.0 * base)                                       # a tensor of the buffer's shape
    ens.wait()                                                   # the CURRENT stream waits (no host synchronisation)
    assert torch.equal(ens.buf.clone(), 3.0 * base)
    assert bool(torch.isfinite(busy).all())
    Distributed.reset()
