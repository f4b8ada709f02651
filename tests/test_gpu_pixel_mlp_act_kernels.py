"""What ``ace_pixel_mlp_*`` (csrc/pixel_mlp.hip) learned for AnkurLocalNet, through the C ABI: ``ace_pixel_mlp_create2`` with the
embedding in front of the activation, bit for bit against the extended statement (tests/_pixel_mlp_ref2.py); single-layer GELU and
SiLU handles against the fp64 activation of the statement's bit-exact accumulator, allowed 2 x the largest error of torch's CPU
fp32 F.gelu / F.silu on the same fp32 values; ``ace_pixel_mlp_create`` and ``create2(..., 0)`` byte for byte on a LandNet golden.
Widths 5, 24, 64, 65 and 256: below a tile, no multiple of it, the narrow kernel's limit, the first wide width, the widest.

Measured on an MI355X (largest absolute error, kernel / torch, widths 5, 24, 64, 65, 256): GELU 3.4e-7 / 9.7e-7, 4.1e-7 / 8.8e-7,
4.4e-7 / 1.1e-6, 4.3e-7 / 1.1e-6, 4.5e-7 / 1.1e-6; SiLU equal to torch's at every width (1.0e-6, 6.6e-7, 9.7e-7, 1.0e-6, 1.1e-6)."""
import ctypes

import numpy as np
import pytest
import torch

import _disco_ref as D
import _pixel_mlp_ref2 as P
from ace_amd import _lib

pytestmark = pytest.mark.gpu
WIDTHS = [5, 24, 64, 65, 256]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _dev(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(dev).contiguous()


def _run(dev, dims, ws, bs, acts, embed_layer, e, x, first, old_entry=False):
    n = len(ws)
    keep_w = [_dev(w, dev) for w in ws]
    keep_b = [_dev(b, dev) if b is not None else None for b in bs]
    h = ctypes.c_void_p()
    L = _lib.lib()
    args = [n, (ctypes.c_int * (n + 1))(*dims), (ctypes.c_void_p * n)(*[t.data_ptr() for t in keep_w]),
            (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in keep_b]), (ctypes.c_int * n)(*acts), embed_layer]
    if old_entry:
        rc = L.ace_pixel_mlp_create(*args, _lib.current_stream(), ctypes.byref(h))
    else:
        rc = L.ace_pixel_mlp_create2(*args, int(first), _lib.current_stream(), ctypes.byref(h))
    assert rc == 0, L.ace_pixel_mlp_last_error()
    try:
        B, _, hw = x.shape
        xd, ed = _dev(x, dev), _dev(e, dev) if e is not None else None
        yd = torch.full((B, dims[-1], hw), 7.5, dtype=torch.float32, device=dev)
        rc = L.ace_pixel_mlp_forward(h, xd.data_ptr(), ed.data_ptr() if ed is not None else None, yd.data_ptr(), B, hw, _lib.current_stream())
        assert rc == 0, L.ace_pixel_mlp_last_error()
        torch.cuda.synchronize()
        return yd.cpu().numpy()
    finally:
        L.ace_pixel_mlp_destroy(h)


def _same(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    bad = got.view(np.int32)[ok] != want.view(np.int32)[ok]
    assert not bad.any(), (int(bad.sum()), got[ok][bad][:4], want[ok][bad][:4])


def _net(dims, seed, hw):
    rng = np.random.default_rng(seed)
    n = len(dims) - 1
    ws = [(rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32) for l in range(n)]
    bs = [rng.standard_normal(dims[l + 1]).astype(np.float32) for l in range(n)]
    e = rng.standard_normal((dims[1], hw)).astype(np.float32)
    x = rng.standard_normal((2, dims[0], hw)).astype(np.float32)
    return ws, bs, e, x


@pytest.mark.parametrize("width", WIDTHS)
def test_embedding_before_the_activation_bit_for_bit(dev, width):
    """7 -> width -> width -> 3 with ReLU, the embedding in front of layer 0's ReLU; hw = 135 (no multiple of 4 or of a tile); one
    NaN in the input"""
    dims, hw = [7, width, width, 3], 135
    ws, bs, e, x = _net(dims, width, hw)
    x[1, 2, 77] = np.nan
    got = _run(dev, dims, ws, bs, [1, 1, 0], 0, e, x, first=True)
    _same(got, P.pixel_mlp2(x, ws, bs, [1, 1, 0], 0, e, embed_before_act=True))
    after = _run(dev, dims, ws, bs, [1, 1, 0], 0, e, x, first=False)
    _same(after, P.pixel_mlp2(x, ws, bs, [1, 1, 0], 0, e, embed_before_act=False))
    assert not np.array_equal(got[0], after[0])


@pytest.mark.parametrize("name", ["gelu", "silu"])
@pytest.mark.parametrize("width", WIDTHS)
def test_single_layer_soft_activation_against_fp64(dev, width, name):
    act = {"gelu": P.ACT_GELU, "silu": P.ACT_SILU}[name]
    dims, hw = [width, width], 135
    ws, bs, e, x = _net(dims, 10 + width, hw)
    x *= np.float32(3.0)                                   # accumulators of a few units: both tails and the bend of the curves
    pre = P.pixel_mlp2(x, ws, bs, [act], 0, e, embed_before_act=True, pre_activation=True)
    got = _run(dev, dims, ws, bs, [act], 0, e, x, first=True)
    truth = (D.gelu64 if name == "gelu" else D.silu64)(pre)
    fn = torch.nn.functional.gelu if name == "gelu" else torch.nn.functional.silu
    yard = float(np.abs(fn(torch.from_numpy(pre)).numpy().astype(np.float64) - truth).max())
    err = float(np.abs(got.astype(np.float64) - truth).max())
    print(f"{name} width {width}: kernel {err:.3e} torch-cpu-fp32 {yard:.3e}")
    assert err <= 2 * yard
    x[0, 0, 5] = np.nan                                    # NaN stays NaN
    got = _run(dev, dims, ws, bs, [act], 0, e, x, first=True)
    assert np.isnan(got[0, :, 5]).all() and np.isnan(got).sum() == width


def test_create_and_create2_with_zero_give_identical_bytes(dev):
    import _landnet_cases as LC
    c = LC.case("small_embed")
    sd, x = c["state_dict"], c["input"]
    B, C, H, W = x.shape
    n = len([k for k in sd if k.endswith(".weight")])
    ws = [sd[f"model.{l}.layers.0.weight"].numpy().reshape(sd[f"model.{l}.layers.0.weight"].shape[:2]) for l in range(n)]
    bs = [sd[f"model.{l}.layers.0.bias"].numpy() for l in range(n)]
    dims = [C] + [w.shape[0] for w in ws]
    e = sd["pos_embed.pos_embed"].numpy().reshape(-1, H * W)
    xs = x.numpy().reshape(B, C, H * W)
    acts = [1] * (n - 1) + [0]
    a = _run(dev, dims, ws, bs, acts, 0, e, xs, first=False, old_entry=True)
    b = _run(dev, dims, ws, bs, acts, 0, e, xs, first=False)
    assert a.tobytes() == b.tobytes()
    _same(a.reshape(B, -1, H, W), c["statement"].numpy())


def test_create2_refusals(dev):
    L = _lib.lib()
    w = torch.zeros(4, 4, device=dev)
    h = ctypes.c_void_p()
    mk = lambda act, first: L.ace_pixel_mlp_create2(1, (ctypes.c_int * 2)(4, 4), (ctypes.c_void_p * 1)(w.data_ptr()),      # noqa: E731
                                                    (ctypes.c_void_p * 1)(None), (ctypes.c_int * 1)(act), 0, first,
                                                    _lib.current_stream(), ctypes.byref(h))
    assert mk(4, 0) == _lib.ACE_ERR_INVALID and b"ACE_PIXEL_MLP_ACT_" in L.ace_pixel_mlp_last_error()
    old = L.ace_pixel_mlp_create(1, (ctypes.c_int * 2)(4, 4), (ctypes.c_void_p * 1)(w.data_ptr()), (ctypes.c_void_p * 1)(None),
                                 (ctypes.c_int * 1)(2), -1, _lib.current_stream(), ctypes.byref(h))
    assert old == _lib.ACE_ERR_INVALID                       # GELU through the entry that never had it: refused as before
    assert mk(1, 2) == _lib.ACE_ERR_INVALID and b"embed_before_act" in L.ace_pixel_mlp_last_error()
    assert not h.value
