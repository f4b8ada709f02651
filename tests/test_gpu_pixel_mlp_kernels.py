"""``ace_pixel_mlp_*`` (csrc/pixel_mlp.hip) through the C ABI, bit for bit against the header's statement in numpy
(tests/_pixel_mlp_ref.py): NaN compared by position, signs of zero included.  Shapes are the smallest at which the kernel can go
wrong: widths that are no multiple of the 16-wide tile, both kernels (narrow: every width <= 64, 64 pixels per wave; wide: up to
256, 16 pixels per wave) in both forms (weights in LDS; a blob over 64 KB streamed from global memory), pixel counts around the
tile and the wave, the 16-byte and the 4-byte access branch, and one size per kernel at which a workgroup runs its unit loop twice (computed from the header's constants)."""
import ctypes

import numpy as np
import pytest
import torch

import _pixel_mlp_ref as R
from ace_amd import _lib

pytestmark = pytest.mark.gpu

K = R.constants()


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
    t.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    return t


class Handle:
    def __init__(self, dev, dims, ws, bs, acts, embed_layer):
        n = len(ws)
        self.keep = [_dev(w, dev) for w in ws] + [_dev(b, dev) for b in bs if b is not None]
        wp = [t.data_ptr() for t in self.keep[:n]]
        it = iter(self.keep[n:])
        bp = [next(it).data_ptr() if b is not None else None for b in bs]
        self.h = ctypes.c_void_p()
        rc = _lib.lib().ace_pixel_mlp_create(n, (ctypes.c_int * (n + 1))(*dims), (ctypes.c_void_p * n)(*wp), (ctypes.c_void_p * n)(*bp),
                                            (ctypes.c_int * n)(*acts), embed_layer, _lib.current_stream(), ctypes.byref(self.h))
        assert rc == 0, _lib.lib().ace_pixel_mlp_last_error()
        self.dims = dims

    def forward(self, x, embed, y, B, hw):
        return _lib.lib().ace_pixel_mlp_forward(self.h, x.data_ptr(), embed.data_ptr() if embed is not None else None, y.data_ptr(),
                                                B, hw, _lib.current_stream())

    def close(self):
        _lib.lib().ace_pixel_mlp_destroy(self.h)


def _net(dims, seed, bias=True, embed=False, hw=1, acts=None):
    rng = np.random.default_rng(seed)
    n = len(dims) - 1
    ws = [rng.standard_normal((dims[l + 1], dims[l])).astype(np.float32) for l in range(n)]
    bs = [rng.standard_normal(dims[l + 1]).astype(np.float32) if bias and not (bias == "some" and l % 2) else None for l in range(n)]
    acts = acts if acts is not None else [1] * (n - 1) + [0]
    e = rng.standard_normal((dims[1], hw)).astype(np.float32) if embed else None
    return ws, bs, acts, e


def _run(dev, dims, ws, bs, acts, e, x, off=(0, 0, 0)):
    """The kernel on x [B][dims[0]][hw]; returns the output as numpy."""
    B, _, hw = x.shape
    h = Handle(dev, dims, ws, bs, acts, 0 if e is not None else -1)
    try:
        xd = _dev(x, dev, off[0])
        ed = _dev(e, dev, off[1]) if e is not None else None
        yd = _dev(np.full((B, dims[-1], hw), 7.5, np.float32), dev, off[2])
        assert h.forward(xd, ed, yd, B, hw) == 0, _lib.lib().ace_pixel_mlp_last_error()
        torch.cuda.synchronize()
        return yd.cpu().numpy().reshape(B, dims[-1], hw)
    finally:
        h.close()


def _same(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    bad = got.view(np.int32)[ok] != want.view(np.int32)[ok]
    assert not bad.any(), (int(bad.sum()), got[ok][bad][:4], want[ok][bad][:4])


def _check(dev, dims, B, hw, seed=0, bias=True, embed=False, off=(0, 0, 0)):
    ws, bs, acts, e = _net(dims, seed, bias, embed, hw)
    x = np.random.default_rng(seed + 1).standard_normal((B, dims[0], hw)).astype(np.float32)
    got = _run(dev, dims, ws, bs, acts, e, x, off)
    _same(got, R.pixel_mlp(x, ws, bs, acts, 0 if embed else -1, e))
    return got


DIMS = [[1, 1, 1], [5, 20, 7, 3], [17, 16, 16], [3, 33, 65, 16, 5, 2], [30, 64, 64, 10], [4, 256, 4], [3, 2], [70, 5]]


@pytest.mark.parametrize("embed", [False, True])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "-".join(map(str, d)))
def test_dims(dev, dims, embed):
    _check(dev, dims, B=2, hw=135, seed=len(dims) + dims[0], embed=embed)


def _blob_bytes(dims):
    """the header's blob size of a chain"""
    t = lambda n: -(-n // K["TILE"])      # noqa: E731
    return 4 * sum(t(o) * K["TILE"] + t(o) * t(k) * 256 for k, o in zip(dims[:-1], dims[1:]))


def test_every_other_case_keeps_its_weights_in_lds():
    assert all(_blob_bytes(d) <= K["LDS_BYTES"] for d in DIMS)


@pytest.mark.parametrize("hw", [192, 135], ids=["hw192_16B", "hw135_4B"])
@pytest.mark.parametrize("embed", [False, True])
@pytest.mark.parametrize("dims", [[30] + [64] * 7 + [10], [4, 256, 256, 4]], ids=["narrow", "wide"])
def test_weights_streamed_from_global_memory(dev, dims, embed, hw):
    """a blob over ACE_PIXEL_MLP_LDS_BYTES is not copied into LDS: both kernels' streamed form, at an aligned and an unaligned hw"""
    assert _blob_bytes(dims) > K["LDS_BYTES"] and len(dims) - 1 <= K["MAX_LAYERS"] and max(dims) <= K["MAX_WIDTH"]
    _check(dev, dims, B=2, hw=hw, seed=21, embed=embed)


@pytest.mark.parametrize("bias", [False, "some"])
@pytest.mark.parametrize("dims", [[5, 20, 7, 3], [4, 80, 3]], ids=["narrow", "wide"])
def test_null_bias(dev, dims, bias):
    _check(dev, dims, B=1, hw=65, seed=3, bias=bias, embed=True)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [1, 15, 16, 17, 63, 64, 65, 135, 2145])
@pytest.mark.parametrize("dims", [[5, 20, 7, 3], [3, 65, 2]], ids=["narrow", "wide"])
def test_sizes(dev, dims, hw, B):
    _check(dev, dims, B=B, hw=hw, seed=hw, embed=True)


@pytest.mark.parametrize("dims,tiles", [([1, 1, 1], K["NARROW_TILES"]), ([2, 65, 1], K["WIDE_TILES"])], ids=["narrow", "wide"])
def test_a_workgroup_loops_over_its_units(dev, dims, tiles):
    """more (sample, run of pixels) units than MAX_GRID * WAVES: every workgroup takes a second unit, some a tail"""
    assert max(dims) <= K["NARROW_WIDTH"] if tiles == K["NARROW_TILES"] else max(dims) > K["NARROW_WIDTH"]
    per_unit = tiles * K["TILE"]
    B = 3
    hw = per_unit * (K["MAX_GRID"] * K["WAVES"] // B + 19) + 5
    assert B * -(-hw // per_unit) > K["MAX_GRID"] * K["WAVES"]
    _check(dev, dims, B=B, hw=hw, seed=8, embed=True)


@pytest.mark.parametrize("dims", [[5, 20, 7, 3], [3, 65, 2]], ids=["narrow", "wide"])
def test_alignment(dev, dims):
    """hw % 4 == 0: the 16-byte branch when x, embed and y are aligned; each of them one float off takes the 4-byte branch; all
    agree with the statement, hence with one another"""
    outs = [_check(dev, dims, B=2, hw=192, seed=5, embed=True, off=off) for off in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]]
    for o in outs[1:]:
        _same(o, outs[0])
    _check(dev, dims, B=2, hw=196, seed=5, embed=True)      # the 16-byte branch with a partial last unit


@pytest.mark.parametrize("dims", [[17, 33, 5], [30, 64, 64, 10], [20, 80, 6]], ids=lambda d: "-".join(map(str, d)))
def test_exact_integers(dev, dims):
    """small asymmetric integer weights and integer inputs: every partial sum is an integer below 2^24, so the result equals the
    int64 product exactly whatever the summation order - what is left to go wrong is the fragment layout"""
    n = len(dims) - 1
    ws = [np.fromfunction(lambda o, k: (3 * o + 5 * k + l) % 7 - 3, (dims[l + 1], dims[l])).astype(np.float32) for l in range(n)]
    bs = [(np.arange(dims[l + 1]) % 5 - 2).astype(np.float32) for l in range(n)]
    hw, B = 70, 2
    x = np.fromfunction(lambda b, c, p: (7 * p + 3 * c + b) % 5 - 2, (B, dims[0], hw)).astype(np.float32)
    e = np.fromfunction(lambda c, p: (c + 2 * p) % 3 - 1, (dims[1], hw)).astype(np.float32)
    a = x.astype(np.int64)
    for l in range(n):
        a = np.einsum("ok,bkp->bop", ws[l].astype(np.int64), a) + bs[l].astype(np.int64)[None, :, None]
        if l < n - 1:
            a = np.maximum(a, 0)
        if l == 0:
            a = a + e.astype(np.int64)[None]
        assert np.abs(a).max() < 2 ** 24
    got = _run(dev, dims, ws, bs, [1] * (n - 1) + [0], e, x)
    assert np.array_equal(got.astype(np.int64), a) and np.array_equal(got, a.astype(np.float32))


@pytest.mark.parametrize("dims", [[5, 20, 7, 3], [5, 70, 3]], ids=["narrow", "wide"])
def test_special_values_stay_in_their_pixels(dev, dims):
    hw, B = 40, 1
    ws, bs, acts, e = _net(dims, 11, True, True, hw)
    ws[0][0] = np.abs(ws[0][0])                     # row 0 of layer 0: positive weights and a -0 bias, so that an all -0 pixel
    bs[0][0] = np.float32(-0.0)                     # keeps acc = -0 through the sum, the channel padding and the relu
    e[0, 5] = np.float32(-0.0)
    x = np.random.default_rng(12).standard_normal((B, dims[0], hw)).astype(np.float32)
    base = _run(dev, dims, ws, bs, acts, e, x)
    x2 = x.copy()
    x2[0, :, 3] = np.nan
    x2[0, 2, 4] = np.inf
    x2[0, :, 5] = -0.0
    x2[0, 1, 6] = np.float32(1e-42)
    x2[0, :, 7] = np.float32(2.0 ** -140)
    touched = [3, 4, 5, 6, 7]
    got = _run(dev, dims, ws, bs, acts, e, x2)
    want = R.pixel_mlp(x2, ws, bs, acts, 0, e)
    _same(got, want)
    assert np.isnan(want[0, :, 3]).all() and not np.isfinite(want[0, :, 4]).all()
    keep = [p for p in range(hw) if p not in touched]
    _same(got[:, :, keep], base[:, :, keep])
    assert not np.isnan(got[:, :, keep]).any()
    # the hidden -0 of the all -0 pixel reaches the output only through products; the one-layer chain shows the sign itself
    ws1, bs1 = [ws[0]], [bs[0]]
    got1 = _run(dev, dims[:2], ws1, bs1, [1], e, x2)
    _same(got1, R.pixel_mlp(x2, ws1, bs1, [1], 0, e))
    assert got1[0, 0, 5] == 0 and np.signbit(got1[0, 0, 5])


def test_determinism_and_capture(dev):
    dims, B, hw = [30, 64, 64, 10], 1, 2145
    ws, bs, acts, e = _net(dims, 13, True, True, hw)
    x = np.random.default_rng(14).standard_normal((B, dims[0], hw)).astype(np.float32)
    h = Handle(dev, dims, ws, bs, acts, 0)
    try:
        xd, ed = _dev(x, dev), _dev(e, dev)
        y1, y2, y3 = (_dev(np.zeros((B, dims[-1], hw), np.float32), dev) for _ in range(3))
        assert h.forward(xd, ed, y1, B, hw) == 0 and h.forward(xd, ed, y2, B, hw) == 0
        torch.cuda.synchronize()
        assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))
        g = torch.cuda.CUDAGraph()
        with _lib.capture_without_gc(), torch.cuda.graph(g):
            assert h.forward(xd, ed, y3, B, hw) == 0
        y3.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y1.view(torch.int32), y3.view(torch.int32))
        _same(y1.cpu().numpy().reshape(B, dims[-1], hw), R.pixel_mlp(x, ws, bs, acts, 0, e))
    finally:
        h.close()


def test_bad_arguments_launch_nothing(dev):
    L = _lib.lib()
    dims, hw = [5, 20, 3], 33
    ws, bs, acts, e = _net(dims, 15, True, True, hw)
    h = Handle(dev, dims, ws, bs, acts, 0)
    try:
        xd, ed = _dev(np.ones((1, 5, hw), np.float32), dev), _dev(e, dev)
        yd = _dev(np.full((1, 3, hw), 7.5, np.float32), dev)
        st = _lib.current_stream()
        assert L.ace_pixel_mlp_forward(None, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), 1, hw, st) == _lib.ACE_ERR_INVALID
        assert b"null handle" in L.ace_pixel_mlp_last_error()
        assert L.ace_pixel_mlp_forward(h.h, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), 1, 0, st) == _lib.ACE_ERR_INVALID
        assert b"hw >= 1" in L.ace_pixel_mlp_last_error()
        assert L.ace_pixel_mlp_forward(h.h, xd.data_ptr(), None, yd.data_ptr(), 1, hw, st) == _lib.ACE_ERR_INVALID
        assert b"embed must not be NULL" in L.ace_pixel_mlp_last_error()
        assert L.ace_pixel_mlp_forward(h.h, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), 0, hw, st) == _lib.ACE_ERR_INVALID
        assert L.ace_pixel_mlp_forward(h.h, None, ed.data_ptr(), yd.data_ptr(), 1, hw, st) == _lib.ACE_ERR_INVALID
        torch.cuda.synchronize()
        assert bool((yd == 7.5).all())              # nothing was launched
    finally:
        h.close()
    # create
    out = ctypes.c_void_p()
    wd = _dev(ws[0], dev)
    one = lambda n, d, w, a, emb: L.ace_pixel_mlp_create(n, (ctypes.c_int * len(d))(*d), (ctypes.c_void_p * len(w))(*w), None,       # noqa: E731
                                                         (ctypes.c_int * len(a))(*a), emb, _lib.current_stream(), ctypes.byref(out))
    p = wd.data_ptr()
    assert one(0, [5], [p], [0], -1) == _lib.ACE_ERR_INVALID
    assert one(K["MAX_LAYERS"] + 1, [2] * (K["MAX_LAYERS"] + 2), [p] * (K["MAX_LAYERS"] + 1), [0] * (K["MAX_LAYERS"] + 1), -1) == _lib.ACE_ERR_INVALID
    assert one(1, [5, K["MAX_WIDTH"] + 1], [p], [0], -1) == _lib.ACE_ERR_INVALID
    assert b"ACE_PIXEL_MLP_MAX_WIDTH" in L.ace_pixel_mlp_last_error()
    assert one(1, [0, 20], [p], [0], -1) == _lib.ACE_ERR_INVALID
    assert one(1, [5, 20], [None], [0], -1) == _lib.ACE_ERR_INVALID
    assert one(1, [5, 20], [p], [2], -1) == _lib.ACE_ERR_INVALID
    assert one(1, [5, 20], [p], [0], 1) == _lib.ACE_ERR_INVALID
    assert out.value is None
    assert one(1, [5, 20], [p], [1], 0) == 0 and out.value        # a one-layer chain with an embedding, no bias array at all
    L.ace_pixel_mlp_destroy(out)
    L.ace_pixel_mlp_destroy(None)
