"""TEST INFRASTRUCTURE: an emulation of ``ace_pixel_mlp_*`` and of the glue a LandNet stepper's engine calls
(``ace_mask_pack_normalize``, ``ace_unpack_denormalize``, ``ace_mask_planes``; include/ace_sfno.h) on host memory - the forward is
the header's statement (tests/_pixel_mlp_ref.py), pack / unpack / masking walk the same pointer tables and strides - so that the
HOST logic of ace_amd/landnet.py (parameter order, handle life, one launch per call) and of ace_amd/land_rollout.py (static
buffers, step tables, masking order) runs in the ``-m "not gpu"`` suite.  Not a fallback: nothing in the product imports it and the
product's own entry points still refuse host tensors; the GPU tests run the real kernels.  Use: ``with fake_landnet() as fake:``."""
import contextlib
import ctypes

import numpy as np

import _pixel_mlp_ref as ref


def _view(ptr, n, ctype):
    return np.ctypeslib.as_array((ctype * int(n)).from_address(int(ptr)))


def _f32(ptr, n):
    return _view(ptr, n, ctypes.c_float)


def _val(p):
    return getattr(p, "value", p)


class FakeLandnet:
    ACE_OK, ACE_ERR_INVALID, ACE_ERR_RUNTIME = 0, -1, -2

    def __init__(self, real):
        self._real = real
        self._handles = {}
        self._next = 1
        self.calls = []          # entry points in call order
        self.created = 0
        self.destroyed = 0
        self.error = b""

    # -- what the product reads from the _lib module
    def lib(self):
        return self

    def check(self, rc):
        if rc != 0:
            raise (ValueError if rc == self.ACE_ERR_INVALID else RuntimeError)(f"emulated C ABI returned {rc}")

    @staticmethod
    def current_stream():
        return None

    @staticmethod
    @contextlib.contextmanager
    def capture_without_gc():
        yield

    # -- ace_pixel_mlp_*
    def ace_pixel_mlp_last_error(self):
        return self.error

    def ace_pixel_mlp_create(self, n_layers, dims, w_dev, bias_dev, act, embed_layer, stream, out):
        dims = list(dims)
        ws, bs = [], []
        for l in range(n_layers):
            O, K = dims[l + 1], dims[l]
            ws.append(_f32(w_dev[l], O * K).copy().reshape(O, K))
            bs.append(_f32(bias_dev[l], O).copy() if bias_dev[l] else None)
        self._handles[self._next] = (dims, ws, bs, list(act), embed_layer)
        out._obj.value = self._next
        self._next += 1
        self.created += 1
        self.calls.append("pixel_mlp_create")
        return 0

    def ace_pixel_mlp_destroy(self, h):
        if self._handles.pop(_val(h), None) is not None:
            self.destroyed += 1

    def ace_pixel_mlp_forward(self, h, x, embed, y, batch, hw, stream):
        self.calls.append("pixel_mlp_forward")
        if not _val(h) or batch < 1 or hw < 1:
            self.error = b"(emulated ace_pixel_mlp) bad argument"
            return self.ACE_ERR_INVALID
        dims, ws, bs, act, embed_layer = self._handles[_val(h)]
        if embed_layer >= 0 and not embed:
            self.error = b"(emulated ace_pixel_mlp) embed must not be NULL"
            return self.ACE_ERR_INVALID
        xin = _f32(x, batch * dims[0] * hw).reshape(batch, dims[0], hw)
        e = _f32(embed, dims[embed_layer + 1] * hw).reshape(-1, hw) if embed_layer >= 0 else None
        _f32(y, batch * dims[-1] * hw).reshape(batch, dims[-1], hw)[...] = ref.pixel_mlp(xin, ws, bs, act, embed_layer, e)
        return 0

    # -- the engine's glue (csrc/masking.hip, csrc/kernels.hip)
    def _planes(self, ptrs, strides, n, batch, hw):
        p, s = _view(ptrs, n, ctypes.c_int64), _view(strides, n, ctypes.c_int64)
        return [None if not int(p[j]) else np.lib.stride_tricks.as_strided(
            _f32(int(p[j]), (batch - 1) * int(s[j]) + hw), (batch, hw), (4 * int(s[j]), 4)) for j in range(n)]

    def _masked(self, src, j, mask_idx, hits, nmask, fill, hw):
        idx = _view(mask_idx, j + 1, ctypes.c_int32)[j]
        if not hits or idx < 0 or idx >= nmask:
            return src
        hit = _view(hits, nmask * hw, ctypes.c_uint8).reshape(nmask, hw)[idx] != 0
        return np.where(hit[None], np.float32(_f32(fill, j + 1)[j]), src)

    def ace_mask_pack_normalize(self, srcs, src_strides, mask_idx, hits, nmask, fill, stage, stage_strides, mean, std, dst, npack,
                                nplanes, batch, hw, stream):
        self.calls.append("mask_pack_normalize")
        assert not stage and npack == nplanes
        out = _f32(dst, batch * npack * hw).reshape(batch, npack, hw)
        m, d = _f32(mean, npack), _f32(std, npack)
        for j, src in enumerate(self._planes(srcs, src_strides, nplanes, batch, hw)):
            v = self._masked(src, j, mask_idx, hits, nmask, fill, hw)
            with np.errstate(all="ignore"):
                out[:, j] = (v - m[j]) / d[j]
        return 0

    def ace_unpack_denormalize(self, src, mean, std, dsts, strides, batch, nch, hw, stream):
        self.calls.append("unpack_denormalize")
        m, d = _f32(mean, nch), _f32(std, nch)
        x = _f32(src, batch * nch * hw).reshape(batch, nch, hw)
        for c, dst in enumerate(self._planes(dsts, strides, nch, batch, hw)):
            with np.errstate(all="ignore"):
                dst[...] = x[:, c] * d[c] + m[c]
        return 0

    def ace_mask_planes(self, srcs, src_strides, dsts, dst_strides, mask_idx, hits, nmask, fill, nplanes, batch, hw, stream):
        self.calls.append("mask_planes")
        src = self._planes(srcs, src_strides, nplanes, batch, hw)
        for j, dst in enumerate(self._planes(dsts, dst_strides, nplanes, batch, hw)):
            dst[...] = self._masked(src[j], j, mask_idx, hits, nmask, fill, hw)
        return 0


@contextlib.contextmanager
def fake_landnet():
    """ace_amd.{landnet, land_rollout, rollout} bound to the emulation; LandNet.forward without its "must be on the GPU" guard."""
    import ace_amd.land_rollout as E
    import ace_amd.landnet as N
    import ace_amd.rollout as R
    from ace_amd import _lib as real
    fake = FakeLandnet(real)
    saved = (N._lib, E._lib, R._lib, N.LandNet.forward, E._on_gpu)
    N._lib = E._lib = R._lib = fake
    N.LandNet.forward = N.LandNet._run
    E._on_gpu = lambda net: True
    try:
        yield fake
    finally:
        N._lib, E._lib, R._lib, N.LandNet.forward, E._on_gpu = saved
