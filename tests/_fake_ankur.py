"""TEST INFRASTRUCTURE: an emulation of ``ace_disco_*`` and ``ace_pixel_mlp_create2`` (include/ace_sfno.h) on host memory, on top of
tests/_fake_landnet.py - the forwards are the header's statements (tests/_disco_ref.py, tests/_pixel_mlp_ref2.py); GELU and SiLU,
which the statements leave to the toolchain, are the fp64 activation rounded to fp32 - so that the HOST logic of ace_amd/ankur.py
(parameter order, which layers go to which kernel, handle life) runs in the ``-m "not gpu"`` suite.  Not a fallback: nothing in the
product imports it.  Use: ``with fake_ankur() as fake:``."""
import contextlib
import ctypes
import types

import numpy as np

import _disco_ref as D
import _pixel_mlp_ref2 as P
from _fake_landnet import FakeLandnet, _f32, _val, _view


def _soft(act, v):
    if act == P.ACT_GELU:
        return D.gelu64(v).astype(np.float32)
    if act == P.ACT_SILU:
        return D.silu64(v).astype(np.float32)
    return v


class FakeAnkur(FakeLandnet):
    # -- ace_pixel_mlp_create2 / forward with the soft activations
    def ace_pixel_mlp_create2(self, n_layers, dims, w_dev, bias_dev, act, embed_layer, embed_before_act, stream, out):
        rc = self.ace_pixel_mlp_create(n_layers, dims, w_dev, bias_dev, act, embed_layer, stream, out)
        self._handles[out._obj.value] += (embed_before_act,)
        return rc

    def ace_pixel_mlp_forward(self, h, x, embed, y, batch, hw, stream):
        rec = self._handles.get(_val(h))
        if rec is None or len(rec) == 5:
            return super().ace_pixel_mlp_forward(h, x, embed, y, batch, hw, stream)
        self.calls.append("pixel_mlp_forward")
        dims, ws, bs, act, embed_layer, first = rec
        if embed_layer >= 0 and not embed:
            self.error = b"(emulated ace_pixel_mlp) embed must not be NULL"
            return self.ACE_ERR_INVALID
        a = _f32(x, batch * dims[0] * hw).reshape(batch, dims[0], hw)
        e = _f32(embed, dims[embed_layer + 1] * hw).reshape(-1, hw) if embed_layer >= 0 else None
        for l in range(len(ws)):                    # layer by layer: a soft activation is applied to the statement's accumulator
            el = 0 if l == embed_layer else -1
            if act[l] in (P.ACT_GELU, P.ACT_SILU):
                pre = P.pixel_mlp2(a, [ws[l]], [bs[l]], [act[l]], el if first else -1, e, bool(first), pre_activation=True)
                a = _soft(act[l], pre)
                if el == 0 and not first:
                    a = (a + e[None]).astype(np.float32)
            else:
                a = P.pixel_mlp2(a, [ws[l]], [bs[l]], [act[l]], el, e, bool(first))
        _f32(y, batch * dims[-1] * hw).reshape(batch, dims[-1], hw)[...] = a
        return 0

    # -- ace_disco_*
    def ace_disco_last_error(self):
        return self.error

    def ace_disco_create(self, H, W, K, row_off, hi, wi, vals, w_dev, in_chans, out_chans, groups, act, has_embed, stream, out):
        if groups < 1 or in_chans % groups or out_chans % groups:
            self.error = b"(emulated ace_disco) groups must divide both channel counts"
            return self.ACE_ERR_INVALID
        offs = _view(row_off, H + 1, ctypes.c_int64).copy()
        P_ = int(offs[-1])
        table = types.SimpleNamespace(row_offsets=offs, hi=_view(hi, P_, ctypes.c_int32).copy(), wi=_view(wi, P_, ctypes.c_int32).copy(),
                                      vals=_f32(vals, P_ * K).copy().reshape(P_, K))
        gs = in_chans // groups
        w = _f32(w_dev, out_chans * gs * K).copy().reshape(out_chans, gs, K)
        self._handles[self._next] = ("disco", table, w, (H, W, in_chans, out_chans, groups, act, has_embed))
        out._obj.value = self._next
        self._next += 1
        self.created += 1
        self.calls.append("disco_create")
        return 0

    def ace_disco_destroy(self, h):
        if self._handles.pop(_val(h), None) is not None:
            self.destroyed += 1

    def ace_disco_forward(self, h, x, embed, y, batch, stream):
        self.calls.append("disco_forward")
        _, table, w, (H, W, cin, cout, groups, act, has_embed) = self._handles[_val(h)]
        if has_embed and not embed:
            self.error = b"(emulated ace_disco) embed must not be NULL"
            return self.ACE_ERR_INVALID
        xin = _f32(x, batch * cin * H * W).reshape(batch, cin, H, W)
        e = _f32(embed, cout * H * W).reshape(cout, H, W) if has_embed else None
        soft = act in (D.ACT_GELU, D.ACT_SILU)
        out = D.disco(xin, table, w, groups, act, e, pre_activation=soft)
        _f32(y, batch * cout * H * W).reshape(batch, cout, H, W)[...] = _soft(act, out) if soft else out
        return 0


@contextlib.contextmanager
def fake_ankur():
    """ace_amd.{ankur, disco, landnet} bound to the emulation; the net's forward without its "must be on the GPU" guard."""
    import ace_amd.ankur as A
    import ace_amd.disco as DD
    import ace_amd.landnet as N
    from ace_amd import _lib as real
    fake = FakeAnkur(real)
    saved = (A._lib, DD._lib, N._lib, A.AnkurLocalNetModel.forward)
    A._lib = DD._lib = N._lib = fake
    A.AnkurLocalNetModel.forward = A.AnkurLocalNetModel._run
    try:
        yield fake
    finally:
        A._lib, DD._lib, N._lib, A.AnkurLocalNetModel.forward = saved
