"""TEST INFRASTRUCTURE: the global-mean-removal entries of the C ABI (ace_gmr_chunks / partials / pack_normalize /
unpack_denormalize; include/ace_sfno.h) added to the emulation of tests/_fake_sfno.py, implemented with the numpy statement of
their contract (tests/_gmr_ref.py) on host memory - same pointer tables, strides and index tables as the kernels - so that the
HOST logic of RolloutEngine with a global-mean-removal stepper runs in the ``-m "not gpu"`` suite.  Not a fallback: nothing in the
product imports it.  Use: ``with fake_gmr(): RolloutEngine(...)``."""
import contextlib
import ctypes
import types

import numpy as np

import _gmr_ref as R
from _fake_sfno import _view, fake_sfno


def _arr(ptr, n, ctype):
    return np.ctypeslib.as_array((ctype * int(n)).from_address(int(ptr)))


def _plane(ptr, stride, b, hw):
    return _arr(int(ptr) + 4 * b * int(stride), hw, ctypes.c_float)


def ace_gmr_chunks(self, hw):
    return R.chunks(hw)


def ace_gmr_partials(self, srcs, strides, plane_idx, nsrc, partials, batch, K, hw, stream):
    p, s = _view(srcs, nsrc, ctypes.c_int64), _view(strides, nsrc, ctypes.c_int64)
    idx = _arr(plane_idx, K, ctypes.c_int32)
    C = R.chunks(hw)
    out = _arr(partials, batch * K * C, ctypes.c_double).reshape(batch, K, C)
    for b in range(batch):
        for k in range(K):
            j = int(idx[k])
            out[b, k] = R.partials(_plane(p[j], s[j], b, hw)) if 0 <= j < nsrc else np.nan
    return 0


def _shift(partials, clim, b, k, hw):
    p = partials[b, k]
    s = p[0]
    for c in range(1, p.size):
        s = s + p[c]
    with np.errstate(invalid="ignore"):
        return np.float32(clim[k]) - np.float32(s / np.float64(hw))


def ace_gmr_pack_normalize(self, srcs, strides, mean, std, shift_idx, partials, clim_mean, extra_idx, extra_std, dst, shift,
                           batch, nin, nextra, K, hw, stream):
    assert 1 <= K <= nin and nextra >= 0
    p, s = _view(srcs, nin, ctypes.c_int64), _view(strides, nin, ctypes.c_int64)
    m, d = _arr(mean, nin, ctypes.c_float), _arr(std, nin, ctypes.c_float)
    idx = _arr(shift_idx, nin, ctypes.c_int32)
    part = _arr(partials, batch * K * R.chunks(hw), ctypes.c_double).reshape(batch, K, -1)
    clim = _arr(clim_mean, K, ctypes.c_float)
    out = _arr(dst, batch * (nin + nextra) * hw, ctypes.c_float).reshape(batch, nin + nextra, hw)
    sh = _arr(shift, batch * K, ctypes.c_float).reshape(batch, K)
    for b in range(batch):
        for k in range(K):
            sh[b, k] = _shift(part, clim, b, k, hw)
        for j in range(nin):
            k = int(idx[j])
            out[b, j] = R.pack(_plane(p[j], s[j], b, hw), sh[b, k] if 0 <= k < K else None, m[j], d[j])
        if nextra:
            ei, es = _arr(extra_idx, nextra, ctypes.c_int32), _arr(extra_std, nextra, ctypes.c_float)
            for e in range(nextra):
                out[b, nin + e] = R.extra(sh[b, int(ei[e])], es[e])
    return 0


def ace_gmr_unpack_denormalize(self, src, mean, std, dsts, strides, shift_idx, shift, batch, nch, K, hw, stream):
    p, s = _view(dsts, nch, ctypes.c_int64), _view(strides, nch, ctypes.c_int64)
    m, d = _arr(mean, nch, ctypes.c_float), _arr(std, nch, ctypes.c_float)
    idx = _arr(shift_idx, nch, ctypes.c_int32)
    sh = _arr(shift, batch * K, ctypes.c_float).reshape(batch, K)
    y = _arr(src, batch * nch * hw, ctypes.c_float).reshape(batch, nch, hw)
    for b in range(batch):
        for j in range(nch):
            k = int(idx[j])
            _plane(p[j], s[j], b, hw)[:] = R.unpack(y[b, j], sh[b, k] if 0 <= k < K else None, m[j], d[j])
    return 0


@contextlib.contextmanager
def fake_gmr():
    """``fake_sfno()`` whose object also answers the ace_gmr_* entries."""
    with fake_sfno() as fake:
        for fn in (ace_gmr_chunks, ace_gmr_partials, ace_gmr_pack_normalize, ace_gmr_unpack_denormalize):
            setattr(fake, fn.__name__, types.MethodType(fn, fake))
        yield fake
