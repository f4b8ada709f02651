"""TEST INFRASTRUCTURE: the step-diagnostics entries of the C ABI (ace_stepdiag_snapshot / ace_stepdiag_delta_window /
ace_diag_correction_partial_doubles / ace_diag_correction_window; include/ace_sfno.h) added to the emulation of tests/_fake_sfno.py,
implemented with the numpy statement of their contract (tests/_stepdiag_ref.py) on host memory - same pointer tables, strides and
index tables as the kernels - so that the HOST logic of ``CorrectionDeltaRecorder``, of ``RolloutEngine(step_diagnostics=True)`` and of
the fused path of ``CorrectionDeltaAggregator`` runs in the ``-m "not gpu"`` suite.  Not a fallback: nothing in the product imports it.
Use: ``with fake_stepdiag(): RolloutEngine(..., step_diagnostics=True)``."""
import contextlib
import ctypes
import types

import numpy as np

import _stepdiag_ref as R
from _fake_sfno import fake_sfno

CHUNK, WAVES, NMOM = 1024, 4, 4


def _arr(ptr, n, ctype):
    return np.ctypeslib.as_array((ctype * int(n)).from_address(int(ptr)))


def _plane(ptr, offset, hw):
    return _arr(int(ptr) + 4 * int(offset), hw, ctypes.c_float)


def ace_stepdiag_snapshot(self, srcs, src_strides, dsts, dst_strides, nplanes, batch, hw, stream):
    assert 0 <= nplanes <= 65535 and 1 <= batch <= 65535 and hw >= 1
    p, s = _arr(srcs, nplanes, ctypes.c_int64), _arr(src_strides, nplanes, ctypes.c_int64)
    q, d = _arr(dsts, nplanes, ctypes.c_int64), _arr(dst_strides, nplanes, ctypes.c_int64)
    for k in range(nplanes):
        for b in range(batch):
            _plane(q[k], b * d[k], hw)[:] = R.snapshot(_plane(p[k], b * s[k], hw))
    return 0


def ace_stepdiag_delta_window(self, outs, out_strides, snaps, snap_strides, nplanes, batch, steps, hw, stream):
    assert 0 <= nplanes <= 65535 and batch >= 1 and steps >= 1 and batch * steps <= 65535 and hw >= 1
    p, s = _arr(outs, nplanes, ctypes.c_int64), _arr(out_strides, 2 * nplanes, ctypes.c_int64)
    q, d = _arr(snaps, nplanes, ctypes.c_int64), _arr(snap_strides, 2 * nplanes, ctypes.c_int64)
    for k in range(nplanes):
        for b in range(batch):
            for t in range(steps):
                snap = _plane(q[k], b * d[2 * k] + t * d[2 * k + 1], hw)
                snap[:] = R.delta(_plane(p[k], b * s[2 * k] + t * s[2 * k + 1], hw), snap)
    return 0


def ace_diag_correction_partial_doubles(self, nplanes, batch, steps, hw):
    if nplanes < 0 or batch < 1 or steps < 1 or hw < 1:
        return -1
    return nplanes * batch * steps * ((hw + CHUNK - 1) // CHUNK) * WAVES * NMOM


def ace_diag_correction_window(self, deltas, strides, stds, rows, wrows, weights, nw, partial, signed_sum, magnitude_sum, series,
                               nrows, n_time, t0, nplanes, batch, steps, hw, stream):
    assert 0 <= nplanes <= 65535 and 1 <= steps <= 65535 and batch >= 1 and hw >= 1 and nw >= 1 and nrows >= 1
    assert 0 <= t0 and t0 + steps <= n_time and partial
    p, s = _arr(deltas, nplanes, ctypes.c_int64), _arr(strides, 2 * nplanes, ctypes.c_int64)
    planes = [np.stack([np.stack([_plane(p[j], b * s[2 * j] + t * s[2 * j + 1], hw) for t in range(steps)]) for b in range(batch)])
              for j in range(nplanes)]
    R.correction_window(planes, _arr(stds, nplanes, ctypes.c_float), _arr(rows, nplanes, ctypes.c_int32),
                        _arr(wrows, nplanes, ctypes.c_int32), _arr(weights, nw * hw, ctypes.c_float).reshape(nw, hw),
                        _arr(signed_sum, nrows * hw, ctypes.c_double).reshape(nrows, hw),
                        _arr(magnitude_sum, nrows * hw, ctypes.c_double).reshape(nrows, hw),
                        _arr(series, 2 * nrows * n_time, ctypes.c_double).reshape(2, nrows, n_time), t0)
    return 0


def _upload_planes(names, gen, target, dev, sections=()):
    """``ace_amd.aggregator._upload_planes`` without the pinned staging buffer, which needs a device"""
    import itertools

    import torch

    from ace_amd.aggregator import _plane_table
    values, off = _plane_table(names, gen, target)
    parts = [np.asarray(values, np.int64), *sections]
    table = torch.from_numpy(np.concatenate([q.reshape(-1).view(np.uint8) for q in parts]).copy())
    at = {k: table.data_ptr() + o for k, o in off.items()}
    at["table"] = table
    return at, list(itertools.accumulate([q.nbytes for q in sections[:-1]], initial=at["end"])) if sections else []


@contextlib.contextmanager
def fake_stepdiag():
    """``fake_sfno()`` whose object also answers the step-diagnostics entries, bound to ``ace_amd._lib`` as well (what
    ace_amd/step_diagnostics.py imports at call time), with a host-only ``_upload_planes``."""
    import ace_amd
    import ace_amd.aggregator as A
    with fake_sfno() as fake:
        for fn in (ace_stepdiag_snapshot, ace_stepdiag_delta_window, ace_diag_correction_partial_doubles, ace_diag_correction_window):
            setattr(fake, fn.__name__, types.MethodType(fn, fake))
        saved = (ace_amd._lib, A._upload_planes)
        ace_amd._lib, A._upload_planes = fake, _upload_planes
        try:
            yield fake
        finally:
            ace_amd._lib, A._upload_planes = saved
