"""TEST INFRASTRUCTURE: the sea-ice budget entries of the C ABI (ace_ice_budget_*; include/ace_sfno.h) emulated on host memory with
the numpy statement of their contract (tests/_ice_ref.py) - same plane structs, strides, flag words and mask bytes as the kernels -
so that the HOST logic of ``FusedIceCorrector`` (plane resolution, scratch, launch counts) runs in the ``-m "not gpu"`` suite on
CPU tensors.  Not a fallback: nothing in the product imports it.  Use: ``with fake_ice() as fake: handle.apply(fields, 0)``."""
import contextlib
import ctypes

import numpy as np

import _ice_ref as R

FLAG_BYTES = 64


def _plane(p, b, hw):
    return np.ctypeslib.as_array((ctypes.c_float * hw).from_address(int(p.p) + 4 * b * int(p.stride)))


class FakeIce:
    def __init__(self):
        self.flags = self.applies = self.clears = 0
        self.error = b""
        self.calls = []

    def ace_ice_budget_last_error(self):
        return self.error

    def ace_ice_budget_scratch_bytes(self, batch, hw):
        return FLAG_BYTES + ((batch * hw + 15) & ~15) if batch >= 1 and hw >= 1 else 0

    def ace_ice_budget_launches(self, a, b, c):
        a._obj.value, b._obj.value, c._obj.value = self.flags, self.applies, self.clears
        return 0

    def _fail(self, msg):
        self.error = msg.encode()
        return -1

    def ace_ice_budget_apply(self, fields, timestep, batch, H, W, scratch, stream):
        f = fields._obj
        hw = H * W
        if not (0 <= f.nvars <= 3) or not (timestep > 0 and np.isfinite(timestep)) or not (1 <= batch <= 65535) or H < 1 or W < 1:
            return self._fail("bad argument")
        if f.nvars == 0:
            return 0
        if not scratch or scratch % 16:
            return self._fail("bad scratch")
        variables = []
        for v in range(f.nvars):
            X = f.var[v]
            if not all(p.p for p in (X.old_mass, X.source, X.sink, X.transport, X.mass)) or (v == 0 and X.masked):
                return self._fail(f"variable {v}")
            rd = lambda p: np.stack([_plane(p, b, hw).copy() for b in range(batch)])
            variables.append({"old": rd(X.old_mass), "source": rd(X.source), "sink": rd(X.sink), "transport": rd(X.transport),
                              "area_mode": bool(X.area_mode), "masked": bool(X.masked)})
        outs, flags, info = R.ice_budget_ref(variables, timestep)
        for v, o in enumerate(outs):
            X = f.var[v]
            for p, key in ((X.source, "source"), (X.sink, "sink"), (X.transport, "transport"), (X.mass, "mass")):
                for b in range(batch):
                    _plane(p, b, hw)[:] = o[key][b]
        words = np.ctypeslib.as_array((ctypes.c_uint32 * (FLAG_BYTES // 4)).from_address(scratch))
        words[:] = 0
        words[:len(flags)] = flags
        if any(X["masked"] for X in variables):
            np.ctypeslib.as_array((ctypes.c_uint8 * (batch * hw)).from_address(scratch + FLAG_BYTES))[:] = (info[0]["mass64"] == 0).ravel()
        self.flags += f.nvars
        self.applies += f.nvars
        self.clears += 1
        self.calls.append({"paths": [tuple(i["path"]) for i in info], "stream": stream, "scratch": scratch, "timestep": timestep})
        return 0


@contextlib.contextmanager
def fake_ice():
    """ace_amd._lib.lib() answering the ace_ice_budget_* entries from the emulation"""
    from ace_amd import _lib
    fake, saved = FakeIce(), _lib.lib
    _lib.lib = lambda: fake
    try:
        yield fake
    finally:
        _lib.lib = saved
