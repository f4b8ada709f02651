"""csrc/ice_budget.hip through the C ABI (ace_ice_budget_apply) against the numpy statement of its contract (tests/_ice_ref.py), bit
for bit, NaN matching NaN.  Every plane lies inside a larger buffer of sentinel floats - guards in front and behind, the other
time levels of a (B, T, H * W) window - and the whole buffer is compared, so a write outside the plane, or to the input, fails.
The scratch is handed over full of 0xFF bytes: the call has to clear its own flags.

Shapes: H * W = 15 (below a wave), 63 (no multiple of 4), 64, 2145 = 33 x 65 (several workgroups, ragged tail: the 4-byte form) and
2176 = 34 x 64 (several workgroups of the 16-byte form, ragged tail); B = 1 and 3.  The statement's returned flag paths are asserted,
so no path is silently missing."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ice_cases as C  # noqa: E402
import _ice_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
DT = 21600.0
DT_ODD = 432000.000001          # dt * x is inexact in fp64
SHAPES = [(3, 5), (7, 9), (8, 8), (33, 65), (34, 64)]
KEYS = ("old", "source", "sink", "transport", "mass")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def lib():
    from ace_amd import _lib
    return _lib.lib()


def launches():
    a, b, c = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
    assert lib().ace_ice_budget_launches(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    return a.value, b.value, c.value


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and bool((nan == np.isnan(b)).all() and (a.view(np.int32)[~nan] == b.view(np.int32)[~nan]).all())


class Buffers:
    """the five planes of every variable inside sentinel-filled buffers: `front` guard floats (4: 16-byte aligned planes, 5: one
    float off), and with `steps` > 1 the plane is time level `level` of a (B, steps, HW) window (per-sample stride steps * HW)"""

    def __init__(self, dev, variables, B, HW, front=4, steps=1, level=0):
        self.B, self.HW, self.front, self.steps, self.level = B, HW, front, steps, level
        self.host, self.device = [], []
        for X in variables:
            h = {}
            for key in KEYS:
                buf = np.full(front + B * steps * HW + 4, SENTINEL, np.float32)
                src = X[key] if key != "mass" else np.full((B, HW), -7.0, np.float32)      # the prognostic is overwritten
                self.window(buf)[:, level] = src
                h[key] = buf
            self.host.append(h)
            self.device.append({k: torch.from_numpy(v).to(dev) for k, v in h.items()})
            for t in self.device[-1].values():
                assert t.data_ptr() % 16 == 0

    def window(self, buf):
        return buf[self.front:self.front + self.B * self.steps * self.HW].reshape(self.B, self.steps, self.HW)

    def fields(self, variables):
        from ace_amd._lib import IceFields
        f = IceFields()
        for v, X in enumerate(variables):
            for key, attr in zip(KEYS, ("old_mass", "source", "sink", "transport", "mass")):
                p = getattr(f.var[v], attr)
                p.p = self.device[v][key].data_ptr() + 4 * (self.front + self.level * self.HW)
                p.stride = self.steps * self.HW
            f.var[v].area_mode, f.var[v].masked = int(X["area_mode"]), int(X["masked"])
        f.nvars = len(variables)
        return f

    def check(self, outs):
        """every buffer whole: the planes are the statement's, everything around them is untouched"""
        for v, o in enumerate(outs):
            for key in KEYS:
                want = self.host[v][key].copy()
                if key != "old":
                    self.window(want)[:, self.level] = o[key]
                got = self.device[v][key].cpu().numpy()
                assert same_bits(got, want), (v, key)


def scratch_for(dev, B, HW):
    n = lib().ace_ice_budget_scratch_bytes(B, HW)
    assert n >= 64 + B * HW
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)


def run(dev, variables, dt, B, H, W, **layout):
    bufs = Buffers(dev, variables, B, H * W, **layout)
    scratch = scratch_for(dev, B, H * W)
    before = launches()
    rc = lib().ace_ice_budget_apply(ctypes.byref(bufs.fields(variables)), dt, B, H, W, scratch.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib().ace_ice_budget_last_error().decode()
    torch.cuda.synchronize()
    n = len(variables)
    assert tuple(a - b for a, b in zip(launches(), before)) == (n, n, 1)       # at most 2 * nvars launches and one clearing
    return bufs, scratch


def expect(variables, dt, paths=None):
    outs, flags, info = R.ice_budget_ref(variables, dt)
    if paths is not None:
        assert [tuple(i["path"]) for i in info] == [tuple(p) for p in paths], [i["path"] for i in info]
    return outs, flags, info


def three_case(B, HW, a1, a2, a3, dt, seed):
    """the eight paths of the masked concentration; between them the four of the masked mass and the two of the unmasked one"""
    sn = (a2, a1 ^ a3)
    on = {0: "A" * (a3 ^ a2), 1: "A" * a1 + "B" * a2 + "C" * a3, 2: "A" * sn[0] + "C" * sn[1]}
    return C.make(B, HW, C.THREE, on, dt, seed), [(a3 ^ a2, 0, 0), (a1, a2, a3), (sn[0], 0, sn[1])]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_path_of_three_variables(dev, shape, B):
    H, W = shape
    for n, (a1, a2, a3) in enumerate([(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]):
        dt = DT if n % 2 else DT_ODD
        variables, paths = three_case(B, H * W, a1, a2, a3, dt, 1000 + 8 * H + n)
        outs, flags, _ = expect(variables, dt, paths)
        bufs, scratch = run(dev, variables, dt, B, H, W)
        bufs.check(outs)
        words = scratch[:12].cpu().numpy().view(np.uint32)
        assert list(words) == flags, (list(words), flags)               # the device's OR over the tensor is the statement's


@pytest.mark.parametrize("shape", SHAPES)
def test_every_path_of_a_lone_variable(dev, shape):
    H, W = shape
    for area in (True, False):
        for a1 in (0, 1):
            for a2 in ((0, 1) if area else (0,)):
                variables = C.make(3, H * W, [(area, False)], {0: "A" * a1 + "B" * a2}, DT, 2000 + H + 2 * a1 + a2)
                outs, _, _ = expect(variables, DT, [(a1, a2, 0)])
                run(dev, variables, DT, 3, H, W)[0].check(outs)


def test_flag_crosses_workgroups_and_samples(dev):
    """the only trigger is the last pixel of the last sample; the violations it has repaired are in the first workgroup of sample 0"""
    H, W, B = 33, 65, 3
    variables = C.make(B, H * W, [(True, False)], {0: "A"}, DT, 31)
    assert C.pixels(H * W)[1][0] == H * W - 1
    quiet = C.make(B, H * W, [(True, False)], {}, DT, 31)
    assert (R._new(quiet[0]["old"].astype(np.float64), [quiet[0][k].astype(np.float64) * DT for k in ("source", "sink", "transport")]) >= 0).all()
    outs, _, _ = expect(variables, DT, [(1, 0, 0)])
    assert outs[0]["source"][0, 1] == 0 and outs[0]["sink"][0, 2] == 0 and variables[0]["source"][0, 1] < 0
    run(dev, variables, DT, B, H, W)[0].check(outs)
    outs, _, _ = expect(quiet, DT, [(0, 0, 0)])
    assert outs[0]["source"][0, 1] < 0 and outs[0]["sink"][0, 2] > 0       # no flag raised: they survive
    run(dev, quiet, DT, B, H, W)[0].check(outs)


@pytest.mark.parametrize("shape", [(8, 8), (34, 64)])
def test_alignment_and_time_slices_give_the_same_bits(dev, shape):
    H, W = shape
    variables, paths = three_case(3, H * W, 1, 1, 1, DT_ODD, 41)
    outs, _, _ = expect(variables, DT_ODD, paths)
    for layout in (dict(front=4), dict(front=5), dict(front=4, steps=3, level=1), dict(front=7, steps=2, level=1)):
        run(dev, variables, DT_ODD, 3, H, W, **layout)[0].check(outs)


@pytest.mark.parametrize("shape", [(8, 8), (33, 65)])
def test_nan_island(dev, shape):
    H, W = shape
    variables, _ = three_case(3, H * W, 1, 0, 1, DT_ODD, 51)
    variables[0]["old"][0, 20] = np.nan                  # a NaN ice mass is "not zero"
    variables[0]["sink"][1, 21] = np.nan
    variables[1]["source"][0, 22:24] = np.nan
    variables[2]["transport"][2, H * W - 5] = np.nan     # on an ice-free pixel
    variables[1]["old"][0, 20] = 0.4
    outs, _, _ = expect(variables, DT_ODD)
    assert np.isnan(outs[0]["mass"][0, 20]) and not np.isnan(outs[1]["mass"][0, 20]) and outs[1]["mass"][0, 20] > 0
    run(dev, variables, DT_ODD, 3, H, W)[0].check(outs)


@pytest.mark.parametrize("shape", [(8, 8), (33, 65)])
def test_ice_mask_is_the_fp64_mass(dev, shape):
    H, W = shape
    variables, _ = three_case(2, H * W, 0, 0, 1, DT_ODD, 61)
    px = C.add_tiny(variables, DT_ODD, 62)
    outs, _, info = expect(variables, DT_ODD)
    m64 = info[0]["mass64"][0, px]
    tiny = (m64 != 0) & (m64.astype(np.float32) == 0)
    assert tiny.any()
    assert info[1]["path"][2] == 1 and (outs[1]["mass"][0, px][tiny] > 0).all()      # stage 3 runs, and keeps these pixels
    bufs, scratch = run(dev, variables, DT_ODD, 2, H, W)
    bufs.check(outs)
    zero = scratch[64:64 + 2 * H * W].cpu().numpy().reshape(2, H * W)
    assert (zero == (info[0]["mass64"] == 0)).all()


def test_repeat_is_bitwise(dev):
    H, W = 33, 65
    variables, paths = three_case(3, H * W, 1, 1, 1, DT_ODD, 71)
    outs, _, _ = expect(variables, DT_ODD, paths)
    a, _ = run(dev, variables, DT_ODD, 3, H, W)
    b, _ = run(dev, variables, DT_ODD, 3, H, W)
    a.check(outs)
    for x, y in zip(a.device, b.device):
        for key in KEYS:
            assert torch.equal(x[key].view(torch.int32), y[key].view(torch.int32)), key


def test_bad_arguments_launch_nothing(dev):
    H, W, B = 8, 8, 2
    variables, _ = three_case(B, H * W, 1, 1, 1, DT, 81)
    bufs = Buffers(dev, variables, B, H * W)
    scratch = scratch_for(dev, B, H * W)
    stream = torch.cuda.current_stream().cuda_stream
    good = lambda: bufs.fields(variables)

    def broken(edit):
        f = good()
        edit(f)
        return f
    before = launches()
    calls = [
        (None, DT, B, H, W, scratch.data_ptr()),
        (broken(lambda f: setattr(f, "nvars", 4)), DT, B, H, W, scratch.data_ptr()),
        (broken(lambda f: setattr(f, "nvars", -1)), DT, B, H, W, scratch.data_ptr()),
        (broken(lambda f: setattr(f.var[1].sink, "p", None)), DT, B, H, W, scratch.data_ptr()),
        (broken(lambda f: setattr(f.var[0], "masked", 1)), DT, B, H, W, scratch.data_ptr()),
        (good(), 0.0, B, H, W, scratch.data_ptr()),
        (good(), -1.0, B, H, W, scratch.data_ptr()),
        (good(), float("nan"), B, H, W, scratch.data_ptr()),
        (good(), float("inf"), B, H, W, scratch.data_ptr()),
        (good(), DT, 0, H, W, scratch.data_ptr()),
        (good(), DT, 65536, H, W, scratch.data_ptr()),
        (good(), DT, B, 0, W, scratch.data_ptr()),
        (good(), DT, B, H, 0, scratch.data_ptr()),
        (good(), DT, B, H, W, None),
        (good(), DT, B, H, W, scratch.data_ptr() + 4),
    ]
    for f, dt, b, h, w, s in calls:
        rc = lib().ace_ice_budget_apply(ctypes.byref(f) if f is not None else None, dt, b, h, w, s, stream)
        assert rc != 0 and lib().ace_ice_budget_last_error().decode()
    torch.cuda.synchronize()
    assert launches() == before
    for v in range(3):
        for key in KEYS:
            assert same_bits(bufs.device[v][key].cpu().numpy(), bufs.host[v][key]), (v, key)
    assert bool((scratch == 0xFF).all())
    empty = broken(lambda f: setattr(f, "nvars", 0))      # nothing to correct: a no-op
    assert lib().ace_ice_budget_apply(ctypes.byref(empty), DT, B, H, W, None, stream) == 0 and launches() == before
