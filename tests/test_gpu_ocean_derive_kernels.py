"""csrc/ocean_derive.hip through the C ABI (ace_ocean_derive_window) against tests/_ocean_derive_ref.py, the numpy statement of the
header contract that tests/test_ocean_derive_ref_cpu.py holds to the reference.

Bar: equality on all seven outputs.  The kernel sums the exact fp64 products in level order, differences and divides in IEEE fp64,
and does the fp32 arithmetic one correctly rounded operation at a time, as the statement does: the same bits where the statement
has a number, NaN where it has NaN.  Every output lies between guards and is pre-filled with a sentinel, so a slot that should have
been written and was not shows, as does an output that was not wanted and was touched; the inputs must come back unchanged.

Shapes: the smallest that reach each branch - B = 2, T <= 9; hw = 15 (3 x 5: no 16-byte path, a tail thread), 32 and 36 (the
16-byte path), 1027 and 1100 (more than one 1024-pixel chunk, ragged); planes one float past a 16-byte boundary; a sample stride
that keeps the 16-byte path (+ 8 floats) and one that does not (+ 3); 1, 7, 8 and 64 levels (below, at and above the 8 levels
whose loads are issued together); 1, 2 and 9 steps in chunks of 1, 4, T and 0 (the library's choice)."""
import ctypes

import numpy as np
import pytest
import torch

import _ocean_derive_ref as R
from _ocean_derive_cases import SPECIAL_ROWS
from test_gpu_diag_kernels import INVALID, dev, lib  # noqa: F401
from test_gpu_timeseg_kernels import Guarded32

pytestmark = pytest.mark.gpu

SENT = -12345.0
DT = 432000.0
FULL = list(R.OUTPUTS)
SURFACE = ("hfds", "hfds_total_area", "hfgeou", "sea_surface_fraction", "land_fraction", "ocean_sea_ice_fraction", "sea_ice_fraction",
           "sea_ice_volume")
# the fields from which all seven can be derived, and the set that takes every other alternative (hfds and both fractions present,
# no hfgeou, HI from sea_ice_fraction)
DERIVE_ALL = ("hfds_total_area", "hfgeou", "land_fraction", "ocean_sea_ice_fraction", "sea_ice_volume")
PRESENT = ("hfds", "sea_surface_fraction", "land_fraction", "sea_ice_fraction", "sea_ice_volume")
WANT_PRESENT = [n for n in FULL if n not in ("hfds", "sea_ice_fraction")]


def make_inputs(seed, B, T, hw, nlev, names=DERIVE_ALL):
    """numpy inputs of the statement: thetao with NaN below a floor, dz with zeros, a mask with land, special sea-ice pixels"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                                       # noqa: E731
    u = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)                                # noqa: E731
    floor = torch.randint(0, nlev + 1, (hw,), generator=g)                     # levels below it hold NaN, 0: a land column
    below = torch.arange(nlev)[:, None] >= floor[None, :]                      # (nlev, hw)
    thetao = [torch.where(below[k], torch.full((), float("nan")), r(B, T + 1, hw) * 2.0 + 14.0 - 0.2 * k) for k in range(nlev)]
    dz = torch.where(below, torch.zeros(()), u(5.0, 400.0, nlev, hw))
    mask0 = (floor > 0).float()
    area = u(1e9, 1e10, hw)
    every = {"hfds": r(B, T, hw) * 40 + 5, "hfds_total_area": r(B, T, hw) * 40 + 3, "hfgeou": r(B, T, hw) * 0.02 + 0.08,
             "sea_surface_fraction": u(0.0, 1.0, B, T, hw), "land_fraction": u(0.0, 1.0, B, T, hw),
             "ocean_sea_ice_fraction": u(0.0, 1.0, B, T, hw), "sea_ice_fraction": u(0.0, 0.9, B, T, hw),
             "sea_ice_volume": u(0.0, 5.0, B, T, hw)}
    n = min(hw, len(SPECIAL_ROWS))                                             # sample 0, last step: rows of HI's table
    vol, frac, fac = (torch.tensor([row[i] for row in SPECIAL_ROWS[:n]]) for i in range(3))
    every["sea_ice_volume"][0, T - 1, :n] = vol
    every["ocean_sea_ice_fraction"][0, T - 1, :n] = frac
    every["sea_ice_fraction"][0, T - 1, :n] = frac
    every["sea_surface_fraction"][0, T - 1, :n] = 1.0
    every["land_fraction"][0, T - 1, :n] = 0.0
    area[:n] = area[:n] * fac
    every["land_fraction"][B - 1, 0, hw - 1] = float("nan")
    every["land_fraction"][B - 1, 0, hw - 2 if hw > 1 else 0] = 1.0
    every["hfds_total_area"][B - 1, 0, 0] = float("inf")
    every["sea_surface_fraction"][B - 1, 0, 1 if hw > 1 else 0] = 0.0
    f = {k: every[k].numpy() for k in names}
    return dict(thetao=[x[:, 1:].contiguous().numpy() for x in thetao], head=[x[:, 0].contiguous().numpy() for x in thetao],
                dz=dz.numpy(), mask0=mask0.numpy(), area_m2=area.numpy(), **f)


class Placed:
    """a (B, T, hw) or (n, hw) fp32 array in device storage under a layout; keeps the host copy to check it is unchanged"""

    def __init__(self, data, layout, dev, g, static=False):
        data = torch.from_numpy(np.ascontiguousarray(data))
        lead, rest = data.shape[0], data[0].numel()
        off = 1 if layout == "offset1" else 0
        pad = 0 if static else {"bstride8": 8, "bstride3": 3}.get(layout, 0)
        host = torch.randn(off + lead * (rest + pad) + 3, generator=g) * 1e30
        host[off:off + lead * (rest + pad)].view(lead, rest + pad)[:, :rest] = data.reshape(lead, rest)
        self.host, self.device = host, host.to(dev)
        self.ptr = self.device.data_ptr() + 4 * off
        self.bstride = rest + pad
        self.tstride = data.shape[-1]

    def unchanged(self):
        return torch.equal(self.device.cpu().view(torch.int32), self.host.view(torch.int32))


def call(dev, inp, want, B, T, hw, nlev, layout="contiguous", head="all", t_chunk=0, expect=0, override=None, null_out=(),
         seed=0):
    """one ace_ocean_derive_window; returns ({name: (B, T, hw) numpy of every one of the seven outputs}, the statement's outputs)"""
    from ace_amd import _lib
    L = lib()
    g = torch.Generator().manual_seed(seed)
    d = _lib.OceanDeriveDesc()
    placed = []

    def put(x, static=False):
        p = Placed(x, layout, dev, g, static)
        placed.append(p)
        return p

    d.nlev = nlev
    for k in range(min(nlev, len(inp["thetao"]), _lib.OCEAN_MAX_LEVELS)):
        p = put(inp["thetao"][k])
        d.thetao[k].f.base, d.thetao[k].f.bstride, d.thetao[k].f.tstride = p.ptr, p.bstride, p.tstride
        if head == "all" or (head == "one_absent" and k != nlev // 2):
            h = put(inp["head"][k])
            d.thetao[k].head, d.thetao[k].head_bstride = h.ptr, h.bstride
    d.dz, d.mask0, d.area_m2 = put(inp["dz"], True).ptr, put(inp["mask0"][None], True).ptr, put(inp["area_m2"][None], True).ptr
    for name in SURFACE:
        if name in inp:
            p = put(inp[name])
            f = getattr(d, name)
            f.base, f.bstride, f.tstride = p.ptr, p.bstride, p.tstride
    off = 1 if layout == "offset1" else 0
    outs = {n: Guarded32(torch.full((B * T * hw + off,), SENT), dev) for n in FULL}
    d.want = 0
    for i, n in enumerate(FULL):
        if n in want:
            d.want |= 1 << i
        d.out[i] = None if n in null_out else outs[n].ptr + 4 * off
    d.out_bstride, d.out_tstride = T * hw, hw
    d.has_head, d.dt_seconds, d.batch, d.steps, d.hw, d.t_chunk = int(head != "none"), DT, B, T, hw, t_chunk
    for k, v in (override or {}).items():
        setattr(d, k, v)
    rc = L.ace_ocean_derive_window(ctypes.byref(d), None)
    assert rc == expect, L.ace_ocean_derive_last_error().decode()
    torch.cuda.synchronize()
    got = {}
    for n in FULL:
        flat = outs[n].read()
        assert off == 0 or float(flat[0]) == SENT
        got[n] = flat[off:].reshape(B, T, hw).numpy()
    assert all(p.unchanged() for p in placed), "an input plane changed"
    ref = {}
    if rc == 0 and want:
        heads = None if head == "none" else [h if (head == "all" or k != nlev // 2) else None for k, h in enumerate(inp["head"])]
        ref = R.derive_window(list(want), DT, head=heads, **{k: v for k, v in inp.items() if k != "head"})
    return got, ref


def same(got, ref, want, what=""):
    for n in FULL:
        if n not in want:
            assert np.all(got[n] == SENT), (what, n, "an output that was not wanted was touched")
            continue
        a, b = got[n], ref[n]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, n, "NaN pattern")
        keep = ~np.isnan(b)
        assert np.array_equal(a.view(np.int32)[keep], b.view(np.int32)[keep]), \
            (what, n, float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64))[keep])))


@pytest.mark.parametrize("layout", ["contiguous", "offset1", "bstride8", "bstride3"])
@pytest.mark.parametrize("hw", [15, 32, 36])
def test_plane_sizes_and_layouts(dev, hw, layout):
    B, T, nlev = 2, 9, 7
    inp = make_inputs(hw, B, T, hw, nlev)
    got, ref = call(dev, inp, FULL, B, T, hw, nlev, layout=layout, t_chunk=4)
    same(got, ref, FULL, (hw, layout))
    assert np.isnan(got["HI"][0, T - 1, 0]) and got["HI"][0, T - 1, 10] == R.FLT_MAX          # rows of the table were reached


@pytest.mark.parametrize("layout", ["contiguous", "offset1"])
@pytest.mark.parametrize("hw", [1027, 1100])
def test_more_than_one_chunk_of_pixels(dev, hw, layout):
    B, T, nlev = 2, 3, 7
    inp = make_inputs(hw, B, T, hw, nlev)
    got, ref = call(dev, inp, FULL, B, T, hw, nlev, layout=layout, t_chunk=2)
    same(got, ref, FULL, (hw, layout))


@pytest.mark.parametrize("hw", [15, 32])
@pytest.mark.parametrize("nlev", [1, 7, 8, 64])
def test_level_counts(dev, nlev, hw):
    B, T = 2, 2
    inp = make_inputs(nlev, B, T, hw, nlev)
    got, ref = call(dev, inp, FULL, B, T, hw, nlev, head="one_absent")
    same(got, ref, FULL, (nlev, hw))


@pytest.mark.parametrize("head", ["all", "none", "one_absent"])
@pytest.mark.parametrize("T", [1, 2, 9])
def test_every_time_chunking_gives_the_same_bytes(dev, T, head):
    B, hw, nlev = 2, 36, 7
    inp = make_inputs(T, B, T, hw, nlev)
    runs = []
    for t_chunk in (1, 4, T, 0):
        got, ref = call(dev, inp, FULL, B, T, hw, nlev, head=head, t_chunk=t_chunk)
        same(got, ref, FULL, (T, head, t_chunk))
        runs.append(got)
    for got in runs[1:]:
        for n in FULL:
            assert np.array_equal(got[n].view(np.int32), runs[0][n].view(np.int32)), n
    if head == "none":                                    # the reference's zeros_like row: + 0.0 everywhere, land included
        assert not np.any(runs[0]["ocean_heat_content_tendency"][:, 0].view(np.int32))
        assert np.isnan(runs[0]["ocean_heat_content"][:, 0]).any()


@pytest.mark.parametrize("want", [[n] for n in FULL])
def test_each_output_alone(dev, want):
    B, T, hw, nlev = 2, 2, 15, 7
    inp = make_inputs(5, B, T, hw, nlev)
    got, ref = call(dev, inp, want, B, T, hw, nlev, null_out=[n for n in FULL if n not in want])
    same(got, ref, want, want)


@pytest.mark.parametrize("hw", [15, 32])
def test_the_other_alternatives_of_the_inputs(dev, hw):
    """hfds and the sea-surface fraction as planes, no hfgeou, HI from sea_ice_fraction * ssf / (1 - land)"""
    B, T, nlev = 2, 3, 7
    inp = make_inputs(6, B, T, hw, nlev, names=PRESENT)
    got, ref = call(dev, inp, WANT_PRESENT, B, T, hw, nlev)
    same(got, ref, WANT_PRESENT, hw)
    assert got["HI"][B - 1, 0, hw - 1] == 0 and got["HI"][B - 1, 0, hw - 2] == 0          # 1 - land NaN, and 1 - land = 0


def test_nothing_wanted_is_a_no_op(dev):
    B, T, hw, nlev = 2, 2, 15, 7
    got, _ = call(dev, make_inputs(7, B, T, hw, nlev), [], B, T, hw, nlev)
    same(got, {}, [])


def test_refused_calls_write_nothing(dev):
    B, T, hw, nlev = 2, 2, 32, 7
    inp = make_inputs(8, B, T, hw, nlev)
    without = lambda *names: {k: v for k, v in inp.items() if k not in names}                           # noqa: E731
    refused = [
        dict(override=dict(nlev=0)), dict(override=dict(nlev=65)), dict(override=dict(nlev=-1)),
        dict(inp=without("hfds_total_area")),                      # hfds, the net flux and the advection lose their input
        dict(inp=without("land_fraction")), dict(inp=without("sea_ice_volume")), dict(inp=without("ocean_sea_ice_fraction")),
        dict(want=["HI"], override=dict(area_m2=None)), dict(want=["ocean_heat_content"], override=dict(dz=None)),
        dict(want=["ocean_heat_content"], override=dict(mask0=None)), dict(want=["ocean_heat_content_tendency"], override=dict(dt_seconds=0.0)),
        dict(want=["hfds"], null_out=["hfds"]), dict(override=dict(batch=0)), dict(override=dict(batch=65536)),
        dict(override=dict(steps=0)), dict(override=dict(hw=0)), dict(override=dict(t_chunk=-1)), dict(override=dict(want=1 << 7)),
        dict(inp={**inp, "hfds": inp["hfds_total_area"]}, want=["hfds"]),              # the plane exists: nothing to derive
        dict(inp={**inp, "sea_ice_fraction": inp["ocean_sea_ice_fraction"]}, want=["sea_ice_fraction"]),
    ]
    for kw in refused:
        kw = dict(kw)
        got, _ = call(dev, kw.pop("inp", inp), kw.pop("want", FULL), B, T, hw, nlev, expect=INVALID, **kw)
        for n in FULL:
            assert np.all(got[n] == SENT), (kw, n)
        assert "ace_ocean_derive_window" in lib().ace_ocean_derive_last_error().decode()
    # a missing thetao level
    one_less = dict(inp, thetao=inp["thetao"][:-1], head=inp["head"][:-1])
    got, _ = call(dev, one_less, FULL, B, T, hw, nlev, expect=INVALID)
    assert all(np.all(got[n] == SENT) for n in FULL)
    assert "level 6" in lib().ace_ocean_derive_last_error().decode()


def test_two_identical_calls_are_bitwise_equal(dev):
    B, T, hw, nlev = 2, 9, 1100, 19
    inp = make_inputs(9, B, T, hw, nlev)
    runs = [call(dev, inp, FULL, B, T, hw, nlev, layout="offset1")[0] for _ in range(2)]
    for n in FULL:
        assert np.array_equal(runs[0][n].view(np.int32), runs[1][n].view(np.int32)), n
