"""The fused instance-norm statistics against fp64 truth when the normalised tensor carries a large per-channel mean.

The forward makes no pass over a tensor for its instance norm: the producing kernel accumulates per-row partial statistics in its
epilogue (conv_ws.hip inner skip / fc2 / encoder, the tile engine's 64-column epilogue in kernels.hip) and
`instnorm_finalize_kernel` merges them.  An error of the variance is multiplied by (mean / std)^2, and the per-block taps hardly see
it (the std-0.02 MLP behind norm1 attenuates it about 20 x), so these tests read the affine (scale, shift) the network actually used
(`ace_sfno_norm_affine`) and apply it to the fp64 oracle's norm input:

  (a) statistic:  err = max|a x64 + b - z64| / max|z64|  <=  max(OP_TOL, 4 floor), overall and per channel.  floor is the same measure
      of the fp32 ORACLE's norm output (two-pass fp32 statistics), never of the code under test.  4 = 2 (reference and kernel round
      the same fp32 data in different orders) x 2 (the kernel's input carries the rounding of its producer).
  (b) bound:      max|z64| (1 - 1e-6) <= published range bound <= 2^14 max|z64|  (below: the fp16 hi plane overflows; above: the
      22-bit hi / lo split loses bits)
  (c) end to end: taps and output against the fp64 oracle, bar max(NET_TOL, m floor_tap), m = 2 for fp32 and 8 for f16x3
      (the same 2, times 2^(24 - 22) for the 22-bit operands that hold the un-normalised stream).

Cases: tests/_norm_dc.py (their conditions are asserted without a GPU in test_norm_dc_cpu.py).  Every test prints its figures."""

import ctypes

import pytest
import torch

import _norm_dc as dc
from _util import build_native_net, rel_max

pytestmark = pytest.mark.gpu

OP_TOL = 2e-6
NET_TOL = 1e-5

ROUTINGS = {            # name -> (precision, ACE_CONV_WS)
    "f16x3-ws": ("f16x3", None),          # default: the partials come from conv_ws.hip
    "f16x3-tile": ("f16x3", "none"),      # ... from the tile engine's 64-column epilogue
    "f16x3-mixed": ("f16x3", "skip,fc2"),
    "fp32": ("fp32", None),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def norm_affine(net, which, B, C):
    from ace_amd import _lib
    a, b = torch.empty(B, C), torch.empty(B, C)
    bound = ctypes.c_float(0.0)
    fp = ctypes.POINTER(ctypes.c_float)
    _lib.check(_lib.lib().ace_sfno_norm_affine(net._native, which, ctypes.cast(a.data_ptr(), fp), ctypes.cast(b.data_ptr(), fp),
                                               ctypes.byref(bound)))
    return a, b, bound.value


def check_case(dev, monkeypatch, C, hw, num_layers, site, ratio, routing):
    precision, conv_ws = ROUTINGS[routing]
    if conv_ws is not None:
        monkeypatch.setenv("ACE_CONV_WS", conv_ws)
    case = dc.make_case(C, hw, num_layers, site, ratio)
    which = 1 if case.target.endswith("norm1") else 0
    assert case.target.startswith(f"blocks.{num_layers - 1}."), "the query reads the LAST block's tables"
    net = build_native_net(case.cfg, case.state, dev, precision)
    xd = case.x.to(dev)
    with torch.no_grad():
        y = net(xd).clone()          # the routing a product forward takes (taps switch the planes-only residual stream off)
        a, b, bound = norm_affine(net, which, dc.BATCH, C)
        _, taps = net.forward_with_taps(xd)
    x64, z64 = case.rec64[case.target]
    tag = f"C{C} {hw[0]}x{hw[1]} {site}/{num_layers} ratio {ratio} {routing}"
    failures = []
    # (a)
    err, err_c = dc.stat_err(dc.z_from_affine(a, b, x64), z64)
    floor, floor_c = dc.floor_of(case, case.target)
    bar, bar_c = max(OP_TOL, 4 * floor), max(OP_TOL, 4 * floor_c)
    print(f"NORMDC {tag} | (a) err {err:.3e} floor {floor:.3e} bar {bar:.3e} | per-channel err {err_c:.3e} floor {floor_c:.3e} bar {bar_c:.3e}")
    if not (err <= bar and err_c <= bar_c):
        failures.append(f"(a) statistic: err {err:.3e} > bar {bar:.3e} or per-channel {err_c:.3e} > {bar_c:.3e}")
    # (b)
    zmax = float(z64.abs().max())
    if precision == "f16x3":
        print(f"NORMDC {tag} | (b) bound {bound:.4e} max|z64| {zmax:.4e} ratio {bound / zmax:.3f}")
        if not (zmax * (1 - 1e-6) <= bound <= 2.0**14 * zmax):
            failures.append(f"(b) bound {bound:.4e} outside [1 - 1e-6, 2^14] x max|z64| = {zmax:.4e}")
    else:
        assert bound == -1.0, bound   # the fp32 engines scale nothing: no bound is published
    # (c)
    m = 8 if precision == "f16x3" else 2
    pairs = [(f"tap {i}", taps[i + 1], case.taps64[i], case.taps32[i]) for i in range(num_layers)] + [("out", y, case.y64, case.y32)]
    for name, got, want, want32 in pairs:
        e, fl = rel_max(got, want), rel_max(want32, want)
        barc = max(NET_TOL, m * fl)
        print(f"NORMDC {tag} | (c) {name} err {e:.3e} floor {fl:.3e} bar {barc:.3e}")
        if not e <= barc:
            failures.append(f"(c) {name}: err {e:.3e} > bar {barc:.3e}")
    assert not failures, (tag, failures)


GRID = dc.grid_cases()
IDS = [f"C{c}-{h[0]}x{h[1]}-{s}{n}-r{r}" for c, h, n, s, r in GRID]


@pytest.mark.parametrize("routing", ["f16x3-ws", "f16x3-tile", "fp32"])
@pytest.mark.parametrize("C,hw,num_layers,site,ratio", GRID, ids=IDS)
def test_norm_statistics_under_a_large_mean(dev, monkeypatch, C, hw, num_layers, site, ratio, routing):
    """Sites x depth x ratio at the shapes of _norm_dc.SHAPES, batch 2.

    One block: norm0 fed by the encoder, norm1 by the inner skip.  Two blocks: norm0 fed by fc2's epilogue."""
    check_case(dev, monkeypatch, C, hw, num_layers, site, ratio, routing)


def test_norm_statistics_mixed_engines(dev, monkeypatch):
    """inner skip and fc2 on conv_ws.hip, fc1 on the tile engine: the partials of the two engines' layouts meet"""
    check_case(dev, monkeypatch, 128, (24, 48), 2, "h1", 300, "f16x3-mixed")


@pytest.mark.parametrize("C,hw,num_layers,site,ratio", dc.LONG_RUN, ids=[f"{s}{n}" for _, _, n, s, _ in dc.LONG_RUN])
def test_norm_statistics_long_accumulation_run(dev, monkeypatch, C, hw, num_layers, site, ratio):
    """A conv_ws workgroup's fp32 running statistics over its longest pixel run.  The headline 384 x 180 x 360 launches give a
    workgroup 24 pixel tiles per segment; at C = 128 (one channel slice, 32 groups per XCD) no grid up to 180 x 360 reaches that, so
    this is 180 x 360, the longest run a C = 128 net of the suite has."""
    here = dc.ws_tiles_per_segment(C, hw[0] * hw[1], True)
    head = (dc.ws_tiles_per_segment(384, 180 * 360, True), dc.ws_tiles_per_segment(384, 180 * 360, False))
    print(f"NORMDC tiles per segment: this case {here}; headline inner skip {head[0]}, fc2 {head[1]}")
    check_case(dev, monkeypatch, C, hw, num_layers, site, ratio, "f16x3-ws")


def test_bound_at_zero_mean_on_the_quarter_degree_grid(dev):
    """(b) where the analytic bound |a| sqrt(HW var) + |beta| is loosest (sqrt(HW) grows with the grid): 721 x 1440, C = 8, one block,
    no constant added.  Truth: F.instance_norm in fp64 on the kernel's own fp32 norm input (the encoder tap = input of blocks.0.norm0).
    At C = 8 no convolution is on conv_ws.hip, so this norm0 takes its statistics - and its bound, the true extremes - from
    instnorm_stats_kernel; the analytic bound is held at 180 x 360 by the long-run cases (50 - 60 x the true maximum there)."""
    from oracle.sfno import SFNOConfig, init_state
    H, W, C = 721, 1440, 8
    cfg = SFNOConfig(in_chans=3, out_chans=2, img_shape=(H, W), embed_dim=C, num_layers=1, operator_type="dhconv")
    st = init_state(cfg, seed=5)
    x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(6))
    net = build_native_net(cfg, st, dev, "f16x3")
    with torch.no_grad():
        _, taps = net.forward_with_taps(x.to(dev))
        a, b, bound = norm_affine(net, 0, 1, C)
    h = taps[0].cpu().double()
    z64 = torch.nn.functional.instance_norm(h, weight=st["blocks.0.norm0.weight"].double(), bias=st["blocks.0.norm0.bias"].double(), eps=1e-6)
    zmax = float(z64.abs().max())
    err, err_c = dc.stat_err(dc.z_from_affine(a, b, h), z64)
    print(f"NORMDC 721x1440 C8 zero mean | (b) bound {bound:.4e} max|z64| {zmax:.4e} ratio {bound / zmax:.1f} | (a) err {err:.3e} per-channel {err_c:.3e}")
    assert zmax * (1 - 1e-6) <= bound <= 2.0**14 * zmax, (bound, zmax)
    assert err <= OP_TOL and err_c <= OP_TOL, (err, err_c)   # exact fp32 data, fp64 truth on the same data: the operator bar
