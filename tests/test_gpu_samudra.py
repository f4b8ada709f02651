"""Samudra ocean emulator on the MI355X: each lat-lon glue kernel of csrc/latlon.hip (ace_ll_*) against torch on the device, every
golden case (tests/golden/gen_samudra_*.pt, emitted by the reference) through the registry against the reference's fp64 output, graph
replay against eager, the shipped configuration at 1 degree against an fp64 torch.nn.functional evaluation of the documented
architecture, and one step of a loaded Samudra stepper."""
import copy
import datetime
import math

import pytest
import torch
import torch.nn.functional as F

import ace_amd
from ace_amd import _lib
from ace_amd.samudra import CapturedSamudraForward, Samudra
from _util import assert_net_close
from test_samudra_cpu import CASES, fp64_output, load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


@pytest.fixture(scope="module")
def gold():
    return {name: load_case(name) for name in CASES}


def _fp64_output(case):
    return fp64_output(case)


def _ok(rc):
    assert rc == 0, _lib.lib().ace_ll_last_error().decode()


def _slot(dev):
    return torch.zeros(64, dtype=torch.int32, device=dev)


def _slot_value(s):
    return float(s.view(torch.float32).max())


def _absmax_slot(x):
    s = _slot(x.device)
    assert _lib.lib().ace_hpx_absmax(x.data_ptr(), x.numel(), s.data_ptr(), _lib.current_stream()) == 0
    return s


def _decode(planes, imgs, c, rows, pitch, bound):
    """P-format planes [2][imgs][cpad / 8][rows x pitch][8] -> fp32 [imgs][c][rows][pitch] ((hi + lo) / scale)"""
    cpad = (c + 7) // 8 * 8
    n = imgs * cpad * rows * pitch
    e = 12 - math.frexp(bound)[1] if bound > 0 else 0
    v = (planes[0, :n].float() + planes[1, :n].float()) / (2.0 ** e)
    v = v.view(imgs, cpad // 8, rows * pitch, 8).permute(0, 1, 3, 2).reshape(imgs, cpad, rows, pitch)
    return v[:, :c], v[:, c:]


def _capped_gelu(v, cap):
    return torch.clamp(F.gelu(v), max=cap)


# ---- kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dil", [1, 2, 4, 8])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("circular", [True, False])
def test_pad_planes_is_fpad(dev, dil, fused, circular):
    """ace_ll_pad_planes decoded ((hi + lo) / scale) against F.pad (circular / zero longitude, zero latitude) of the same input, through
    an optional fused per-(image, channel) affine and CappedGELU; odd sizes, a pitched source, channels not a multiple of 8"""
    g = torch.Generator(device="cpu").manual_seed(dil)
    imgs, c, H, W, xp = 2, 13, 11, 23, 28
    x = torch.zeros(imgs, c, H, xp)
    x[..., :W] = 3.0 * torch.randn(imgs, c, H, W, generator=g)
    x = x.to(dev)
    ref = x[..., :W]
    ss = None
    cap = 1.5
    if fused:
        ss = torch.stack([0.5 + torch.rand(imgs, c, generator=g), torch.randn(imgs, c, generator=g)], dim=-1).to(dev).contiguous()
        ref = ref * ss[..., 0, None, None] + ss[..., 1, None, None]
        ref = _capped_gelu(ref, cap)
        bound = _slot(dev)                                        # a bound on |scale x + shift|, as ace_ll_norm_stats publishes
        bound[0] = torch.tensor(float(x.abs().max() * ss[..., 0].max() + ss[..., 1].abs().max()), device=dev).view(torch.int32)
        xmax, bscale, boff = bound, 1.0, 0.0
    else:
        xmax, bscale, boff = _absmax_slot(x), 1.0, 0.0
    refp = F.pad(ref, (dil, dil, 0, 0), mode="circular" if circular else "constant")
    refp = F.pad(refp, (0, 0, dil, dil), mode="constant")
    pitch = (W + 2 * dil + 3) // 4 * 4 + 4
    rows = H + 2 * dil
    cpad = 16
    planes = torch.full((2, imgs * cpad * rows * pitch + 16 * 8), float("nan"), dtype=torch.float16, device=dev)
    pmax = _slot(dev)
    _ok(_lib.lib().ace_ll_pad_planes(x.data_ptr(), x.stride(0), x.stride(1), xp, c, H, W, dil, int(circular), planes[0].data_ptr(),
                                     planes[1].data_ptr(), pitch, imgs, ss.data_ptr() if ss is not None else None, c if ss is not None else 0,
                                     1 if fused else 0, cap if fused else float("inf"), xmax.data_ptr(), bscale, boff, pmax.data_ptr(),
                                     _lib.current_stream()))
    torch.cuda.synchronize()
    b = _slot_value(pmax)
    got, extra = _decode(planes, imgs, c, rows, pitch, b)
    assert torch.all(planes[:, imgs * cpad * rows * pitch:] == 0)                       # slack entries
    assert torch.all(extra == 0) and torch.all(got[..., W + 2 * dil:] == 0)             # padding channels, gap columns
    err = float((got[..., : W + 2 * dil] - refp).abs().max())
    assert err <= 1e-6 * b, (err, b)
    if fused:
        assert b <= max(cap, 0.17) and b >= float(refp.abs().max())                   # the capped GELU's bound, no reduction


@pytest.mark.parametrize("mean_over_std", [1.0, 1e2, 1e4])
def test_norm_stats_without_the_cancellation_cliff(dev, mean_over_std):
    """ace_ll_norm_stats on pitched planes (gap columns hold garbage that must be ignored): the variance within 1e-6 relative of fp64,
    the emitted affine normalises, the bound covers the normalised plane"""
    g = torch.Generator(device="cpu").manual_seed(3)
    imgs, c, H, W, pitch = 2, 5, 37, 75, 80
    std = 0.7
    x = torch.randn(imgs, c, H, pitch, generator=g) * std + mean_over_std * std
    x[..., W:] = 1e30
    x = x.to(dev)
    gamma = (1.0 + 0.1 * torch.randn(c, generator=g)).to(dev)
    beta = (0.1 * torch.randn(c, generator=g)).to(dev)
    ss = torch.empty(imgs * c * 2, device=dev)
    mv = torch.empty(imgs * c * 2, device=dev)
    slot = _slot(dev)
    _ok(_lib.lib().ace_ll_norm_stats(x.data_ptr(), x.stride(0), x.stride(1), pitch, imgs, c, H, W, 1e-5, gamma.data_ptr(), beta.data_ptr(),
                                     ss.data_ptr(), mv.data_ptr(), slot.data_ptr(), _lib.current_stream()))
    torch.cuda.synchronize()
    xd = x[..., :W].double()
    mean = xd.mean(dim=(-2, -1))
    var = xd.var(dim=(-2, -1), unbiased=False)
    mv = mv.view(imgs, c, 2).double()
    assert float(((mv[..., 1] - var) / var).abs().max()) <= 1e-6
    assert float(((mv[..., 0] - mean) / mean.abs()).abs().max()) <= 1e-7
    ss = ss.view(imgs, c, 2).double()
    ref = (xd - mean[..., None, None]) / torch.sqrt(var[..., None, None] + 1e-5) * gamma.double()[:, None, None] + beta.double()[:, None, None]
    y = xd * ss[..., 0, None, None] + ss[..., 1, None, None]
    assert float((y - ref).abs().max()) <= 1e-6 * mean_over_std + 1e-6
    assert _slot_value(slot) >= float(ref.abs().max())


def test_pool2_odd_sizes(dev):
    """AvgPool2d(2) with floor at odd H / W into a wider output pitch: interior equal to torch, gap columns zero, bound = max|y|"""
    x = torch.randn(3, 4, 23, 48, device=dev)
    W = 45
    y = torch.full((3, 4, 11, 28), float("nan"), device=dev)
    slot = _slot(dev)
    _ok(_lib.lib().ace_ll_pool2(x.data_ptr(), y.data_ptr(), 12, 23, W, 48, 23 * 48, 28, 11 * 28, slot.data_ptr(), _lib.current_stream()))
    torch.cuda.synchronize()
    ref = F.avg_pool2d(x[..., :W], 2)
    assert ref.shape[-2:] == (11, 22)
    assert torch.equal(y[..., :22], ref)
    assert torch.all(y[..., 22:] == 0)
    assert _slot_value(slot) == float(ref.abs().max())


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("circular", [True, False])
@pytest.mark.parametrize("hw, HW", [((11, 22), (22, 45)), ((5, 11), (11, 23)), ((8, 8), (16, 16))])
def test_upsample2_add(dev, periodic, circular, hw, HW):
    """bilinear x 2 (align_corners false; the reference's ZonallyPeriodicBilinearUpsample when periodic), padded to the skip's shape
    ((p // 2, p - p // 2): circular / zero in longitude, zero in latitude) plus the skip"""
    (h, w), (H, W) = hw, HW
    px, ps = (w + 3) // 4 * 4 + 4, (W + 3) // 4 * 4
    x = torch.randn(2, 3, h, px, device=dev)
    skip = torch.randn(2, 3, H, ps, device=dev)
    skip[..., W:] = 0
    y = torch.full((2, 3, H, ps), float("nan"), device=dev)
    slot = _slot(dev)
    _ok(_lib.lib().ace_ll_upsample2_add(x.data_ptr(), 6, h, w, px, h * px, skip.data_ptr(), ps, H * ps, y.data_ptr(), H, W, ps, H * ps,
                                        int(circular), int(periodic), slot.data_ptr(), _lib.current_stream()))
    torch.cuda.synchronize()
    xi = x[..., :w].double()
    if periodic:
        up = F.interpolate(F.pad(xi, (1, 1, 0, 0), mode="circular"), scale_factor=2, mode="bilinear", align_corners=False)[..., 2:2 + 2 * w]
    else:
        up = F.interpolate(xi, scale_factor=2, mode="bilinear", align_corners=False)
    pr, pc = H - 2 * h, W - 2 * w
    up = F.pad(up, (pc // 2, pc - pc // 2, 0, 0), mode="circular" if circular else "constant")
    up = F.pad(up, (0, 0, pr // 2, pr - pr // 2), mode="constant")
    ref = up + skip[..., :W].double()
    assert float((y[..., :W].double() - ref).abs().max()) <= 1e-6
    assert torch.all(y[..., W:] == 0)
    assert _slot_value(slot) >= float(y.abs().max())


# ---- the network -------------------------------------------------------------------------------------------------------
def _net(case, dev):
    net = ace_amd.ModuleSelector(type="Samudra", config=case["config"]).build(case["n_in"], case["n_out"],
                                                                              ace_amd.DatasetInfo((case["H"], case["W"]))).torch_module
    net.load_state_dict(case["state_dict"], strict=True)
    return net.to(dev).eval()


@pytest.mark.parametrize("name", CASES)
def test_samudra_golden_vs_reference(dev, gold, name):
    """every golden case through the registry with the reference's weights against the reference's fp64 output (1e-5 of the output
    maximum, channel by channel within 3e-5); two forwards are bitwise equal"""
    case = gold[name]
    net = _net(case, dev)
    x = case["input"].float().to(dev)
    with torch.no_grad():
        y = net(x)
        y2 = net(x)
    torch.cuda.synchronize()
    assert y.shape == case["output_fp32"].shape
    assert torch.equal(y, y2)
    assert_net_close(y, _fp64_output(case), 1e-5, what=name)


def test_samudra_graph_replay_is_eager(dev, gold):
    case = gold["l4_instance_circular"]
    net = _net(case, dev)
    x = case["input"].float().to(dev)
    with torch.no_grad():
        eager = net(x).clone()
    cap = CapturedSamudraForward(net, x)
    y = cap(x).clone()
    x2 = x.flip(-1).contiguous()
    y2 = cap(x2).clone()
    with torch.no_grad():
        e2 = net(x2)
    torch.cuda.synchronize()
    assert torch.equal(y, eager)
    assert torch.equal(y2, e2)


# ---- the shipped configuration --------------------------------------------------------------------------------------------------
def _f_block(x, p, d, norm_eps, pad):
    """the documented ConvNeXt block, fp64: skip + 1x1( CappedGELU(IN(conv(pad(CappedGELU(IN(conv(pad(x)))))))) )"""
    def padll(v):
        v = F.pad(v, (d, d, 0, 0), mode=pad)
        return F.pad(v, (0, 0, d, d), mode="constant")
    skip = F.conv2d(x, p["skip.w"], p["skip.b"]) if "skip.w" in p else x
    h = F.conv2d(padll(x), p["c1.w"], p["c1.b"], dilation=d)
    h = torch.clamp(F.gelu(F.instance_norm(h, eps=norm_eps)), max=p["cap1"])
    h = F.conv2d(padll(h), p["c2.w"], p["c2.b"], dilation=d)
    h = torch.clamp(F.gelu(F.instance_norm(h, eps=norm_eps)), max=p["cap2"])
    return skip + F.conv2d(h, p["c3.w"], p["c3.b"])


def _f_samudra(x, net):
    """fp64 torch.nn.functional evaluation of the architecture from the module's parameters"""
    def params(blk):
        p = {}
        if blk.skip_module is not None:
            p["skip.w"], p["skip.b"] = blk.skip_module.weight.double(), blk.skip_module.bias.double()
        c1, _, a1, c2, _, a2, c3 = blk.stages()
        for k, c in (("c1", c1), ("c2", c2), ("c3", c3)):
            p[k + ".w"], p[k + ".b"] = c.weight.double(), c.bias.double()
        p["cap1"], p["cap2"] = float(a1.cap), float(a2.cap)
        return p

    n = net.num_steps
    blocks = net.blocks_by_level()
    skips = []
    for i in range(n):
        blk = blocks[i][0]
        x = _f_block(x, params(blk), blk.dil, 1e-5, net.pad)
        skips.append(x)
        x = F.avg_pool2d(x, 2)
    x = _f_block(x, params(blocks[n][0]), blocks[n][0].dil, 1e-5, net.pad)
    for j in range(n):
        s = skips[n - 1 - j]
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        pr, pc = s.shape[-2] - x.shape[-2], s.shape[-1] - x.shape[-1]
        x = F.pad(x, (pc // 2, pc - pc // 2, 0, 0), mode=net.pad)
        x = F.pad(x, (0, 0, pr // 2, pr - pr // 2), mode="constant") + s
        blk = blocks[n + 1 + j][0]
        x = _f_block(x, params(blk), blk.dil, 1e-5, net.pad)
    conv = net.layers[4 * n + 1]
    x = F.pad(F.pad(x, (1, 1, 0, 0), mode=net.pad), (0, 0, 1, 1), mode="constant")
    return F.conv2d(x, conv.weight.double(), conv.bias.double())


def test_samudra_shipped_configuration_full_size(dev):
    """90 -> 80 channels, ch_width [200, 250, 300, 400], dilation [1, 2, 4, 8], instance norm, 180 x 360, seeded weights: the native
    forward within 1e-5 of the output maximum of an fp64 functional evaluation (run on the device with the native-kernel-free
    convolution path of torch)"""
    torch.manual_seed(0)
    net = ace_amd.ModuleSelector(type="Samudra", config={}).build(90, 80, ace_amd.DatasetInfo((180, 360))).torch_module
    with torch.no_grad():
        for m in net.modules():
            if type(m).__name__ == "CappedGELU":
                m.cap.fill_(3.0)
    net = net.to(dev).eval()
    x = torch.randn(1, 90, 180, 360, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        y = net(x)
        with torch.backends.cudnn.flags(enabled=False):
            ref = _f_samudra(x.double(), net)
    torch.cuda.synchronize()
    assert y.shape == (1, 80, 180, 360)
    err = float((y.double() - ref).abs().max() / ref.abs().max())
    assert err <= 1e-5, err


def test_samudra_stepper_step(dev, gold):
    """one step of a loaded Samudra stepper (no corrector) = normalise -> the golden network -> denormalise"""
    from ace_amd.checkpoint import load_stepper
    from test_samudra_cpu import _stepper_state
    case = gold["l1_width_mod8_4"]
    state = _stepper_state(case)
    loaded = load_stepper(state, device=dev)
    stepper = loaded.stepper
    stepper.set_eval()
    names = [f"v{i}" for i in range(case["n_in"])]
    means = {n: 0.1 * i for i, n in enumerate(names)}
    stds = {n: 1.0 + 0.5 * i for i, n in enumerate(names)}
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, case["H"], case["W"]
    ic = {n: torch.randn(B, 1, H, W, generator=g).to(dev) for n in names[: case["n_out"]]}
    forcing = {n: torch.randn(B, 2, H, W, generator=g).to(dev) for n in names[case["n_out"]:]}
    out, _ = stepper.predict(ic, forcing)
    net = _net(case, dev)
    xin = torch.stack([((ic[n][:, 0] if n in ic else forcing[n][:, 0]) - means[n]) / stds[n] for n in names], dim=1)
    with torch.no_grad():
        y = net(xin)
    for i, n in enumerate(names[: case["n_out"]]):
        ref = y[:, i] * stds[n] + means[n]
        got = out[n][:, -1]
        assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max()), n
