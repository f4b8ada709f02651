"""ace_mask_planes, ace_mask_pack_normalize (csrc/masking.hip), ace_pack_normalize and ace_unpack_denormalize (csrc/kernels.hip)
through the C ABI, at every shape and layout their grids and their vector path branch on: a plane below a wave, ragged grid-stride
trips, the 64-workgroup cap (scalar: HW > 65536; float4: HW / 4 > 16384 threads), and the per-(plane, sample) alignment test -
a source base one float off, a per-sample stride = 1 (mod 4) that sends sample 0 down the float4 path and samples 1 and 2 down the
scalar one in the same launch, a hit plane one byte off.

The reference is the same expressions in torch fp32 ON THE CPU - hit = round(mask).to(int64) == mask_value,
where(hit, fill, src), (v - mu) / sd, y * sd + mu with two roundings each - not another kernel of this project.  Masked and staged
planes are compared bitwise, NaN payloads included; normalised and denormalised values bitwise where they are numbers and as NaN
where they are NaN.  Sources hold +-0, +-inf and NaNs with payloads, no subnormals (their flushing is the build's, not these
kernels').  Every buffer is compared whole - the gaps between the samples of a strided plane and the guard floats around it too -
so a source that is not also a destination comes back bitwise and nothing is written outside a plane."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
GUARD = -777.0
SHAPES = [(5, 7), (33, 35), (257, 257), (32, 36), (256, 256), (180, 365)]
MASK_VALUES = torch.tensor([0.0, 0.49, 0.5, 0.51, 1.0, 1.5, 2.5, float("nan")])
SPECIALS = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x7fc12345, 0xffc00abc], dtype=np.uint32).view(np.int32)


def _layouts(hw, masked):
    if (hw[0] * hw[1]) % 4:
        return [(hw, "window")]
    return [(hw, lay) for lay in ["window", "base_off", "stride_1mod4"] + (["hits_off"] if masked else [])]


def _id(v):
    return "%dx%d-%s" % (v[0][0], v[0][1], v[1])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _lib():
    from ace_amd import _lib as L
    return L.lib(), L.current_stream()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_numbers(got, want):
    """bitwise where ``want`` is a number, NaN where it is NaN"""
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(_bits(got)[~nan], _bits(want)[~nan])


def _values(g, HW):
    """(B, HW) normal draws with every special value in each sample, one of them in the last element"""
    v = torch.randn(B, HW, generator=g) * 3.0 + 1.0
    bits = v.view(torch.int32)
    for b in range(B):
        pos = torch.randperm(HW - 1, generator=g)[:min(HW - 1, 2 * len(SPECIALS))]
        bits[b, pos] = torch.from_numpy(np.resize(SPECIALS, len(pos)))
        bits[b, HW - 1] = int(SPECIALS[(b + 1) % len(SPECIALS)])
    return v


class Plane:
    """(B, HW) values inside a flat buffer of guard floats: sample b at offset + b * stride.  ``host`` is what the buffer held at
    the start (and, edited through ``expect``, what it should hold at the end), ``device`` its copy for the kernel."""

    def __init__(self, dev, values, HW, layout, off_base=False):
        self.HW = HW
        self.stride = 2 * HW + (1 if layout == "stride_1mod4" else 0)      # a step of a two-step window
        self.offset = 4 + (1 if off_base else 0)
        self.host = torch.full((self.offset + (B - 1) * self.stride + HW + 4,), GUARD)
        if values is not None:
            self.expect().copy_(values)
        self.device = self.host.to(dev)
        assert self.device.data_ptr() % 16 == 0
        self.ptr = self.device.data_ptr() + 4 * self.offset

    def expect(self):
        return self.host.as_strided((B, self.HW), (self.stride, 1), self.offset)

    def check(self, what, numbers_only=False):
        got = self.device.cpu()
        assert (_same_numbers if numbers_only else lambda a, b: torch.equal(_bits(a), _bits(b)))(got, self.host), what


def _i64(dev, values):
    return torch.tensor(values, dtype=torch.int64, device=dev)


def _hits(g, dev, HW, off):
    """two hit planes (mask values 0 and 1) as the caller computes them, on the CPU; ``off``: the table starts one byte off"""
    masks = MASK_VALUES[torch.randint(0, len(MASK_VALUES), (2, HW), generator=g)]
    hit = torch.stack([torch.round(masks[0]).to(torch.int64) == 0, torch.round(masks[1]).to(torch.int64) == 1])
    assert hit.any() and not hit.all()
    start = 1 if off else 0
    buf = torch.zeros(2 * HW + 16, dtype=torch.uint8)
    buf[start:start + 2 * HW] = hit.reshape(-1).to(torch.uint8)
    d = buf.to(dev)
    assert d.data_ptr() % 4 == 0
    return hit, d, d.data_ptr() + start


@pytest.mark.parametrize("case", [c for hw in SHAPES for c in _layouts(hw, True)], ids=_id)
def test_mask_planes(dev, case):
    (H, W), layout = case
    HW = H * W
    g = torch.Generator().manual_seed(HW)
    hit, hits_dev, hits_ptr = _hits(g, dev, HW, layout == "hits_off")
    nmask = 2
    # plane: (hit plane index, in place?)   -1 and nmask both mean unmasked
    plan = [(0, True), (1, False), (-1, True), (-1, False), (nmask, False), (0, False), (nmask + 5, True)]
    fill = torch.tensor([0.3, -1.5, 9.0, 9.0, 9.0, float("nan"), 9.0])
    srcs = [Plane(dev, _values(g, HW), HW, layout, off_base=layout == "base_off") for _ in plan]
    dsts = [s if inplace else Plane(dev, None, HW, layout) for s, (_, inplace) in zip(srcs, plan)]
    for j, (m, inplace) in enumerate(plan):
        v = srcs[j].expect().clone()
        dsts[j].expect().copy_(torch.where(hit[m], fill[j], v) if 0 <= m < nmask else v)
    tab = _i64(dev, [s.ptr for s in srcs] + [s.stride for s in srcs] + [d.ptr for d in dsts] + [d.stride for d in dsts])
    idx = torch.tensor([m for m, _ in plan], dtype=torch.int32, device=dev)
    fill_dev = fill.to(dev)
    n = len(plan)
    L, stream = _lib()
    a = tab.data_ptr()
    assert L.ace_mask_planes(a, a + 8 * n, a + 16 * n, a + 24 * n, idx.data_ptr(), hits_ptr, nmask, fill_dev.data_ptr(), n, B, HW,
                             stream) == 0, L.ace_mask_last_error()
    torch.cuda.synchronize()
    for j, (m, inplace) in enumerate(plan):
        dsts[j].check(("destination", j, m, inplace))
        srcs[j].check(("source", j, m, inplace))


@pytest.mark.parametrize("case", [c for hw in SHAPES for c in _layouts(hw, True)], ids=_id)
def test_mask_pack_normalize(dev, case):
    (H, W), layout = case
    HW = H * W
    g = torch.Generator().manual_seed(HW + 1)
    hit, hits_dev, hits_ptr = _hits(g, dev, HW, layout == "hits_off")
    nmask, npack = 2, 4
    # plane: (hit plane index, stage: None, "own" = a separate plane, "src" = the source itself); planes >= npack are staged only
    plan = [(0, None), (1, "own"), (-1, "src"), (nmask, "own"), (0, "src"), (-1, "own"), (1, None)]
    fill = torch.tensor([0.3, float("nan"), 9.0, 9.0, -1.5, 9.0, 4.0])
    mean = torch.tensor([0.0, 0.5, -1.5, 2.0])
    std = torch.tensor([1.0, 1.3, 0.7, 2.5])
    srcs = [Plane(dev, _values(g, HW), HW, layout, off_base=layout == "base_off") for _ in plan]
    stages = [None if st is None else s if st == "src" else Plane(dev, None, HW, layout) for s, (_, st) in zip(srcs, plan)]
    x = torch.full((B, npack, HW), GUARD)
    for j, (m, st) in enumerate(plan):
        v = srcs[j].expect().clone()
        v = torch.where(hit[m], fill[j], v) if 0 <= m < nmask else v
        if stages[j] is not None:
            stages[j].expect().copy_(v)
        if j < npack:
            x[:, j] = (v - mean[j]) / std[j]
    tab = _i64(dev, [s.ptr for s in srcs] + [s.stride for s in srcs] + [0 if s is None else s.ptr for s in stages]
               + [0 if s is None else s.stride for s in stages])
    idx = torch.tensor([m for m, _ in plan], dtype=torch.int32, device=dev)
    fill_dev, mean_dev, std_dev = fill.to(dev), mean.to(dev), std.to(dev)
    x_dev = torch.full((B, npack, HW), GUARD, device=dev)
    n = len(plan)
    L, stream = _lib()
    a = tab.data_ptr()
    assert L.ace_mask_pack_normalize(a, a + 8 * n, idx.data_ptr(), hits_ptr, nmask, fill_dev.data_ptr(), a + 16 * n, a + 24 * n,
                                     mean_dev.data_ptr(), std_dev.data_ptr(), x_dev.data_ptr(), npack, n, B, HW, stream) == 0, \
        L.ace_mask_last_error()
    torch.cuda.synchronize()
    got = x_dev.cpu()
    for j in range(npack):
        assert _same_numbers(got[:, j], x[:, j]), ("packed", j)
    for j, (m, st) in enumerate(plan):
        if stages[j] is not None:
            stages[j].check(("stage", j, m, st))
        srcs[j].check(("source", j, m, st))
    # no stage table at all: the packed planes alone, the same bits
    x_dev.fill_(GUARD)
    assert L.ace_mask_pack_normalize(a, a + 8 * n, idx.data_ptr(), hits_ptr, nmask, fill_dev.data_ptr(), None, None,
                                     mean_dev.data_ptr(), std_dev.data_ptr(), x_dev.data_ptr(), npack, npack, B, HW, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(x_dev.cpu()), _bits(got))
    for j in range(n):
        srcs[j].check(("source, no stage", j))


@pytest.mark.parametrize("case", [c for hw in SHAPES for c in _layouts(hw, False)], ids=_id)
def test_pack_normalize(dev, case):
    from ace_amd import _lib as lib
    (H, W), layout = case
    HW = H * W
    g = torch.Generator().manual_seed(HW + 2)
    mean = torch.tensor([0.0, 0.5, -1.5])
    std = torch.tensor([1.0, 1.3, 0.7])
    nch = len(mean)
    srcs = [Plane(dev, _values(g, HW), HW, layout, off_base=layout == "base_off") for _ in range(nch)]
    want = torch.stack([(s.expect() - mean[j]) / std[j] for j, s in enumerate(srcs)], dim=1)
    tab = _i64(dev, [s.ptr for s in srcs] + [s.stride for s in srcs])
    mean_dev, std_dev = mean.to(dev), std.to(dev)
    x_dev = torch.full((B, nch, HW), GUARD, device=dev)
    L, stream = _lib()
    lib.check(L.ace_pack_normalize(tab.data_ptr(), tab.data_ptr() + 8 * nch, mean_dev.data_ptr(), std_dev.data_ptr(),
                                   x_dev.data_ptr(), B, nch, HW, stream))
    torch.cuda.synchronize()
    got = x_dev.cpu()
    for j in range(nch):
        assert _same_numbers(got[:, j], want[:, j]), ("packed", j)
    for j, s in enumerate(srcs):
        s.check(("source", j))


@pytest.mark.parametrize("case", [c for hw in SHAPES for c in _layouts(hw, False)], ids=_id)
def test_unpack_denormalize(dev, case):
    from ace_amd import _lib as lib
    (H, W), layout = case
    HW = H * W
    g = torch.Generator().manual_seed(HW + 3)
    mean = torch.tensor([0.0, 0.5, -1.5])
    std = torch.tensor([1.0, 1.3, 0.7])
    nch = len(mean)
    y = torch.stack([_values(g, HW) for _ in range(nch)], dim=1)           # (B, nch, HW)
    dsts = [Plane(dev, None, HW, layout, off_base=layout == "base_off") for _ in range(nch)]
    for j, d in enumerate(dsts):
        d.expect().copy_(y[:, j] * std[j] + mean[j])
    tab = _i64(dev, [d.ptr for d in dsts] + [d.stride for d in dsts])
    mean_dev, std_dev, y_dev = mean.to(dev), std.to(dev), y.to(dev)
    L, stream = _lib()
    lib.check(L.ace_unpack_denormalize(y_dev.data_ptr(), mean_dev.data_ptr(), std_dev.data_ptr(), tab.data_ptr(),
                                       tab.data_ptr() + 8 * nch, B, nch, HW, stream))
    torch.cuda.synchronize()
    for j, d in enumerate(dsts):
        d.check(("destination", j), numbers_only=True)
    assert torch.equal(_bits(y_dev.cpu()), _bits(y))
