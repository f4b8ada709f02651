"""The cases of tests/_norm_dc.py do what the GPU tests (test_gpu_norm_dc.py) rely on: the constant reaches the targeted norm at
the stated |mean| / std in EVERY channel, and no channel is degenerate.  CPU only (fp64 oracle passes)."""

import pytest
import torch

import _norm_dc as dc

CASES = dc.grid_cases() + list(dc.LONG_RUN)


@pytest.mark.parametrize("C,hw,num_layers,site,ratio", CASES, ids=[f"C{c}-{h[0]}x{h[1]}-{s}{n}-r{r}" for c, h, n, s, r in CASES])
def test_case_realises_its_ratio(C, hw, num_layers, site, ratio):
    case = dc.make_case(C, hw, num_layers, site, ratio)
    x64 = case.rec64[case.target][0]
    med, lo, std_spread = dc.realised(x64)
    print(f"{case.target}: realised |mean|/std median {med:.2f} min {lo:.2f} (target {ratio}), std min/max {std_spread:.2f}")
    assert 0.8 * ratio <= med <= 1.25 * ratio, med
    assert lo >= 0.5 * ratio, lo
    assert std_spread >= 0.3, std_spread          # no degenerate channel: eps stays out of it
    # the constant reaches no other norm at size: instance norm removes it
    for name, (t, _) in case.rec64.items():
        if name != case.target:
            assert dc.realised(t)[0] < max(2.0, 0.1 * ratio), (name, dc.realised(t)[0])


def test_z_from_affine_is_the_norm():
    """z_from_affine with the exact affine reproduces F.instance_norm in fp64 (the measure of the GPU tests has no slack of its own)"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 6, 9, 18, generator=g, dtype=torch.float64) * 0.3 + 40.0
    gamma, beta = torch.randn(6, generator=g, dtype=torch.float64), torch.randn(6, generator=g, dtype=torch.float64)
    ref = torch.nn.functional.instance_norm(x, weight=gamma, bias=beta, eps=1e-6)
    a = gamma / torch.sqrt(x.var(dim=(2, 3), unbiased=False) + 1e-6)
    b = beta - x.mean(dim=(2, 3)) * a
    whole, chan = dc.stat_err(dc.z_from_affine(a, b, x), ref)
    assert whole <= 1e-12 and chan <= 1e-12


def test_headline_tiles_per_segment():
    """the long-run cases: no C = 128 grid up to 180 x 360 gives a conv_ws workgroup the 24 tiles per segment of the headline launches"""
    head = (dc.ws_tiles_per_segment(384, 180 * 360, True), dc.ws_tiles_per_segment(384, 180 * 360, False))
    assert head == (24, 24)
    assert dc.ws_tiles_per_segment(128, 180 * 360, True) == 8 < min(head)
