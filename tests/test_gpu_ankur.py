"""AnkurLocalNet on the device: every golden case (tests/golden/gen_ankur_*.pt; with and without the DISCO encoder, with and without
the positional embedding, ReLU / GELU / SiLU) within 2 x the reference's own fp32 error of the fp64 truth; with ReLU bit for bit
the composed statements (tests/_disco_ref.py, tests/_pixel_mlp_ref2.py); two forwards bitwise equal; ``forward_into`` without an
allocation; ``Stepper.predict`` over 3 steps from a checkpoint built here equal to the module applied by hand.

Measured on an MI355X, max |y - truth| / max |truth|, kernel / reference: disco_gelu 2.5e-7 / 2.6e-7, disco_relu_embed
2.3e-7 / 2.9e-7, disco_silu_embed 1.3e-7 / 1.2e-7, depthwise_relu 2.3e-7 / 2.6e-7, conv_gelu_embed 2.6e-7 / 3.3e-7,
conv_relu_embed 2.0e-7 / 2.1e-7."""
import pytest
import torch

import ace_amd

import _ankur_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", C.CASES)
def test_module_matches_the_truth_and_the_statement(dev, name):
    c = C.case(name)
    net = C.build(c, dev)
    x = c["input"].to(dev)
    with torch.no_grad():
        y = net(x).clone()
        again = net(x, labels=None)
    torch.cuda.synchronize()
    err = C.rel_err(y.cpu(), c["output64"])
    print(f"{name}: kernel vs fp64 {err:.3e}; reference fp32 vs fp64 {c['reference_error']:.3e}")
    assert err <= 2 * c["reference_error"], (name, err, c["reference_error"])
    assert C.bits_equal(y, again)
    if "statement" in c:
        assert C.bits_equal(y, c["statement"])


@pytest.mark.parametrize("name", ["disco_relu_embed", "conv_gelu_embed"])
def test_forward_into_allocates_nothing_after_the_first_call(dev, name):
    c = C.case(name)
    net = C.build(c, dev)
    x = c["input"].to(dev)
    y = torch.empty(x.shape[0], c["n_out_channels"], *c["img_shape"], device=dev)
    with torch.no_grad():
        net.forward_into(x, y)
        torch.cuda.synchronize()
        first = y.clone()
        before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
        net.forward_into(x, y)
        after = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    assert after == before and C.bits_equal(y, first)


def test_weights_changed_in_place_are_picked_up(dev):
    c = C.case("disco_relu_embed")
    net = C.build(c, dev)
    x = c["input"].to(dev)
    with torch.no_grad():
        y0 = net(x).clone()
        net.module.mlp[0].conv.weight.mul_(2.0)
        y1 = net(x).clone()
        net.load_state_dict(c["state_dict"])
        y2 = net(x)
    assert not torch.equal(y0, y1) and C.bits_equal(y2, y0) and C.bits_equal(y0, c["statement"])


def test_stepper_predict_equals_the_module_applied_by_hand(dev):
    from ace_amd.checkpoint import load_stepper
    name = "disco_relu_embed"
    ck, in_names, out_names = C.checkpoint(name)
    c = C.case(name)
    stepper = load_stepper(ck, device=dev).stepper
    net = stepper._step_obj.module.torch_module
    assert isinstance(net, ace_amd.AnkurLocalNet)
    H, W = c["img_shape"]
    T = 3
    g = torch.Generator().manual_seed(3)
    forcing_names = [n for n in in_names if n not in out_names]
    ic = {n: torch.randn(2, 1, H, W, generator=g).to(dev) for n in out_names}
    forcing = {n: torch.randn(2, T + 1, H, W, generator=g).to(dev) for n in forcing_names}
    out, _ = stepper.predict(ic, forcing)
    norm = ck["stepper"]["config"]["step"]["config"]["normalization"]["network"]
    mean = lambda names: torch.tensor([norm["means"][n] for n in names], device=dev).view(1, -1, 1, 1)     # noqa: E731
    std = lambda names: torch.tensor([norm["stds"][n] for n in names], device=dev).view(1, -1, 1, 1)       # noqa: E731
    state = torch.cat([ic[n][:, 0:1] for n in out_names], dim=1)
    worst = 0.0
    with torch.no_grad():
        for s in range(T):
            x = torch.cat([state] + [forcing[n][:, s:s + 1] for n in forcing_names], dim=1)
            y = net((x - mean(in_names)) / std(in_names))
            state = y * std(out_names) + mean(out_names)
            for i, n in enumerate(out_names):
                assert out[n].shape == (2, T, H, W)
                worst = max(worst, float((out[n][:, s] - state[:, i]).abs().max() / state[:, i].abs().max()))
    print(f"stepper.predict against the module by hand, worst relative difference over {T} steps: {worst:.3e}")
    assert worst == 0.0
