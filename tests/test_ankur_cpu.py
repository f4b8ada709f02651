"""AnkurLocalNet on the host (``-m "not gpu"``): the registry entry with the reference's fields and defaults, the reference's
state-dict layout loaded strictly, a ``load_stepper`` round trip, the refusals, and the module's handle life on an emulation of the
C ABI (tests/_fake_ankur.py: the headers' statements behind the real host code) against the reference's own outputs
(tests/golden/gen_ankur_*.pt)."""
import dataclasses
import gc

import pytest
import torch

import ace_amd

import _ankur_cases as C
from _fake_ankur import fake_ankur


def test_registry_type_fields_and_defaults():
    from ace_amd.ankur import AnkurLocalNet, AnkurLocalNetBuilder
    sel = ace_amd.ModuleSelector(type="AnkurLocalNet", config={})
    net = sel.build(6, 3, ace_amd.DatasetInfo((8, 16))).torch_module
    assert isinstance(net, AnkurLocalNet) and net.module.dims == [6, 256, 256, 256, 3]
    assert net.module.use_disco_encoder and not net.module.use_pos_embed and net.module.kernel_size == 3
    fields = [f.name for f in dataclasses.fields(AnkurLocalNetBuilder)]
    assert fields == ["embed_dim", "use_disco_encoder", "disco_kernel_size", "pos_embed", "activation_function"]
    b = AnkurLocalNetBuilder()
    assert (b.embed_dim, b.use_disco_encoder, b.disco_kernel_size, b.pos_embed, b.activation_function) == (256, True, 3, False, "gelu")
    assert sel.config == dataclasses.asdict(b)
    assert ace_amd.AnkurLocalNet is AnkurLocalNet and ace_amd.AnkurLocalNetBuilder is AnkurLocalNetBuilder
    with pytest.raises(ValueError, match="Conditional predictions require a conditional builder"):
        ace_amd.ModuleSelector(type="AnkurLocalNet", config={}, conditional=True)


@pytest.mark.parametrize("name", C.CASES)
def test_reference_state_dict_loads_strictly(name):
    c = C.case(name)
    torch.manual_seed(0)
    net = C.build(c)       # load_state_dict(strict=True) inside
    assert list(net.state_dict()) == list(c["state_dict"])
    for k, v in net.state_dict().items():
        assert v.shape == c["state_dict"][k].shape and torch.equal(v, c["state_dict"][k]), k
    assert not any("psi" in k for k in net.state_dict())
    if c["config"]["use_disco_encoder"]:
        import math
        g = math.gcd(c["n_in_channels"], c["config"]["embed_dim"])
        ks = c["config"]["disco_kernel_size"]
        assert net.state_dict()["module.mlp.0.conv.weight"].shape == (c["config"]["embed_dim"], c["n_in_channels"] // g, ks * ks)


def test_builder_refusals():
    info = ace_amd.DatasetInfo((8, 16))
    sel = lambda **cfg: ace_amd.ModuleSelector(type="AnkurLocalNet", config=cfg)     # noqa: E731
    with pytest.raises(NotImplementedError, match="ACE_PIXEL_MLP_MAX_WIDTH = 256"):
        sel(embed_dim=257).build(3, 2, info)
    with pytest.raises(NotImplementedError, match="ACE_PIXEL_MLP_MAX_WIDTH = 256"):
        sel(embed_dim=8, use_disco_encoder=False).build(300, 2, info)
    with pytest.raises(NotImplementedError, match="ACE_DISCO_MAX_PRODUCTS = 512"):
        sel(embed_dim=7).build(60, 2, info)                                          # one group of 60: 540 products
    with pytest.raises(NotImplementedError, match="ACE_DISCO_MAX_K = 25"):
        sel(embed_dim=8, disco_kernel_size=6).build(4, 2, info)
    with pytest.raises(ValueError, match="Unknown activation function tanh"):
        sel(embed_dim=8, activation_function="tanh").build(4, 2, info)
    sel(embed_dim=256, disco_kernel_size=5).build(40, 256, info)                     # at the limits


def test_limits_match_the_header():
    import _disco_ref as R
    import _pixel_mlp_ref as PR
    from ace_amd import disco
    k, p = R.constants(), PR.constants()
    assert (disco.MAX_K, disco.MAX_PRODUCTS) == (k["MAX_K"], k["MAX_PRODUCTS"])
    assert (disco.ACT_NONE, disco.ACT_RELU, disco.ACT_GELU, disco.ACT_SILU) == (k["ACT_NONE"], k["ACT_RELU"], k["ACT_GELU"], k["ACT_SILU"])
    assert (p["ACT_NONE"], p["ACT_RELU"], p["ACT_GELU"], p["ACT_SILU"]) == (0, 1, 2, 3)      # one numbering for both kernels


def test_table_refusals():
    from ace_amd.disco import disco_table
    for kw, word in [({"basis": "zernike"}, "basis 'zernike'"), ({"basis_norm_mode": "individual"}, "basis_norm_mode 'individual'"),
                     ({"grid": "equiangular"}, "grid 'equiangular'"), ({"out_shape": (4, 8)}, "out_shape")]:
        with pytest.raises(NotImplementedError, match=word):
            disco_table((8, 16), 3, **kw)


def test_forward_refuses_the_host_and_gradients():
    net = C.build(C.case("disco_relu_embed"))
    with pytest.raises(RuntimeError, match=r"the AnkurLocalNet \(ace_amd\) runs on an MI355X only: move the module and its input to "
                                           "'cuda'. There is no CPU fallback."):
        net(torch.zeros(1, 12, 9, 20))
    with pytest.raises(ValueError, match="expected \\(batch, channels, rows, columns\\)"):
        net(torch.zeros(12, 9, 20))
    land = ace_amd.LandNet((3, 5), 4, [6], 2)
    with pytest.raises(RuntimeError) as e:
        land(torch.zeros(1, 4, 3, 5))
    with pytest.raises(RuntimeError) as e2:
        net(torch.zeros(1, 12, 9, 20))
    assert str(e.value).replace("the LandNet", "the AnkurLocalNet") == str(e2.value)      # LandNet's text, apart from the name

    class OnDevice(torch.Tensor):
        is_cuda = True
    x = torch.zeros(1, 12, 9, 20).requires_grad_().as_subclass(OnDevice)
    with pytest.raises(RuntimeError, match="ace_amd implements the inference forward only; call under torch.no_grad\\(\\)"):
        net(x)


@pytest.mark.parametrize("name", C.CASES)
def test_module_on_the_emulation_matches_the_reference(name):
    c = C.case(name)
    net = C.build(c)
    with fake_ankur() as fake, torch.no_grad():
        y = net(c["input"], labels=None)
        if c["config"]["use_disco_encoder"]:
            assert fake.calls == ["disco_create", "pixel_mlp_create", "disco_forward", "pixel_mlp_forward"]
        else:
            assert fake.calls == ["pixel_mlp_create", "pixel_mlp_forward"]
    if "statement" in c:
        assert C.bits_equal(y, c["statement"])
    assert C.rel_err(y, c["output64"]) <= 2 * c["reference_error"]


def test_handles_are_rebuilt_after_an_in_place_weight_change():
    c = C.case("disco_relu_embed")
    net = C.build(c)
    x = c["input"]
    with fake_ankur() as fake, torch.no_grad():
        y0 = net(x)
        net(x)
        assert fake.created == 2 and fake.calls[-2:] == ["disco_forward", "pixel_mlp_forward"]
        net.module.mlp[0].conv.weight.mul_(2.0)                  # in place: same storage, new version
        y1 = net(x)
        assert fake.created == 4 and fake.destroyed == 2 and not torch.equal(y0, y1)
        net.module.mlp[1].pos_embed.add_(1.0)                    # any parameter counts
        net(x)
        assert fake.created == 6 and fake.destroyed == 4
        net.load_state_dict(c["state_dict"])
        assert C.bits_equal(net(x), y0) and fake.created == 8
        del net
        gc.collect()
        assert fake.destroyed == 8 and not fake._handles         # destroyed with the module


def test_load_stepper_round_trip_and_predict_on_the_emulation():
    from ace_amd.checkpoint import load_stepper
    ck, in_names, out_names = C.checkpoint("disco_relu_embed")
    c = C.case("disco_relu_embed")
    stepper = load_stepper(ck, device="cpu").stepper
    net = stepper._step_obj.module.torch_module
    assert isinstance(net, ace_amd.AnkurLocalNet)
    for k, v in c["state_dict"].items():
        assert torch.equal(net.state_dict()[k], v), k
    ck["stepper"]["step"] = stepper._step_obj.get_state()                                 # what it writes (the net's own keys), it reads
    again = load_stepper(ck, device="cpu").stepper
    for k, v in again._step_obj.module.torch_module.state_dict().items():
        assert torch.equal(v, c["state_dict"][k]), k
    H, W = c["img_shape"]
    g = torch.Generator().manual_seed(3)
    ic = {n: torch.randn(1, 1, H, W, generator=g) for n in out_names}
    forcing = {n: torch.randn(1, 3, H, W, generator=g) for n in in_names if n not in out_names}
    with fake_ankur():
        out, state = stepper.predict(ic, forcing)
    assert sorted(out) == sorted(out_names) and all(v.shape == (1, 2, H, W) and torch.isfinite(v).all() for v in out.values())
