"""LandNet on the host (``-m "not gpu"``): the registry entry and its refusals, the reference's parameter layout, the module's
handle life and the host logic of ``LandRolloutEngine`` on an emulation of the C ABI (tests/_fake_landnet.py: the header's
statement behind the real host code), against the reference's own outputs (tests/golden/gen_landnet_*.pt, gen_land_rollout.pt)."""
import dataclasses
import types

import pytest
import torch

import ace_amd
from ace_amd.step import NormalizationConfig

import _landnet_cases as C
from _fake_landnet import fake_landnet


# ---- registry and module -------------------------------------------------------------------------------------------------
def test_registry_type_fields_and_defaults():
    from ace_amd.landnet import LandNet, LandNetBuilder
    sel = ace_amd.ModuleSelector(type="LandNet", config={})
    net = sel.build(7, 3, ace_amd.DatasetInfo((4, 6))).torch_module
    assert isinstance(net, LandNet) and net.dims == [7, 64, 64, 3] and not net.use_positional_embedding
    fields = {f.name: f for f in dataclasses.fields(LandNetBuilder)}
    assert list(fields) == ["hidden_dims", "network_type", "use_positional_embedding"]
    b = LandNetBuilder()
    assert b.hidden_dims == [64, 64] and b.network_type == "MLP" and b.use_positional_embedding is False
    assert ace_amd.LandNet is LandNet and ace_amd.LandNetBuilder is LandNetBuilder


@pytest.mark.parametrize("name", C.CASES)
def test_reference_state_dict_loads_strictly(name):
    c = C.case(name)
    torch.manual_seed(0)
    net = C.build(c)       # load_state_dict(strict=True) inside
    assert list(net.state_dict()) == list(c["state_dict"])
    for k, v in net.state_dict().items():
        assert v.shape == c["state_dict"][k].shape and torch.equal(v, c["state_dict"][k]), k


def test_seeded_initialisation_follows_the_reference_order():
    """The embedding is drawn first, then the layers in order: the generator consumption of the reference's constructor."""
    torch.manual_seed(4)
    net = ace_amd.LandNet((3, 5), 4, [6], 2, use_positional_embedding=True)
    torch.manual_seed(4)
    embed = torch.randn(1, 6, 3, 5)
    first = torch.nn.Conv2d(4, 6, kernel_size=(1, 1))
    assert torch.equal(net.pos_embed.pos_embed, embed)
    assert torch.equal(net.model[0].layers[0].weight, first.weight) and torch.equal(net.model[0].layers[0].bias, first.bias)


def test_builder_refusals():
    info = ace_amd.DatasetInfo((4, 6))
    with pytest.raises(ValueError, match="LandNet does not support labels"):
        ace_amd.ModuleSelector(type="LandNet", config={}).build(3, 2, ace_amd.DatasetInfo((4, 6), all_labels={"a"}))
    with pytest.raises(ValueError, match="network_type"):
        ace_amd.ModuleSelector(type="LandNet", config={"network_type": "CNN"}).build(3, 2, info)
    with pytest.raises(NotImplementedError, match="ACE_PIXEL_MLP_MAX_WIDTH = 256"):
        ace_amd.ModuleSelector(type="LandNet", config={"hidden_dims": [257]}).build(3, 2, info)
    with pytest.raises(NotImplementedError, match="ACE_PIXEL_MLP_MAX_WIDTH = 256"):
        ace_amd.ModuleSelector(type="LandNet", config={"hidden_dims": [8]}).build(300, 2, info)
    with pytest.raises(NotImplementedError, match="ACE_PIXEL_MLP_MAX_LAYERS = 8"):
        ace_amd.ModuleSelector(type="LandNet", config={"hidden_dims": [4] * 8}).build(3, 2, info)
    ace_amd.ModuleSelector(type="LandNet", config={"hidden_dims": [4] * 7 }).build(256, 256, info)      # at the limits


def test_limits_match_the_header():
    import _pixel_mlp_ref as R
    from ace_amd import landnet
    k = R.constants()
    assert (landnet.MAX_LAYERS, landnet.MAX_WIDTH) == (k["MAX_LAYERS"], k["MAX_WIDTH"]) and k["MAX_LAYERS"] >= 8 and k["MAX_WIDTH"] >= 256
    assert (landnet.ACT_NONE, landnet.ACT_RELU) == (k["ACT_NONE"], k["ACT_RELU"]) == (0, 1)


def test_forward_refuses_the_host_and_gradients():
    net = ace_amd.LandNet((3, 5), 4, [6], 2)
    with pytest.raises(RuntimeError, match=r"the LandNet \(ace_amd\) runs on an MI355X only: move the module and its input to 'cuda'. "
                                           "There is no CPU fallback."):
        net(torch.zeros(1, 4, 3, 5))
    with pytest.raises(ValueError, match="expected \\(batch, channels, rows, columns\\)"):
        net(torch.zeros(4, 3, 5))
    # the same wording as ColumnMLP's, apart from the family's name
    mlp = ace_amd.ColumnMLP(4, 2, 8, 2)
    with pytest.raises(RuntimeError) as e:
        mlp(torch.zeros(1, 4, 3, 5))
    with pytest.raises(RuntimeError) as e2:
        net(torch.zeros(1, 4, 3, 5))
    assert str(e.value).replace("the MLP", "the LandNet") == str(e2.value)


@pytest.mark.parametrize("name", C.CASES)
def test_module_on_the_emulation_matches_the_reference(name):
    c = C.case(name)
    net = C.build(c)
    with fake_landnet() as fake, torch.no_grad():
        y = net(c["input"])
        assert fake.calls == ["pixel_mlp_create", "pixel_mlp_forward"]
    assert C.bits_equal(y, c["statement"])
    assert C.rel_err(y, c["output64"]) <= C.TOL


def test_one_launch_per_call_and_handle_life():
    c = C.case("small_embed")
    net = C.build(c)
    x = c["input"]
    with fake_landnet() as fake, torch.no_grad():
        y0 = net(x)
        net(x)
        assert fake.calls == ["pixel_mlp_create", "pixel_mlp_forward", "pixel_mlp_forward"] and fake.created == 1
        net.model[1].layers[0].weight.mul_(2.0)                  # in place: same storage, new version
        y1 = net(x)
        assert fake.created == 2 and fake.destroyed == 1 and fake.calls[-2:] == ["pixel_mlp_create", "pixel_mlp_forward"]
        assert not torch.equal(y0, y1)
        net.pos_embed.pos_embed.add_(1.0)                        # any parameter counts
        net(x)
        assert fake.created == 3 and fake.destroyed == 2
        net.load_state_dict(c["state_dict"])
        assert C.bits_equal(net(x), y0) and fake.created == 4
        del net
        import gc
        gc.collect()
        assert fake.destroyed == 4 and not fake._handles         # destroyed with the module


def test_a_deep_copy_prepares_its_own_handle():
    import copy
    c = C.case("small_embed")
    net = C.build(c)
    x = c["input"]
    with fake_landnet() as fake, torch.no_grad():
        y0 = net(x)
        twin = copy.deepcopy(net)
        assert twin._prepared is None and net._prepared is not None
        y1 = twin(x)
        assert fake.created == 2 and fake.destroyed == 0         # the copy did not take, nor destroy, the original's handle
        assert twin._prepared[1] != net._prepared[1]
        assert C.bits_equal(net(x), y0) and C.bits_equal(y1, y0) and fake.created == 2
        del twin
        import gc
        gc.collect()
        assert fake.destroyed == 1 and C.bits_equal(net(x), y0)


def test_forward_refuses_a_gradient_requiring_input():
    class OnDevice(torch.Tensor):      # a tensor that claims to be on the device: the guards run in their order, nothing is launched
        is_cuda = True
    net = ace_amd.LandNet((3, 5), 4, [6], 2)
    x = torch.zeros(1, 4, 3, 5).requires_grad_().as_subclass(OnDevice)
    with pytest.raises(RuntimeError, match="ace_amd implements the inference forward only; call under torch.no_grad\\(\\)"):
        net(x)


# ---- checkpoint and stepper ----------------------------------------------------------------------------------------------
def test_load_stepper_builds_a_landnet_stepper():
    stepper, c = C.golden_stepper("cpu")
    net = stepper._step_obj.module.torch_module
    assert isinstance(net, ace_amd.LandNet) and net.dims == [7, 16, 8, 4] and net.use_positional_embedding
    assert stepper._masks and stepper._step_obj._corrector is None
    assert sorted(stepper.prognostic_names) == ["SNOWD", "SOILM", "TSOIL"]
    for k, v in c["stepper"]["step"]["module"].items():
        if k != "label_encoding":
            assert torch.equal(net.state_dict()[k[len("module."):]], v.float()), k


def _io(c, T=None):
    T = T or c["output"]["TSOIL"].shape[1]
    return ({k: v.clone() for k, v in c["initial_condition"].items()}, {k: v[:, : T + 1].clone() for k, v in c["forcing"].items()}, T)


def test_stepper_predict_on_the_emulation_matches_the_reference_rollout():
    stepper, c = C.golden_stepper("cpu")
    ic, forcing, T = _io(c)
    with fake_landnet():
        out, state = stepper.predict(ic, forcing)
    errs = C.rollout_errors(out, c)
    assert max(errs.values()) <= C.TOL, errs
    assert sorted(state) == sorted(stepper.prognostic_names)


# ---- the engine's host logic ---------------------------------------------------------------------------------------------
def test_engine_on_the_emulation_equals_stepper_predict_and_the_reference():
    from ace_amd.land_rollout import LandRolloutEngine
    stepper, c = C.golden_stepper("cpu")
    ic, forcing, T = _io(c)
    with fake_landnet() as fake:
        want, _ = stepper.predict(ic, forcing)
        del fake.calls[:]
        eng = LandRolloutEngine(stepper, batch=2, n_forward_steps=T, graph=None)
        out, state = eng.predict(ic, forcing)
        assert fake.calls == ["mask_pack_normalize", "pixel_mlp_forward", "unpack_denormalize", "mask_planes"] * T   # handle: predict's
        for k in want:
            assert C.bits_equal(out[k], want[k]), k
        assert max(C.rollout_errors(out, c).values()) <= C.TOL
        for k in stepper.prognostic_names:
            assert C.bits_equal(state[k], out[k][:, -1:])
        # two windows of the engine equal one
        whole = {k: v.clone() for k, v in out.items()}
        eng2 = LandRolloutEngine(stepper, batch=2, n_forward_steps=1, graph=None)
        a = {k: v.clone() for k, v in eng2.predict(ic, {k: v[:, :2] for k, v in forcing.items()})[0].items()}
        eng2.continue_from_last()
        for n in eng2.forcing_names:
            eng2.forcing[n].copy_(forcing[n][:, 1:3])
        eng2.run_window()
        for k in whole:
            assert C.bits_equal(torch.cat([a[k], eng2.out[k]], dim=1), whole[k][:, :2]), k


def test_engine_predict_picks_the_land_engine():
    from ace_amd.land_rollout import LandRolloutEngine
    stepper, c = C.golden_stepper("cpu")
    ic, forcing, T = _io(c)
    with fake_landnet():
        predict = ace_amd.EnginePredict(stepper, batch=2, graph=None)
        out, _ = predict(ic, forcing)
        assert isinstance(predict._engines[T], LandRolloutEngine)
        want, _ = stepper.predict(ic, forcing)
    for k in want:
        assert C.bits_equal(out[k], want[k]), k


def _plain_stepper(**kw):
    names = ["f", "a", "b"]
    norm = NormalizationConfig(means={k: 0.0 for k in names}, stds={k: 1.0 for k in names})
    builder = kw.pop("builder", ace_amd.ModuleSelector(type="LandNet", config={"hidden_dims": [4]}))
    cfg = ace_amd.SingleModuleStepConfig(builder=builder, in_names=names, out_names=["a", "b"], normalization=norm, **kw)
    return ace_amd.Stepper.from_config(cfg, ace_amd.DatasetInfo((3, 5)), device="cpu")


def _engine(stepper, **kw):
    from ace_amd.land_rollout import LandRolloutEngine
    return LandRolloutEngine(stepper, batch=1, n_forward_steps=2, **kw)


def test_engine_refusals_by_name_before_any_device_work():
    """every refusal is raised on a host stepper, i.e. before the device is looked at"""
    from ace_amd.corrector import AtmosphereCorrectorConfig
    with pytest.raises(NotImplementedError, match="LandRolloutEngine: a corrector .*force_positive"):
        _engine(_plain_stepper(corrector=AtmosphereCorrectorConfig(force_positive_names=["a"])))
    s = _plain_stepper()
    s._step_obj._ocean = object()
    with pytest.raises(NotImplementedError, match="LandRolloutEngine: an `ocean` configuration"):
        _engine(s)
    s = _plain_stepper()
    s._step_obj._global_mean_removal = object()
    with pytest.raises(NotImplementedError, match="LandRolloutEngine: global_mean_removal"):
        _engine(s)
    s = _plain_stepper()
    s._multi_call_config = object()
    with pytest.raises(NotImplementedError, match="LandRolloutEngine: multi-call"):
        _engine(s)
    s = _plain_stepper()
    s._step_obj.secondary_decoder = object()
    with pytest.raises(NotImplementedError, match="LandRolloutEngine: a secondary decoder"):
        _engine(s)
    s = _plain_stepper()
    s._step_obj.module._label_encoding = object()
    with pytest.raises(NotImplementedError, match="LandRolloutEngine: a label-conditioned module"):
        _engine(s)
    with pytest.raises(NotImplementedError, match="LandRolloutEngine: prescribed prognostic names"):
        _engine(_plain_stepper(prescribed_prognostic_names=["a"]))
    with pytest.raises(NotImplementedError, match="LandRolloutEngine: step_diagnostics"):
        _engine(_plain_stepper(), step_diagnostics=True)
    with pytest.raises(NotImplementedError, match="LandRolloutEngine: the module is a ColumnMLP, not LandNet"):
        _engine(_plain_stepper(builder=ace_amd.ModuleSelector(type="MLP", config={"hidden_dim": 4, "depth": 2})))
    with pytest.raises(ValueError, match="graph must be"):
        _engine(_plain_stepper(), graph="all")
    with pytest.raises(RuntimeError, match="LandRolloutEngine runs on an MI355X"):
        _engine(_plain_stepper())
    with fake_landnet():
        eng = _engine(_plain_stepper(), graph=None)
        with pytest.raises(TypeError, match="Labels are not allowed"):
            eng.set_labels(types.SimpleNamespace())
