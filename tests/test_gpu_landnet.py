"""LandNet on the device: the module against the reference's own outputs (tests/golden/gen_landnet_*.pt) and bitwise against the
header's statement, the stepper loaded from the reference-layout checkpoint against the reference rollout
(tests/golden/gen_land_rollout.pt), and ``LandRolloutEngine`` bitwise against ``Stepper.predict`` in every graph mode."""
import pytest
import torch

import ace_amd

import _landnet_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", C.CASES)
def test_module_matches_the_reference_and_the_statement(dev, name):
    c = C.case(name)
    net = C.build(c, dev)
    with torch.no_grad():
        y = net(c["input"].to(dev))
    torch.cuda.synchronize()
    err, ref_err = C.rel_err(y.cpu(), c["output64"]), C.rel_err(c["output"], c["output64"])
    print(f"{name}: kernel vs fp64 {err:.3e}; reference fp32 vs fp64 {ref_err:.3e}")
    assert err <= C.TOL, (name, err)
    assert C.bits_equal(y, c["statement"])


def test_a_width_that_is_no_multiple_of_four_runs_without_a_copy(dev):
    c = C.case("small_embed")            # 9 x 15
    net = C.build(c, dev)
    x = c["input"].to(dev)
    assert x.shape[-1] % 4 != 0
    with torch.no_grad():
        net(x)                           # the handle
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
        y = net(x)
        after = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    assert after - before == 1           # the output, nothing else: no padded copy of the input
    assert C.bits_equal(y, c["statement"])


def test_weights_changed_in_place_are_picked_up(dev):
    c = C.case("one_hidden")
    net = C.build(c, dev)
    x = c["input"].to(dev)
    with torch.no_grad():
        y0 = net(x).clone()
        net.model[0].layers[0].bias.add_(1.0)
        y1 = net(x).clone()
        net.load_state_dict(c["state_dict"])
        y2 = net(x)
    assert not torch.equal(y0, y1) and C.bits_equal(y2, y0)


def _io(c, dev, T=None):
    T = T or c["output"]["TSOIL"].shape[1]
    return ({k: v.to(dev) for k, v in c["initial_condition"].items()}, {k: v[:, : T + 1].to(dev) for k, v in c["forcing"].items()}, T)


def test_loaded_stepper_matches_the_reference_rollout(dev):
    """Every field within 1e-5 of its largest finite magnitude at every step, NaN exactly on the masked cells.  Measured on an
    MI355X (max over the steps): TSOIL 5.4e-08, SOILM 1.1e-07, SNOWD 1.2e-07, LHTFLsfc 8.9e-08; the reference's own fp32 rollout
    is 5.4e-08, 9.8e-08, 1.6e-07, 8.7e-08 from its fp64 one."""
    stepper, c = C.golden_stepper(dev)
    ic, forcing, T = _io(c, dev)
    out, state = stepper.predict(ic, forcing)
    torch.cuda.synchronize()
    errs = C.rollout_errors(out, c)
    print("rollout vs the reference's fp64:", {k: f"{v:.3e}" for k, v in errs.items()})
    assert max(errs.values()) <= C.TOL, errs
    assert sorted(state) == sorted(stepper.prognostic_names)


def test_engine_is_bitwise_stepper_predict_in_every_graph_mode(dev):
    from ace_amd.land_rollout import LandRolloutEngine
    stepper, c = C.golden_stepper(dev)
    ic, forcing, T = _io(c, dev)
    want, _ = stepper.predict(ic, forcing)
    for graph in (None, "step", "window"):
        eng = LandRolloutEngine(stepper, batch=2, n_forward_steps=T, graph=graph)
        first = {k: v.clone() for k, v in eng.predict(ic, forcing)[0].items()}
        second, state = eng.predict(ic, forcing)
        torch.cuda.synchronize()
        for k in want:
            assert C.bits_equal(first[k], want[k]), (graph, k)
            assert C.bits_equal(second[k], want[k]), (graph, k)
        for k in stepper.prognostic_names:
            assert C.bits_equal(state[k], first[k][:, -1:])
        assert max(C.rollout_errors(first, c).values()) <= C.TOL


@pytest.mark.parametrize("graph", [None, "step", "window"])
def test_two_consecutive_windows_equal_stepper_predict(dev, graph):
    from ace_amd.land_rollout import LandRolloutEngine
    stepper, c = C.golden_stepper(dev)
    ic, forcing, T = _io(c, dev)
    assert T == 3
    want, _ = stepper.predict(ic, {k: v[:, :3] for k, v in forcing.items()})
    eng = LandRolloutEngine(stepper, batch=2, n_forward_steps=1, graph=graph)
    a = {k: v.clone() for k, v in eng.predict(ic, {k: v[:, :2] for k, v in forcing.items()})[0].items()}
    eng.continue_from_last()
    for n in eng.forcing_names:
        eng.forcing[n].copy_(forcing[n][:, 1:3])
    eng.run_window()
    torch.cuda.synchronize()
    for k in want:
        assert C.bits_equal(torch.cat([a[k], eng.out[k]], dim=1), want[k]), k


def test_engine_predict_builds_a_land_engine(dev):
    from ace_amd.land_rollout import LandRolloutEngine
    stepper, c = C.golden_stepper(dev)
    ic, forcing, T = _io(c, dev)
    predict = ace_amd.EnginePredict(stepper, batch=2, graph="step")
    out, _ = predict(ic, forcing)
    assert isinstance(predict._engines[T], LandRolloutEngine)
    want, _ = stepper.predict(ic, forcing)
    for k in want:
        assert C.bits_equal(out[k], want[k]), k
