"""The sea-ice corrector on the device: every golden case of the reference (tests/golden/gen_ice_corrector_*.pt) through
``IceCorrector.__call__`` - the fused kernels and the torch ops - bit for bit; ``Stepper.predict`` with the fused corrector on and off;
``OceanRolloutEngine`` in its three graph modes against ``Stepper.predict``; and one captured window replayed on initial conditions
whose flag paths differ, which a flag read on the host at capture time would fail."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ice_corrector_ref_cpu import EXPECTED, build, load, same_bits  # noqa: E402
from test_ice_corrector_cpu import golden_stepper  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _bits_equal(a, b) -> bool:
    """bitwise, NaN payloads included"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("case", [c for c in EXPECTED if c != "none"])
def test_golden_cases_on_the_device(dev, case, fused):
    rec = load(case)
    corrector = build(rec)
    corrector.fused = fused
    inp = {k: v.to(dev) for k, v in rec["input"].items()}
    gen = {k: v.to(dev) for k, v in rec["output"].items()}
    where = {k: v.data_ptr() for k, v in gen.items()}
    out, state = corrector(inp, gen, {}, None)
    torch.cuda.synchronize()
    n = len(corrector.plan)
    assert state is None and corrector.launches() == ((n, n) if fused else (0, 0))
    assert set(out) == set(rec["corrected"])
    for k, want in rec["corrected"].items():
        assert same_bits(out[k].cpu(), want), k
        if fused:
            assert out[k].data_ptr() == where[k], k       # corrected in place
    for k, v in rec["input"].items():
        assert same_bits(inp[k].cpu(), v), k


def test_nothing_corrected_is_no_corrector():
    assert build(load("none")) is None


# ---- the stepper and the engine ---------------------------------------------------------------------------------------------
def _setup(dev, edit=None):
    loaded, case = golden_stepper(dev, edit)
    ic = {k: v.to(dev) for k, v in case["initial_condition"].items()}
    forcing = {k: v.to(dev) for k, v in case["forcing"].items()}
    return loaded.stepper, case, ic, forcing


def _close_to_reference(got, case, k):
    """the bar of tests/test_gpu_ocean_rollout.py"""
    out32 = case["output"][k].double()
    ref = out32 + case["output64_delta"][k].double() / case["output64_delta_scale"]
    got = got.double().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), k
    ok = ~torch.isnan(ref)
    scale = ref[ok].abs().max()
    err = (got - ref)[ok].abs().max() / scale
    ref_err = (out32 - ref)[ok].abs().max() / scale
    assert err <= 2.0 * ref_err + 1e-6, (k, float(err), float(ref_err))


def test_stepper_predict_fused_on_and_off(dev):
    stepper, case, ic, forcing = _setup(dev)
    corrector = stepper._step_obj._corrector
    corrector.fused = False
    want, _ = stepper.predict(ic, forcing)
    assert corrector.launches() == (0, 0)
    corrector.fused = True
    got, _ = stepper.predict(ic, forcing)
    torch.cuda.synchronize()
    T = case["output"]["siconc"].shape[1]
    assert corrector.launches() == (3 * T, 3 * T)
    for k in want:
        assert _bits_equal(got[k], want[k]), k
    for k in case["output"]:
        _close_to_reference(got[k], case, k)


def test_engine_is_stepper_predict_in_every_graph_mode(dev):
    from ace_amd.ocean_rollout import OceanRolloutEngine
    stepper, case, ic, forcing = _setup(dev)
    want = {k: v.clone() for k, v in stepper.predict(ic, forcing)[0].items()}
    T = case["output"]["siconc"].shape[1]
    for graph in (None, "step", "window"):
        eng = OceanRolloutEngine(stepper, batch=2, n_forward_steps=T, graph=graph)
        assert set(eng.stage) >= {"siconc", "simass", "sisnmass"}       # the masked old masses the corrector reads are staged
        first = {k: v.clone() for k, v in eng.predict(ic, forcing)[0].items()}
        second, _ = eng.predict(ic, forcing)
        torch.cuda.synchronize()
        worst = max(float((first[k].double() - want[k].double()).nan_to_num().abs().max() / want[k].double().nan_to_num().abs().max())
                    for k in want)
        print(f"ICEENGINE graph={graph}: worst max|engine - predict| / max|predict| = {worst:.3e}")
        for k in want:
            assert _bits_equal(first[k], second[k]), (graph, k)
            assert _bits_equal(first[k], want[k]), (graph, k)


def _quiet_terms(state):
    """no land, and budget terms a thousand times smaller: whether a stage runs is decided by the initial condition alone"""
    norm = state["config"]["step"]["config"]["normalization"]["network"]
    for k in norm["stds"]:
        if k not in ("siconc", "simass", "sisnmass", "DSWRFsfc"):
            norm["stds"][k] *= 1e-3
            norm["means"][k] = 0.0
    masks = state["dataset_info"]["mask_provider"]["masks"]
    for k in masks:
        masks[k] = torch.ones_like(masks[k])


def test_captured_window_follows_the_flags_of_each_initial_condition(dev):
    from ace_amd.ocean_rollout import OceanRolloutEngine
    stepper, case, ic, forcing = _setup(dev, _quiet_terms)
    g = torch.Generator().manual_seed(3)
    quiet = {k: v.clone() for k, v in ic.items()}
    for name, c in (("siconc", 1.0), ("simass", 40.0), ("sisnmass", 7.0)):
        quiet[name] = ((0.3 + 0.4 * torch.rand(ic[name].shape, generator=g)) * c).to(dev)
    one = {k: v.clone() for k, v in quiet.items()}
    one["siconc"][1, 0, -1, -1] = -0.5                         # a single trigger: the last pixel of the last sample
    forcing = {k: v[:, :3] for k, v in forcing.items()}
    eager = OceanRolloutEngine(stepper, batch=2, n_forward_steps=2, graph=None)
    want = {name: {k: v.clone() for k, v in eager.predict(x, forcing)[0].items()} for name, x in (("quiet", quiet), ("one", one))}
    # the paths differ: with no stage run the network's negative sources survive, with stage 1 run not one does
    assert bool((want["quiet"]["LSRCc"][:, 0] < 0).any()) and bool((want["quiet"]["LSNKc"][:, 0] > 0).any())
    assert bool((want["one"]["LSRCc"][:, 0] >= 0).all()) and bool((want["one"]["LSNKc"][:, 0] <= 0).all())
    for graph in ("window", "step"):
        eng = OceanRolloutEngine(stepper, batch=2, n_forward_steps=2, graph=graph)
        for name, x in (("quiet", quiet), ("one", one), ("quiet", quiet), ("one", one)):      # captured on the first, replayed after
            got, _ = eng.predict(x, forcing)
            torch.cuda.synchronize()
            for k in got:
                assert _bits_equal(got[k], want[name][k]), (graph, name, k)
    ref = {k: v.clone() for k, v in stepper.predict(one, forcing)[0].items()}
    for k in ref:
        assert _bits_equal(ref[k], want["one"][k]), k
