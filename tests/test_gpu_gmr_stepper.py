"""Global-mean removal on the device: reference-written stepper states with the option (tests/golden/make_golden_gmr.py) through
``Stepper.predict`` with the real network against the REAL reference's rollouts, the host transform's native means against
``t.mean``, and ``RolloutEngine`` (csrc/gmr.hip folded into its pack / unpack) against ``Stepper.predict`` in every graph mode."""
import copy
import math

import pytest
import torch

import ace_amd
from ace_amd.checkpoint import load_stepper
from _util import load_golden, rel_max

pytestmark = pytest.mark.gpu

CASES = ["shared", "per_channel", "subset"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("gen_gmr.pt")


@pytest.fixture(scope="module")
def predicted(dev, golden):
    """case -> (the loaded stepper, device inputs, Stepper.predict's outputs): computed once, shared, left unchanged"""
    out = {}
    for case in CASES:
        g = golden[case]
        st = load_stepper(g["state"], device="cuda").stepper
        ic = {k: v.to(dev) for k, v in g["ic"].items()}
        forcing = {k: v.to(dev) for k, v in g["forcing"].items()}
        with torch.no_grad():
            got, state = st.predict(ic, forcing)
        out[case] = (st, ic, forcing, {k: v.clone() for k, v in got.items()}, state)
    return out


@pytest.mark.parametrize("case", CASES)
def test_stepper_predict_vs_reference_rollout_on_the_device(predicted, golden, case):
    """the bar of the device test of tests/test_step_options.py.  The sample means are the fp64 sums of csrc/gmr.hip rounded once,
    the reference's are fp32 sums in torch's order: the one stated numerical difference of the feature."""
    _, _, _, out, _ = predicted[case]
    steps = golden[case]["steps"]
    assert set(out) == set(steps[0])
    worst = {k: rel_max(out[k], torch.stack([s[k] for s in steps], dim=1)) for k in out}
    print(f"\n[gmr] {case}: worst rel_max against the reference rollout {max(worst.values()):.3e} ({max(worst, key=worst.get)})")
    for k, v in worst.items():
        assert v <= 1e-5, (case, k, v)


def _ulp32(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23) if x else 2.0 ** -149


@pytest.mark.parametrize("kind", ["shared", "per_channel"])
def test_fused_means_against_torch_means(dev, kind):
    """The transform with ``fused=True`` (ace_gmr_sample_means) against ``fused=False`` (t.mean) on the device, at the workload's
    plane.  The fused mean is within 1 fp32 ulp of the exactly rounded mean (tests/test_gmr_ref_cpu.py holds the contract to that,
    tests/test_gpu_gmr_kernels.py the kernel to the contract); torch's is off by its own error, measured here against the fp64
    mean of the same data; each shift is one more fp32 subtraction.  So
        |shift_fused - shift_torch| <= ulp(mean) + |torch_mean - exact| + 2 ulp(shift)."""
    from ace_amd.step import NormalizationConfig
    names = ["Ts", "T_1", "q"]
    B, H, W = 3, 180, 360
    g = torch.Generator().manual_seed(3)
    x = {"Ts": 288.0 + 30.0 * (2 * torch.rand(B, H, W, generator=g) - 1), "T_1": 250.0 + 4.0 * torch.randn(B, H, W, generator=g),
         "q": 1e-3 * (1 + 0.5 * torch.rand(B, H, W, generator=g))}
    norm = NormalizationConfig(means={"Ts": 287.0, "T_1": 251.0, "q": 1.1e-3}, stds={"Ts": 5.0, "T_1": 6.0, "q": 2e-4}).build(names, device=dev)
    cfg = (ace_amd.SharedGlobalMeanRemovalConfig(reference_field="Ts", field_names=["Ts", "T_1"], append_as_input=True) if kind == "shared"
           else ace_amd.PerChannelGlobalMeanRemovalConfig(append_as_input=True))
    xd = {k: v.to(dev) for k, v in x.items()}
    fused, unfused = cfg.build(norm, names), cfg.build(norm, names, fused=False)
    assert fused.fused and not unfused.fused
    a_in, a = fused.forward_transform(xd, None)
    b_in, b = unfused.forward_transform(xd, None)
    assert set(a.shifts) == set(b.shifts) and list(a.extras) == list(b.extras)
    worst = 0.0
    for name in a.shifts:
        src = "Ts" if kind == "shared" else name
        exact = x[src].double().mean(dim=(1, 2))
        torch_err = (xd[src].mean(dim=(1, 2)).double().cpu() - exact).abs()
        diff = (a.shifts[name].double() - b.shifts[name].double()).abs().cpu()
        for i in range(B):
            bound = _ulp32(float(exact[i])) + float(torch_err[i]) + 2 * _ulp32(float(a.shifts[name][i]))
            worst = max(worst, float(diff[i]) / _ulp32(float(exact[i])))
            assert float(diff[i]) <= bound, (name, i, float(diff[i]), bound)
        # downstream of the mean both paths are the same torch ops
        if name in xd:
            assert torch.equal(a_in[name], xd[name] + a.shifts[name].view(-1, 1, 1))
    print(f"\n[gmr] {kind}: fused against torch shifts, worst difference {worst:.2f} ulp of the mean")
    for name, extra in a.extras.items():
        field = ace_amd.extra_channel_source_field(name)
        assert torch.equal(extra, (-a.shifts[field] / norm.stds[field]).view(-1, 1, 1).expand(B, H, W))
    # a non-contiguous field takes the same path
    sliced = {k: torch.stack([v, v], dim=1)[:, 1] for k, v in xd.items()}
    _, c = fused.forward_transform(sliced, None)
    assert all(torch.equal(c.shifts[k], a.shifts[k]) for k in a.shifts)


@pytest.mark.parametrize("graph", [None, "step", "window"])
@pytest.mark.parametrize("case", CASES)
def test_rollout_engine_vs_stepper_predict(predicted, case, graph):
    from ace_amd.rollout import RolloutEngine
    st, ic, forcing, want, want_state = predicted[case]
    eng = RolloutEngine(st, batch=2, n_forward_steps=3, graph=graph)
    assert eng._gmr is not None
    out, state = eng.predict(ic, forcing)
    torch.cuda.synchronize()
    assert set(out) == set(want)
    worst = {k: rel_max(out[k], want[k]) for k in out}
    print(f"\n[gmr] {case} graph={graph}: engine against Stepper.predict, worst rel_max {max(worst.values()):.3e}")
    for k, v in worst.items():
        assert v <= 5e-6, (case, graph, k, v)
    for k in want_state:
        assert rel_max(state[k], want_state[k]) <= 5e-6, k
    if graph == "window":       # the captured window replayed: bitwise itself
        first = {k: v.clone() for k, v in out.items()}
        again, _ = eng.predict(ic, forcing)
        torch.cuda.synchronize()
        for k in first:
            assert torch.equal(first[k], again[k]), k


def test_stepper_without_the_option_is_unchanged(dev, golden, predicted):
    """the same weights with the option taken out of the state (the "subset" case has no synthetic channels): the engine keeps
    the plain calls - an evaluation is bitwise the plain ace_pack_normalize / forward / ace_unpack_denormalize sequence, the
    rollout Stepper.predict's at the existing bar - and the option's rollout is another one (a removed mean matters)"""
    from ace_amd import _lib
    from ace_amd.rollout import RolloutEngine
    g = golden["subset"]
    state = copy.deepcopy(g["state"])
    state["config"]["step"]["config"]["global_mean_removal"] = None
    st = load_stepper(state, device="cuda").stepper
    assert st._step_obj.global_mean_removal is None
    _, ic, forcing, with_option, _ = predicted["subset"]
    with torch.no_grad():
        want, _ = st.predict(ic, forcing)
    for graph in (None, "step", "window"):
        eng = RolloutEngine(st, batch=2, n_forward_steps=3, graph=graph)
        assert eng._gmr is None and eng.x.shape[1] == len(eng.in_names)
        out, _ = eng.predict(ic, forcing)
        torch.cuda.synchronize()
        for k in want:          # the existing engine-against-predict bar (the post-step hooks are fused kernels in the engine)
            assert rel_max(out[k], want[k]) <= 5e-6, (graph, k, rel_max(out[k], want[k]))
    # (the small network's T_1 varies by a few hundredths around 251: the difference is held against that spread)
    spread = float(want["T_1"].max() - want["T_1"].min())
    assert float((with_option["T_1"] - want["T_1"]).abs().max()) > 1e-3 * spread
    # one evaluation by hand with the plain entries, on the engine's own tables (before the post-step hooks edit the planes)
    L, stream = _lib.lib(), _lib.current_stream()
    eng = RolloutEngine(st, batch=2, n_forward_steps=3, graph=None)
    eng.load(ic, forcing)
    x, y = torch.zeros_like(eng.x), torch.zeros_like(eng.y)
    _lib.check(L.ace_pack_normalize(eng._src_ptr_addr[0], eng._src_stride_addr[0], eng.in_mean.data_ptr(), eng.in_std.data_ptr(),
                                    x.data_ptr(), 2, len(eng.in_names), eng.HW, stream))
    _lib.check(L.ace_sfno_forward(eng.net._native, x.data_ptr(), y.data_ptr(), 2, stream))
    eng._evaluate(L, stream, 0, False, eng._src_ptr_addr[0], eng._dst_ptr_addr[0], eng._dst_strides, True)
    torch.cuda.synchronize()
    assert torch.equal(eng.x, x) and torch.equal(eng.y, y)
    planes = torch.stack([eng.out_plane(n, 0) for n in eng.out_names], dim=1)
    mean, std = eng.out_mean.view(1, -1, 1, 1), eng.out_std.view(1, -1, 1, 1)
    assert torch.equal(planes, y * std + mean)
