"""TEST INFRASTRUCTURE shared by the LandNet tests: the golden cases (tests/golden/gen_landnet_<case>.pt, gen_land_rollout.pt; emitted
by the reference itself, make_golden_landnet.py / make_golden_land_rollout.py), loaded once per session and never modified."""
import copy
import functools

import torch

from _util import load_golden

CASES = ["small_embed", "shipped_embed", "one_hidden", "no_hidden"]
TOL = 1e-5          # the project's per-step target: max |got - fp64 reference| / max |fp64 reference|


@functools.lru_cache(maxsize=None)
def case(name):
    """The fixture with the bfloat16-stored tensors widened to fp32, the reference's fp64 output rebuilt, and the header's
    statement (tests/_pixel_mlp_ref.py) evaluated on it: computed once, shared by every test."""
    import _pixel_mlp_ref as R
    c = load_golden(f"gen_landnet_{name}.pt")
    c["state_dict"] = {k: v.float() for k, v in c["state_dict"].items()}
    c["input"] = c["input"].float()
    c["output64"] = c["output"].double() + c["output64_delta"].double() / c["output64_delta_scale"]
    c["statement"] = torch.from_numpy(R.landnet_statement(c["state_dict"], c["input"], c["config"]["use_positional_embedding"]))
    return c


def build(c, device=None):
    """The registry's module of a case with the reference's weights loaded strictly."""
    import ace_amd
    mod = ace_amd.ModuleSelector(type="LandNet", config=dict(c["config"])).build(
        c["n_in_channels"], c["n_out_channels"], ace_amd.DatasetInfo(tuple(c["img_shape"])))
    net = mod.torch_module
    net.load_state_dict(c["state_dict"], strict=True)
    return net.to(device) if device is not None else net


def rel_err(got, want64):
    return float((got.double() - want64).abs().max() / want64.abs().max())


def bits_equal(a, b) -> bool:
    """bitwise (signs of zero included); NaN compared by position"""
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    ok = ~torch.isnan(a)
    return torch.equal(a.view(torch.int32)[ok], b.view(torch.int32)[ok])


@functools.lru_cache(maxsize=None)
def rollout_case():
    c = load_golden("gen_land_rollout.pt")
    c["output64"] = {k: v.double() + c["output64_delta"][k].double() / c["output64_delta_scale"] for k, v in c["output"].items()}
    return c


def golden_stepper(device):
    """``load_stepper`` on the rollout fixture's checkpoint (a fresh stepper per call), and the case."""
    from ace_amd.checkpoint import load_stepper
    c = rollout_case()
    state = copy.deepcopy(c["stepper"])
    state["step"]["module"] = {k: (v.float() if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
                               for k, v in state["step"]["module"].items()}
    di = state["dataset_info"]
    di["mask_provider"]["masks"] = {k: v.float() for k, v in di["mask_provider"]["masks"].items()}
    return load_stepper({"stepper": state}, device=device).stepper, c


def rollout_errors(got, c):
    """Per field: NaN positions equal the reference's, and max over steps of max |got - ref64| / max finite |ref64| of that step."""
    errs = {}
    for k, ref in c["output64"].items():
        g = got[k].double().cpu()
        assert torch.equal(torch.isnan(g), torch.isnan(ref)), k
        worst = 0.0
        for s in range(ref.shape[1]):
            ok = ~torch.isnan(ref[:, s])
            worst = max(worst, float((g[:, s] - ref[:, s])[ok].abs().max() / ref[:, s][ok].abs().max()))
        errs[k] = worst
    return errs
