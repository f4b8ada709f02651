"""TEST INFRASTRUCTURE shared by the AnkurLocalNet tests: the golden cases (tests/golden/gen_ankur_<case>.pt, emitted by the
reference itself, make_golden_ankur.py), loaded once per session and never modified, the composed statement of a ReLU net
(tests/_disco_ref.py, then tests/_pixel_mlp_ref2.py), and a reference-layout stepper checkpoint around a case."""
import datetime
import functools

import numpy as np
import torch

from _util import load_golden

CASES = ["disco_gelu", "disco_relu_embed", "disco_silu_embed", "depthwise_relu", "conv_gelu_embed", "conv_relu_embed"]
RELU_CASES = [n for n in CASES if "relu" in n]


def statement(state, x, cfg):
    """The net as the two kernels' statements composed (ReLU only): numpy (B, out, H, W)."""
    import _disco_ref as D
    import _pixel_mlp_ref2 as P
    from ace_amd.disco import disco_table
    assert cfg["activation_function"] == "relu"
    B, C, H, W = x.shape
    pre = "module.mlp."
    embed = state[pre + "1.pos_embed"].numpy().reshape(-1, H, W) if cfg["pos_embed"] else None
    idx = [i for i in range(1, 9) if f"{pre}{i}.weight" in state]
    ws = [state[f"{pre}{i}.weight"].numpy().reshape(state[f"{pre}{i}.weight"].shape[:2]) for i in idx]
    bs = [state[f"{pre}{i}.bias"].numpy() if f"{pre}{i}.bias" in state else None for i in idx]
    xn = x.numpy()
    if cfg["use_disco_encoder"]:
        w0 = state[pre + "0.conv.weight"].numpy()
        groups = C // w0.shape[1]
        h = D.disco(xn, disco_table((H, W), cfg["disco_kernel_size"]), w0, groups, D.ACT_RELU, embed)
        y = P.pixel_mlp2(h.reshape(B, -1, H * W), ws, bs, [1, 1, 0])
    else:
        ws = [state[pre + "0.weight"].numpy().reshape(state[pre + "0.weight"].shape[:2])] + ws
        bs = [state[pre + "0.bias"].numpy()] + bs
        y = P.pixel_mlp2(xn.reshape(B, C, H * W), ws, bs, [1, 1, 1, 0], 0 if embed is not None else -1,
                         embed.reshape(-1, H * W) if embed is not None else None, embed_before_act=True)
    return y.reshape(B, -1, H, W)


@functools.lru_cache(maxsize=None)
def case(name):
    c = load_golden(f"gen_ankur_{name}.pt")
    c["state_dict"] = {k: v.float() for k, v in c["state_dict"].items()}
    c["input"] = c["input"].float()
    c["output64"] = c["output"].double() + c["output64_delta"].double() / c["output64_delta_scale"]
    c["reference_error"] = rel_err(c["output"], c["output64"])
    if c["config"]["activation_function"] == "relu":
        c["statement"] = torch.from_numpy(statement(c["state_dict"], c["input"], c["config"]))
    return c


def build(c, device=None):
    """The registry's module of a case with the reference's weights loaded strictly."""
    import ace_amd
    mod = ace_amd.ModuleSelector(type="AnkurLocalNet", config=dict(c["config"])).build(
        c["n_in_channels"], c["n_out_channels"], ace_amd.DatasetInfo(tuple(c["img_shape"])))
    net = mod.torch_module
    net.load_state_dict(c["state_dict"], strict=True)
    return net.to(device) if device is not None else net


def rel_err(got, want64):
    return float((got.double() - want64).abs().max() / want64.abs().max())


def bits_equal(a, b) -> bool:
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    ok = ~torch.isnan(a)
    return torch.equal(a.view(torch.int32)[ok], b.view(torch.int32)[ok])


def checkpoint(name):
    """A reference-layout stepper checkpoint around a case: the case's net as the single module (keys under the wrappers'
    "module.module."), its first n_out inputs prognostic, the rest forcing, seeded normalisation.  Returns (checkpoint, in, out)."""
    c = case(name)
    cin, cout = c["n_in_channels"], c["n_out_channels"]
    assert cout <= cin
    out_names = [f"p{i}" for i in range(cout)]
    in_names = out_names + [f"f{i}" for i in range(cin - cout)]
    rng = np.random.default_rng(5)
    means = {n: float(rng.normal()) for n in in_names}
    stds = {n: float(0.5 + rng.random()) for n in in_names}
    stepper = {"config": {"step": {"type": "single_module", "config": {
                   "builder": {"type": "AnkurLocalNet", "config": dict(c["config"])}, "in_names": in_names, "out_names": out_names,
                   "normalization": {"network": {"means": means, "stds": stds}}, "ocean": None}}},
               "dataset_info": {"img_shape": list(c["img_shape"]), "timestep": datetime.timedelta(hours=6) // datetime.timedelta(microseconds=1)},
               "step": {"module": {**{f"module.{k}": v.clone() for k, v in c["state_dict"].items()}, "label_encoding": None}}}
    return {"stepper": stepper}, in_names, out_names
