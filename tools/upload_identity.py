#!/usr/bin/env python
"""Bitwise identity of two builds of libace_sfno.so across weight upload and forward (same MI355X, one library after the other).

    python tools/upload_identity.py --parent /path/to/parent/libace_sfno.so [--new ace_amd/libace_sfno.so] [--timing N]

For every case below a child process per library (ACE_SFNO_LIB; a fresh process each, started with subprocess - no process image is
ever replaced) loads seeded weights, runs one eager forward, one forward_graph and one timed forward (taps where the case says so)
and writes the sha256 of every output and tap and the per-stage call counts; the parent process compares the two records.  The
operator-level entries that prepare a weight on every call are hashed the same way, each at one small shape.  It stops at the first
child that exits non-zero.  --timing N: also the wall time of the first sync_weights() of the headline net, N alternating runs.
"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTING = dict(in_chans=5, out_chans=4, img_shape=(24, 48), embed_dim=128, num_layers=3, operator_type="dhconv")
SMALL = dict(in_chans=5, out_chans=4, img_shape=(24, 48), embed_dim=32, num_layers=2, operator_type="dhconv")
SF2 = dict(in_chans=5, out_chans=4, img_shape=(48, 96), embed_dim=128, operator_type="dhconv", scale_factor=2)
HEADLINE = dict(in_chans=44, out_chans=72, img_shape=(180, 360), embed_dim=384, num_layers=8, operator_type="dhconv")
SWITCHES = [("ACE_NO_STRIP", "1"), ("ACE_NO_FOLD", "1"), ("ACE_NO_FFT", "1"), ("ACE_NO_DHCONV_STRIP", "1"), ("ACE_NO_ENC_WS", "1"),
            ("ACE_NO_ENC_PK", "1"), ("ACE_FUSED_PACK", "0"), ("ACE_PLANES_STREAM", "0"), ("ACE_CONV_WS", "none"), ("ACE_CONV_WS", "skip,fc2"),
            ("ACE_CONV_WL", "0")]
CSFNO = dict(embed_dim=256, noise_embed_dim=8, noise_type="gaussian", num_layers=2, use_mlp=True, mlp_ratio=2.0, affine_norms=True,
             normalize_big_skip=True, filter_num_groups=1)


def sfno_cases():
    """(name, config, precision, batch, environment, taps)"""
    c = []
    for b in (1, 2):
        for prec in ("f16x3", "fp32"):
            c.append((f"headline_B{b}_{prec}", HEADLINE, prec, b, {}, False))
    c.append(("routing_default", ROUTING, "f16x3", 2, {}, False))
    c.append(("routing_taps", ROUTING, "f16x3", 2, {}, True))
    c.append(("routing_fp32", ROUTING, "fp32", 2, {}, False))
    c += [(f"routing_{k}={v}", ROUTING, "f16x3", 2, {k: v}, False) for k, v in SWITCHES]
    # (layer_norm with one mixed-grid block is left out: the configuration ADVICE.md asks the library to reject)
    c.append(("sf2_L1_instance_norm", {**SF2, "num_layers": 1}, "f16x3", 2, {}, False))
    for nl in (2, 3):
        for norm in ("instance_norm", "layer_norm"):
            c.append((f"sf2_L{nl}_{norm}", {**SF2, "num_layers": nl, "normalization_layer": norm}, "f16x3", 2, {}, False))
    c.append(("sf2_L3_fp32", {**SF2, "num_layers": 3}, "fp32", 2, {}, False))
    c.append(("sf2_L4", {**SF2, "num_layers": 4}, "f16x3", 2, {}, False))
    c.append(("residual_filter_2", {**SMALL, "residual_filter_factor": 2, "data_grid": "equiangular"}, "f16x3", 2, {}, False))
    c.append(("equiangular", {**ROUTING, "data_grid": "equiangular"}, "f16x3", 2, {}, False))
    for name, kw, prec in [("norm_none", dict(normalization_layer="none"), "f16x3"), ("layer_norm", dict(normalization_layer="layer_norm"), "f16x3"),
                           ("no_mlp", dict(use_mlp=False), "f16x3"), ("no_mlp_none_fp32", dict(use_mlp=False, normalization_layer="none"), "fp32"),
                           ("enc0", dict(encoder_layers=0), "f16x3"), ("enc2", dict(encoder_layers=2), "f16x3"),
                           ("no_pos_embed", dict(pos_embed=False), "f16x3"), ("no_big_skip", dict(big_skip=False), "f16x3"),
                           ("diagonal", dict(operator_type="diagonal"), "f16x3"), ("diagonal_fp32", dict(operator_type="diagonal"), "fp32"),
                           ("embed_20", dict(embed_dim=20), "f16x3"), ("embed_16", dict(embed_dim=16), "f16x3"),
                           ("relu", dict(activation_function="relu"), "f16x3")]:
        c.append((name, {**SMALL, **kw}, prec, 2, {}, False))
    c.append(("embed_128_enc0", {**ROUTING, "encoder_layers": 0}, "f16x3", 2, {}, False))
    c.append(("embed_256_B1", {**ROUTING, "embed_dim": 256, "num_layers": 10}, "f16x3", 1, {}, False))
    return c


def csfno_cases():
    """(name, builder kwargs, environment)"""
    c = [("csfno_g1", CSFNO, {}), ("csfno_g2", {**CSFNO, "filter_num_groups": 2}, {}), ("csfno_nomlp", {**CSFNO, "use_mlp": False}, {})]
    c += [(f"csfno_g2_{k}", {**CSFNO, "filter_num_groups": 2}, {k: "1"}) for k in ("ACE_NO_CLN_MFMA", "ACE_NO_CLN_PLANES", "ACE_DENSE_GROUPED_FILTER")]
    return c


def sha(t):
    import torch
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def build_net(cfg, state, precision):
    from ace_amd.sfno import SphericalFourierNeuralOperatorNet
    keys = ("operator_type", "scale_factor", "residual_filter_factor", "embed_dim", "num_layers", "hard_thresholding_fraction",
            "normalization_layer", "use_mlp", "activation_function", "encoder_layers", "pos_embed", "big_skip", "data_grid")
    params = types.SimpleNamespace(**{k: getattr(cfg, k) for k in keys})
    net = SphericalFourierNeuralOperatorNet(params=params, in_chans=cfg.in_chans, out_chans=cfg.out_chans, img_shape=tuple(cfg.img_shape),
                                            mlp_ratio=cfg.mlp_ratio)
    net.load_state_dict(state, strict=True)
    return net.set_precision(precision).to("cuda").eval()


class Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in self.env:
            del os.environ[k]


def timed_calls(L, call):
    import torch
    ns = L.ace_sfno_num_stages()
    ms, calls = (ctypes.c_float * ns)(), (ctypes.c_int * ns)()
    call(ms, calls)
    torch.cuda.synchronize()
    return list(calls)


_STATES = {}


def run_sfno(name, kw, precision, batch, env, taps):
    import torch
    from ace_amd import _lib
    from oracle.sfno import SFNOConfig, init_state
    cfg = SFNOConfig(**kw)
    key = repr(sorted(kw.items()))
    if key not in _STATES:      # (the headline's 1.7 GB of filter weights are drawn once per process)
        _STATES.clear()
        state = init_state(cfg, seed=21)
        g = torch.Generator().manual_seed(22)
        for k in state:
            if "norm" in k:
                state[k] = state[k] + 0.2 * torch.randn(state[k].shape, generator=g)
        _STATES[key] = state
    state = _STATES[key]
    g = torch.Generator().manual_seed(23)
    x = torch.randn(batch, cfg.in_chans, *cfg.img_shape, generator=g).cuda()
    rec = {}
    with Env(env), torch.no_grad():
        net = build_net(cfg, state, precision)
        L = _lib.lib()
        if taps:
            y, tp = net.forward_with_taps(x)
            rec["taps"] = [sha(t) for t in tp]
        else:
            y = net(x)
        rec["eager"] = sha(y)
        out = torch.empty_like(y)
        net.forward_graph(x, out)
        rec["graph"] = sha(out)
        out.zero_()
        rec["calls"] = timed_calls(L, lambda ms, calls: _lib.check(L.ace_sfno_forward_timed(net._native, _lib.ptr(x), _lib.ptr(out), batch,
                                                                                              _lib.current_stream(), ms, calls)))
        rec["timed"] = sha(out)
        rec["generation"] = int(L.ace_sfno_weights_generation(net._native))
        del net
    return rec


def run_csfno(name, kwargs, env):
    import torch
    import ace_amd
    from ace_amd import _lib
    hw = (16, 32)
    rec = {}
    with Env(env), torch.no_grad():
        torch.manual_seed(11)
        net = ace_amd.ModuleSelector(type="NoiseConditionedSFNO", config=dict(kwargs)).build(5, 4, ace_amd.DatasetInfo(hw)).torch_module
        g = torch.Generator().manual_seed(3)
        state = {k: v.detach().clone() for k, v in net.state_dict().items()}
        for k, v in state.items():
            if v.ndim <= 1 or "W_scale" in k or "W_bias" in k:
                state[k] = v + 0.1 * torch.randn(v.shape, generator=g)
        net.load_state_dict(state, strict=True)
        net.to("cuda").set_precision("f16x3")
        x = torch.randn(2, 5, *hw, generator=g).cuda()
        noise = torch.randn(2, kwargs["noise_embed_dim"], *hw, generator=g).cuda()
        y = net(x, noise=noise)
        rec["eager"] = sha(y)
        L = _lib.lib()
        out = torch.zeros_like(y)
        rec["calls"] = timed_calls(L, lambda ms, calls: _lib.check(L.ace_sfno_forward_conditioned_timed(
            net._native, _lib.ptr(x), _lib.ptr(noise), _lib.ptr(out), 2, _lib.current_stream(), ctypes.cast(ms, ctypes.c_void_p),
            ctypes.cast(calls, ctypes.c_void_p))))
        rec["timed"] = sha(out)
        rec["generation"] = int(L.ace_sfno_weights_generation(net._native))
        del net
    return rec


def run_ops():
    """the operator-level entries that prepare their weight on every call, each at one small shape"""
    import torch
    from ace_amd import _lib
    from ace_amd.healpix import _check as hpx_check
    L, st, dev = _lib.lib(), _lib.current_stream(), "cuda"
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s, f=1.0: (f * torch.randn(*s, generator=g)).to(dev)
    rec = {}
    n, cin, cout, hw = 2, 44, 128, 1152
    x, w, b = rnd(n, cin, hw), rnd(cout, cin, f=0.3), rnd(cout, f=0.1)
    y = torch.empty(n, cout, hw, device=dev)
    _lib.check(L.ace_conv1x1_f16x3(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), n, cin, cout, hw, 1, st))
    rec["ace_conv1x1_f16x3"] = sha(y)
    y = torch.empty(n, cout, hw, device=dev)
    omax = torch.zeros(64, dtype=torch.int32, device=dev)
    d = _lib.Conv1x1FusedDesc(x=_lib.ptr(x), weight=_lib.ptr(w), bias=_lib.ptr(b), y=_lib.ptr(y), out_absmax=omax.data_ptr(), n=n, cin=cin, cin2=0,
                              cout=cout, hw=hw, in_pitch=hw, out_pitch=hw, act=1, cap=float("inf"), engine=2)
    route = _lib.GemmRoute()
    _lib.check(L.ace_conv1x1_fused(ctypes.byref(d), ctypes.byref(route), st))
    rec["ace_conv1x1_fused_engine2"] = [sha(y), sha(omax), route.family, route.tile]
    cin, hid, cout = 128, 256, 128
    t = [rnd(n, cin, hw), rnd(hid, cin, f=0.1), rnd(hid, f=0.1), rnd(cout, hid, f=0.1), rnd(cout, f=0.1)]
    y = torch.empty(n, cout, hw, device=dev)
    _lib.check(L.ace_mlp_f16x3(*[_lib.ptr(v) for v in t], _lib.ptr(y), n, cin, hid, cout, hw, 1, st))
    rec["ace_mlp_f16x3"] = sha(y)
    c, j, hw = 256, 8, 512
    t = [rnd(n, c, hw, f=3.0), rnd(n, j, hw, f=1.7), 1.0 + rnd(c, f=0.3), rnd(c, f=0.2), rnd(c, j, f=0.3), rnd(c, j, f=0.02)]
    y = torch.empty(n, c, hw, device=dev)
    _lib.check(L.ace_conditional_layer_norm_f16x3(*[_lib.ptr(v) for v in t], 1e-5, _lib.ptr(y), n, c, j, hw, st))
    rec["ace_conditional_layer_norm_f16x3"] = sha(y)
    n, c, Lm, Mm = 3, 128, 24, 25
    xs = rnd(n, c, Lm, Mm, 2) * (torch.arange(Mm)[None, :] <= torch.arange(Lm)[:, None]).float().to(dev)[None, None, :, :, None]
    ws = rnd(c, c, Lm, 2, f=1.0 / c)
    out = torch.empty_like(xs)
    _lib.check(L.ace_dhconv_f16x3(_lib.ptr(xs.contiguous()), _lib.ptr(ws), _lib.ptr(out), n, c, Lm, Mm, st))
    rec["ace_dhconv_f16x3"] = sha(out)
    imgs, cin, cout, H, pitch = 12, 24, 40, 16, 16      # a 1 x 1 HEALPix convolution through a prepared weight
    x, w, b = rnd(imgs, cin, H, pitch), rnd(cout, cin, f=0.2), rnd(cout, f=0.1)
    xmax, ymax = torch.zeros(64, dtype=torch.int32, device=dev), torch.zeros(64, dtype=torch.int32, device=dev)
    hpx_check(L.ace_hpx_absmax(x.data_ptr(), x.numel(), xmax.data_ptr(), st))
    h = ctypes.c_void_p()
    hpx_check(L.ace_hpx_weight_create(w.data_ptr(), cout, cin, st, ctypes.byref(h)))
    y = torch.empty(imgs, cout, H, pitch, device=dev)
    hpx_check(L.ace_hpx_conv(x.data_ptr(), None, cin, 0, h, None, b.data_ptr(), None, y.data_ptr(), imgs, cout, H, H, pitch, 1, 1, 1,
                             float("inf"), xmax.data_ptr(), None, ymax.data_ptr(), st))
    rec["ace_hpx_conv"] = [sha(y), sha(ymax)]
    L.ace_hpx_weight_destroy(h)
    return rec


def child(out_path):
    rec = {}
    for name, kw, prec, batch, env, taps in sfno_cases():
        rec[name] = run_sfno(name, kw, prec, batch, env, taps)
        print("ran", name, flush=True)
    for name, kwargs, env in csfno_cases():
        rec[name] = run_csfno(name, kwargs, env)
        print("ran", name, flush=True)
    rec["ops"] = run_ops()
    print("ran ops", flush=True)
    with open(out_path, "w") as f:
        json.dump(rec, f)


def child_upload_time(out_path):
    """wall time of the first sync_weights() of the headline net (f16x3), handle already created"""
    import torch
    from oracle.sfno import SFNOConfig, init_state
    cfg = SFNOConfig(**HEADLINE)
    net = build_net(cfg, init_state(cfg, seed=21), "f16x3")
    net._ensure_native(torch.device("cuda", torch.cuda.current_device()), 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    count = net.sync_weights()
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump({"seconds": time.perf_counter() - t0, "parameters": count}, f)


def spawn(lib, mode, out_path):
    env = dict(os.environ, ACE_SFNO_LIB=os.path.abspath(lib))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), mode, out_path], env=env, timeout=600 if mode == "--child" else 240)
    if res.returncode != 0:   # (a time limit raises, which ends the run as well)
        sys.exit(f"child ({mode}, {lib}) exited with {res.returncode}: stopping")
    with open(out_path) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libace_sfno.so built from the parent commit (ace_amd.build.build(out=..., objdir=...))")
    ap.add_argument("--new", default=os.path.join(ROOT, "ace_amd", "libace_sfno.so"))
    ap.add_argument("--timing", type=int, default=0, metavar="N")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    recs = [spawn(lib, "--child", os.path.join(tmp, f"{tag}.json")) for tag, lib in (("parent", a.parent), ("new", a.new))]
    different = 0
    for name in recs[0]:
        if name == "ops":
            continue
        same = recs[0][name] == recs[1].get(name)
        different += not same
        r = recs[1].get(name, {})
        print(f"   {'EQUAL ' if same else 'DIFFERENT'} {name} calls {r.get('calls')} graph==eager {r.get('graph') == r.get('eager')} uploads {r.get('generation')}")
    print(f"   cases {len(recs[0]) - 1} different {different}")
    for name in recs[0]["ops"]:
        same = recs[0]["ops"][name] == recs[1]["ops"].get(name)
        different += not same
        print(f"   {'EQUAL ' if same else 'DIFFERENT'} op {name}")
    if a.timing:
        secs = {"parent": [], "new": []}
        for i in range(a.timing):
            for tag, lib in (("parent", a.parent), ("new", a.new)):
                secs[tag].append(round(spawn(lib, "--upload-time", os.path.join(tmp, "t.json"))["seconds"], 4))
        for tag in secs:
            print(f"   first sync_weights(), headline f16x3, seconds: {tag} {secs[tag]} median {sorted(secs[tag])[len(secs[tag]) // 2]}")
    return 1 if different else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "--upload-time":
        child_upload_time(sys.argv[2])
    else:
        sys.exit(main())
