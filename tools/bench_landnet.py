#!/usr/bin/env python
"""LandNet at 1 degree (180 x 360), B = 1, 30 inputs -> [64, 64] -> 10 outputs (the channel counts are an assumption, not taken
from a shipped checkpoint), with and without the positional embedding, on one MI355X.  Every measurement follows a warm-up and is
a host clock around work that ends in a device synchronise; the variants alternate in one process; outputs are compared at the
timed size.
  forward  ``LandNet.forward`` (one ace_pixel_mlp_forward) against the same weights through (a) the layer-by-layer ``ace_hpx_conv``
           chain ColumnMLP is built on (ace_hpx_absmax + one compensated-fp16 1 x 1 convolution per layer with ReLU in the
           epilogue, the embedding added by torch) and (b) ``torch.nn.functional.conv2d`` / ``relu`` on the device
  kernel   ``ace_pixel_mlp_forward`` alone: 50 back-to-back calls of the C entry point on resolved arguments per synchronise.  The
           figure is the launch-to-launch interval, an UPPER BOUND on the kernel's duration (host issue rate and launch gaps are in
           it; no kernel trace is taken), given with the bytes the kernel must move (input, output, embedding); no share of the 8 TB/s peak is claimed where a launch takes under 10 microseconds: that is latency
  engine   a ``LandRolloutEngine`` step in each graph mode (T = 8) against ``Stepper.predict`` on the same stepper
Writes profiles/landnet_bench.json and prints it as one JSON line.
usage: python tools/bench_landnet.py [--iters 30] [--warmup 5] [--no-engine]"""
import argparse
import ctypes
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

H, W, B = 180, 360, 1
CIN, HIDDEN, COUT = 30, [64, 64], 10
HBM = 8e12


def wall(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


class HpxChain:
    """the same weights on the existing per-layer operator: what a LandNet costs without the fused kernel"""

    def __init__(self, net):
        from ace_amd import _lib
        from ace_amd.healpix import _check
        self.net, self.handles, self.bias = net, [], []
        for layer in net.model:
            c = layer.conv
            w = c.weight.detach().reshape(c.out_channels, c.in_channels).contiguous()
            h = ctypes.c_void_p()
            _check(_lib.lib().ace_hpx_weight_create(w.data_ptr(), w.shape[0], w.shape[1], _lib.current_stream(), ctypes.byref(h)))
            self.handles.append(h)
            self.bias.append(c.bias.detach().contiguous())

    def __call__(self, x):
        from ace_amd import _lib
        from ace_amd.healpix import _INF, _check
        L, st = _lib.lib(), _lib.current_stream()
        n = len(self.handles)
        slots = torch.zeros(64 * (n + 1), dtype=torch.int32, device=x.device)
        _check(L.ace_hpx_absmax(x.data_ptr(), x.numel(), slots.data_ptr(), st))
        cur = x
        for i, layer in enumerate(self.net.model):
            c = layer.conv
            y = torch.empty(B, c.out_channels, H, W, dtype=torch.float32, device=x.device)
            _check(L.ace_hpx_conv(cur.data_ptr(), None, c.in_channels, 0, self.handles[i], None, self.bias[i].data_ptr(), None,
                                  y.data_ptr(), B, c.out_channels, H, W, W, 1, 1, 2 if layer.relu else 0, _INF,
                                  slots[64 * i:].data_ptr(), None, slots[64 * (i + 1):].data_ptr(), st))
            if i == 0 and self.net.use_positional_embedding:
                # the range slot of y was taken before the addition: refresh it, as a second absmax launch
                y = y + self.net.pos_embed.pos_embed
                slots[64 * (i + 1): 64 * (i + 2)].zero_()
                _check(L.ace_hpx_absmax(y.data_ptr(), y.numel(), slots[64 * (i + 1):].data_ptr(), st))
            cur = y
        return cur

    def close(self):
        from ace_amd import _lib
        for h in self.handles:
            _lib.lib().ace_hpx_weight_destroy(h)


def torch_chain(net, x):
    for i, layer in enumerate(net.model):
        x = F.conv2d(x, layer.conv.weight, layer.conv.bias)
        if layer.relu:
            x = F.relu(x)
        if i == 0 and net.use_positional_embedding:
            x = x + net.pos_embed.pos_embed
    return x


def bench_forward(embed, dev, iters, warmup):
    from ace_amd.landnet import LandNet
    torch.manual_seed(0)
    net = LandNet((H, W), CIN, HIDDEN, COUT, use_positional_embedding=embed).to(dev).eval()
    x = torch.randn(B, CIN, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    chain = HpxChain(net)
    with torch.no_grad():
        fused, layered, eager = net(x), chain(x), torch_chain(net, x)
        ref64 = torch_chain(net.double(), x.double())
        net.float()
        torch.cuda.synchronize()
        out = {"fused_vs_fp64": rel(fused, ref64), "hpx_chain_vs_fp64": rel(layered, ref64), "torch_vs_fp64": rel(eager, ref64)}
        rows = {"fused": [], "hpx_chain": [], "torch": []}
        for _ in range(3):                  # alternate the three
            rows["fused"].append(wall(lambda: net(x), iters, warmup))
            rows["hpx_chain"].append(wall(lambda: chain(x), iters, warmup))
            rows["torch"].append(wall(lambda: torch_chain(net, x), iters, warmup))
        for k, r in rows.items():
            out[f"{k}_seconds"] = statistics.median(t[0] for t in r)
            out[f"{k}_min_max"] = [min(t[1] for t in r), max(t[2] for t in r)]
        out["speedup_over_hpx_chain"] = out["hpx_chain_seconds"] / out["fused_seconds"]
        out["speedup_over_torch"] = out["torch_seconds"] / out["fused_seconds"]
        # the launch alone
        y = torch.empty(B, COUT, H, W, device=dev)
        reps = 50

        from ace_amd import _lib
        fwd, st = _lib.lib().ace_pixel_mlp_forward, _lib.current_stream()
        args = (net._handle(), x.data_ptr(), net.pos_embed.pos_embed.data_ptr() if embed else None, y.data_ptr(), B, H * W, st)

        def launches():                     # the C entry point on resolved arguments: no Python bookkeeping between two launches
            for _ in range(reps):
                fwd(*args)
        t = wall(launches, iters, warmup)
        per = t[0] / reps
        nbytes = 4 * H * W * (B * (CIN + COUT) + (HIDDEN[0] if embed else 0))
        latency_bound = per < 10e-6
        out.update({"kernel_seconds_is": "the launch-to-launch interval of 50 back-to-back C-ABI calls under one synchronise: an upper "
                                         "bound on the kernel's duration (no kernel trace was taken)",
                    "kernel_seconds": per, "kernel_min_max": [t[1] / reps, t[2] / reps], "kernel_bytes": nbytes,
                    "kernel_bytes_per_second": nbytes / per, "latency_bound": latency_bound,
                    "share_of_8TBps_peak": None if latency_bound else nbytes / per / HBM,
                    "flop": 2 * B * H * W * sum(a * b for a, b in zip([CIN] + HIDDEN, HIDDEN + [COUT]))})
        out["flop_per_second"] = out["flop"] / per
    chain.close()
    return out


def bench_engine(dev, iters, warmup, T=8):
    from ace_amd.checkpoint import load_stepper
    from ace_amd.land_rollout import LandRolloutEngine
    from ace_amd.landnet import LandNet
    prog = [f"p{i}" for i in range(COUT - 2)]
    out_names = prog + ["d0", "d1"]
    forcing_names = [f"f{i}" for i in range(CIN - len(prog))]
    in_names = forcing_names + prog
    torch.manual_seed(0)
    cfg = {"hidden_dims": HIDDEN, "network_type": "MLP", "use_positional_embedding": True}
    net = LandNet((H, W), CIN, HIDDEN, COUT, use_positional_embedding=True)
    names = in_names + ["d0", "d1"]
    mask = (torch.rand(H, W, generator=torch.Generator().manual_seed(1)) > 0.7).float()
    state = {"stepper": {
        "config": {"input_masking": {"mask_value": 0, "fill_value": "mean"},
                   "step": {"type": "single_module", "config": {
                       "builder": {"type": "LandNet", "config": cfg}, "in_names": in_names, "out_names": out_names,
                       "normalization": {"network": {"means": {n: 0.1 for n in names}, "stds": {n: 1.5 for n in names}}}, "ocean": None}}},
        "dataset_info": {"img_shape": [H, W], "timestep": datetime.timedelta(hours=6) // datetime.timedelta(microseconds=1),
                         "mask_provider": {"masks": {"mask_2d": mask}}},
        "step": {"module": {**{f"module.{k}": v for k, v in net.state_dict().items()}, "label_encoding": None}}}}
    stepper = load_stepper(state, device=dev).stepper
    g = torch.Generator().manual_seed(2)
    ic = {n: torch.randn(B, 1, H, W, generator=g).to(dev) for n in prog}
    forcing = {n: torch.randn(B, T + 1, H, W, generator=g).to(dev) for n in forcing_names}
    want, _ = stepper.predict(ic, forcing)
    torch.cuda.synchronize()
    res = {"steps_per_window": T}
    t = wall(lambda: stepper.predict(ic, forcing), iters, warmup)
    res["stepper_predict"] = {"step_seconds": t[0] / T, "min_max": [t[1] / T, t[2] / T]}
    for graph in (None, "step", "window"):
        eng = LandRolloutEngine(stepper, batch=B, n_forward_steps=T, graph=graph)
        got, _ = eng.predict(ic, forcing)
        torch.cuda.synchronize()
        same = all(torch.equal(torch.isnan(got[k]), torch.isnan(want[k]))
                   and torch.equal(got[k].nan_to_num().view(torch.int32), want[k].nan_to_num().view(torch.int32)) for k in want)
        t = wall(eng.run_window, iters, warmup)
        res[f"engine_graph_{graph}"] = {"step_seconds": t[0] / T, "min_max": [t[1] / T, t[2] / T], "bitwise_equal_to_predict": same,
                                        "speedup_over_predict": res["stepper_predict"]["step_seconds"] / (t[0] / T)}
        del eng
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-engine", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_landnet needs an MI355X: nothing is measured without one")
    dev = torch.device("cuda", 0)
    from ace_amd import build
    result = {"device": torch.cuda.get_device_name(0), "shape": [B, H, W], "channels": [CIN] + HIDDEN + [COUT],
              "channel_counts_are_an_assumption": True, "kernel_source_sha256": build.source_sha256()[:12], "iters": args.iters,
              "warmup": args.warmup, "clock": "host perf_counter around work ending in a device synchronise; medians",
              "forward": {"with_embedding": bench_forward(True, dev, args.iters, args.warmup),
                          "without_embedding": bench_forward(False, dev, args.iters, args.warmup)}}
    if not args.no_engine:
        result["engine_step"] = bench_engine(dev, max(5, args.iters // 3), args.warmup)
    path = os.path.join(ROOT, "profiles", "landnet_bench.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
