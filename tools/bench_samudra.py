#!/usr/bin/env python
"""The Samudra ocean emulator in its shipped configuration (configs/baselines/cm4-piControl: 90 in / 80 out channels, ch_width
[200, 250, 300, 400], dilation [1, 2, 4, 8], instance norm, circular padding) at 1 degree (180 x 360), B = 1, seeded weights:
ms per forward on one MI355X, timed with events over hipGraph replays after a warm-up.  Prints one JSON line with the dense FLOP
count of the convolutions, its fraction of the f16x3 MFMA rate (three fp16 MFMAs per product: 2.5 PFLOP/s dense fp16 / 3), and
the GPU time of one eager forward split between the convolution engine and the lat-lon glue kernels (events around each
native call).  usage: python tools/bench_samudra.py [--iters 20] [--warmup 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import ace_amd  # noqa: E402
from ace_amd import samudra  # noqa: E402

F16_DENSE = 2.5e15
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--H", type=int, default=180)
ap.add_argument("--W", type=int, default=360)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.manual_seed(0)
net = ace_amd.ModuleSelector(type="Samudra", config={}).build(90, 80, ace_amd.DatasetInfo((args.H, args.W))).torch_module.to(dev).eval()
x = torch.randn(1, 90, args.H, args.W, device=dev)

# dense FLOPs of the convolutions at the resolution each one runs at
plan = net.plan(args.H, args.W)
flops = 0
nconv = 0
for blk, lvl in net.blocks_by_level():
    H, W = plan.sizes[lvl]
    convs = [m for m in blk.modules() if isinstance(m, torch.nn.Conv2d)]
    for c in convs:
        flops += 2 * c.out_channels * c.in_channels * c.kernel_size[0] * c.kernel_size[1] * H * W
    nconv += len(convs)
last = net.layers[-1]
flops += 2 * last.out_channels * last.in_channels * 9 * args.H * args.W
nconv += 1

with torch.no_grad():
    for _ in range(args.warmup):
        net(x)
    torch.cuda.synchronize()
    cap = samudra.CapturedSamudraForward(net, x, warmup=1)
    for _ in range(args.warmup):
        cap(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        cap(x)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.iters

    # split of one eager forward: events around every native call, grouped by engine / glue
    ENGINE = ("ace_hpx_conv_packed", "ace_hpx_conv1_packed")
    real_lib = samudra._lib.lib()
    marks = []

    class _Timed:
        def __getattr__(self, name):
            fn = getattr(real_lib, name)
            if not name.startswith(("ace_hpx_", "ace_ll_")) or name.endswith("last_error") or name.startswith("ace_hpx_weight"):
                return fn

            def call(*a):
                s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                rc = fn(*a)
                t.record()
                marks.append((name, s, t))
                return rc
            return call

    class _LibProxy:
        def __getattr__(self, name):
            return getattr(samudra_lib_module, name)

        @staticmethod
        def lib():
            return _Timed()

    samudra_lib_module = samudra._lib
    samudra._lib = _LibProxy()
    try:
        net(x)
        torch.cuda.synchronize()
    finally:
        samudra._lib = samudra_lib_module
    split = {}
    for name, s, t in marks:
        split[name] = split.get(name, 0.0) + s.elapsed_time(t)
engine_ms = sum(v for k, v in split.items() if k in ENGINE)
glue_ms = sum(v for k, v in split.items() if k not in ENGINE)
print(json.dumps({
    "model": "Samudra", "grid": [args.H, args.W], "batch": 1, "in_channels": 90, "out_channels": 80, "ch_width": net.ch_width,
    "dilation": net.dilation, "norm": net.norm, "device": torch.cuda.get_device_name(0), "iters": args.iters,
    "ms_per_forward": round(ms, 4), "convolutions": nconv, "tflop_per_forward": round(flops / 1e12, 4),
    "tflops": round(flops / (ms * 1e-3) / 1e12, 1), "fraction_of_f16x3_rate": round(flops / (ms * 1e-3) / (F16_DENSE / 3), 4),
    "eager_split_ms": {"gemm_engine": round(engine_ms, 4), "glue": round(glue_ms, 4),
                       "by_entry": {k: round(v, 4) for k, v in sorted(split.items())}},
}))
