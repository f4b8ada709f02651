#!/usr/bin/env python
"""AnkurLocalNet at 1 degree (180 x 360), B = 1, 40 inputs -> 256 -> 256 -> 256 -> 20 outputs (the channel counts are an assumption,
not taken from a shipped checkpoint), GELU, DISCO kernel_size 3, on one MI355X.  Every measurement follows a warm-up; the variants
alternate in one process; outputs are compared at the timed size.
  forward  the module's forward (ace_disco_forward + ace_pixel_mlp_forward; with ``use_disco_encoder=False`` one
           ace_pixel_mlp_forward) against a torch path on the same device with the same weights: rfft of the input rows, a banded
           einsum with the conjugate rfft of the psi rows (K, nlat, band, nfreq), irfft, the grouped einsum with the weight, then
           conv2d / activation.  A host clock around work that ends in a device synchronise.
  disco    ``ace_disco_forward`` alone: device events around 20 back-to-back calls of the C entry point on resolved arguments (the
           events see the launches' gaps too: an upper bound on the kernel; no kernel trace is taken), against the torch DISCO
           layer under the same events.  Given with the operations of the statement (2 K per point, pixel and input channel, 2 per
           product of the mix) as a share of the fp32 MFMA / VALU peak (157.3 TF), with x read once and y written once as a share of
           the 8 TB/s HBM peak, and with the heaviest unit's share of the launch's cost (ace_disco_info: the plan, not a trace).
  act      the DISCO launch with GELU / SiLU against the fp64 activation of the same launch's activation-free output, beside
           torch's CPU fp32 F.gelu / F.silu on those values.
Writes profiles/ankur_bench.json and prints it as one JSON line.
usage: python tools/bench_ankur.py [--iters 20] [--warmup 3]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

H, W, B = 180, 360, 1
CIN, EMBED, COUT, KS = 40, 256, 20, 3
HBM, FP32_PEAK = 8e12, 157.3e12


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


def events(fn, reps, iters, warmup):
    """seconds per call: device events around `reps` back-to-back calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / reps)
    return statistics.median(times), min(times), max(times)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


class TorchDisco:
    """The DISCO layer by the detour: rfft, banded contraction with conj(rfft(psi)), irfft, grouped einsum."""

    def __init__(self, table, weight, groups, dev):
        Hh, Ww = table.img_shape
        K = table.K
        rows = np.repeat(np.arange(Hh), np.diff(table.row_offsets))
        lo = np.array([table.hi[table.row_offsets[h]:table.row_offsets[h + 1]].min() for h in range(Hh)])
        hi = np.array([table.hi[table.row_offsets[h]:table.row_offsets[h + 1]].max() for h in range(Hh)])
        band = int((hi - lo).max()) + 1
        lo = np.minimum(lo, Hh - band)
        psi = np.zeros((K, Hh, band, Ww), np.float32)
        psi[:, rows, table.hi - lo[rows], table.wi] = table.vals.T
        self.psi_fft_conj = torch.fft.rfft(torch.from_numpy(psi).to(dev), dim=-1).conj().contiguous()      # (K, H, band, F)
        self.gather = torch.from_numpy((lo[:, None] + np.arange(band)[None, :]).astype(np.int64)).to(dev)      # (H, band)
        self.weight, self.groups, self.W = weight, groups, Ww

    def __call__(self, x):
        Bb, C = x.shape[:2]
        X = torch.fft.rfft(x, dim=-1)                                   # (B, C, H, F)
        Xb = X[:, :, self.gather]                                       # (B, C, H, band, F)
        Z = torch.einsum("bchjf,khjf->bckhf", Xb, self.psi_fft_conj)
        z = torch.fft.irfft(Z, n=self.W, dim=-1)                        # (B, C, K, H, W)
        w = self.weight
        z = z.reshape(Bb, self.groups, C // self.groups, *z.shape[2:])
        out = torch.einsum("bgckxy,gock->bgoxy", z, w.reshape(self.groups, -1, w.shape[1], w.shape[2]))
        return out.reshape(Bb, -1, *out.shape[3:])


def torch_net(net, disco, x, act):
    m = net.module
    mods = list(m.mlp)
    if m.use_disco_encoder:
        x = disco(x)
    else:
        x = F.conv2d(x, mods[0].weight, mods[0].bias)
    i = 1
    if m.use_pos_embed:
        x = x + mods[1].pos_embed
        i = 2
    x = act(x)
    for mod in mods[i + 1:]:
        x = F.conv2d(x, mod.weight, mod.bias) if isinstance(mod, torch.nn.Conv2d) else act(x)
    return x


def bench_forward(use_disco, pos_embed, dev, iters, warmup):
    import ace_amd
    torch.manual_seed(0)
    cfg = {"embed_dim": EMBED, "use_disco_encoder": use_disco, "disco_kernel_size": KS, "pos_embed": pos_embed,
           "activation_function": "gelu"}
    net = ace_amd.ModuleSelector(type="AnkurLocalNet", config=cfg).build(CIN, COUT, ace_amd.DatasetInfo((H, W))).torch_module.to(dev).eval()
    x = torch.randn(B, CIN, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    m = net.module
    disco = TorchDisco(m.table, m.mlp[0].conv.weight.detach(), m.mlp[0].conv.groups, dev) if use_disco else None
    with torch.no_grad():
        fused, eager = net(x), torch_net(net, disco, x, F.gelu)
        torch.cuda.synchronize()
        out = {"config": cfg, "fused_vs_torch": rel(fused, eager)}
        rows = {"fused": [], "torch": []}
        for _ in range(3):
            rows["fused"].append(wall(lambda: net(x), iters, warmup))
            rows["torch"].append(wall(lambda: torch_net(net, disco, x, F.gelu), iters, warmup))
        for k, r in rows.items():
            out[f"{k}_seconds"] = statistics.median(t[0] for t in r)
            out[f"{k}_min_max"] = [min(t[1] for t in r), max(t[2] for t in r)]
        out["speedup_over_torch"] = out["torch_seconds"] / out["fused_seconds"]
    return out


def bench_disco(dev, iters, warmup):
    from ace_amd import disco as D
    groups = math.gcd(CIN, EMBED)
    gs = CIN // groups
    table = D.disco_table((H, W), KS)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, CIN, H, W, generator=g).to(dev)
    w = (torch.randn(EMBED, gs, KS * KS, generator=g) / math.sqrt(gs * KS * KS)).to(dev)
    y = torch.empty(B, EMBED, H, W, device=dev)
    ref = TorchDisco(table, w, groups, dev)
    res = {}
    points = int(table.row_offsets[-1])
    flop = 2 * B * W * (points * CIN * KS * KS + H * EMBED * gs * KS * KS)
    nbytes = 4 * B * H * W * (CIN + EMBED)
    with torch.no_grad():
        outs = {}
        for name, act in (("none", D.ACT_NONE), ("gelu", D.ACT_GELU), ("silu", D.ACT_SILU)):
            h = D.DiscoHandle(table, w, CIN, EMBED, groups, act, False)
            if name == "none":
                res["plan"] = h.info()
                res["plan"]["heaviest_unit_share_of_cost"] = res["plan"]["heaviest_unit_cost"] / res["plan"]["total_cost"]
            call = lambda: h.forward(x.data_ptr(), None, y.data_ptr(), B)     # noqa: E731
            call()
            torch.cuda.synchronize()
            outs[name] = y.cpu().clone()
            if name != "silu":
                t = events(call, 20, iters, warmup)
                tw = wall(call, iters, warmup)
                res[f"launch_{name}"] = {"seconds": t[0], "min_max": [t[1], t[2]], "host_clock_single_call_seconds": tw[0],
                                         "flop_per_second": flop / t[0], "share_of_fp32_peak": flop / t[0] / FP32_PEAK,
                                         "bytes_per_second": nbytes / t[0], "share_of_8TBps_peak": nbytes / t[0] / HBM}
            h.close()
        want = ref(x)
        torch.cuda.synchronize()
        res["fused_vs_torch_layer"] = rel(outs["none"].to(dev), want)
        t = events(lambda: ref(x), 5, max(3, iters // 2), warmup)
        res["torch_layer"] = {"seconds": t[0], "min_max": [t[1], t[2]]}
        res["speedup_over_torch_layer"] = res["torch_layer"]["seconds"] / res["launch_none"]["seconds"]
        res["seconds_is"] = ("device events around back-to-back C-ABI calls: launch gaps included, an upper bound on the kernel's "
                             "duration (no kernel trace was taken, no per-workgroup spread measured)")
        res["flop"], res["bytes_x_once_y_once"], res["support_points"] = flop, nbytes, points
        least = max(flop / FP32_PEAK, nbytes / HBM)
        res["bound"] = "fp32 rate" if flop / FP32_PEAK > nbytes / HBM else "HBM"
        res["least_seconds_the_hardware_could_take"] = least
        res["share_of_peak"] = least / res["launch_none"]["seconds"]
        pre = outs["none"].double()
        acts = {}
        for name, truth, fn in (("gelu", 0.5 * pre * (1.0 + torch.special.erf(pre / math.sqrt(2.0))), F.gelu),
                                ("silu", pre / (1.0 + torch.exp(-pre)), F.silu)):
            acts[name] = {"kernel_max_abs_error": float((outs[name].double() - truth).abs().max()),
                          "torch_cpu_fp32_max_abs_error": float((fn(outs["none"]).double() - truth).abs().max())}
        res["activation_errors_against_fp64"] = acts
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ankur needs an MI355X: nothing is measured without one")
    dev = torch.device("cuda", 0)
    from ace_amd import build
    result = {"device": torch.cuda.get_device_name(0), "shape": [B, H, W], "channels": [CIN, EMBED, EMBED, EMBED, COUT],
              "channel_counts_are_an_assumption": True, "kernel_source_sha256": build.source_sha256()[:12], "iters": args.iters,
              "warmup": args.warmup,
              "forward_clock": "host perf_counter around work ending in a device synchronise; medians of three alternating rounds",
              "forward": {"disco_encoder": bench_forward(True, False, dev, args.iters, args.warmup),
                          "disco_encoder_pos_embed": bench_forward(True, True, dev, args.iters, args.warmup),
                          "conv_encoder_pos_embed": bench_forward(False, True, dev, args.iters, args.warmup)},
              "disco": bench_disco(dev, args.iters, args.warmup)}
    path = os.path.join(ROOT, "profiles", "ankur_bench.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
