"""The paired windows the evaluator's trend / enso_coefficient / near_zero_fraction tests record, on the CPU and on the GPU: one
initial condition and two windows of (B, T, H, W) with a time axis of 365-day steps and an index table, and the fp64 truth of the
ENSO coefficients with the fp32 floor the GPU test's bar is made of."""
import datetime

import torch

from ace_amd.dataset_info import DatasetInfo
from ace_amd.timeaxis import TimeAxis

B, T = 2, 3
N_TIME = 1 + 2 * T
STEP = datetime.timedelta(days=365)              # 7 time levels x 365 days > the ENSO coefficient's 1800 days
SHAPES = {(9, 18): 3, (45, 90): 4}               # (H, W) -> seed; tests/test_regress_ref_cpu.py checks the floor these seeds give
NAMES = ["t", "pr"]


def info(H, W, timestep=STEP):
    lat = torch.tensor([-90 + (i + 0.5) * 180 / H for i in range(H)], dtype=torch.float64)
    lon = torch.tensor([j * 360 / W for j in range(W)], dtype=torch.float64)
    return DatasetInfo((H, W), timestep=timestep, lat=lat, lon=lon)


def case(H, W):
    """"t": an anomaly field carrying a trend and the index signal; "pr": zero-inflated, for the near-zero fraction"""
    g = torch.Generator().manual_seed(SHAPES[(H, W)])
    time = TimeAxis.regular((2011, 3, 1), STEP, N_TIME, n_samples=B)
    time = TimeAxis(time.calendar, time.us + (torch.arange(B)[:, None] * 40 * 86_400_000_000).numpy())      # samples start 40 days apart
    index = torch.randn(B, N_TIME, generator=g, dtype=torch.float64)
    centred = (index - index.mean(dim=1, keepdim=True)).float()
    pattern = torch.randn(2, H, W, generator=g)
    record = []
    for side in range(2):
        ramp = (0.2 + 0.1 * side) * torch.arange(N_TIME, dtype=torch.float32)[None, :, None, None]
        t = ramp + centred[:, :, None, None] * pattern[side] + 0.5 * torch.randn(B, N_TIME, H, W, generator=g)
        wet = torch.rand(B, N_TIME, H, W, generator=g) < 0.3
        pr = torch.where(wet, 3e-4 * torch.randn(B, N_TIME, H, W, generator=g).abs() ** 3, torch.zeros(()))
        record.append({"t": t.float(), "pr": pr.float()})
    gen, target = record
    windows = [(({n: gen[n][:, 1 + w * T:1 + (w + 1) * T] for n in NAMES}, {n: target[n][:, 1 + w * T:1 + (w + 1) * T] for n in NAMES}),
                time[:, 1 + w * T:1 + (w + 1) * T]) for w in range(2)]
    ic = {n: target[n][:, :1] for n in NAMES}
    return {"info": info(H, W), "time": time, "index": index, "centred": centred, "record": record, "windows": windows, "ic": ic}


def enso_truth(c):
    """name -> [target, prediction] fp64 coefficients over the recorded steps 1.., on the fp32 index values both paths regress on"""
    idx = c["centred"].double()[:, 1:]
    out = {}
    for n in NAMES:
        per_side = []
        for side in (1, 0):
            x = c["record"][side][n][:, 1:].double()
            cov = (x * idx[:, :, None, None]).sum(dim=1)
            per_side.append((cov / (idx ** 2).sum(dim=1)[:, None, None]).mean(dim=0))
        out[n] = per_side
    return out


def enso_fp32(c):
    """the same in the reference's fp32 arithmetic, window by window (enso_coefficient.py:136-187), on the CPU"""
    out = {}
    for n in NAMES:
        per_side = []
        for side in (1, 0):
            coefs = []
            for b in range(B):
                cov, var = None, torch.tensor(0.0)
                for w in range(2):
                    iw = c["centred"][b, 1 + w * T:1 + (w + 1) * T]
                    var = var + (iw ** 2).sum()
                    part = (c["record"][side][n][b, 1 + w * T:1 + (w + 1) * T] * iw.view(T, 1, 1)).sum(dim=0)
                    cov = part if cov is None else cov + part
                coefs.append(cov / var)
            per_side.append(torch.stack(coefs).mean(dim=0))
        out[n] = per_side
    return out


def enso_floor(c):
    """name -> the largest |fp32 path - fp64 truth| over both sides and all pixels, and max |truth|"""
    truth, low = enso_truth(c), enso_fp32(c)
    return {n: (max(float((low[n][s].double() - truth[n][s]).abs().max()) for s in (0, 1)),
                max(float(truth[n][s].abs().max()) for s in (0, 1))) for n in NAMES}
