"""tests/golden/gen_histogram.pt from the reference's own ComparedDynamicHistograms(n_bins=200, percentiles=[99.9999])
(fme/core/histogram.py, fme/core/metrics.py:355-385; imported through oracle/ref_loader.load_stepper_ref's stubs): three names over
four windows of (2, 3, 9, 18) whose ranges grow and shift, so that every name doubles its range on both sides.  The five value
families: "a" unit Gaussians, then (windows 2, 3) an offset of 250; "q" a scale of 3e-5, then a zero-inflated cubic "precipitation"
field; "ps" an offset of 1e5 with a scale of 900 and a NaN land mask on the target.  Stored: the windows, the raw counts and edges of
both sides, and the float entries of get_wandb()."""
import importlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader  # noqa: E402

SHAPE = (2, 3, 9, 18)


def windows(seed: int):
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(SHAPE, generator=g)                                # noqa: E731
    land = torch.rand(SHAPE[-2:], generator=torch.Generator().manual_seed(99)) < 0.3
    out = []
    for w in range(4):
        a = [r(), 3.0 * r() - 1.0, 250.0 + 20.0 * r(), 250.0 + 45.0 * r() - 60.0][w]
        if w < 2:
            q = 3e-5 * (1.0, 4.0)[w] * r() + (0.0, -2e-5)[w]
        else:
            wet = torch.rand(SHAPE, generator=g) < 0.08
            q = torch.where(wet, (3e-4, 2e-3)[w - 2] * r().abs() ** 3, torch.zeros(SHAPE))
        ps = 1e5 + 900.0 * (1.0, 2.5, 2.5, 7.0)[w] * r() + (0.0, 500.0, -4000.0, 9000.0)[w]
        out.append({"a": a.float(), "q": q.float(), "ps": ps.float(), "land": land})
    return out


def main():
    ref_loader.load_stepper_ref()
    hist = importlib.import_module("fme.core.histogram")
    importlib.import_module("fme.core.metrics")
    names = ["a", "q", "ps"]
    target = [{n: w[n].clone() for n in names} for w in windows(1)]
    prediction = [{n: w[n].clone() for n in names} for w in windows(2)]
    land = windows(1)[0]["land"]
    for t in target:
        t["ps"][..., land] = float("nan")                                     # the mask comes from the target alone
    agg = hist.ComparedDynamicHistograms(n_bins=200, percentiles=[99.9999])
    for t, p in zip(target, prediction):
        agg.record_batch(t, p)
    sides = {"target": agg.target_aggregator, "prediction": agg.prediction_aggregator}
    counts = {s: {n: torch.from_numpy(a.histograms[n].counts[0].copy()) for n in names} for s, a in sides.items()}
    edges = {s: {n: torch.from_numpy(a.histograms[n].bin_edges.copy()) for n in names} for s, a in sides.items()}
    logs = {k: float(v) for k, v in agg.get_wandb().items() if isinstance(v, float)}
    assert len(logs) == 6 and all(int(c.sum()) > 0 for s in counts.values() for c in s.values())
    dst = os.path.join(HERE, "gen_histogram.pt")
    torch.save({"names": names, "target": target, "prediction": prediction, "counts": counts, "edges": edges, "logs": logs}, dst)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
