"""tests/golden/gen_regress.pt from the reference's own functions (imported through oracle/ref_loader.load_stepper_ref's stubs, the
aggregator packages as bare namespaces and their plotting / build-context / data modules as permissive stubs):
  * ``TrendEvaluatorAggregator._add_running_sums`` (fme/ace/aggregator/inference/trend.py:104-130) over the windows, sliced as its
    ``record_batch`` slices them (trend.py:136-147), and the slope formula of ``_get_trends`` (trend.py:185-192);
  * ``data_index_covariance`` (enso/enso_coefficient.py:418-437) per sample and window, accumulated as ``record_batch`` does
    (enso_coefficient.py:136-168), with the fp32 index variance;
  * ``NearZeroFractionAggregator`` (near_zero_fraction.py:97-216) with a plain weighted mean and ``include_maps``.
Two windows of (2, 4, 9, 18), the first at time index 0 (its first step is dropped by the trend and the near-zero fraction, not by
the ENSO sums), two names: "t" a temperature-like field with a trend and an index signal, "pr" a zero-inflated field."""
import importlib
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader  # noqa: E402

B, T, H, W = 2, 4, 9, 18
EPS = {"t": 287.0, "pr": 0.0}


def inputs():
    g = torch.Generator().manual_seed(7)
    lat = torch.tensor([-90 + (i + 0.5) * 180 / H for i in range(H)], dtype=torch.float64)
    weights = torch.cos(torch.deg2rad(lat)).float()[:, None].expand(H, W).contiguous()
    weights[0] = 0.0                                                            # a row of weight 0 leaves the fractions
    years = 14.0 + 0.25 * torch.arange(2 * T, dtype=torch.float64)[None] + torch.tensor([[0.0], [3.5]], dtype=torch.float64)
    raw = torch.randn(B, 2 * T, generator=g, dtype=torch.float64)
    index = (raw - raw.mean(dim=1, keepdim=True)).float()
    pattern = torch.randn(H, W, generator=g)
    sides = []
    for side in range(2):
        wins = []
        for w in range(2):
            sl = slice(w * T, (w + 1) * T)
            noise = torch.randn(B, T, H, W, generator=g)
            t = 287.0 + (0.3 + 0.1 * side) * years[:, sl, None, None].float() + index[:, sl, None, None] * pattern + noise
            wet = torch.rand(B, T, H, W, generator=g) < 0.3
            pr = torch.where(wet, 3e-4 * torch.randn(B, T, H, W, generator=g).abs() ** 3, torch.zeros(()))
            wins.append({"t": t.float(), "pr": pr.float()})
        sides.append(wins)
    return weights, years, index, sides[0], sides[1]


def main():
    ref_loader.load_stepper_ref()
    ref = os.path.join(ref_loader.REF, "fme", "ace", "aggregator")
    for name, path in (("fme.ace.aggregator", ref), ("fme.ace.aggregator.inference", os.path.join(ref, "inference")),
                       ("fme.ace.aggregator.inference.enso", os.path.join(ref, "inference", "enso"))):
        ref_loader._ns(name, path)
    permissive = type(sys.modules["xarray"])
    for name in ("fme.ace.aggregator.plotting", "fme.ace.aggregator.inference.build_context",
                 "fme.ace.aggregator.inference.data"):
        sys.modules[name] = permissive(name)
    trend = importlib.import_module("fme.ace.aggregator.inference.trend")
    enso = importlib.import_module("fme.ace.aggregator.inference.enso.enso_coefficient")
    nzf = importlib.import_module("fme.ace.aggregator.inference.near_zero_fraction")

    weights, years, index, gen, target = inputs()
    out = {"weights": weights, "years": years, "index": index, "gen": gen, "target": target, "eps": EPS}

    # trend
    n = sum_t = sum_tt = torch.zeros((), dtype=torch.float64)
    sums = {"gen": ({}, {}), "target": ({}, {})}
    for w in range(2):
        sl = slice(1, None) if w == 0 else slice(None)                          # trend.py:136: i_time_start == 0
        t = years[:, w * T:(w + 1) * T][:, sl]
        n, sum_t, sum_tt = n + t.numel(), sum_t + t.sum(), sum_tt + (t * t).sum()
        for key, wins in (("gen", gen), ("target", target)):
            trend.TrendEvaluatorAggregator._add_running_sums(sums[key][0], sums[key][1], {k: v[:, sl] for k, v in wins[w].items()}, t)
    denom = n * sum_tt - sum_t * sum_t
    out["trend"] = {key: {"sum_y": sy, "sum_ty": sty, "slope": {k: (n * sty[k] - sum_t * sy[k]) / denom for k in sy}}
                    for key, (sy, sty) in sums.items()}
    out["trend"]["n_sum_t_sum_tt"] = torch.stack([n, sum_t, sum_tt])

    # ENSO covariance
    cov = {key: [{} for _ in range(B)] for key in ("gen", "target")}
    var = [torch.tensor(0.0) for _ in range(B)]
    for w in range(2):
        for b in range(B):
            iw = index[b, w * T:(w + 1) * T]
            var[b] = var[b] + (iw ** 2).sum()
            for key, wins in (("gen", gen), ("target", target)):
                for k, v in wins[w].items():
                    c = enso.data_index_covariance(v[b, :], iw)
                    cov[key][b][k] = cov[key][b][k] + c if k in cov[key][b] else c
    out["enso"] = {"covariance": cov, "index_variance": torch.stack(var),
                   "coefficient": {key: {k: torch.stack([cov[key][b][k] / var[b] for b in range(B)]).mean(dim=0) for k in ("t", "pr")}
                                   for key in ("gen", "target")}}

    # near-zero fraction
    def weighted_mean(x, name=None):
        return (x * weights).sum(dim=(-2, -1)) / weights.sum()
    agg = nzf.NearZeroFractionAggregator(area_weighted_mean=weighted_mean, eps=123.0, per_variable_eps=EPS, include_maps=True)
    for w in range(2):
        agg.record_batch(types.SimpleNamespace(prediction=gen[w], target=target[w], has_target=True, i_time_start=w * T))
    out["nzf"] = {"gen_sum": agg._gen_sum, "gen_count": agg._gen_count, "target_sum": agg._target_sum,
                  "target_count": agg._target_count, "gen_map_sum": agg._gen_map_sum, "target_map_sum": agg._target_map_sum,
                  "map_count": agg._gen_map_count}
    dst = os.path.join(HERE, "gen_regress.pt")
    torch.save(out, dst)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
