"""The fused inference evaluator aggregator (csrc/diag.hip: ace_diag_paired_window, ace_diag_spectrum) at 180 x 360 against fp64
restatements of the reference's InferenceEvaluatorAggregator, against its own torch path, bitwise against itself, with a normaliser
that counts its calls, and under ``run_evaluator`` on the SFNO and Samudra fixtures of test_gpu_aggregator.py.

Tolerances as in tests/test_evaluator_aggregator_cpu.py: 1e-6 relative for means and linear quantities, 1e-5 for std-like ones; a
difference is judged against the scale of its minuend; against the fp32 torch path a normalised quantity is judged against
(scale + |mu|) / sigma."""
import copy

import pytest
import torch

from ace_amd.evaluator import InferenceEvaluatorAggregatorConfig, ZonalMeanMetricConfig
from ace_amd.normalizer import StandardNormalizer
from oracle.sht import RealSHT as OracleSHT
from _util import load_golden
from test_gpu_aggregator import NLAT, NLON, dev, fields, one_degree_info  # noqa: F401

pytestmark = pytest.mark.gpu

STATS = {"a": (0.2, 1.1), "smooth": (0.0, 0.7), "q": (5e-4, 3e-4), "PRESsfc": (1e5, 1.5e2), "sst": (289.0, 5.5)}   # not "derived"
# the statistics as the normaliser holds them (fp32): the fp64 restatement normalises with the same numbers
STATS = {k: (float(torch.tensor(m, dtype=torch.float32)), float(torch.tensor(s, dtype=torch.float32))) for k, (m, s) in STATS.items()}
STD_LIKE = ("weighted_std_gen", "weighted_rmse", "weighted_grad_mag_percent_diff")


class CountingNormalizer(StandardNormalizer):
    calls = 0

    def normalize(self, tensors, apply_mean=True):
        self.calls += 1
        return super().normalize(tensors, apply_mean)


def normalizer(dev):
    return CountingNormalizer({k: v[0] for k, v in STATS.items()}, {k: v[1] for k, v in STATS.items()}, device=dev)


def record(dev, windows=(3, 3, 2), B=2):
    g = torch.Generator().manual_seed(4)
    ic = {k: v for k, v in fields(g, B, 1, dev).items() if k != "derived"}
    wins = [fields(g, B, t, dev) for t in windows]
    tgts = []
    for win in wins:
        tgts.append({n: x + (0.05 * STATS[n][1]) * torch.randn(x.shape, generator=g).to(dev) for n, x in win.items() if n in STATS})
    return ic, wins, tgts


def build(info, n_time, norm, fused=True, max_size=4096):
    cfg = InferenceEvaluatorAggregatorConfig(zonal_mean=ZonalMeanMetricConfig(zonal_mean_max_size=max_size))
    agg = cfg.build(info, 1, n_time - 1, normalize=norm)
    agg.fused = fused
    return agg


def run(info, ic, wins, tgts, norm, fused=True, max_size=4096):
    agg = build(info, 1 + sum(next(iter(w.values())).shape[1] for w in wins), norm, fused, max_size)
    agg.record_initial_condition(ic)
    for win, tgt in zip(wins, tgts):
        assert agg.route(win, tgt) == ("fused" if fused else "torch")
        agg.record_batch(win, tgt)
    return agg


# ---- fp64 restatement (reduced.py:221-316, time_mean.py:103-162, 339-401, zonal_mean.py:153-306, metrics.py:63-224) -------------
def wmean(x, w):
    return (x.where(w != 0, 0.0) * w).sum((-2, -1)) / w.sum()


def gradmean(x, w):
    gy, gx = torch.gradient(x, dim=(-2, -1))
    g = torch.sqrt(gy ** 2 + gx ** 2)
    return (g * w).nansum((-2, -1)) / torch.where(torch.isnan(g), 0.0, w.expand(g.shape)).sum((-2, -1))


def expected(agg, ic, wins, tgts, factor=1):
    n_time = 1 + sum(next(iter(w.values())).shape[1] for w in wins)
    out = {"mean": {}, "mean_norm": {}}
    scale = {}
    recs, t0 = [(0, ic, ic)], 1
    for win, tgt in zip(wins, tgts):
        recs.append((t0, win, tgt))
        t0 += next(iter(win.values())).shape[1]

    def add(label, metric, n, t0, v):
        out[label].setdefault(f"{metric}-{n}", torch.zeros(n_time, dtype=torch.float64))[t0:t0 + v.shape[1]] += v.mean(0)
    for t0, gen, tgt in recs:
        for n, x in gen.items():
            x, w = x.double().cpu(), agg.weights_for(n, "cpu").double()
            y = tgt[n].double().cpu() if n in tgt else None
            scale[n] = max(scale.get(n, 0.0), float(wmean(x.abs(), w).max()))
            for label in ("mean", "mean_norm"):
                if label == "mean_norm":
                    if n not in STATS:
                        continue
                    x, y = (x - STATS[n][0]) / STATS[n][1], None if y is None else (y - STATS[n][0]) / STATS[n][1]
                m = wmean(x, w)
                add(label, "weighted_mean_gen", n, t0, m)
                add(label, "weighted_std_gen", n, t0, wmean((x - m[..., None, None]) ** 2, w).sqrt())
                if y is None:
                    continue
                add(label, "weighted_mean_target", n, t0, wmean(y, w))
                add(label, "weighted_bias", n, t0, wmean(x - y, w))
                add(label, "weighted_rmse", n, t0, wmean((x - y) ** 2, w).sqrt())
                if label == "mean":
                    gg, gt = gradmean(x, w), gradmean(y, w)
                    add(label, "weighted_grad_mag_percent_diff", n, t0, 100 * (gg - gt) / gt)
    steps, B = n_time - 1, next(iter(ic.values())).shape[0]
    maps = {}
    for n in STATS:
        maps[n] = tuple(sum(d[n].double().cpu().sum((0, 1)) for d in side) / steps / B for side in (wins, tgts))
    zon = {}
    for n in STATS:                       # every window here is a multiple of the factor: plain coarsening
        sides = []
        for side in (wins, tgts):
            zm = torch.cat([d[n].double().cpu().nanmean(-1) for d in side], dim=1)
            k = zm.shape[1] // factor
            z = zm[:, :k * factor].unfold(1, factor, factor).mean(-1).mean(0)
            sides.append(torch.cat([z, torch.full(((steps + 1) // factor - k, z.shape[1]), float("nan"), dtype=torch.float64)]))
        zon[n] = sides
    return out, scale, maps, zon


def close(got, want, tol, scale):
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    return float((got[ok] - want[ok]).abs().max()) <= tol * scale if bool(ok.any()) else True


def series_scale(key, want, scale, norm):
    metric, n = key.split("-", 1)
    s = float(want.abs().max())
    if metric == "weighted_bias":
        s = scale[n] / (STATS[n][1] if norm else 1.0)
    if metric == "weighted_grad_mag_percent_diff":
        s = 100.0 + s
    return max(s, 1e-30), (1e-5 if metric in STD_LIKE else 1e-6)


def test_fused_matches_fp64_and_never_normalises(dev):
    info = one_degree_info()
    ic, wins, tgts = record(dev)
    norm = normalizer(dev)
    agg = run(info, ic, wins, tgts, norm)
    assert agg._path == "fused" and norm.calls == 0
    ds = agg.get_dataset()
    summary = agg.get_summary()
    assert norm.calls == 0                                               # the _norm outputs are derived, not recomputed
    want, scale, maps, zon = expected(agg, ic, wins, tgts)
    for label in ("mean", "mean_norm"):
        assert set(ds[label]) == set(want[label]), label
        for k, v in want[label].items():
            s, tol = series_scale(k, v, scale, label == "mean_norm")
            assert close(ds[label][k], v, tol, s), (label, k)
    assert "weighted_mean_gen-derived" in ds["mean"] and "weighted_rmse-derived" not in ds["mean"]
    assert not any(k.endswith("-derived") for k in ds["mean_norm"])
    rmse_norm = {}
    for n, (g, t) in maps.items():
        mu, sigma = STATS[n]
        w = agg.weights_for(n, "cpu").double()
        gs = float(g.nan_to_num(0.0).abs().max())
        assert close(ds["time_mean"][f"gen_map-{n}"], g, 1e-6, gs) and close(ds["time_mean"][f"bias_map-{n}"], g - t, 1e-6, gs), n
        gn = (g - mu) / sigma                # derived in fp64: held to the normalised value's own scale
        assert close(ds["time_mean_norm"][f"gen_map-{n}"], gn, 1e-6, float(gn.nan_to_num(0.0).abs().max())), n
        assert close(ds["time_mean_norm"][f"bias_map-{n}"], (g - t) / sigma, 1e-6, gs / sigma), n
        rmse = float(wmean((g - t) ** 2, w).sqrt())
        rmse_norm[n] = rmse / sigma
        assert summary.logs[f"time_mean/rmse/{n}"] == pytest.approx(rmse, rel=1e-5)
        assert summary.logs[f"time_mean/bias/{n}"] == pytest.approx(float(wmean(g - t, w)), abs=1e-6 * gs)
        assert summary.logs[f"time_mean_norm/rmse/{n}"] == pytest.approx(rmse_norm[n], rel=1e-5)
    assert summary.loss == pytest.approx(sum(rmse_norm.values()) / len(rmse_norm), rel=1e-5)
    for n, (g, t) in zon.items():
        gs = float(g.nan_to_num(0.0).abs().max())
        assert close(ds["zonal_mean"][f"gen-{n}"], g, 1e-6, gs) and close(ds["zonal_mean"][f"error-{n}"], g - t, 1e-6, gs), n
    sht = OracleSHT(NLAT, NLON, grid="legendre-gauss", dtype=torch.float64)
    assert agg.omitted == ["sst"] and set(ds["power_spectrum"]) == {"a", "smooth", "q", "PRESsfc", "derived"}
    for n, got in ds["power_spectrum"].items():
        for side, src in enumerate((wins, tgts)):
            if n not in src[0]:
                assert bool(torch.isnan(got[side]).all())
                continue
            tot = 0
            for d in src:
                c = sht(d[n].double().cpu())
                tot = tot + (c.real ** 2 + c.imag ** 2).sum(-1).sum((0, 1))
            w = tot / (8 * 2)
            assert close(got[side], w, 1e-5, float(w.abs().max())), (n, side)
    assert "power_spectrum/mean_abs_norm_bias/a" in summary.logs and "power_spectrum/mean_abs_norm_bias/derived" not in summary.logs


def test_fused_matches_its_torch_path_and_itself_bitwise(dev):
    info = one_degree_info()
    ic, wins, tgts = record(dev)
    fused = run(info, ic, wins, tgts, normalizer(dev)).get_dataset()
    again = run(info, ic, wins, tgts, normalizer(dev)).get_dataset()
    for sub, d in fused.items():
        assert set(d) == set(again[sub])
        for k, v in d.items():
            assert torch.equal(v.view(torch.int32), again[sub][k].view(torch.int32)), (sub, k)
    norm = normalizer(dev)
    tagg = run(info, ic, wins, tgts, norm, fused=False)
    assert tagg._path == "torch" and norm.calls == 2 * (1 + len(wins))
    torch_ds = tagg.get_dataset()
    _, scale, _, _ = expected(tagg, ic, wins, tgts)
    assert set(fused) == set(torch_ds)
    for label in ("mean", "mean_norm"):
        assert set(fused[label]) == set(torch_ds[label])
        for k, v in torch_ds[label].items():
            n = k.split("-", 1)[1]
            s, tol = series_scale(k, v.double().cpu(), scale, label == "mean_norm")
            raw = (scale[n] + abs(STATS[n][0])) / STATS[n][1] if label == "mean_norm" else scale[n]
            assert close(fused[label][k], v, tol, max(s, raw)), (label, k)
    for label in ("time_mean", "time_mean_norm", "zonal_mean"):
        assert set(fused[label]) == set(torch_ds[label])
        for k, v in torch_ds[label].items():
            n = k.split("-", 1)[1]
            raw = (scale[n] + abs(STATS[n][0])) / STATS[n][1] if label == "time_mean_norm" else scale[n]
            assert close(fused[label][k], v, 1e-6, max(raw, float(v.nan_to_num(0.0).abs().max()))), (label, k)
    for k, v in torch_ds["power_spectrum"].items():
        assert close(fused["power_spectrum"][k], v, 1e-5, float(v.nan_to_num(0.0).abs().max())), k


def test_initial_condition_name_without_a_window_target(dev):
    """"PRESsfc" is in the initial condition (its own target there) and no window has a target for it: on both paths it is not
    paired in the maps - no bias map, time-mean RMSE, zonal error or share of the loss"""
    info = one_degree_info()
    ic, wins, tgts = record(dev)
    tgts = [{n: y for n, y in tgt.items() if n != "PRESsfc"} for tgt in tgts]
    out = {}
    for fused in (True, False):
        agg = run(info, ic, wins, tgts, normalizer(dev), fused=fused)
        out[fused] = (agg.get_dataset(), agg.get_summary())
    (ds, summary), (tds, tsummary) = out[True], out[False]
    for sub in ds:
        assert set(ds[sub]) == set(tds[sub]), sub
    assert set(summary.logs) == set(tsummary.logs)
    assert "bias_map-PRESsfc" not in ds["time_mean"] and "error-PRESsfc" not in ds["zonal_mean"]
    assert "time_mean/rmse/PRESsfc" not in summary.logs and "time_mean/gen_map/PRESsfc" in summary.logs
    paired = [n for n in STATS if n != "PRESsfc"]
    assert summary.loss == pytest.approx(sum(summary.logs[f"time_mean_norm/rmse/{n}"] for n in paired) / len(paired), rel=1e-12)
    assert summary.loss == pytest.approx(tsummary.loss, rel=1e-4)
    rmse = ds["mean"]["weighted_rmse-PRESsfc"]
    assert bool((rmse == 0).all())                                        # its own target at step 0, absent afterwards
    assert bool(torch.isnan(ds["power_spectrum"]["PRESsfc"][1]).all())


def test_coarsened_zonal_mean_fused(dev):
    info = one_degree_info()
    ic, wins, tgts = record(dev, windows=(4, 2, 2))
    agg = run(info, ic, wins, tgts, normalizer(dev), max_size=5)         # 9 steps: factor 2, 4 slots
    assert (agg._factor, agg._n_slots) == (2, 4)
    ds = agg.get_dataset()["zonal_mean"]
    _, _, _, zon = expected(agg, ic, wins, tgts, factor=2)
    for n, (g, t) in zon.items():
        assert ds[f"gen-{n}"].shape == (4, NLAT)
        gs = float(g.nan_to_num(0.0).abs().max())
        assert close(ds[f"gen-{n}"], g, 1e-6, gs) and close(ds[f"error-{n}"], g - t, 1e-6, gs), n
    short = build(info, 9, normalizer(dev), max_size=2)
    assert short._factor == 5
    with pytest.raises(ValueError, match="coarsening factor"):
        short.record_batch(wins[0], tgts[0])


def test_launches_and_path_switch(dev):
    info = one_degree_info()
    ic, wins, tgts = record(dev)
    agg = build(info, 9, normalizer(dev))
    agg.record_initial_condition(ic)
    assert agg.launches() == 1                                            # the initial condition: the paired kernel only
    agg.record_batch(wins[0], tgts[0])
    assert agg.launches() == 1 + 1 + 2 + 2                                # one paired call, one SHT + one spectrum per side
    small = build(info, 9, normalizer(dev))
    small.spectrum_chunk_bytes = 1                                        # one name per chunk: 5 generated and 4 target names
    small.record_batch(wins[0], tgts[0])
    assert small.launches() == 1 + 2 * 5 + 2 * 4
    with pytest.raises(ValueError, match="fused path.*torch path"):
        agg.record_batch({n: x.double() for n, x in wins[1].items()}, {n: x.double() for n, x in tgts[1].items()})


def _evaluate(dev, stepper, dataset_info, ic, record, total, T, derived, target_of):
    """run_evaluator over ``record`` (forcings and, through ``target_of``, targets); returns the aggregator and the prediction"""
    from ace_amd.inference import EnginePredict, ForcingWindows, InferenceData, TensorFileWriter, run_evaluator
    import tempfile
    out = {}
    for fused in (True, False):
        loader = ForcingWindows(record, total_forward_steps=total, forward_steps_in_memory=T, device=dev)
        agg = InferenceEvaluatorAggregatorConfig().build(dataset_info, 1, total, normalize=stepper.normalizer)
        agg.fused = fused
        with tempfile.TemporaryDirectory() as tmp:
            writer = TensorFileWriter(tmp)
            run_evaluator(EnginePredict(stepper, batch=2, graph="step"), InferenceData(ic, loader), agg, writer=writer,
                          compute_derived_variables=derived)
            out[fused] = (agg, torch.load(tmp + "/autoregressive_predictions.pt", weights_only=True))
    assert out[True][0]._path == "fused" and out[False][0]._path == "torch"
    # the two paths on the same pair: every series of the denormalised mean, derived names included
    series = out[True][1]
    fds, tds = out[True][0].get_dataset()["mean"], out[False][0].get_dataset()["mean"]
    assert set(fds) == set(tds)
    for k, v in tds.items():
        metric, n = k.split("-", 1)
        w = out[True][0].weights_for(n, "cpu").double()
        mag = float(wmean(series[n].double().abs(), w).nan_to_num(0.0).max())
        if metric == "weighted_grad_mag_percent_diff":
            mag = 100.0
        scale = max(mag, float(v.nan_to_num(0.0, posinf=0.0, neginf=0.0).abs().max()), 1e-30)
        got, ref = fds[k].double(), v.double()
        fin = torch.isfinite(ref)
        assert torch.equal(torch.isfinite(got), fin), k
        assert float((got[fin] - ref[fin]).abs().max() if bool(fin.any()) else 0.0) <= (1e-5 if metric in STD_LIKE else 1e-6) * scale, k
    return out[True]


def _self_target_then_perturbed(dev, stepper, dataset_info, ic, forcing, total, T, derived):
    from ace_amd.inference import EnginePredict, ForcingWindows, InferenceData, TensorFileWriter, run_inference
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        loader = ForcingWindows(forcing, total_forward_steps=total, forward_steps_in_memory=T, device=dev)
        run_inference(EnginePredict(stepper, batch=2, graph="step"), InferenceData(ic, loader), writer=TensorFileWriter(tmp),
                      compute_derived_variables=False)
        pred = torch.load(tmp + "/autoregressive_predictions.pt", weights_only=True)
    names = [n for n in pred if n not in forcing]
    first = {n: (ic[n].cpu() if n in ic else torch.full_like(pred[n][:, :1], float("nan"))) for n in names}
    g = torch.Generator().manual_seed(8)
    # the rollout's own output as target: zero RMSE and bias, bit for bit
    record = {**forcing, **{n: torch.cat([first[n], pred[n]], dim=1) for n in names}}
    agg, _ = _evaluate(dev, stepper, dataset_info, ic, record, total, T, derived, None)
    ds = agg.get_dataset()["mean"]
    for n in names:                       # exactly zero wherever the generated series itself is defined
        ok = ~torch.isnan(ds[f"weighted_mean_gen-{n}"][1:])
        assert torch.equal(torch.isnan(ds[f"weighted_rmse-{n}"][1:]), ~ok), n
        assert bool((ds[f"weighted_rmse-{n}"][1:][ok] == 0).all()) and bool((ds[f"weighted_bias-{n}"][1:][ok] == 0).all()), n
    if derived:                           # derive_target gave the target the derived variables of the same fields: zero RMSE too
        extra = [k.split("-", 1)[1] for k in ds if k.startswith("weighted_rmse-") and k.split("-", 1)[1] not in names
                 and k.split("-", 1)[1] not in forcing]
        assert extra, sorted(ds)
        for n in extra:
            v = ds[f"weighted_rmse-{n}"][1:]
            assert bool(torch.isfinite(v).any()) and bool((v[torch.isfinite(v)] == 0).all()), n
    # a perturbed target: the fp64 values
    noise = {n: 0.01 * pred[n].nan_to_num(0.0).abs().mean() * torch.randn(pred[n].shape, generator=g) for n in names}
    record = {**forcing, **{n: torch.cat([first[n], pred[n] + noise[n]], dim=1) for n in names}}
    agg, series = _evaluate(dev, stepper, dataset_info, ic, record, total, T, derived, None)
    ds = agg.get_dataset()["mean"]
    for n in names:
        w = agg.weights_for(n, "cpu").double()
        x, y = series[n].double(), (pred[n] + noise[n]).double()
        rmse, bias = wmean((x - y) ** 2, w).sqrt().mean(0), wmean(x - y, w).mean(0)
        xs = max(float(wmean(x.abs(), w).nan_to_num(0.0).max()), 1e-30)
        assert close(ds[f"weighted_rmse-{n}"][1:], rmse, 1e-5, max(float(rmse.nan_to_num(0.0).max()), 1e-30)), n
        assert close(ds[f"weighted_bias-{n}"][1:], bias, 1e-6, xs), n
    return agg


def test_run_evaluator_sfno_fixture(dev):
    import ace_amd
    g = load_golden("gen_checkpoint.pt")["ace2_like"]
    loaded = ace_amd.load_stepper(g["state"], device=dev)
    ic = {k: v.to(dev) for k, v in g["ic"].items()}
    _self_target_then_perturbed(dev, loaded.stepper, loaded.dataset_info, ic, g["forcing"], len(g["steps"]), 2, derived=True)


def test_run_evaluator_samudra_fixture(dev):
    from ace_amd.checkpoint import load_stepper
    case = load_golden("gen_ocean_rollout.pt")
    state = copy.deepcopy(case["stepper"])
    state["step"]["module"] = {k: (v.float() if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
                               for k, v in state["step"]["module"].items()}
    di = state["dataset_info"]
    di["mask_provider"]["masks"] = {k: v.float() for k, v in di["mask_provider"]["masks"].items()}
    di["vertical_coordinate"]["mask"] = di["vertical_coordinate"]["mask"].float()
    loaded = load_stepper({"stepper": state}, device=dev)
    ic = {k: v.to(dev) for k, v in case["initial_condition"].items()}
    agg = _self_target_then_perturbed(dev, loaded.stepper, loaded.dataset_info, ic, case["forcing"], 4, 2, derived=False)
    assert agg.omitted
