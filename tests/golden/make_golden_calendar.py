"""tests/golden/gen_calendar.pt from the reference's own functions (imported through oracle/ref_loader.load_stepper_ref's stubs, the
aggregator packages as bare namespaces and their plotting / build-context / data modules as permissive stubs), on the records of
tests/_calendar_cases.py (exact arithmetic, rebuilt by every test; the file pins their checksums and holds results only):
  * ``LatLonRegion`` (fme/ace/aggregator/inference/utils.py:22-43) for the Nino 3.4 box and the three tripole boxes;
  * ``metrics.weighted_mean`` (fme/core/metrics.py:63-90) for the area means and the Nino 3.4 means, with the regional weights
    multiplied by the area weights in fp32 (gridded_ops.py:336), and ``_nan_aware_regional_mean`` (ipo/ipo_index.py:43-58);
  * ``anomalies_from_monthly_climo``, ``running_monthly_mean``, ``compute_power_spectrum``, ``_compute_sample_mean_std`` and
    ``compute_psd_band_power`` (utils.py) for the index metrics, ``low_pass_filter`` (ipo/ipo_index.py:61-87) with the 13-year trim
    for the filtered tripole index;
  * ``get_crps`` (fme/core/ensemble.py:4-44) and ``_get_min_samples`` (annual.py:418-420) for the annual metric.
The ``time`` these functions take only needs ``.dt.year.values`` / ``.dt.month.values``: a SimpleNamespace serves.  xarray is not on
this machine, so the groupby sums of annual.py:193-208 (per sample and year) and seasonal.py:47-69 (per season, skipna=False) and
the xarray arithmetic of their ``get_logs`` are restated here in numpy, window by window as the reference accumulates them.

Everything is computed twice: "f32" in the reference's dtypes, and "f64" with the same functions on fp64 inputs under a fp64
default dtype.  tests/test_evaluator_calendar_cpu.py takes its bars from the gap between the two."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import _calendar_cases as C  # noqa: E402
from oracle import ref_loader  # noqa: E402

NINO34 = {"lat_bounds": (-5, 5), "lon_bounds": (190, 240)}
SEASON_OF_MONTH = {12: 0, 1: 0, 2: 0, 3: 1, 4: 1, 5: 1, 6: 2, 7: 2, 8: 2, 9: 3, 10: 3, 11: 3}          # DJF, MAM, JJA, SON


def load():
    ref_loader.load_stepper_ref()
    ref = os.path.join(ref_loader.REF, "fme", "ace", "aggregator")
    for name, path in (("fme.ace.aggregator", ref), ("fme.ace.aggregator.inference", os.path.join(ref, "inference")),
                       ("fme.ace.aggregator.inference.enso", os.path.join(ref, "inference", "enso")),
                       ("fme.ace.aggregator.inference.ipo", os.path.join(ref, "inference", "ipo"))):
        ref_loader._ns(name, path)
    permissive = type(sys.modules["xarray"])
    for name in ("fme.ace.aggregator.plotting", "fme.ace.aggregator.inference.build_context", "fme.ace.aggregator.inference.data"):
        sys.modules[name] = permissive(name)
    return types.SimpleNamespace(
        utils=importlib.import_module("fme.ace.aggregator.inference.utils"),
        ipo=importlib.import_module("fme.ace.aggregator.inference.ipo.ipo_index"),
        annual=importlib.import_module("fme.ace.aggregator.inference.annual"),
        metrics=importlib.import_module("fme.core.metrics"),
        ensemble=importlib.import_module("fme.core.ensemble"))


def time_like(year, month):
    ns = types.SimpleNamespace
    return ns(dt=ns(year=ns(values=year), month=ns(values=month)))


def spectrum(R, index):
    """_calculate_sample_average_power_spectrum (utils.py:97-124) without xarray: NaNs dropped, truncated to the shortest sample"""
    rows = [row[~np.isnan(row)] for row in index]
    n = min(len(r) for r in rows)
    return R.utils.compute_power_spectrum(np.array([r[:n] for r in rows]))


def index_metrics(R, pred, tgt):
    """PairedRegionalIndexAggregator.get_logs (enso/dynamic_index.py:241-337) on numpy indices"""
    out = {"std": R.utils._compute_sample_mean_std(pred), "std_norm": R.utils._compute_sample_mean_std(pred, tgt)}
    (pf, pp), (tf, tp) = spectrum(R, pred), spectrum(R, tgt)
    out["freq"], out["power"], out["power_target"] = torch.from_numpy(pf), torch.from_numpy(pp), torch.from_numpy(tp)
    for tag, bounds in (("2_5yr", (2.0, 5.0)), ("1_16yr", (1.0, 16.0))):
        p, t = R.utils.compute_psd_band_power(pf, pp, period_bounds=bounds), R.utils.compute_psd_band_power(tf, tp, period_bounds=bounds)
        out[f"power_{tag}"] = p
        if t != 0 and not np.isnan(t):
            out[f"power_{tag}_norm"] = p / t
    return out


def chain(R, c, dtype, with_maps):
    """every quantity of the four metrics on record ``c`` with the fields cast to ``dtype``"""
    torch.set_default_dtype(dtype)
    try:
        year, month = c["time"].year_month()
        time = time_like(year, month)
        lat, lon = torch.tensor(C.LAT, dtype=torch.float32), torch.tensor(C.LON, dtype=torch.float32)
        region = lambda spec: R.utils.LatLonRegion(lat=lat, lon=lon, **spec).regional_weights      # noqa: E731
        area = c["info"].area_weights.to(torch.float32)
        nino_w = (region(NINO34) * area).to(dtype)                             # the product in fp32, gridded_ops.py:336
        tpi_w = {k: region(spec).to(dtype) for k, spec in R.ipo.TPI_REGIONS.items()}
        out = {"regions": {"nino34": region(NINO34), **{k: region(spec) for k, spec in R.ipo.TPI_REGIONS.items()}}}
        fields = {side: {n: x.to(dtype) for n, x in c[side].items()} for side in ("gen", "target")}
        bounds = [0] + [w[1].shape[1] for w in c["windows"]]
        bounds = np.cumsum(bounds)

        # the raw regional series
        def windowed(fn, x):                                                   # window by window, as record_batch sees the record
            return torch.cat([fn(x[:, a:b]) for a, b in zip(bounds[:-1], bounds[1:])], dim=1)

        raw = {side: {"globe": {n: windowed(lambda v: R.metrics.weighted_mean(v, area.to(dtype), dim=(-2, -1)), x) for n, x in d.items()}}
               for side, d in fields.items()}
        for side, d in fields.items():
            raw[side]["nino34"] = windowed(lambda v: R.metrics.weighted_mean(v, nino_w, dim=(-2, -1)), d["sst"])
            for k, w in tpi_w.items():
                raw[side][k] = windowed(lambda v, w=w: R.ipo._nan_aware_regional_mean(v, w), d["sst"])
        out["raw"] = raw

        # enso_index
        nino = {side: R.utils.running_monthly_mean(R.utils.anomalies_from_monthly_climo(raw[side]["nino34"], time), time, n_months=5)
                for side in raw}
        out["enso"] = {"index": {side: v[0] for side, v in nino.items()}, "years": nino["gen"][1].years, "months": nino["gen"][1].months,
                       **index_metrics(R, nino["gen"][0].numpy(), nino["target"][0].numpy())}

        # ipo_index
        tpi = {}
        for side in raw:
            an = {k: R.utils.running_monthly_mean(R.utils.anomalies_from_monthly_climo(raw[side][k], time), time, n_months=1)[0]
                  for k in tpi_w}
            tpi[side] = an["T2"] - 0.5 * (an["T1"] + an["T3"])
        out["ipo"] = {"tpi": tpi}
        trim = int(13.0 * 12)
        if tpi["gen"].shape[1] >= R.ipo.MIN_YEARS_FOR_FILTERED_TPI * 12:
            filt = {side: np.stack([R.ipo.low_pass_filter(row[~np.isnan(row)])[trim:-trim] for row in v.numpy()]) for side, v in tpi.items()}
            out["ipo"].update(filtered={side: torch.from_numpy(v) for side, v in filt.items()},
                              std=R.utils._compute_sample_mean_std(filt["gen"]),
                              std_norm=R.utils._compute_sample_mean_std(filt["gen"], filt["target"]))
            (pf, pp), (_, tp) = spectrum(R, tpi["gen"].numpy()), spectrum(R, tpi["target"].numpy())
            out["ipo"].update(freq=torch.from_numpy(pf), power=torch.from_numpy(pp), power_target=torch.from_numpy(tp))

        # annual: the groupby(year).sum() of every window per sample, added up (annual.py:193-208), then annual.py:226-235
        labels = np.unique(year)
        counts = np.zeros((C.B, len(labels)), np.float32)
        sums = {side: {n: np.zeros((C.B, len(labels)), raw[side]["globe"][n].numpy().dtype) for n in c["names"]} for side in raw}
        for a, b in zip(bounds[:-1], bounds[1:]):
            for k, y in enumerate(labels):
                sel = year[:, a:b] == y
                counts[:, k] += sel.sum(axis=1)
                for side in raw:
                    for n in c["names"]:
                        x = raw[side]["globe"][n].numpy()[:, a:b]
                        sums[side][n][:, k] += np.stack([x[s][sel[s]].sum(dtype=x.dtype) for s in range(C.B)])
        keep = counts > R.annual._get_min_samples(c["timestep"])
        kept = labels[keep.any(axis=0)]
        years = np.arange(kept.min(), kept.max() + 1)
        annual = {"years": torch.from_numpy(years), "series": {}, "rmse": {}, "crps": {}}
        for n in c["names"]:
            means = {}
            for side in raw:
                with np.errstate(all="ignore"):
                    m = np.where(keep, sums[side][n] / counts, np.nan)
                full = np.full((C.B, len(years)), np.nan, m.dtype)
                for k, y in enumerate(labels):
                    if y in kept:
                        full[:, y - years[0]] = m[:, k]
                means[side] = full
            annual["series"][n] = {side: torch.from_numpy(v) for side, v in means.items()}
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                tmean, gmean = np.nanmean(means["target"], axis=0), np.nanmean(means["gen"], axis=0)          # .mean("sample") skips NaN
                annual["rmse"][n] = float(np.sqrt(np.nanmean((gmean - tmean) ** 2)))                         # annual.py:335-340
                crps = R.ensemble.get_crps(torch.as_tensor(means["gen"].T.copy(), dtype=torch.float32),
                                           torch.as_tensor(tmean, dtype=torch.float32).unsqueeze(1))         # annual.py:343-359
                annual["crps"][n] = float(np.nanmean(crps.numpy()))
        out["annual"] = annual

        # seasonal: the groupby(season).sum(skipna=False) of every window, added up (seasonal.py:47-69), then seasonal.py:87-168
        if with_maps:
            season = np.vectorize(SEASON_OF_MONTH.get)(month)
            scount = np.zeros(4)
            ssum = {side: {n: np.zeros((4, C.H, C.W), fields[side][n].numpy().dtype) for n in c["names"]} for side in fields}
            for a, b in zip(bounds[:-1], bounds[1:]):
                for m in range(4):
                    sel = season[:, a:b] == m
                    scount[m] += sel.sum()
                    if sel.any():
                        for side in fields:
                            for n in c["names"]:
                                x = fields[side][n].numpy()[:, a:b]
                                ssum[side][n][m] += x[sel].sum(axis=0, dtype=x.dtype)
            seasonal = {"counts": torch.from_numpy(scount), "anomaly": {}, "bias": {}, "r2": {}, "rmse": {}, "rmse_season": {}}
            for n in c["names"]:
                tgt, gen = (ssum[side][n] / scount[:, None, None] for side in ("target", "gen"))              # fp64 counts: fp64 means
                bias = gen - tgt
                pattern = tgt.mean(axis=0)
                ganom, tanom = gen - pattern, tgt - pattern
                seasonal["anomaly"][n] = torch.from_numpy(np.stack([tanom, ganom]))
                seasonal["bias"][n] = torch.from_numpy(bias)
                seasonal["r2"][n] = float(1 - np.sum((ganom - tanom) ** 2) / np.sum((tanom - np.mean(tanom)) ** 2))      # seasonal.py:200-204
                mse = R.metrics.weighted_mean(torch.as_tensor(bias ** 2), area, dim=(-2, -1))                            # seasonal.py:156-159
                seasonal["rmse_season"][n] = mse.sqrt().double()
                seasonal["rmse"][n] = float(mse.mean().sqrt())
            out["seasonal"] = seasonal
        return out
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    R = load()
    out = {}
    for key, c, with_maps in (("main", C.main(), True), ("long", C.long(), False)):
        out[key] = {"checksum": C.checksum(c), "f32": chain(R, c, torch.float32, with_maps), "f64": chain(R, c, torch.float64, with_maps)}
        if key == "long":                                  # regional means only: the raw series of 984 steps are the bulk
            for k in ("f32", "f64"):
                del out[key][k]["raw"]["gen"]["globe"], out[key][k]["raw"]["target"]["globe"]
    dst = os.path.join(HERE, "gen_calendar.pt")
    torch.save(out, dst)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
