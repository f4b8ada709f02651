"""The ``seasonal``, ``annual``, ``enso_index`` and ``ipo_index`` metrics of the evaluator: their host formulas and ``_Calendar``."""
import datetime
import warnings
from typing import Any, Dict, List, Mapping, Optional

import numpy as np
import torch

from ..aggregator import _check, _grow, _upload, _upload_planes
from .common import _check_time, _only, _wmean

SEA_SURFACE_TEMPERATURE_NAMES = ["sst", "surface_temperature", "TS"]      # enso/dynamic_index.py:33
NINO34_LAT, NINO34_LON = (-5, 5), (190, 240)                              # enso/dynamic_index.py:354-355
IPO_SST_NAMES = ["sst"]                                                   # ipo/ipo_index.py:32
MIN_YEARS_FOR_FILTERED_TPI = 80                                           # ipo/ipo_index.py:34
IPO_CUTOFF_YEARS = 13.0                                                   # ipo/ipo_index.py:226
TPI_REGIONS = {"T1": {"lat_bounds": (25.0, 45.0), "lon_bounds": (140.0, 215.0)},      # ipo/ipo_index.py:36-40
               "T2": {"lat_bounds": (-10.0, 10.0), "lon_bounds": (170.0, 270.0)},
               "T3": {"lat_bounds": (-50.0, -15.0), "lon_bounds": (150.0, 200.0)}}
SEASONS = ("DJF", "MAM", "JJA", "SON")                                    # seasonal.py:185, the order of the bins and of the maps
MIN_COMPLETE_YEAR_DAYS = 350                                              # annual.py:415
MAX_CALENDAR_BINS = 8                                                     # ACE_DIAG_CALENDAR_MAX_BINS (include/ace_sfno.h)


def latlon_region_weights(lat, lon, lat_bounds, lon_bounds) -> torch.Tensor:
    """LatLonRegion (utils.py:30-39): mask x cos(lat) as fp32 (H, W), computed in the dtype of ``lat`` as the reference does"""
    lat, lon = torch.as_tensor(lat), torch.as_tensor(lon)
    lat_mask = ((lat >= lat_bounds[0]) & (lat <= lat_bounds[1])).unsqueeze(-1)
    lon_mask = ((lon >= lon_bounds[0]) & (lon <= lon_bounds[1])).unsqueeze(-2)
    mask = torch.logical_and(lat_mask, lon_mask).float()
    return (mask * torch.cos(torch.deg2rad(lat)).unsqueeze(-1)).to(torch.float32)


def nan_aware_regional_mean(data: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """ipo/ipo_index.py:43-58"""
    valid = ~torch.isnan(data)
    filled = torch.where(valid, data, torch.zeros_like(data))
    w = weights.to(data.device).unsqueeze(0).unsqueeze(0)
    return (filled * w * valid).sum(dim=(-2, -1)) / (w * valid).sum(dim=(-2, -1))


def anomalies_from_monthly_climo(data: torch.Tensor, month) -> torch.Tensor:
    """utils.py:127-144: data (B, T) minus its per-sample mean over the steps of the same calendar month; month (B, T) ints"""
    nan = torch.tensor(float("nan"), dtype=data.dtype)
    anomalies = torch.full_like(data, float("nan"))
    for m in range(1, 13):
        mask = torch.from_numpy(np.asarray(month) == m)
        climo = (data.where(mask, nan).nansum(dim=1) / mask.sum(dim=1)).unsqueeze(dim=1)
        anomalies = torch.where(mask, data - climo, anomalies)
    return anomalies


def running_monthly_mean(data: torch.Tensor, year, month, n_months: int):
    """utils.py:184-220: the per-sample mean of every (year, month) of the record, then the mean of the last ``n_months`` of them;
    returns ((B, n unique months), the sorted (year, month) pairs)"""
    year, month = np.asarray(year), np.asarray(month)
    keys = sorted(set(zip(year.ravel().tolist(), month.ravel().tolist())))
    nan = torch.tensor(float("nan"), dtype=data.dtype)
    monthly = torch.full((data.shape[0], len(keys)), float("nan"), dtype=data.dtype)
    running = torch.full_like(monthly, float("nan"))
    for i, (y, m) in enumerate(keys):
        mask = torch.from_numpy((year == y) & (month == m))
        monthly[:, i] = data.where(mask, nan).nanmean(dim=1)
        if i >= n_months - 1:
            running[:, i] = monthly[:, i - n_months + 1:i + 1].nanmean(dim=1)
    return running, keys


def sample_mean_std(data, target=None) -> float:
    """utils.py:76-94: the standard deviation over time of every sample, optionally over the target's, averaged over samples"""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        std = np.nanstd(data, axis=1)
        if target is not None:
            std = std / np.nanstd(target, axis=1)
    return std.mean().item()


def sample_average_power_spectrum(index):
    """utils.py:46-73, 97-124: (cycles per year, |rfft|^2 averaged over samples) of monthly (B, n) series, NaNs dropped and the
    samples truncated to the shortest; None when a sample has nothing left"""
    rows = [row[~np.isnan(row)] for row in np.asarray(index)]
    n = min(len(r) for r in rows)
    if n == 0:
        return None
    power = (np.abs(np.fft.rfft(np.array([r[:n] for r in rows]), axis=1)) ** 2).mean(axis=0)
    return np.fft.rfftfreq(n, d=1.0) * 12.0, power


def psd_band_power(freqs, power, period_bounds=(2.0, 5.0)) -> float:
    """utils.py:238-261"""
    mask = (freqs >= 1.0 / period_bounds[1]) & (freqs <= 1.0 / period_bounds[0])
    if mask.sum() < 2:
        return float("nan")
    trapezoid = np.trapezoid if hasattr(np, "trapezoid") else np.trapz
    return float(trapezoid(power[mask], freqs[mask]))


def fair_crps(gen: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """fme/core/ensemble.py:4-44 with alpha = 1: gen (n, members), target (n, 1)"""
    first = torch.mean(torch.abs(gen - target), dim=1)
    if gen.shape[1] == 1:
        return first
    i, j = torch.triu_indices(gen.shape[1], gen.shape[1], offset=1)
    return first - 0.5 * (gen[:, i] - gen[:, j]).abs().mean(dim=1)


def low_pass_filter(data, cutoff_period_yrs: float = IPO_CUTOFF_YEARS):
    """ipo/ipo_index.py:61-87: a fifth-order Chebyshev type I low pass (0.5 dB ripple) of monthly values, run forwards and back"""
    from scipy import signal
    b, a = signal.cheby1(N=5, rp=0.5, Wn=(1.0 / cutoff_period_yrs) / 6.0, btype="low", analog=False)
    return signal.filtfilt(b, a, data)


class _Calendar:
    """The four metrics that group a record by its calendar: ``seasonal`` (SeasonalAggregator, seasonal.py:22-175), ``annual``
    (PairedGlobalMeanAnnualAggregator, annual.py:24-275), ``enso_index`` (PairedRegionalIndexAggregator, enso/dynamic_index.py:36-351)
    and ``ipo_index`` (PairedIPOIndexAggregator, ipo/ipo_index.py:90-322).  Per window both paths form the same two things: the sum
    of the steps of each season per pixel, and per (sample, step) the regional means the other three start from - the area mean of
    every name (a region of ones), the Nino 3.4 box of the sea-surface-temperature names, the three tripole boxes of ``sst``.  The
    torch path states the reference's formulas in the reference's dtypes (fp32 sums and means); the fused path makes one
    ``ace_diag_calendar_window`` per window for everything that is on (csrc/calendar.hip; the header contract in
    include/ace_sfno.h) and keeps fp64 sums and series on the device until ``get_*``.  The (year, month) of every time level and the
    season counts stay on the host.  Every step handed to ``record_batch`` enters - none of the four drops a first step as the time
    mean does - and the initial condition never does (main.py:660-661 feeds it to the time series only).

    At ``get_*`` time the small series go through the reference's host formulas, restated on (year, month) arrays where the
    reference groups by xarray / cftime: yearly means of more than 350 days' worth of steps, monthly anomalies, the 5-month running
    mean, the sample-averaged power spectrum and its band powers, the tripole index and its 13-year Chebyshev low pass, the seasonal
    means with their bias, anomaly, R2 and area-mean RMSE.  Tensors stand where the reference logs figures.  Differences: no
    ``r2/<name>_target`` / ``_gen`` of the annual series (they need the monthly reference data); the seasonal R2, which the
    reference only shows in a caption, is logged as ``r2/<name>``; a generated name without a target is left out of the paired
    outputs; a sample without one complete year stays in the annual series as a row of NaN, where the reference's
    ``where(..., drop=True)`` (annual.py:227) drops it from the sample axis (the nan-means give the same scalars)."""
    uses_time = True
    needs_norm = False
    counted = False                      # ``calls`` is reported apart from ``launches()``, whose total the other families define

    def __init__(self, agg, configs: Mapping[str, Any], dataset_info):
        self._agg = agg
        self.seasonal, self.annual, self.enso, self.ipo = (configs.get(k) for k in ("seasonal", "annual", "enso_index", "ipo_index"))
        self._timestep = getattr(dataset_info, "timestep", None)
        coords = getattr(dataset_info, "horizontal_coordinates", None)
        H, W = agg._shape
        self._region_names: List[str] = []
        planes, self._modes = [], []
        if self.annual is not None:
            self._region_names.append("globe")                                # x 1 in fp32 leaves the area weights as they are
            planes.append(torch.ones(H, W))
            self._modes.append(0)
        if self.enso is not None:
            self._region_names.append("nino34")
            planes.append(latlon_region_weights(coords.lat, coords.lon, NINO34_LAT, NINO34_LON))
            self._modes.append(0)
        if self.ipo is not None:
            for name, spec in TPI_REGIONS.items():
                self._region_names.append(name)
                planes.append(latlon_region_weights(coords.lat, coords.lon, spec["lat_bounds"], spec["lon_bounds"]))
                self._modes.append(1)
        self._regions = torch.stack(planes) if planes else torch.zeros(0, H, W)
        self._year = self._month = None                                       # (B, n_time) int64, filled window by window
        self._seen = [False] * agg._n_time
        self._season_counts = [0.0] * len(SEASONS)
        self._have: List[set] = [set(), set()]                                # per side the (region, name) series recorded
        self._season_names: List[List[str]] = [[], []]
        self.calls = 0                                                        # ace_diag_calendar_window calls made
        # torch path
        self._t_series: List[Dict[Any, torch.Tensor]] = [{}, {}]
        self._t_bins: List[Dict[str, torch.Tensor]] = [{}, {}]
        # fused path: _bins (2, rows, 4, H W) fp64, _series (2, series rows, B, n_time) fp64 (NaN: not recorded)
        self._rows: Dict[str, int] = {}
        self._srows: Dict[Any, int] = {}
        self._bins = self._series = self._dev_regions = self._dev_modes = None

    def on(self) -> list:
        return [m for m in (self.seasonal, self.annual, self.enso, self.ipo) if m is not None]

    @property
    def needs_time(self) -> bool:
        """a strict metric is on (a ``SeasonalMetricConfig`` is strict unless told otherwise)"""
        return any(m.strict for m in self.on())

    def without_time(self) -> List[str]:
        """``record_batch`` came without a time axis: the names of the metrics to drop, all of them - they are on by default - unless
        one is strict or a window already went into them"""
        names = [m.name for m in self.on()]
        if self.needs_time or any(self._seen):
            raise ValueError(f"the {', '.join(names)} metrics need the window's time axis: record_batch(prediction, target, time=...)")
        return names

    def _prepare(self, gen, tgt, i_time_start, time):
        """the host side of a window: its (year, month) levels, the season bin of every step, the names each output takes"""
        B, T = next(iter(gen.values())).shape[:2]
        if time is None:
            raise ValueError("the seasonal, annual, enso_index and ipo_index metrics need the window's time axis: "
                             "record_batch(prediction, target, time=...)")
        _check_time(time, B, T)
        year, month = time.year_month()
        if self._year is None:
            self._year, self._month = (np.zeros((B, self._agg._n_time), np.int64) for _ in range(2))
        elif self._year.shape[0] != B:
            raise ValueError("the number of samples changed between windows")
        self._year[:, i_time_start:i_time_start + T], self._month[:, i_time_start:i_time_start + T] = year, month
        for i in range(i_time_start, i_time_start + T):
            self._seen[i] = True
        season = ((month % 12) // 3).astype(np.int32)                        # DJF = 12, 1, 2 -> 0, MAM -> 1, JJA -> 2, SON -> 3
        wanted = []
        for side, d in enumerate((gen, tgt)):
            w = {}
            for r in self._region_names:
                w[r] = _only(d, self.annual.variables) if r == "globe" else \
                    [n for n in (SEA_SURFACE_TEMPERATURE_NAMES if r == "nino34" else IPO_SST_NAMES) if n in d]
                self._have[side].update((r, n) for n in w[r])
            w["seasonal"] = _only(d, self.seasonal.variables) if self.seasonal is not None else []
            self._season_names[side] += [n for n in w["seasonal"] if n not in self._season_names[side]]
            wanted.append(w)
        if self.seasonal is not None:
            for m, c in enumerate(np.bincount(season.ravel(), minlength=len(SEASONS))):
                self._season_counts[m] += float(c)
        return B, T, season, wanted

    def record(self, w) -> int:
        prepared = self._prepare(w.gen, w.tgt, w.i_time_start, w.time)
        return (self._record_fused if w.fused else self._record_torch)(w, *prepared)

    # ---- the torch path -----------------------------------------------------------------------------------------------
    def _record_torch(self, w, B, T, season, wanted) -> int:
        gen, tgt, dev, sl = w.gen, w.tgt, w.device, slice(w.i_time_start, w.i_time_start + T)
        # the (sample, step) indices of the seasons this window has steps of, found on the host and uploaded once: indexing with
        # them gathers what a boolean mask would, in the same order, without the host synchronisation a mask's nonzero() costs
        steps = {m: tuple(torch.from_numpy(i).to(dev) for i in np.nonzero(season == m)) for m in range(len(SEASONS))
                 if (season == m).any()} if self.seasonal is not None else {}
        for side, d in enumerate((gen, tgt)):
            for ri, r in enumerate(self._region_names):
                for n in wanted[side][r]:
                    x = d[n]
                    if r == "globe":                                              # annual.py:185-188 on gridded_ops.py:350-359
                        v = _wmean(x, self._agg.weights_for(n, x.device).to(x.dtype))
                    elif self._modes[ri] == 0:                                    # dynamic_index.py:77-79 on gridded_ops.py:361-371
                        v = _wmean(x, self._regions[ri].to(x.device) * self._agg.weights_for(n, x.device).to(x.dtype))
                    else:                                                         # ipo_index.py:121-124
                        v = nan_aware_regional_mean(x, self._regions[ri])
                    buf = self._t_series[side].get((r, n))
                    if buf is None:
                        buf = self._t_series[side][(r, n)] = torch.full((B, self._agg._n_time), float("nan"), dtype=v.dtype,
                                                                        device=v.device)
                    buf[:, sl] = v
            for n in wanted[side]["seasonal"]:                                    # seasonal.py:40-69: groupby(season).sum(skipna=False)
                x = d[n]
                acc = self._t_bins[side].get(n)
                if acc is None:
                    acc = self._t_bins[side][n] = torch.zeros((len(SEASONS),) + tuple(x.shape[-2:]), dtype=x.dtype, device=x.device)
                for m, (bi, ti) in steps.items():
                    acc[m] += x[bi, ti].sum(dim=0)
        return 0

    # ---- the fused path -----------------------------------------------------------------------------------------------
    def _layout(self, gen, wanted, B: int, HW: int, dev):
        """the planes of a window's call, their rows in ``_bins`` and the (plane, region) rows in ``_series``, both buffers grown
        to hold them: a plane takes part in the binned sums whenever they are on (the header contract ties the series of a plane
        to a valid row), and what the seasonal variable filter excludes is left out at get_* time"""
        planes = [n for n in gen if any(n in w[k] for w in wanted for k in w)]
        for n in planes:
            self._rows.setdefault(n, len(self._rows))
        for w in wanted:
            for r in self._region_names:
                for n in w[r]:
                    self._srows.setdefault((r, n), len(self._srows))
        if self.seasonal is not None and (self._bins is None or self._bins.shape[1] < len(self._rows)):
            self._bins = _grow(self._bins, (2, max(1, len(self._rows)), len(SEASONS), HW), torch.float64, dev)
        S = max(1, len(self._srows))
        if self._region_names and (self._series is None or self._series.shape[1] < S):
            fresh = torch.full((2, S, B, self._agg._n_time), float("nan"), dtype=torch.float64, device=dev)
            if self._series is not None:
                fresh[:, :self._series.shape[1]] = self._series
            self._series = fresh
        srow = [[self._srows[(r, nm)] if any(nm in w[r] for w in wanted) else -1 for r in self._region_names] for nm in planes]
        return planes, [self._rows[nm] for nm in planes], srow

    def _record_fused(self, w, B, T, season, wanted) -> int:
        """one ``ace_diag_calendar_window`` for all the metrics that are on, both sides and all names (fields with contiguous
        planes); returns the calls made"""
        from .. import _lib
        agg, gen, tgt, dev, HW, i_time_start = self._agg, w.gen, w.tgt, w.device, w.HW, w.i_time_start
        nreg, n_time = len(self._region_names), agg._n_time
        planes, rows, srow = self._layout(gen, wanted, B, HW, dev)
        if not planes:
            return 0
        if nreg and self._dev_regions is None:
            self._dev_regions = self._regions.reshape(nreg, HW).to(dev, torch.float32).contiguous()
            self._dev_modes = _upload(self._modes, torch.int32, dev)
        n = len(planes)
        wrows = agg._weight_rows(planes, dev)
        # one pinned blob: the plane table, then from its end the rows, the season bins and the series rows
        at, (p_rows, p_bin, p_srow) = _upload_planes(planes, gen, tgt, dev, [
            np.asarray(rows, np.int32), np.ascontiguousarray(season, np.int32), np.asarray(srow, np.int32)])
        lib = _lib.lib()
        do_bins = self.seasonal is not None
        partial = torch.empty(int(lib.ace_diag_calendar_partial_doubles(n, nreg, B, T, HW)), dtype=torch.float64, device=dev) \
            if nreg else None
        _check(lib.ace_diag_calendar_window(
            at["gen"], at["gen_strides"], at["target"], at["target_strides"], p_rows, p_bin if do_bins else None,
            self._bins.data_ptr() if do_bins else None, self._dev_regions.data_ptr() if nreg else None, p_srow if nreg else None,
            self._dev_modes.data_ptr() if nreg else None, wrows.data_ptr() if nreg else None,
            agg._wplanes.data_ptr() if nreg else None, agg._wplanes.shape[0] if nreg else 0,
            partial.data_ptr() if nreg else None, self._series.data_ptr() if nreg else None, len(self._rows),
            len(SEASONS) if do_bins else 0, nreg, self._series.shape[1] if nreg else 0, n_time, i_time_start, 0, n, B, T, HW,
            _lib.current_stream()))
        self.calls += 1
        return 1

    # ---- results ------------------------------------------------------------------------------------------------------
    def _recorded(self):
        return [i for i, s in enumerate(self._seen) if s]

    def _raw(self, side: int, region: str, name: str) -> Optional[torch.Tensor]:
        """the (B, recorded steps) series of a region and name on the CPU: fp64 (fused) or the field's dtype (torch); None if the
        side never had the name"""
        if (region, name) not in self._have[side]:
            return None
        idx = self._recorded()
        if self._series is not None:
            return self._series[side, self._srows[(region, name)]].cpu()[:, idx]
        return self._t_series[side][(region, name)].cpu()[:, idx]

    def _names(self, region: str) -> List[str]:
        """the names both sides recorded for a region, sorted"""
        return sorted(n for r, n in self._have[0] if r == region and (r, n) in self._have[1])

    def _annual_means(self):
        """annual.py:210-235: (years int64 array, name -> [target, generated] (B, years) arrays); a year a sample holds no more
        than 350 days' worth of steps of is NaN, a year no sample holds that many of is dropped, gap years are NaN"""
        idx = self._recorded()
        year = np.ascontiguousarray(self._year[:, idx])
        labels = np.unique(year)
        counts = np.stack([(year == y).sum(axis=1) for y in labels], axis=1).astype(np.float32)      # (B, labels)
        min_samples = MIN_COMPLETE_YEAR_DAYS * (datetime.timedelta(days=1) / self._timestep)
        keep = counts > min_samples
        kept = labels[keep.any(axis=0)]
        years = np.arange(kept.min(), kept.max() + 1, dtype=np.int64) if kept.size else np.zeros(0, np.int64)
        out = {}
        for name in self._names("globe"):
            sides = []
            for side in (1, 0):
                x = self._raw(side, "globe", name).numpy()
                means = np.full((x.shape[0], len(years)), np.nan, dtype=x.dtype)
                for k, y in enumerate(labels):
                    if y in kept:
                        with np.errstate(all="ignore"):
                            total = np.stack([x[b, year[b] == y].sum(dtype=x.dtype) for b in range(x.shape[0])])
                            means[:, y - years[0]] = np.where(keep[:, k], total / counts[:, k], np.nan)
                sides.append(means)
            out[name] = sides
        return years, out

    def _index_series(self, side: int, kind: str):
        """enso_index (dynamic_index.py:94-113): name -> the 5-month running mean of the monthly anomalies of the Nino 3.4 mean;
        ipo_index (ipo_index.py:139-165): name -> T2 - (T1 + T3) / 2 of the monthly anomalies of the three boxes; (B, months)
        tensors, and the sorted (year, month) pairs"""
        idx = self._recorded()
        # C order: torch follows the layout of a mask in its sums, and the reference's masks are C-ordered
        year, month = np.ascontiguousarray(self._year[:, idx]), np.ascontiguousarray(self._month[:, idx])
        out, keys = {}, []
        if kind == "enso":
            for name in SEA_SURFACE_TEMPERATURE_NAMES:
                raw = self._raw(side, "nino34", name)
                if raw is not None:
                    out[name], keys = running_monthly_mean(anomalies_from_monthly_climo(raw, month), year, month, 5)
        else:
            for name in IPO_SST_NAMES:
                raws = {r: self._raw(side, r, name) for r in TPI_REGIONS}
                if all(v is not None for v in raws.values()):
                    an = {}
                    for r, raw in raws.items():
                        an[r], keys = running_monthly_mean(anomalies_from_monthly_climo(raw, month), year, month, 1)
                    out[name] = an["T2"] - 0.5 * (an["T1"] + an["T3"])
        return out, keys

    def _seasonal_means(self):
        """name -> [target, generated] fp64 (4, H, W) seasonal means (seasonal.py:90-91), in DJF, MAM, JJA, SON order, on the CPU
        as the reference's are: what follows them does not depend on the device the sums were taken on"""
        counts = torch.tensor(self._season_counts, dtype=torch.float64)
        out = {}
        for name in sorted(n for n in self._season_names[0] if n in self._season_names[1]):
            sides = []
            for side in (1, 0):
                if self._bins is not None:
                    sums = self._bins[side, self._rows[name]].reshape((len(SEASONS),) + tuple(self._agg._shape))
                else:
                    sums = self._t_bins[side][name]
                sides.append(sums.cpu().to(torch.float64) / counts[:, None, None])
            out[name] = sides
        return out

    def dataset(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """label -> variables.  annual (annual.py:155-166): ``<name>`` (2, samples, years), the leading axis source = [target,
        prediction], and ``year``; enso_index (dynamic_index.py:339-351) and ipo_index (ipo_index.py:287-298): ``<name>`` (2,
        samples, months) and the ``year`` and ``month`` of each column.  seasonal has none (seasonal.py:177-182)."""
        ds: Dict[str, Dict[str, torch.Tensor]] = {}
        if not any(self._seen):
            return ds
        if self.annual is not None:
            years, means = self._annual_means()
            d = ds[self.annual.name or "annual"] = {n: torch.stack([torch.from_numpy(t), torch.from_numpy(g)]) for n, (t, g) in means.items()}
            d["year"] = torch.from_numpy(years)
        for kind, m, default in (("enso", self.enso, "enso_index"), ("ipo", self.ipo, "ipo_index")):
            if m is None:
                continue
            (tgt, keys), (gen, _) = self._index_series(1, kind), self._index_series(0, kind)
            d = {n: torch.stack([tgt[n], gen[n]]) for n in gen if n in tgt}
            if d:
                d["year"] = torch.tensor([k[0] for k in keys], dtype=torch.int64)
                d["month"] = torch.tensor([k[1] for k in keys], dtype=torch.int64)
                ds[m.name or default] = d
        return ds

    def _annual_logs(self) -> Dict[str, Any]:
        """annual.py:86-153: ``<name>`` the (2, samples, years) series [target, generated] (the reference's figure), and with
        more than one year ``rmse/<name>`` and ``crps/<name>``"""
        logs: Dict[str, Any] = {}
        years, means = self._annual_means()
        for name, (tgt, gen) in means.items():
            logs[name] = torch.from_numpy(np.stack([tgt, gen]))
            if len(years) > 1:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")                                 # a gap year is an all-NaN slice
                    tmean, gmean = np.nanmean(tgt, axis=0), np.nanmean(gen, axis=0)
                    if self.annual.report_rmse:
                        logs[f"rmse/{name}"] = float(np.sqrt(np.nanmean((gmean - tmean) ** 2)))
                    if self.annual.report_crps:
                        crps = fair_crps(torch.as_tensor(gen.T.copy(), dtype=torch.float32),
                                         torch.as_tensor(tmean, dtype=torch.float32).unsqueeze(1))
                        logs[f"crps/{name}"] = float(np.nanmean(crps.numpy()))
        return logs

    @staticmethod
    def _spectrum_logs(prefix: str, pred, tgt, with_bands: bool) -> Dict[str, Any]:
        """``<prefix>_power_spectrum`` (2, frequencies): cycles per year and the prediction's power, ``..._target`` the target's;
        with bands ``<prefix>_power_2_5yr`` / ``_1_16yr`` and their ``_norm`` (dynamic_index.py:289-333)"""
        logs: Dict[str, Any] = {}
        ps, ts = sample_average_power_spectrum(pred), sample_average_power_spectrum(tgt)
        if ps is None:
            return logs
        logs[f"{prefix}_power_spectrum"] = torch.from_numpy(np.stack(ps))
        if ts is not None:
            logs[f"{prefix}_power_spectrum_target"] = torch.from_numpy(np.stack(ts))
        for tag, bounds in (("2_5yr", (2.0, 5.0)), ("1_16yr", (1.0, 16.0))) if with_bands else ():
            p = psd_band_power(*ps, period_bounds=bounds)
            t = psd_band_power(*ts, period_bounds=bounds) if ts is not None else float("nan")
            logs[f"{prefix}_power_{tag}"] = p
            if t != 0 and not np.isnan(t):
                logs[f"{prefix}_power_{tag}_norm"] = p / t
        return logs

    def _enso_logs(self) -> Dict[str, Any]:
        """dynamic_index.py:241-337: ``<sst>_nino34_index`` (2, samples, months) [target, generated], ``_std``, ``_std_norm``, the
        spectra and band powers"""
        logs: Dict[str, Any] = {}
        (tgt, _), (gen, _) = self._index_series(1, "enso"), self._index_series(0, "enso")
        for name in SEA_SURFACE_TEMPERATURE_NAMES:
            if name not in gen or name not in tgt:
                continue
            g, t = gen[name].numpy(), tgt[name].numpy()
            if g.shape[1] > 1:
                logs[f"{name}_nino34_index"] = torch.stack([tgt[name], gen[name]])
                logs[f"{name}_nino34_index_std"] = sample_mean_std(g)
                logs[f"{name}_nino34_index_std_norm"] = sample_mean_std(g, t)
            if bool((~np.isnan(g)).any()):
                logs.update(self._spectrum_logs(f"{name}_nino34_index", g, t, True))
        return logs

    def _ipo_logs(self) -> Dict[str, Any]:
        """ipo_index.py:253-322: with every sample at least 80 years of months long ``<sst>_ipo_tpi_filtered`` (2, samples, months
        - 2 x 156) [target, generated], ``_ipo_tpi_std``, ``_std_norm`` and the spectra of the unfiltered index"""
        logs: Dict[str, Any] = {}
        (tgt, _), (gen, _) = self._index_series(1, "ipo"), self._index_series(0, "ipo")
        trim = int(IPO_CUTOFF_YEARS * 12)

        def filtered(index):
            rows = []
            for row in index:
                row = row[~np.isnan(row)]
                if len(row) < MIN_YEARS_FOR_FILTERED_TPI * 12:
                    return None
                rows.append(low_pass_filter(row)[trim:-trim])
            return rows

        for name in IPO_SST_NAMES:
            if name not in gen or name not in tgt or gen[name].shape[1] < 2:
                continue
            g, t = gen[name].numpy(), tgt[name].numpy()
            fg, ft = filtered(g), filtered(t)
            if fg is not None and ft is not None:
                n = min(len(r) for r in fg + ft)                                 # samples of one record are equally long
                fg, ft = (np.stack([r[:n] for r in rows]) for rows in (fg, ft))
                logs[f"{name}_ipo_tpi_filtered"] = torch.from_numpy(np.stack([ft, fg]))
                logs[f"{name}_ipo_tpi_std"] = sample_mean_std(fg)
                logs[f"{name}_ipo_tpi_std_norm"] = sample_mean_std(fg, ft)
                logs.update(self._spectrum_logs(f"{name}_ipo_tpi", g, t, False))
        return logs

    def _seasonal_logs(self) -> Dict[str, Any]:
        """seasonal.py:72-175: nothing unless all four seasons were recorded; ``anomaly/<name>`` (2, 4, H, W) [target, generated]
        minus the target's mean over the seasons, ``bias/<name>`` (4, H, W), ``r2/<name>``, ``time-mean-rmse/<name>-<season>`` and
        ``time-mean-rmse/<name>`` (the area mean, then the mean over seasons, then the root)"""
        logs: Dict[str, Any] = {}
        if any(c == 0 for c in self._season_counts):
            return logs
        for name, (tgt, gen) in self._seasonal_means().items():
            bias = gen - tgt
            pattern = tgt.mean(dim=0)
            ganom, tanom = gen - pattern, tgt - pattern
            logs[f"anomaly/{name}"] = torch.stack([tanom, ganom])
            logs[f"bias/{name}"] = bias
            logs[f"r2/{name}"] = float(1 - ((ganom - tanom) ** 2).sum() / ((tanom - tanom.mean()) ** 2).sum())
            mse = _wmean(bias ** 2, self._agg.weights_for(name, bias.device))
            for i, season in enumerate(SEASONS):
                logs[f"time-mean-rmse/{name}-{season}"] = float(mse[i].sqrt())
            logs[f"time-mean-rmse/{name}"] = float(mse.mean().sqrt())
        return logs

    def logs(self) -> Dict[str, Dict[str, Any]]:
        logs: Dict[str, Dict[str, Any]] = {}
        if not any(self._seen):
            return logs
        for m, default, fn in ((self.seasonal, "seasonal", self._seasonal_logs), (self.annual, "annual", self._annual_logs),
                               (self.enso, "enso_index", self._enso_logs), (self.ipo, "ipo_index", self._ipo_logs)):
            if m is not None:
                logs[m.name or default] = fn()
        return logs
