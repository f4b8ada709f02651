"""The records the calendar-metric tests (annual, seasonal, enso_index, ipo_index) run on, made of exact arithmetic only - integer
hashes and rationals, no transcendental function - so that tests/golden/make_golden_calendar.py and every test machine build the
same fp32 bits without storing the fields (2 x 2 x 249 planes would not fit a committed file):

  * ``main()``: 9 x 18, latitudes -80 ... 80 and longitudes 10 ... 350 (cells in Nino 3.4 and in all three tripole boxes), two
    samples on a ``noleap`` axis at a 5-day step, sample 1 starting 40 days after sample 0; 249 steps = three years of 73 steps and
    a partial one, so sample 0 has three complete years (73 > the 70 steps annual.py asks for), its fourth is dropped, and sample
    1's first year (65 steps) is NaN.  Names: ``sst`` with NaN over a "land" patch that reaches into the T1 box, and ``t``.
  * ``long()``: the same grid, ``sst`` only, 984 steps of 30 days on a ``360_day`` axis (82 years, one step per month) for the
    tripole index and its 13-year filter."""
import datetime

import numpy as np
import torch

from ace_amd.dataset_info import DatasetInfo
from ace_amd.timeaxis import TimeAxis

H, W, B = 9, 18, 2
LAT = np.arange(-80.0, 81.0, 20.0)
LON = np.arange(10.0, 351.0, 20.0)
LAND = (slice(5, 7), slice(6, 8))                     # 20N and 40N, 130E and 150E: (40N, 150E) lies in the T1 box


def _noise(shape, salt):
    """uniform in [-0.5, 0.5) from a 64-bit multiplicative hash of the element index: the same bits on every machine"""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        h = (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(6364136223846793005) + np.uint64(1442695040888963407)
        h ^= h >> np.uint64(29)
        h = h * np.uint64(0x9E3779B97F4A7C15)
    return ((h >> np.uint64(40)).astype(np.float64) / 2.0 ** 24 - 0.5).reshape(shape)


def _triangle(phase):
    """a triangle wave of period 1 and range [-1, 1]"""
    f = phase - np.floor(phase)
    return 4.0 * np.abs(f - 0.5) - 1.0


def info(timestep):
    return DatasetInfo((H, W), timestep=timestep, lat=torch.tensor(LAT, dtype=torch.float32), lon=torch.tensor(LON, dtype=torch.float32))


def _fields(n_time, days, salt, names):
    """(gen, target): name -> (B, n_time, H, W) fp32; days (B, n_time) since the start of sample 0's first year"""
    year_phase = days / 365.0
    lat = LAT[:, None] / 90.0
    pacific = ((LON[None, :] >= 150) & (LON[None, :] <= 270)) * (1.0 - np.abs(lat))              # an ENSO-like tropical pattern
    slow = _triangle(year_phase / 3.7)[:, :, None, None] + 0.5 * _triangle(year_phase / 17.0 + 0.3)[:, :, None, None]
    season = _triangle(year_phase)[:, :, None, None] * lat                                       # opposite in the two hemispheres
    out = []
    for side in range(2):
        d = {}
        for k, name in enumerate(names):
            base = 288.0 + 12.0 * (1.0 - np.abs(lat)) + (0.4 if side == 0 else 0.0) * lat          # the prediction's bias pattern
            x = base + 3.0 * season + (0.8 + 0.3 * side) * slow * pacific + 0.02 * year_phase[:, :, None, None] \
                + 1.5 * _noise((B, n_time, H, W), salt + 1000 * side + 100 * k)
            x = x.astype(np.float32)
            if name == "sst":
                x[:, :, LAND[0], LAND[1]] = np.nan
            d[name] = torch.from_numpy(x)
        out.append(d)
    return out


def _case(calendar, start, step_days, n_time, offsets, cuts, names, salt):
    step = datetime.timedelta(days=step_days)
    time = TimeAxis.regular(start, step, n_time, n_samples=B, calendar=calendar)
    shift = np.asarray(offsets, np.int64)[:, None]
    time = TimeAxis(time.calendar, time.us + shift * 86_400_000_000)
    days = (np.arange(n_time)[None, :] * step_days + shift).astype(np.float64)
    gen, target = _fields(n_time, days, salt, names)
    bounds = [0] + list(cuts) + [n_time]
    windows = [(({n: gen[n][:, a:b] for n in names}, {n: target[n][:, a:b] for n in names}), time[:, a:b])
               for a, b in zip(bounds[:-1], bounds[1:])]
    return {"info": info(step), "timestep": step, "time": time, "gen": gen, "target": target, "windows": windows, "names": names,
            "n_time": n_time}


def main(cuts=(83, 166)):
    """three windows by default; ``cuts`` are the first steps of the later windows"""
    return _case("noleap", (2001, 1, 1), 5, 249, (0, 40), cuts, ["sst", "t"], 7)


def long(cuts=(500,)):
    return _case("360_day", (1901, 1, 1), 30, 984, (0, 0), cuts, ["sst"], 11)


def checksum(c):
    """a few exact numbers of the record a golden file can pin: the fp64 sum of the finite values of every field"""
    return {f"{side}/{n}": float(torch.nan_to_num(c[side][n].double()).sum()) for side in ("gen", "target") for n in c["names"]}
