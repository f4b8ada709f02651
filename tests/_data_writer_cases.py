"""The records the data-writer tests (time coarsening, monthly means) run on, made of exact arithmetic only - an integer hash scaled by
powers of two - so that tests/golden/make_golden_data_writer.py and every test machine build the same fp32 bits without storing the
fields.  5 x 8 pixels, two samples, three names:

  * ``t``   256 + 32 h, h the hash in [-0.5, 0.5): after the rounding to fp32 a multiple of 2^-16 below 2^9;
  * ``pr``  2^-13 h: a multiple of 2^-37 below 2^-14, exact in fp32;
  * ``sst`` 16 h + 280 with NaN over a patch of "land" pixels, every step.

Every value is a multiple of one power of two at most 2^25 times smaller than the largest, so a fp64 sum of up to 2^27 of them is
EXACT in any order: the exact monthly mean is known, and fp64 totals do not depend on how a record is cut into windows.  The fp32
sums of the reference do round (24 bits against sums of up to 300 such values).

  * ``coarsen()``: T = 10 steps for the factors 1, 2, 5.
  * ``monthly("sixhourly")``: ``proleptic_gregorian``, 300 steps of 6 hours; sample 0 from 2020-01-20 (the boundaries 1 February,
    1 March - after the leap day - and 1 April: months 0 .. 3), sample 1 from 2020-02-10 (months 0 .. 2).
  * ``monthly("fivedaily")``: ``noleap``, 30 steps of 5 days; sample 0 from 2021-01-03, sample 1 from 2021-02-27 (28 February is
    followed by 1 March)."""
import datetime

import numpy as np
import torch

from ace_amd.timeaxis import TimeAxis

H, W, B = 5, 8, 2
NAMES = ("t", "pr", "sst")
LAND = (slice(1, 3), slice(2, 5))
FACTORS = (1, 2, 5)
CUTS = (1, 7, 40)                                     # window lengths a monthly record is delivered in
MONTHLY = {
    "sixhourly": dict(calendar="proleptic_gregorian", step=datetime.timedelta(hours=6), n=300, starts=((2020, 1, 20), (2020, 2, 10))),
    "fivedaily": dict(calendar="noleap", step=datetime.timedelta(days=5), n=30, starts=((2021, 1, 3), (2021, 2, 27))),
}


def _hash(shape, salt):
    """uniform multiples of 2^-24 in [-0.5, 0.5) from a 64-bit multiplicative hash of the element index"""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        h = (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(6364136223846793005) + np.uint64(1442695040888963407)
        h ^= h >> np.uint64(29)
        h = h * np.uint64(0x9E3779B97F4A7C15)
    return ((h >> np.uint64(40)).astype(np.float64) / 2.0 ** 24 - 0.5).reshape(shape)


def fields(n_time, salt):
    """name -> (B, n_time, H, W) fp32"""
    shape = (B, n_time, H, W)
    t = (256.0 + 32.0 * _hash(shape, salt)).astype(np.float32)
    pr = (2.0 ** -13 * _hash(shape, salt + 101)).astype(np.float32)
    sst = (280.0 + 16.0 * _hash(shape, salt + 202)).astype(np.float32)
    sst[:, :, LAND[0], LAND[1]] = np.nan
    return {"t": torch.from_numpy(t), "pr": torch.from_numpy(pr), "sst": torch.from_numpy(sst)}


def coarsen():
    time = TimeAxis.regular((2020, 2, 27, 3), datetime.timedelta(hours=6), 10, n_samples=1).us
    time = np.concatenate([time, time + 3 * 3_600_000_000 + 1])          # sample 1 at odd microseconds: the floor of the mean shows
    return {"data": fields(10, 7), "time": TimeAxis("proleptic_gregorian", time)}


def monthly(key):
    spec = MONTHLY[key]
    time = np.concatenate([TimeAxis.regular(s, spec["step"], spec["n"], n_samples=1, calendar=spec["calendar"]).us for s in spec["starts"]])
    return {"data": fields(spec["n"], 11 if key == "sixhourly" else 13), "time": TimeAxis(spec["calendar"], time), **spec}


def windows(n, cut):
    return [(a, min(a + cut, n)) for a in range(0, n, cut)]


def checksum(data):
    """a few exact numbers of a record a golden file can pin: the fp64 sum of the finite values of every field"""
    return {n: float(torch.nan_to_num(x.double()).sum()) for n, x in data.items()}
