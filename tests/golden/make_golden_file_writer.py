"""tests/golden/gen_file_writer.pt from the reference's own pure functions (loaded as tests/golden/make_golden_data_writer.py loads
them: oracle/ref_loader.load_stepper_ref's stubs, the data-writer packages as bare namespaces, their xarray / netCDF / zarr siblings
as permissive stubs) and from pandas, which xarray's label selection rests on.  Results only:
  * ``slice``: ``range(T)[Slice.shift_left(Slice(start, stop, step), n_seen).slice]`` (fme/core/typing_.py:19-85, the way
    file_writer.py:151-153 uses it) for a grid of (start, stop, step, n_seen, T) - the kept steps as a list, or "ValueError" for a
    negative bound;
  * ``month_string``: ``_month_string_to_int`` (file_writer.py:50-66) for every full and three-letter name, some in other letter
    cases, and strings it refuses ("ValueError");
  * ``mask``: ``_get_time_mask`` (file_writer.py:69-94) on a stand-in time whose ``dt.month`` is a numpy array and whose
    ``dt.season`` is the season of that month as xarray names it (DJF = 12, 1, 2; MAM; JJA; SON) - xarray is not on this machine,
    so the accessor is restated, the function is the reference's;
  * ``extent``: ``pandas.Index(coord).slice_indexer(lo, hi)``, which is what ``.sel(lat=slice(lo, hi))`` (file_writer.py:252-261,
    406-410, 530-537) resolves to, on increasing and decreasing coordinates: interior bounds, exact cell-centre hits, open ends,
    reversed bounds, bounds out of range - the kept indices as a list.
pandas is used here only; the package restates the rule with numpy.searchsorted."""
import importlib
import itertools
import os
import sys
import types

import numpy as np
import pandas as pd
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_loader  # noqa: E402

SEASON_OF = {12: "DJF", 1: "DJF", 2: "DJF", 3: "MAM", 4: "MAM", 5: "MAM", 6: "JJA", 7: "JJA", 8: "JJA", 9: "SON", 10: "SON", 11: "SON"}
MONTHS = ["January", "February", "March", "April", "May", "June", "July", "August", "September", "October", "November", "December"]
SELECTIONS = [["JJA"], ["DJF"], ["MAM", "SON"], ["January"], ["Feb", "DJF"], ["december", "JUN", "Sep"], ["May", "may", "MAY"],
              ["JJA", "July"], MONTHS, [m[:3] for m in MONTHS]]
COORDS = {
    "lat_1deg": np.arange(-89.5, 90.0, 1.0),                       # cell centres, increasing
    "lat_1deg_desc": np.arange(89.5, -90.0, -1.0),                 # the same, north first
    "lon_1deg": np.arange(0.5, 360.0, 1.0),
    "lat_gauss8": np.array([-73.8, -52.8, -31.7, -10.6, 10.6, 31.7, 52.8, 73.8]),
    "single": np.array([12.0]),
    "repeated": np.array([0.0, 1.0, 1.0, 2.0, 3.0]),
}
EXTENTS = [(-10, 10.5), (-10.5, 10.5), (-10.5, 10), (-9.99, 9.99), (10.5, -10.5), (10, -10), (None, 0), (0, None), (None, None),
           (-500, 500), (500, -500), (-500, -100), (100, 500), (400, 500), (89.5, 89.5), (-89.5, -89.5), (0.5, 0.5), (0.6, 0.9),
           (120.5, 160), (359.5, 400), (1, 1), (1, 2), (12, 12), (11, 13), (13, 14), (-73.8, 73.8), (73.8, -73.8), (-31.7, 10.6)]


def load():
    ref_loader.load_stepper_ref()
    ref = os.path.join(ref_loader.REF, "fme", "ace", "inference")
    for name, path in (("fme.ace.inference", ref), ("fme.ace.inference.data_writer", os.path.join(ref, "data_writer"))):
        ref_loader._ns(name, path)
    permissive = type(sys.modules["xarray"])
    for name in ("fme.ace.inference.data_writer.dataset_metadata", "fme.ace.inference.data_writer.raw", "fme.core.cloud",
                 "fme.core.writer", "fme.core.dataset.data_typing", "fme.ace.inference.data_writer.zarr", "fme.core.dataset.time"):
        if name not in sys.modules:
            sys.modules[name] = permissive(name)
    return types.SimpleNamespace(typing=importlib.import_module("fme.core.typing_"),
                                 fw=importlib.import_module("fme.ace.inference.data_writer.file_writer"))


def slice_cases(R):
    out = {}
    grid = itertools.product([None, 0, 3, 7, 12, -2], [None, 0, 5, 10, 12, 30, -1], [None, 1, 2, 3], [0, 4, 5, 8, 12, 16], [1, 4, 5])
    for start, stop, step, n_seen, T in grid:
        try:
            out[(start, stop, step, n_seen, T)] = list(range(T)[R.typing.Slice.shift_left(R.typing.Slice(start, stop, step), n_seen).slice])
        except ValueError:
            out[(start, stop, step, n_seen, T)] = "ValueError"
    return out


def month_cases(R):
    out = {}
    for name in MONTHS + [m[:3] for m in MONTHS] + ["january", "FEBRUARY", "mar", "DEC", "Sept", "Janu", "", "13", "JJA", "Febr."]:
        try:
            out[name] = R.fw._month_string_to_int(name)
        except ValueError:
            out[name] = "ValueError"
    return out


def mask_cases(R):
    import xarray as xr                                   # the permissive stub: DataArray is a bare class
    month = np.array([11, 12, 12, 1, 1, 2, 3, 4, 5, 5, 6, 7, 8, 8, 9, 10, 11, 12, 1, 6])
    time = xr.DataArray()
    time.dt = types.SimpleNamespace(month=month, season=np.array([SEASON_OF[int(m)] for m in month]))
    out = {"month": month.tolist(), "masks": []}
    for sel in SELECTIONS:
        out["masks"].append((list(sel), np.asarray(R.fw._get_time_mask(time, sel)).astype(bool).tolist()))
    return out


def extent_cases():
    out = []
    for key, coord in COORDS.items():
        index = pd.Index(coord)
        for lo, hi in EXTENTS:
            kept = np.arange(len(coord))[index.slice_indexer(lo, hi)]
            out.append((key, lo, hi, kept.tolist()))
    # the example of the issue: 1-degree cell centres, (-10, 10.5) keeps rows 80 .. 100
    assert [c for c in out if c[:3] == ("lat_1deg", -10, 10.5)][0][3] == list(range(80, 101))
    return {"coords": {k: v.tolist() for k, v in COORDS.items()}, "cases": out}


def main():
    R = load()
    out = {"slice": slice_cases(R), "month_string": month_cases(R), "mask": mask_cases(R), "extent": extent_cases()}
    dst = os.path.join(HERE, "gen_file_writer.pt")
    torch.save(out, dst)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
