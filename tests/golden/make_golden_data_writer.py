"""tests/golden/gen_data_writer.pt from the reference's own functions (imported through oracle/ref_loader.load_stepper_ref's stubs, the
data-writer packages as bare namespaces and their xarray / netCDF siblings as permissive stubs), on the records of
tests/_data_writer_cases.py (exact arithmetic, rebuilt by every test; the file pins their checksums and holds results only):
  * ``_coarsen_tensor_dict`` (fme/ace/inference/data_writer/time_coarsen.py:187-196) for the factors 1, 2, 5;
  * ``MonthlyDataWriter._get_month_indices`` (monthly.py:159-190) on a ``SimpleNamespace`` time and a stand-in ``self``, and
    ``add_data`` with ``find_boundary`` (monthly.py:339-390) window by window, around them the array handling of
    ``append_batch`` (monthly.py:268-324) restated on numpy arrays of the netCDF variables' types (fp32 means, int64 counts) -
    netCDF4 is not on this machine.
``valid_time`` needs cftime in the reference (monthly.py:393-432); here the 15th of each month is counted with ``datetime.date``
(proleptic_gregorian) and by hand (noleap, 365 days a year).

The generator computes the exact answer too - the fields are built so that their fp64 sums are exact - and asserts that the
reference itself lies within the bars the tests hold the project to (u = 2^-24, m = max |x| over the steps of one output pixel):
|reference - exact| <= (f + 1) u m for a block of f steps and <= (N + 3 k) u m for a month of N steps delivered in k windows, which
with |ours - exact| <= u |mean| gives the tests' (f + 2) u m and (N + 3 k + 1) u m.  That keeps the bar a condition on the code
under test, not on the fixture."""
import datetime
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import _data_writer_cases as C  # noqa: E402
from oracle import ref_loader  # noqa: E402

U = 2.0 ** -24
_NOLEAP_CUM = (0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334)


def load():
    ref_loader.load_stepper_ref()
    ref = os.path.join(ref_loader.REF, "fme", "ace", "inference")
    for name, path in (("fme.ace.inference", ref), ("fme.ace.inference.data_writer", os.path.join(ref, "data_writer"))):
        ref_loader._ns(name, path)
    permissive = type(sys.modules["xarray"])
    for name in ("fme.ace.inference.data_writer.dataset_metadata", "fme.ace.inference.data_writer.raw", "fme.core.cloud",
                 "fme.core.writer", "fme.core.dataset.data_typing"):
        if name not in sys.modules:
            sys.modules[name] = permissive(name)
    return types.SimpleNamespace(coarsen=importlib.import_module("fme.ace.inference.data_writer.time_coarsen"),
                                 monthly=importlib.import_module("fme.ace.inference.data_writer.monthly"))


def time_like(year, month):
    ns = types.SimpleNamespace
    return ns(dt=ns(year=ns(values=year), month=ns(values=month)))


def absmax(x, axis):
    return np.max(np.abs(np.nan_to_num(x)), axis=axis)


def coarsen_case(R):
    c = C.coarsen()
    out = {"checksum": C.checksum(c["data"]), "ref": {}, "exact": {}}
    for f in C.FACTORS:
        ref = R.coarsen._coarsen_tensor_dict(c["data"], f)
        out["ref"][f] = ref
        out["exact"][f] = {}
        for n, x in c["data"].items():
            blocks = x.double().numpy().reshape(C.B, 10 // f, f, C.H, C.W)
            exact = blocks.sum(axis=2) / f                                     # the sums are exact: any order
            out["exact"][f][n] = torch.from_numpy(exact)
            m = absmax(blocks, axis=2)
            with np.errstate(invalid="ignore"):
                err = np.abs(ref[n].double().numpy() - exact)
            assert np.array_equal(np.isnan(err), np.isnan(exact)), (f, n)
            assert np.all(np.nan_to_num(err) <= (f + 1) * U * m), (f, n, float(np.nanmax(err / np.maximum(m, 1e-300)) / U))
    return out


def valid_time(calendar, starts, n_months):
    out = np.zeros((len(starts), n_months), np.int64)
    for b, (y0, m0, _) in enumerate(starts):
        for k in range(n_months):
            y, m = y0 + (m0 - 1 + k) // 12, (m0 - 1 + k) % 12 + 1
            if calendar == "proleptic_gregorian":
                out[b, k] = (datetime.date(y, m, 15) - datetime.date(1970, 1, 1)).days
            else:
                assert calendar == "noleap"
                out[b, k] = (y - 1970) * 365 + _NOLEAP_CUM[m - 1] + 14
    return out


def monthly_case(R, key):
    c = C.monthly(key)
    year, month = c["time"].year_month()
    n = c["n"]
    out = {"checksum": C.checksum(c["data"]), "ref": {}}
    M = R.monthly.MonthlyDataWriter
    windows_of = {}
    for cut in C.CUTS:
        me = types.SimpleNamespace(_init_years=np.full([C.B], -1, dtype=int), _init_months=np.full([C.B], -1, dtype=int))
        me._get_initial_year_and_month = types.MethodType(M._get_initial_year_and_month, me)
        size = 0
        counts = np.zeros((C.B, 0), np.int64)
        means = {name: np.zeros((C.B, 0, C.H, C.W), np.float32) for name in C.NAMES}
        nwin = np.zeros((C.B, 0), np.int64)                                 # windows that delivered steps of a (sample, month)
        for a, b in C.windows(n, cut):
            months = M._get_month_indices(me, time_like(year[:, a:b], month[:, a:b]))
            month_min = np.min(months)
            month_range = np.max(months) - month_min + 1
            new_size = month_min + month_range
            if new_size > size:                                             # _extend_variable: zeros
                grow = lambda v: np.concatenate([v, np.zeros((C.B, new_size - size) + v.shape[2:], v.dtype)], axis=1)  # noqa: E731
                counts, nwin, means, size = grow(counts), grow(nwin), {k: grow(v) for k, v in means.items()}, new_size
            count_data = counts[:, month_min:month_min + month_range]
            for name in C.NAMES:
                month_data = means[name][:, month_min:month_min + month_range].copy()
                R.monthly.add_data(target=month_data, target_start_counts=count_data, source=c["data"][name].numpy()[:, a:b],
                                   months_elapsed=months - month_min)
                means[name][:, month_min:month_min + month_range] = month_data
            for i in range(C.B):
                add = np.bincount(months[i], minlength=size)
                counts[i] += add
                nwin[i] += add > 0
        out["ref"][cut] = {**{k: torch.from_numpy(v) for k, v in means.items()}, "counts": torch.from_numpy(counts)}
        windows_of[cut] = nwin
    # the exact answer, and the reference against its bar
    me = types.SimpleNamespace(_init_years=np.full([C.B], -1, dtype=int), _init_months=np.full([C.B], -1, dtype=int))
    me._get_initial_year_and_month = types.MethodType(M._get_initial_year_and_month, me)
    months = M._get_month_indices(me, time_like(year, month))
    n_months = int(months.max()) + 1
    counts = np.stack([np.bincount(row, minlength=n_months) for row in months])
    exact, amax = {}, {}
    for name in C.NAMES:
        x = c["data"][name].double().numpy()
        e, m = np.zeros((C.B, n_months, C.H, C.W)), np.zeros((C.B, n_months, C.H, C.W))
        for b in range(C.B):
            for k in range(n_months):
                sel = months[b] == k
                if sel.any():
                    e[b, k] = x[b, sel].sum(axis=0) / sel.sum()              # exact sums: any order
                    m[b, k] = absmax(x[b, sel], axis=0)
        exact[name], amax[name] = e, m
    for cut in C.CUTS:
        assert np.array_equal(out["ref"][cut]["counts"].numpy(), counts), cut
        for name in C.NAMES:
            with np.errstate(invalid="ignore"):
                err = np.abs(out["ref"][cut][name].double().numpy() - exact[name])
            assert np.array_equal(np.isnan(err), np.isnan(exact[name])), (cut, name)
            bar = (counts + 3 * windows_of[cut])[:, :, None, None] * U * amax[name]
            assert np.all(np.nan_to_num(err) <= bar), (key, cut, name, float(np.nanmax(err / np.maximum(bar, 1e-300))))
    out["exact"] = {k: torch.from_numpy(v) for k, v in exact.items()}
    out["absmax"] = {k: torch.from_numpy(v) for k, v in amax.items()}
    out["counts"] = torch.from_numpy(counts)
    out["windows"] = {cut: torch.from_numpy(v) for cut, v in windows_of.items()}
    out["valid_time"] = torch.from_numpy(valid_time(c["calendar"], c["starts"], n_months))
    return out


def main():
    R = load()
    out = {"coarsen": coarsen_case(R), "monthly": {key: monthly_case(R, key) for key in C.MONTHLY}}
    dst = os.path.join(HERE, "gen_data_writer.pt")
    torch.save(out, dst)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
