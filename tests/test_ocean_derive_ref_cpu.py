"""tests/_ocean_derive_ref.py - the numpy statement of ace_ocean_derive_window's contract (include/ace_sfno.h) - against the
reference's own fp32 outputs (tests/golden/gen_ocean_derived.pt, emitted by tests/golden/make_golden_ocean_derived.py).

Bars, with u = 2^-24, L the level count and A = CP RHO sum_k |thetao_k| dz_k (computed in fp64 here):
  ocean_heat_content       |stmt - ref| <= (L + 3) u A: three fp32 products per term and at most L - 1 fp32 adds in the reference,
                           one rounding in the statement
  its tendency             |stmt - ref| <= ((L + 3) u (A_t + A_{t-1}) + u |S_t - S_{t-1}|) / dt + u |stmt|
  the implied advection    the tendency's bar + u |stmt|
  net flux, hfds, sea_ice_fraction   bitwise
  HI, finite positive      relative error <= 2 u M + 2 u, M = 9 ln 10 + |ln vol| + |ln area| + |ln frac| (the reference's fp32 logs
                           were measured at 1.10 u M over 1e5 random inputs)
  HI, special rows         exactly the table
NaN patterns equal everywhere.  Every bar is asserted to be below 1e-4 of the output's largest magnitude on its case."""
import math
import os

import numpy as np
import pytest
import torch

import _ocean_derive_cases as C
import _ocean_derive_ref as R

U = 2.0 ** -24
ADV = "implied_tendency_of_ocean_heat_content_due_to_advection"


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(os.path.join(golden_dir, "gen_ocean_derived.pt"), weights_only=False)


def flat(t):
    return t.reshape(*t.shape[:-2], -1).numpy()


def statement_inputs(rec):
    """the keyword arguments of ``_ocean_derive_ref.derive_window`` for a golden case (every time level, no head)"""
    merged = {**rec["forcing"], **rec["data"]}
    kw = {n: flat(merged[n]) for n in ("hfds", "hfds_total_area", "hfgeou", "sea_surface_fraction", "land_fraction",
                                       "ocean_sea_ice_fraction", "sea_ice_fraction", "sea_ice_volume") if n in merged}
    if all(n in merged for n in C.THETAO):
        kw["thetao"] = [flat(merged[n]) for n in C.THETAO]
    kw["dz"] = np.ascontiguousarray(flat(rec["dz"].permute(2, 0, 1)))
    kw["mask0"] = flat(rec["mask"][..., 0].float())
    kw["area_m2"] = flat(rec["area_m2"].float())
    return kw


def bars(rec, stmt):
    """name -> (B, T, hw) bar on |stmt - ref| (0: bitwise), from the inputs and the statement alone"""
    out = {}
    L, dt = C.NLEV, C.TIMESTEP_SECONDS
    merged = {**rec["forcing"], **rec["data"]}
    if "ocean_heat_content" in stmt:
        th = np.stack([flat(merged[n]) for n in C.THETAO]).astype(np.float64)                  # (L, B, T, hw)
        dz = flat(rec["dz"].permute(2, 0, 1)).astype(np.float64)[:, None, None]
        A = R.CP_RHO * np.nansum(np.abs(th) * dz, axis=0)
        S = R.column_sum(list(th.astype(np.float32)), flat(rec["dz"].permute(2, 0, 1)))
        out["ocean_heat_content"] = (L + 3) * U * A
        tb = np.zeros_like(A)
        tb[:, 1:] = ((L + 3) * U * (A[:, 1:] + A[:, :-1]) + U * np.abs(S[:, 1:] - S[:, :-1])) / dt
        out["ocean_heat_content_tendency"] = tb + U * np.abs(np.nan_to_num(stmt["ocean_heat_content_tendency"].astype(np.float64)))
        if ADV in stmt:
            out[ADV] = out["ocean_heat_content_tendency"] + U * np.abs(np.nan_to_num(stmt[ADV].astype(np.float64)))
    for name in ("net_energy_flux_into_ocean_column", "hfds", "sea_ice_fraction"):
        if name in stmt:
            out[name] = np.zeros(stmt[name].shape)
    return out


def hi_inputs(kw):
    """(vol, area, frac) of the sea-ice thickness as the contract forms them, fp32"""
    one = np.float32(1)
    ssf = kw["sea_surface_fraction"] if "sea_surface_fraction" in kw else one - kw["land_fraction"]
    with np.errstate(all="ignore"):
        frac = (kw["ocean_sea_ice_fraction"] * ssf if "ocean_sea_ice_fraction" in kw
                else (kw["sea_ice_fraction"] * ssf) / (one - kw["land_fraction"]))
    return kw["sea_ice_volume"], np.broadcast_to(kw["area_m2"], frac.shape), frac


def check_against_reference(rec, got, timestep_seconds, what="", expected=None):
    """``got``: name -> (B, T, hw) fp32 of every variable the reference derived on this case, held to the reference's fp32 outputs
    (or to ``expected``, another fp32 evaluation of the reference's op sequence) within the bars of this module's docstring (the
    bars come from the inputs and the statement, never from ``got``)"""
    expected = rec["expected"] if expected is None else expected
    want = [n for n in C.OUTPUTS if n in rec["expected"]]
    assert set(got) == set(want), (what, sorted(got), want)
    kw = statement_inputs(rec)
    stmt = R.derive_window(want, timestep_seconds, **kw)
    bar = bars(rec, stmt)
    for n in want:
        ref = flat(expected[n])
        assert got[n].dtype == np.float32 and got[n].shape == ref.shape, (what, n)
        assert np.array_equal(np.isnan(got[n]), np.isnan(ref)), (what, n, "NaN pattern")
        ok = ~np.isnan(ref)
        err = np.abs(got[n].astype(np.float64) - ref.astype(np.float64))
        if n == "HI":
            vol, area, frac = hi_inputs(kw)
            with np.errstate(all="ignore"):
                regular = np.isfinite(vol) & np.isfinite(frac) & np.isfinite(area) & (vol > 0) & (frac > 0) & (area > 0) \
                    & (ref < R.FLT_MAX)
                M = 9 * math.log(10) + np.abs(np.log(vol.astype(np.float64))) + np.abs(np.log(area.astype(np.float64))) \
                    + np.abs(np.log(frac.astype(np.float64)))
                rel = err / np.abs(stmt[n].astype(np.float64))
            assert regular.sum() > 0.8 * regular.size        # the special cases hold two pixels of special cell area at every step
            hbar = 2 * U * M + 2 * U
            print(f"{what} HI: max rel err {rel[regular].max():.4g} = {(rel / (U * M))[regular].max():.3f} u M, "
                  f"max bar {hbar[regular].max():.4g}")
            assert (rel[regular] <= hbar[regular]).all(), (what, float((rel / hbar)[regular].max()))
            assert hbar[regular].max() < 1e-4
            special = ~regular & ok                          # exactly equal
            assert np.array_equal(got[n][special], ref[special]), (what, "HI at special inputs")
            continue
        print(f"{what} {n}: max err {err[ok].max():.4g}, max bar {bar[n][ok].max():.4g}, max |out| {np.abs(ref[ok]).max():.4g}")
        if not bar[n].any():
            assert np.array_equal(got[n].view(np.int32)[ok], ref.view(np.int32)[ok]), (what, n, "not bitwise")
            continue
        assert (err[ok] <= bar[n][ok]).all(), (what, n, float((err[ok] / bar[n][ok]).max()))
        assert bar[n][ok].max() < 1e-4 * np.abs(ref[ok]).max(), (what, n, "the bar does not bite")


@pytest.mark.parametrize("name", list(C.CASES))
def test_statement_against_the_reference(gold, name):
    rec = gold["cases"][name]
    want = [n for n in C.OUTPUTS if n in rec["expected"]]
    assert tuple(want) == tuple(n for n in C.OUTPUTS if n in C.CASES[name]["derived"])
    stmt = R.derive_window(want, gold["timestep_seconds"], **statement_inputs(rec))
    check_against_reference(rec, stmt, gold["timestep_seconds"], name)


@pytest.mark.parametrize("name", [n for n, c in C.CASES.items() if c.get("special")])
def test_sea_ice_thickness_at_the_special_rows(gold, name):
    rec = gold["cases"][name]
    kw = statement_inputs(rec)
    stmt = R.derive_window(["HI"], gold["timestep_seconds"], **kw)["HI"]
    ref = flat(rec["expected"]["HI"])
    n = len(C.SPECIAL_ROWS)
    want = np.array(C.SPECIAL_EXPECTED, np.float32)
    assert np.array_equal(stmt[0, 0, :n], want, equal_nan=True) and np.array_equal(ref[0, 0, :n], want, equal_nan=True)
    if C.CASES[name]["special"] == "total_fraction":      # 1 - land NaN, and 1 - land = 0 (an infinite fraction)
        assert stmt[0, 1, 0] == 0 and stmt[0, 1, 1] == 0 and ref[0, 1, 0] == 0 and ref[0, 1, 1] == 0


def test_the_statement_takes_the_first_tendency_from_the_head(gold):
    """with a head the window's rows are the rows 1 .. of the whole series; an absent head level counts as nothing"""
    rec = gold["cases"]["budget_hfds_ssf_geo"]
    kw = statement_inputs(rec)
    want = list(C.OUTPUTS[:4])
    whole = R.derive_window(want, gold["timestep_seconds"], **kw)
    tail = {k: (v[:, 1:] if v.ndim == 3 and k not in ("dz",) else v) for k, v in kw.items() if k != "thetao"}
    tail["thetao"] = [x[:, 1:] for x in kw["thetao"]]
    got = R.derive_window(want, gold["timestep_seconds"], head=[x[:, 0] for x in kw["thetao"]], **tail)
    for n in want:
        assert np.array_equal(got[n], whole[n][:, 1:], equal_nan=True), n
    head = [x[:, 0] for x in kw["thetao"]]
    head[2] = None
    nan_level = [x.copy() for x in kw["thetao"]]
    nan_level[2][:, 0] = np.nan
    whole = R.derive_window(want, gold["timestep_seconds"], **{**kw, "thetao": nan_level})
    got = R.derive_window(want, gold["timestep_seconds"], head=head, **tail)
    for n in want:
        assert np.array_equal(got[n], whole[n][:, 1:], equal_nan=True), n
