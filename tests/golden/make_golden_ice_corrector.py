"""Golden vectors for the sea-ice corrector, emitted by the REAL reference (fme/core/corrector/ice.py) imported under the stubs of
oracle/ref_loader.load_corrector - build container only.  One small file per case, tests/golden/gen_ice_corrector_<case>.pt, at
B = 2, 6 x 9: the corrector config as a checkpoint carries it, the timestep, the step's input and output in fp32, the reference's
corrected fp32 fields, and the flag path the reference took per variable - recorded from its own ``torch.any`` calls while it
ran, and asserted to be the path the case was built for.

The field of a variable is quiet (0 < new mass < 1 everywhere) except for what a case switches on, each a single pixel of
sample 1: A (new mass < 0), B (new mass > 1), C (new mass > 0 on an ice-free pixel).  Sample 0 always carries sign violations
(a negative source, a positive sink), which survive exactly when no stage runs.  Ice-free pixels (row 4) have a zero old mass and
zero terms of the first variable."""
import datetime
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_loader  # noqa: E402
import _ice_ref  # noqa: E402

B, H, W = 2, 6, 9
SIX_HOURS = datetime.timedelta(hours=6)
FIVE_DAYS_ODD = datetime.timedelta(days=5, microseconds=1)      # 432000.000001 s: dt * x is inexact in fp64
TERMS = {"simass": ["SIMSRC", "SIMSNK", "SIMXPRT"], "siconc": ["LSRCc", "LSNKc", "XPRTc"], "sisnmass": ["SNSRC", "SNSNK", "SNXPRT"],
         "sea_ice_fraction": ["LSRCc", "LSNKc", "XPRTc"]}
SIC = ("siconc", "sea_ice_fraction", "ocean_sea_ice_fraction")
SCALE = {"simass": 40.0, "sisnmass": 7.0}
# the trigger pixels (sample 1) of each variable, apart from one another: A, B, C (C on the ice-free row)
PIX = {"simass": ((2, 1), None, None), "siconc": ((2, 5), (3, 7), (4, 4)), "sea_ice_fraction": ((2, 5), (3, 7), (4, 4)),
       "sisnmass": ((1, 7), None, (4, 6))}


def quiet_field(name, seed, dt, first, others_a=()):
    """old, source, sink, transport of one variable with no stage mask set anywhere"""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(B, H, W, generator=g)
    c = SCALE.get(name, 1.0)
    old = u(0.3, 0.7) * c
    s, k, t = u(0.0, 0.05) * c / dt, -u(0.0, 0.05) * c / dt, u(-0.05, 0.05) * c / dt
    for x in (s, k, t):                                  # every count of non-zero terms occurs
        x[torch.rand(B, H, W, generator=g) < 0.2] = 0.0
    # sign violations in sample 0 (small: the new mass stays inside (0, 1))
    s[0, 0, 1] = -0.01 * c / dt
    k[0, 0, 2] = 0.01 * c / dt
    s[0, 1, 3], k[0, 1, 3] = -0.02 * c / dt, 0.015 * c / dt
    # the ice-free row: the first variable is exactly zero there, the others have nothing to remove
    for x in (old, s, k, t):
        x[:, 4] = 0.0
    # where the first variable is driven to (about) zero by its stage 1, the others hold nothing either
    if not first:
        for (i, j) in others_a:
            for x in (old, s, k, t):
                x[1, i, j] = 0.0
    return [x.float() for x in (old, s, k, t)]


def build_case(variables, on, dt, seed, special=None):
    """variables: names in processing order; on: {name: "ABC" subset}"""
    inp, gen = {}, {}
    first_a = [PIX[variables[0]][0]]
    for v, name in enumerate(variables):
        old, s, k, t = quiet_field(name, seed + 17 * v, dt, v == 0, first_a)
        c = SCALE.get(name, 1.0)
        pa, pb, pc = PIX[name]
        trig = on.get(name, "")
        if "A" in trig:
            k[1][pa] = -2.0 * c / dt                      # new mass about -1.5 c
            if float(old[1][pa]) == 0.0:
                old[1][pa] = 0.4 * c
        if "B" in trig:
            s[1][pb] = 1.0 * c / dt                       # new mass about 1.5
        if "C" in trig:
            old[1][pc], s[1][pc], k[1][pc], t[1][pc] = 0.4 * c, 0.03 * c / dt, -0.01 * c / dt, 0.0
        if special == "all_zero":                         # the whole residual goes to the transport
            for p, o in ((pa, -0.25), (pb, 1.5)):
                old[1][p], s[1][p], k[1][p], t[1][p] = o, 0.0, 0.0, 0.0
        if special == "overshoot":
            old[1][pa], s[1][pa], k[1][pa], t[1][pa] = 0.1, 1e-3 / dt, -0.05 / dt, -0.9 / dt      # k + share > 0
            old[1][pb], s[1][pb], k[1][pb], t[1][pb] = 0.9, 0.01 / dt, 0.0, 0.8 / dt              # s - share < 0
        inp[name] = old
        for term, x in zip(TERMS[name], (s, k, t)):
            gen[term] = x
        gen[name] = torch.rand(B, H, W, generator=torch.Generator().manual_seed(seed + 99 + v))      # overwritten
    gen["sst"] = torch.full((B, H, W), 271.5)            # an uncorrected field passes through
    inp["sst"] = torch.full((B, H, W), 271.0)
    if special == "nan":
        first = variables[0]
        inp[first][0, 2, 2] = float("nan")               # a NaN ice mass is "not zero"
        gen[TERMS[first][1]][1, 3, 3] = float("nan")
        gen[TERMS[variables[1]][0]][0, 3, 4:6] = float("nan")
        gen[TERMS[variables[-1]][2]][1, 4, 1] = float("nan")      # on the ice-free row
        inp[variables[1]][0, 2, 2] = 0.4
    if special == "tiny":                                # candidates for a first-variable mass that is non-zero only in fp64
        g = torch.Generator().manual_seed(seed + 5)
        first = variables[0]
        a = (torch.rand(W, generator=g) + 0.5) * 1e-36
        b = (torch.rand(W, generator=g) + 0.5) * 1e-36
        inp[first][0, 5] = 0.0
        gen[TERMS[first][0]][0, 5], gen[TERMS[first][1]][0, 5], gen[TERMS[first][2]][0, 5] = a + b, -a, -b
        for name in variables[1:]:                       # ice present in fp64: these stay as they are
            c = SCALE.get(name, 1.0)
            inp[name][0, 5] = 0.4 * c
            gen[TERMS[name][0]][0, 5], gen[TERMS[name][1]][0, 5], gen[TERMS[name][2]][0, 5] = 0.03 * c / dt, -0.01 * c / dt, 0.0
    return inp, gen


def run_reference(ice, config_state, inp, gen, timestep):
    """the reference's corrected fields, and the value of every ``torch.any`` it evaluated, in order"""
    cfg = ice.IceCorrectorConfig(budget_correction=ice.IceBudgetCorrectionConfig(**config_state["budget_correction"])
                                 if config_state.get("budget_correction") is not None else None)
    corrector = cfg._build(None, timestep)
    seen = []
    real_any = torch.any

    def recording_any(*a, **k):
        r = real_any(*a, **k)
        seen.append(bool(r))
        return r
    torch.any = recording_any
    try:
        out = corrector(inp, gen, {}, None)
    finally:
        torch.any = real_any
    corrected = out.corrected if hasattr(out, "corrected") else out[0]
    return dict(corrected), seen


def paths_from_any(plan, seen):
    """the recorded ``torch.any`` values, one per stage a variable has, as (a1, a2, a3) per variable"""
    paths, i = {}, 0
    for name, _, area, masked in plan:
        a1 = seen[i]; i += 1
        a2 = a3 = False
        if area:
            a2 = seen[i]; i += 1
        if masked:
            a3 = seen[i]; i += 1
        paths[name] = (int(a1), int(a2), int(a3))
    assert i == len(seen), (i, seen)
    return paths


def plan_of(cv):
    order = [n for n in ("simass",) if n in cv] + [n for n in SIC if n in cv] + [n for n in ("sisnmass",) if n in cv]
    return [(n, tuple(cv[n]), n in SIC, i > 0) for i, n in enumerate(order)]


def cases():
    three = ["simass", "siconc", "sisnmass"]
    seed = 100
    # every path of a masked concentration (8), of a masked mass (4, twice) and of an unmasked mass (2, four times)
    for a1 in (0, 1):
        for a2 in (0, 1):
            for a3 in (0, 1):
                sn = (a2, a1 ^ a3)                       # sisnmass (a1, a3): all four pairs over the eight cases
                on = {"siconc": "A" * a1 + "B" * a2 + "C" * a3, "sisnmass": "A" * sn[0] + "C" * sn[1], "simass": "A" * (a3 ^ a2)}
                want = {"simass": (a3 ^ a2, 0, 0), "siconc": (a1, a2, a3), "sisnmass": (sn[0], 0, sn[1])}
                seed += 1
                yield f"masked_{a1}{a2}{a3}", three, on, want, SIX_HOURS if a1 else FIVE_DAYS_ODD, seed, None
    for a1 in (0, 1):                                    # every path of an unmasked concentration
        for a2 in (0, 1):
            seed += 1
            yield f"alone_{a1}{a2}", ["siconc"], {"siconc": "A" * a1 + "B" * a2}, {"siconc": (a1, a2, 0)}, SIX_HOURS, seed, None
    yield "all_zero", ["siconc"], {"siconc": "AB"}, {"siconc": (1, 1, 0)}, SIX_HOURS, 201, "all_zero"
    yield "overshoot", ["siconc"], {"siconc": "AB"}, {"siconc": (1, 1, 0)}, SIX_HOURS, 202, "overshoot"
    yield "nan", three, {"siconc": "AC", "sisnmass": "C", "simass": "A"}, {"simass": (1, 0, 0), "siconc": (1, 0, 1), "sisnmass": (0, 0, 1)}, \
        FIVE_DAYS_ODD, 203, "nan"
    yield "tiny", three, {"siconc": "C"}, {"simass": None, "siconc": None, "sisnmass": None}, FIVE_DAYS_ODD, 204, "tiny"
    yield "sea_ice_fraction", ["simass", "sea_ice_fraction"], {"sea_ice_fraction": "BC"}, \
        {"simass": (0, 0, 0), "sea_ice_fraction": (0, 1, 1)}, SIX_HOURS, 205, None
    yield "mass_snow", ["simass", "sisnmass"], {"simass": "A", "sisnmass": "C"}, {"simass": (1, 0, 0), "sisnmass": (0, 0, 1)}, SIX_HOURS, 206, None
    yield "none", [], {}, {}, SIX_HOURS, 207, None


def main():
    ref_loader.load_corrector()
    ice = importlib.import_module("fme.core.corrector.ice")
    covered = {"masked_conc": set(), "masked_mass": set(), "alone_conc": set(), "alone_mass": set()}
    for case, variables, on, want, timestep, seed, special in cases():
        dt = timestep.total_seconds()
        if variables:
            inp, gen = build_case(variables, on, dt, seed, special)
            cv = {n: TERMS[n] for n in variables}
            if case == "alone_00":                       # a key outside the five known names is ignored
                cv["not_a_sea_ice_variable"] = ["a", "b", "c"]
            state = {"budget_correction": {"corrected_variables": cv}}
        else:
            inp, gen = build_case(["siconc"], {}, dt, seed)
            state = {"budget_correction": {"corrected_variables": None}}
        corrected, seen = run_reference(ice, state, inp, gen, timestep)
        plan = plan_of({n: TERMS[n] for n in variables})
        paths = paths_from_any(plan, seen)
        for name in variables:
            if want[name] is not None:
                assert paths[name] == want[name], (case, name, paths[name], want[name])
        assert set(corrected) == set(gen), (case, sorted(corrected))       # the sequence hands back the whole output
        assert torch.equal(corrected["sst"], gen["sst"])
        # what the numpy statement says about this case: the same path, and the events the case is there for
        npv = _ice_ref.variables_from_case(plan, {k: v.numpy() for k, v in inp.items()}, {k: v.numpy() for k, v in gen.items()})
        _, _, info = _ice_ref.ice_budget_ref(npv, dt)
        for (name, _, area, masked), i in zip(plan, info):
            assert tuple(i["path"]) == paths[name], (case, name, i["path"], paths[name])
            covered[("masked_" if masked else "alone_") + ("conc" if area else "mass")].add(paths[name])
        if special == "all_zero":
            assert info[0]["stages"][1]["all_zero"] == 1 and info[0]["stages"][2]["all_zero"] == 1, info[0]["stages"]
        if special == "overshoot":
            assert info[0]["stages"][1]["k_overshoot"] >= 1 and info[0]["stages"][2]["s_overshoot"] >= 1, info[0]["stages"]
        if special == "tiny":
            m64 = info[0]["mass64"][0, 5]
            tiny = (m64 != 0) & (m64.astype(np.float32) == 0)
            assert tiny.any(), m64
            assert (corrected["simass"][0, 5].numpy()[tiny] == 0).all()
            # a corrector that re-read the fp32 mass would call these pixels ice free and empty them
            assert (corrected["siconc"][0, 5].numpy()[tiny] > 0).all() and paths["siconc"][2] == 1
            print(f"  tiny: {int(tiny.sum())} pixels with a mass non-zero in fp64 only, e.g. {m64[tiny][0]:.3e}")
        if case == "masked_000":      # the violations survive when nothing runs
            assert float(corrected["LSRCc"][0, 0, 1]) < 0 and float(corrected["LSNKc"][0, 0, 2]) > 0
        if case == "masked_100":      # ... and are repaired, in the other sample, by a single pixel's trigger
            assert float(corrected["LSRCc"][0, 0, 1]) == 0 and float(corrected["LSNKc"][0, 0, 2]) == 0
        rec = {"config": {"type": "ice_corrector", "config": state}, "timestep_seconds": dt,
               "timestep_microseconds": timestep // datetime.timedelta(microseconds=1), "input": inp, "output": gen,
               "corrected": corrected, "paths": paths}
        path = os.path.join(HERE, f"gen_ice_corrector_{case}.pt")
        torch.save(rec, path)
        print(case, paths, os.path.getsize(path), "bytes")
    assert len(covered["masked_conc"]) == 8 and len(covered["masked_mass"]) == 4, covered
    assert len(covered["alone_conc"]) == 4 and len(covered["alone_mass"]) == 2, covered


if __name__ == "__main__":
    main()
