"""Sea-ice budget fields at any (B, H * W) for the kernel tests, in the manner of tests/golden/make_golden_ice_corrector.py: a
quiet field per variable (0 < new mass < 1 everywhere, every count of non-zero terms) plus what a case switches on, each a single
pixel of the LAST sample: A (new mass < 0), B (new mass > 1), C (new mass > 0 on an ice-free pixel).  Sample 0 carries sign
violations in its first pixels, which survive exactly when no stage runs.  numpy only.

    variables = make(B, HW, spec, on, dt, seed)      # spec: [(area_mode, masked), ...]; on: {v: "ABC" subset}
"""
import numpy as np

THREE = [(False, False), (True, True), (False, True)]      # simass, siconc, sisnmass
SCALES = [40.0, 1.0, 7.0]


def pixels(HW):
    """trigger pixels of each variable, from the end of the plane (HW >= 15): {v: (A, B, C)}; C is on an ice-free pixel"""
    return {0: (HW - 11, None, None), 1: (HW - 1, HW - 3, HW - 5), 2: (HW - 7, None, HW - 9)}


def make(B, HW, spec, on, dt, seed):
    assert HW >= 15 and len(spec) <= 3
    rng = np.random.default_rng(seed)
    P = pixels(HW)
    ice_free = [HW - 5, HW - 9, 0]
    # a lone variable takes the concentration's pixels, so that its A trigger is the last pixel of the last sample
    slots = [1] if len(spec) == 1 else list(range(len(spec)))
    out = []
    for v, (area, masked) in enumerate(spec):
        slot = slots[v]
        c = 1.0 if area else SCALES[slot]
        u = lambda lo, hi: rng.uniform(lo, hi, (B, HW))
        old, s, k, t = u(0.3, 0.7) * c, u(0.0, 0.05) * c / dt, -u(0.0, 0.05) * c / dt, u(-0.05, 0.05) * c / dt
        for x in (s, k, t):
            x[rng.uniform(size=(B, HW)) < 0.2] = 0.0
        s[0, 1] = -0.01 * c / dt
        k[0, 2] = 0.01 * c / dt
        s[0, 3], k[0, 3] = -0.02 * c / dt, 0.015 * c / dt
        for x in (old, s, k, t):
            x[:, ice_free] = 0.0
            if v > 0:
                x[B - 1, P[slots[0]][0]] = 0.0        # where variable 0's stage 1 leaves (about) nothing
        pa, pb, pc = P[slot]
        trig = on.get(v, "")
        if "A" in trig:
            old[B - 1, pa], k[B - 1, pa] = 0.4 * c, -2.0 * c / dt
        if "B" in trig:
            assert area
            s[B - 1, pb] = 1.0 / dt
        if "C" in trig:
            assert masked
            old[B - 1, pc], s[B - 1, pc], k[B - 1, pc], t[B - 1, pc] = 0.4 * c, 0.03 * c / dt, -0.01 * c / dt, 0.0
        out.append({"old": old.astype(np.float32), "source": s.astype(np.float32), "sink": k.astype(np.float32),
                    "transport": t.astype(np.float32), "area_mode": area, "masked": masked})
    return out


def add_tiny(variables, dt, seed):
    """candidates, in sample 0, for a mass of variable 0 that is non-zero in fp64 and rounds to 0.0f (the timestep must make
    dt * x inexact); the other variables hold ice there, which stays only if the fp64 predicate is the one handed on"""
    rng = np.random.default_rng(seed)
    px = np.arange(4, 12)
    a, b = rng.uniform(0.5, 1.5, px.size) * 1e-36, rng.uniform(0.5, 1.5, px.size) * 1e-36
    a, b = a.astype(np.float32), b.astype(np.float32)
    X = variables[0]
    X["old"][0, px], X["source"][0, px], X["sink"][0, px], X["transport"][0, px] = 0.0, a + b, -a, -b
    for v, Y in enumerate(variables[1:], 1):
        c = 1.0 if Y["area_mode"] else SCALES[v]
        Y["old"][0, px], Y["source"][0, px], Y["sink"][0, px], Y["transport"][0, px] = 0.4 * c, 0.03 * c / dt, -0.01 * c / dt, 0.0
    return px
