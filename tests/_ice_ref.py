"""numpy statement of the sea-ice budget corrector's contract (include/ace_sfno.h, "Sea-ice budget corrector"): the fp64
arithmetic per pixel, the seven flag bits per variable - each stage's mask under every hypothesis about the earlier stages, ORed
over the tensor - the path they resolve to, and the fp64 "ice mass == 0" predicate of variable 0 that later variables read.

    outs, flags, info = ice_budget_ref(variables, dt)

``variables``: a list, in processing order, of dicts with float32 arrays ``old``, ``source``, ``sink``, ``transport`` (one shape)
and booleans ``area_mode``, ``masked``.  ``outs[v]``: float32 ``source``, ``sink``, ``transport``, ``mass``.  ``flags[v]``: the flag
word (bit 0 = F1, bit 1 + a1 = F2[a1], bit 3 + 2 a1 + a2 = F3[a1][a2]).  ``info[v]``: ``path`` (a1, a2, a3), ``mass64`` and, per
stage that ran, how many pixels were in its mask, had all three terms zero there, and hit k_overshoot / s_overshoot."""
import numpy as np


def _new(o, x):
    return o + ((x[0] + x[1]) + x[2])


def _rebalance(x, m, mass, sign, hits=None):
    s, k, t = x
    nz_s, nz_k, nz_t = np.abs(s) > 0, np.abs(k) > 0, np.abs(t) > 0
    n = (nz_s.astype(np.float64) + nz_k.astype(np.float64)) + nz_t.astype(np.float64)
    share = np.where(m & (n > 0), mass / np.maximum(n, 1.0), 0.0)
    r_s = np.where(m & nz_s, share, 0.0)
    r_k = np.where(m & nz_k, share, 0.0)
    r_t = np.where(m & nz_t, share, 0.0)
    r_t = np.where(m & (n == 0), mass, r_t)
    tmp = k + sign * r_k
    ko = np.where(tmp > 0, tmp, 0.0)
    r_k = r_k - ko
    r_t = r_t + ko
    tmp = s + sign * r_s
    so = np.where(tmp < 0, tmp, 0.0)
    r_s = r_s - sign * so
    r_t = r_t + sign * so
    if hits is not None:
        hits.update(mask=int(m.sum()), all_zero=int((m & (n == 0)).sum()), k_overshoot=int((ko != 0).sum()),
                    s_overshoot=int((so != 0).sum()))
    return s + sign * r_s, k + sign * r_k, t + sign * r_t


def _stage(i, o, x, ice_zero, hits=None):
    nm = _new(o, x)
    if i == 1:
        m = nm < 0
        return m, _rebalance(x, m, np.where(m, -nm, 0.0), 1.0, hits)
    if i == 2:
        m = nm > 1
        return m, _rebalance(x, m, np.where(m, nm - 1.0, 0.0), -1.0, hits)
    m = ice_zero & (nm > 0)
    return m, _rebalance(x, m, np.where(m, nm, 0.0), -1.0, hits)


def ice_budget_ref(variables, dt):
    dt = float(dt)
    outs, flags, info = [], [], []
    ice_zero = None
    with np.errstate(all="ignore"):
        for v, X in enumerate(variables):
            area, masked = bool(X["area_mode"]), bool(X["masked"])
            assert not (masked and v == 0)
            o = np.asarray(X["old"], np.float32).astype(np.float64)
            x0 = tuple(np.asarray(X[n], np.float32).astype(np.float64) * dt for n in ("source", "sink", "transport"))
            z = ice_zero if masked else np.zeros(o.shape, bool)
            # ---- the flags pass: every stage mask under every hypothesis
            m1, x1 = _stage(1, o, x0, z)
            word = int(m1.any())
            for a1, xa in enumerate((x0, x1)):
                m2, x2 = _stage(2, o, xa, z)
                if area:
                    word |= int(m2.any()) << (1 + a1)
                if masked:
                    for a2, xb in enumerate((xa, x2) if area else (xa,)):
                        m3, _ = _stage(3, o, xb, z)
                        word |= int(m3.any()) << (3 + 2 * a1 + a2)
            # ---- the apply pass: one path
            a1 = word & 1
            a2 = (word >> (1 + a1)) & 1 if area else 0
            a3 = (word >> (3 + 2 * a1 + a2)) & 1 if masked else 0
            x, stages = x0, {}
            for i, on in ((1, a1), (2, a2), (3, a3)):
                if on:
                    stages[i] = {}
                    _, x = _stage(i, o, x, z, stages[i])
            b = tuple(c / dt for c in x)
            mass = o + dt * ((b[0] + b[1]) + b[2])
            if v == 0:
                ice_zero = mass == 0
            outs.append({"source": b[0].astype(np.float32), "sink": b[1].astype(np.float32), "transport": b[2].astype(np.float32),
                         "mass": mass.astype(np.float32)})
            flags.append(word)
            info.append({"path": (a1, a2, a3), "mass64": mass, "stages": stages})
    return outs, flags, info


def variables_from_case(plan, inp, gen):
    """``IceBudgetCorrectionConfig.plan()`` rows and the step's input / output (name -> float32 array) as ``variables``."""
    return [{"old": inp[name], "source": gen[terms[0]], "sink": gen[terms[1]], "transport": gen[terms[2]], "area_mode": area,
             "masked": masked} for name, terms, area, masked in plan]
