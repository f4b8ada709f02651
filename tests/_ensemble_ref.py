"""The header contract of ``ace_diag_ensemble_step`` (include/ace_sfno.h) in plain numpy fp64, written from the header: per pixel
the member sums in ascending order (pairs: e outer, f inner), every product rounded before it is added, the four maps and the
``seen`` flags.  tests/test_ensemble_ref_cpu.py holds it to the reference's three metric classes; the GPU tests hold the kernel to
it."""
import numpy as np

ALPHA = 0.95
PAIR_WEIGHT = 0.5 * (1.0 - (1.0 - ALPHA) / 2.0)


def ensemble_step(gen, target, rows, maps, seen, slot, t, n_ic, n_members, pair_weight=PAIR_WEIGHT):
    """One call, in place on ``maps`` (nslots, 4, nrows, hw) fp64 and ``seen`` (nslots, nrows) int32.  gen / target: lists of
    (n_ic * n_members, T, hw) fp32 arrays, a target entry may be None."""
    nrows, E = maps.shape[2], n_members
    for j, x in enumerate(gen):
        r, y = rows[j], target[j]
        if x is None or y is None or r < 0 or r >= nrows:
            continue
        g = np.asarray(x, dtype=np.float32)[:, t].astype(np.float64).reshape(n_ic, E, -1)
        y = np.asarray(y, dtype=np.float32)[:, t].astype(np.float64).reshape(n_ic, E, -1)
        hw = g.shape[-1]
        crps, mse, var = (np.zeros(hw) for _ in range(3))
        with np.errstate(all="ignore"):
            for i in range(n_ic):
                m, a, s, q, v = (np.zeros(hw) for _ in range(5))
                for e in range(E):
                    m = m + g[i, e]
                m = m / E
                for e in range(E):
                    a = a + np.abs(g[i, e] - y[i, e])
                    dq, dv = m - y[i, e], g[i, e] - m
                    q = q + dq * dq
                    v = v + dv * dv
                for e in range(E):
                    for f in range(e + 1, E):
                        s = s + np.abs(g[i, e] - g[i, f])
                crps = crps + (a / E - pair_weight * (s / (E * (E - 1) // 2)))
                mse = mse + q / E
                var = var + v / (E - 1)
            crps, mse, var = crps / n_ic, mse / n_ic, var / n_ic
            maps[slot, 0, r] += crps
            maps[slot, 1, r] += np.sqrt(mse)
            maps[slot, 2, r] += mse - var / E
            maps[slot, 3, r] += var
        if not np.isnan(y).all():
            seen[slot, r] = 1
