// Host-side plan of an ace_disco_forward launch (csrc/disco.hip): per output row the band of input rows and the window of input
// columns a workgroup stages in LDS, per support point its offset into that stage, and the list of work units
// (output row, run of output columns, run of groups), heaviest first.  Plain C++: tests/emul/disco_units_emul.cpp compiles it for
// the CPU and checks that every output is produced by exactly one unit.
//
//   stage   row ho needs the input rows hi0 .. hi0 + nrows - 1 and, seen from output column 0, the columns wlo .. wlo + span - 1
//           (cyclic; span == W and wlo == 0 where the disk wraps every longitude).  A unit whose pixels start at wo0 stages, per
//           channel, stage[r][j] = x[hi0 + r][(wo0 + wlo + j) mod W] for j < ncol = span + ACE_DISCO_RUN - 1, so that point e at
//           pixel p of the unit is stage[off_e + p] with off_e = (hi_e - hi0) * ncol + ((wi_e - wlo) mod W): no modulo in the loop.
//           The channel stride cs >= nrows * ncol is padded to 16 mod 32 floats: two channels of a 32-lane group then sit on
//           disjoint LDS banks.
//   units   cost = support points x pixels x channels.  A row starts with as many groups per unit as the z budget allows and
//           ACE_DISCO_RUN pixels; while a unit costs more than the launch's target (total cost / ACE_DISCO_TARGET_UNITS, at least
//           ACE_DISCO_MIN_UNIT_COST) the groups per unit are halved, then the pixel run, down to ACE_DISCO_MIN_RUN.  The arithmetic of an output never
//           depends on the split: a unit only decides which outputs a workgroup computes.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ace_sfno.h"

namespace ace_disco {

struct Row {
    int hi0, nrows, wlo, ncol, cs, p0, npts;
};
struct Unit {
    int ho, wo0, npix, g0, ng, cc, pad0, pad1;      // cc: channels staged per pass
};
struct Plan {
    int H = 0, W = 0, K = 0, in_chans = 0, out_chans = 0, groups = 0, gs = 0, opg = 0, J = 0, Jp = 0;
    std::vector<Row> rows;
    std::vector<int> off;                            // per support point
    std::vector<Unit> units;
    std::vector<long> cost;                          // per unit, non-increasing
    long lds_floats = 0;                             // the largest unit's stage + z
};

inline long unit_cost(const Plan& p, const Unit& u) { return (long)p.rows[u.ho].npts * u.npix * ((long)u.ng * p.gs); }
inline long stage_floats(const Plan& p, const Unit& u) { return (long)u.cc * p.rows[u.ho].cs; }
inline long z_floats(const Plan& p, const Unit& u) { return (long)u.ng * p.Jp * ACE_DISCO_RUN; }

// "" on success, the reason of the refusal otherwise.  row_off [H + 1], hi / wi [row_off[H]] in ascending (hi, wi) per row.
inline std::string make_plan(int H, int W, int K, int in_chans, int out_chans, int groups, const long* row_off, const int* hi,
                             const int* wi, Plan& p) {
    if (H < 1 || W < 1) return "need H >= 1 and W >= 1";
    if (K < 1 || K > ACE_DISCO_MAX_K) return "need 1 <= K <= ACE_DISCO_MAX_K (" + std::to_string(ACE_DISCO_MAX_K) + ")";
    if (in_chans < 1 || out_chans < 1 || groups < 1 || in_chans % groups || out_chans % groups)
        return "need in_chans >= 1, out_chans >= 1 and groups >= 1 dividing both";
    const int gs = in_chans / groups;
    if ((long)gs * K > ACE_DISCO_MAX_PRODUCTS)
        return "groupsize * K = " + std::to_string((long)gs * K) + " exceeds ACE_DISCO_MAX_PRODUCTS (" +
               std::to_string(ACE_DISCO_MAX_PRODUCTS) + ")";
    p = Plan();
    p.H = H; p.W = W; p.K = K; p.in_chans = in_chans; p.out_chans = out_chans; p.groups = groups;
    p.gs = gs; p.opg = out_chans / groups; p.J = gs * K; p.Jp = (p.J + 3) / 4 * 4;
    p.rows.resize(H);
    p.off.resize((size_t)row_off[H]);
    long total = 0;
    for (int ho = 0; ho < H; ++ho) {
        Row& r = p.rows[ho];
        r.p0 = (int)row_off[ho];
        r.npts = (int)(row_off[ho + 1] - row_off[ho]);
        if (r.npts < 1) return "output row " + std::to_string(ho) + " has no support point";
        int lo = H, top = -1;
        std::vector<char> used(W, 0);
        for (int e = r.p0; e < r.p0 + r.npts; ++e) {
            if (hi[e] < 0 || hi[e] >= H || wi[e] < 0 || wi[e] >= W) return "a support point lies outside the grid";
            if (e > r.p0 && (hi[e] < hi[e - 1] || (hi[e] == hi[e - 1] && wi[e] <= wi[e - 1])))
                return "the support points of output row " + std::to_string(ho) + " are not in ascending (hi, wi) order";
            lo = std::min(lo, hi[e]); top = std::max(top, hi[e]);
            used[wi[e]] = 1;
        }
        r.hi0 = lo; r.nrows = top - lo + 1;
        // the longest cyclic run of unused columns ends just before wlo
        int best = 0;
        r.wlo = 0;
        for (int s = 0; s < W; ++s) {
            if (used[s] || !used[(s + W - 1) % W]) continue;   // not the first column of a cyclic run
            int len = 0;
            while (!used[(s + len) % W]) ++len;
            if (len > best) { best = len; r.wlo = (s + len) % W; }
        }
        const int span = W - best;
        r.ncol = span + ACE_DISCO_RUN - 1;
        long cs = (long)r.nrows * r.ncol;
        cs += ((16 - cs % 32) + 32) % 32;
        if (cs * 4 > ACE_DISCO_STAGE_BYTES)
            return "the band of output row " + std::to_string(ho) + " (" + std::to_string(r.nrows) + " rows x " + std::to_string(r.ncol) +
                   " columns) exceeds ACE_DISCO_STAGE_BYTES (" + std::to_string(ACE_DISCO_STAGE_BYTES) + ") for one channel";
        r.cs = (int)cs;
        for (int e = r.p0; e < r.p0 + r.npts; ++e) p.off[e] = (hi[e] - r.hi0) * r.ncol + ((wi[e] - r.wlo + W) % W);
        total += (long)r.npts * W * in_chans;
    }
    const long target = std::max<long>(ACE_DISCO_MIN_UNIT_COST, total / ACE_DISCO_TARGET_UNITS);
    const int ng_max = std::max(1, std::min(groups, (int)(ACE_DISCO_Z_BYTES / 4 / ACE_DISCO_RUN / p.Jp)));
    for (int ho = 0; ho < H; ++ho) {
        const Row& r = p.rows[ho];
        int ng = ng_max, run = std::min(W, (int)ACE_DISCO_RUN);
        while (ng > 1 && (long)r.npts * run * ng * gs > target) ng = (ng + 1) / 2;
        while (run > ACE_DISCO_MIN_RUN && (long)r.npts * run * ng * gs > target) run = (run + 1) / 2;
        for (int wo0 = 0; wo0 < W; wo0 += run)
            for (int g0 = 0; g0 < groups; g0 += ng) {
                Unit u{};
                u.ho = ho; u.wo0 = wo0; u.npix = std::min(run, W - wo0); u.g0 = g0; u.ng = std::min(ng, groups - g0);
                u.cc = (int)std::max<long>(1, std::min<long>((long)u.ng * gs, ACE_DISCO_STAGE_BYTES / 4 / r.cs));
                p.units.push_back(u);
            }
    }
    std::stable_sort(p.units.begin(), p.units.end(), [&](const Unit& a, const Unit& b) { return unit_cost(p, a) > unit_cost(p, b); });
    p.cost.reserve(p.units.size());
    for (const Unit& u : p.units) {
        p.cost.push_back(unit_cost(p, u));
        p.lds_floats = std::max(p.lds_floats, stage_floats(p, u) + z_floats(p, u));
    }
    return "";
}

}  // namespace ace_disco
