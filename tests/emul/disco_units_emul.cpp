// CPU check of the plan of an ace_disco_forward launch (ace_amd/csrc/disco_units.h, the very code disco.hip's create runs).
// usage: disco_units_emul TABLE in out groups [in out groups ...]
// TABLE is text: "H W K P", then H + 1 row offsets, then P input rows, then P input columns (ace_amd.disco.disco_table).
// Per channel case: every (ho, wo, o) is produced by exactly one unit; costs are non-increasing along the list; every LDS address
// the kernel forms lies inside the unit's stage and holds the input element the statement names; stage and z fit their budgets.
// With "refuse" as the first argument: the limits are refused with their names.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

#include "../../ace_amd/csrc/disco_units.h"

using namespace ace_disco;

static int fail(const std::string& m) {
    std::printf("FAILED: %s\n", m.c_str());
    return 1;
}

static int refusals() {
    const long off1[3] = {0, 1, 2};
    const int hi[2] = {0, 1}, wi[2] = {0, 0};
    Plan p;
    auto has = [](const std::string& s, const char* w) { return s.find(w) != std::string::npos; };
    if (!has(make_plan(2, 4, 26, 1, 1, 1, off1, hi, wi, p), "ACE_DISCO_MAX_K")) return fail("K over the limit accepted");
    if (!has(make_plan(2, 4, 9, 60, 1, 1, off1, hi, wi, p), "ACE_DISCO_MAX_PRODUCTS")) return fail("products over the limit accepted");
    if (!has(make_plan(2, 4, 9, 6, 4, 4, off1, hi, wi, p), "groups")) return fail("groups not dividing accepted");
    if (!has(make_plan(0, 4, 9, 1, 1, 1, off1, hi, wi, p), "H >= 1")) return fail("H = 0 accepted");
    const long off0[3] = {0, 0, 2};
    if (!has(make_plan(2, 4, 9, 1, 1, 1, off0, hi, wi, p), "no support point")) return fail("an empty row accepted");
    const int hib[2] = {0, 2};
    if (!has(make_plan(2, 4, 9, 1, 1, 1, off1, hib, wi, p), "outside the grid")) return fail("a point outside the grid accepted");
    const long off2[3] = {0, 2, 2};
    const int hio[2] = {1, 0};
    if (!has(make_plan(2, 4, 9, 1, 1, 1, off2, hio, wi, p), "ascending")) return fail("points out of order accepted");
    {   // a band too wide for the stage: 5 rows x (W + 15) columns over 64 KB
        const int W = 4000, H = 5;
        std::vector<long> off(H + 1);
        std::vector<int> h, w;
        for (int r = 0; r < H; ++r) {
            off[r] = (long)h.size();
            for (int i = 0; i < H; ++i)
                for (int c = 0; c < W; ++c) { h.push_back(i); w.push_back(c); }
        }
        off[H] = (long)h.size();
        if (!has(make_plan(H, W, 9, 1, 1, 1, off.data(), h.data(), w.data(), p), "ACE_DISCO_STAGE_BYTES")) return fail("a band over the stage accepted");
    }
    std::printf("refusals ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "refuse")) return refusals();
    if (argc < 5 || (argc - 2) % 3) return fail("usage");
    std::ifstream f(argv[1]);
    int H, W, K;
    long P;
    if (!(f >> H >> W >> K >> P)) return fail("table header");
    std::vector<long> off(H + 1);
    std::vector<int> hi(P), wi(P);
    for (auto& v : off) f >> v;
    for (auto& v : hi) f >> v;
    for (auto& v : wi) f >> v;
    if (!f) return fail("table body");
    for (int a = 2; a < argc; a += 3) {
        const int cin = std::atoi(argv[a]), cout = std::atoi(argv[a + 1]), groups = std::atoi(argv[a + 2]);
        Plan p;
        const std::string why = make_plan(H, W, K, cin, cout, groups, off.data(), hi.data(), wi.data(), p);
        if (!why.empty()) return fail(why);
        std::vector<int> seen((size_t)H * W * cout, 0);
        long total = 0, heaviest = 0;
        for (size_t i = 0; i < p.units.size(); ++i) {
            const Unit& u = p.units[i];
            const Row& r = p.rows[u.ho];
            if (p.cost[i] != unit_cost(p, u)) return fail("cost list");
            if (i && p.cost[i] > p.cost[i - 1]) return fail("costs increase along the list");
            total += p.cost[i];
            heaviest = std::max(heaviest, p.cost[i]);
            if (u.npix < 1 || u.npix > ACE_DISCO_RUN || u.wo0 < 0 || u.wo0 + u.npix > W) return fail("pixel run");
            if (u.ng < 1 || u.g0 < 0 || u.g0 + u.ng > groups) return fail("group run");
            if (u.cc < 1 || u.cc > u.ng * p.gs) return fail("channels per pass");
            if (stage_floats(p, u) * 4 > ACE_DISCO_STAGE_BYTES) return fail("stage over its budget");
            if (z_floats(p, u) * 4 > ACE_DISCO_Z_BYTES) return fail("z over its budget");
            if ((stage_floats(p, u) + z_floats(p, u)) > p.lds_floats) return fail("lds_floats is not the maximum");
            if (stage_floats(p, u) % 4) return fail("z is not 16-byte aligned");
            if (r.cs % 32 != 16 || r.cs < r.nrows * r.ncol) return fail("channel stride");
            if (r.hi0 < 0 || r.hi0 + r.nrows > H) return fail("band rows");
            const int wstart = (u.wo0 + r.wlo) % W;
            for (int e = r.p0; e < r.p0 + r.npts; ++e)
                for (int px = 0; px < ACE_DISCO_RUN; ++px) {               // every lane reads, also past npix
                    const int a2 = p.off[e] + px;
                    if (a2 < 0 || a2 >= r.nrows * r.ncol) return fail("a stage address outside the channel's band");
                    const int rr = a2 / r.ncol, j = a2 - rr * r.ncol;
                    if (r.hi0 + rr != hi[e]) return fail("a stage address in the wrong row");
                    if ((wstart + j) % W != (wi[e] + u.wo0 + px) % W) return fail("a stage address in the wrong column");
                }
            for (int g = u.g0; g < u.g0 + u.ng; ++g)
                for (int o = g * p.opg; o < (g + 1) * p.opg; ++o)
                    for (int wo = u.wo0; wo < u.wo0 + u.npix; ++wo) ++seen[((size_t)u.ho * W + wo) * cout + o];
        }
        for (int v : seen)
            if (v != 1) return fail("an output is produced " + std::to_string(v) + " times");
        std::printf("%d x %d K %d, %d -> %d in %d groups: %zu units ok, heaviest %ld of %ld (%.4f%%), lds %ld bytes\n", H, W, K, cin, cout,
                    groups, p.units.size(), heaviest, total, 100.0 * heaviest / total, p.lds_floats * 4);
    }
    return 0;
}
