// CPU check of the workgroup -> unit mappings and of the lane-offset bound of the two-level longitude FFT kernels
// (ace_amd/csrc/fft_units.h, the very code fft.hip runs).  For every gx in 1 .. 40 channel blocks, every H in 1 .. 70 transform rows
// and every nride in {0, 1, gx - 1, gx, gx + 1, 8, 8 gx, 300}, over the grid (gx, H + ceil(nride / gx)):
//   * the non-rider workgroups hit every (cblk < gx, lat < H) exactly once;
//   * every rider id below nride is produced exactly once, ids from nride on are idle;
//   * when the XCD branch is taken, XCD x (workgroup ids = x mod 8, in dispatch order) owns a contiguous unit range;
//   * the riders are the first units of every XCD's range.
// fft_unit (the inverse kernel's form, no riders) with and without XCD over the same (gx, H).
// fft_lane_offsets_fit at its boundaries: a launch it lets through never forms a lane offset whose access ends past 2^31 - 1.
#include <cstdio>
#include <vector>

#include "../../ace_amd/csrc/fft_units.h"

using namespace ace;

#define FAIL(...) do { printf("FAIL " __VA_ARGS__); printf("\n"); return 1; } while (0)

template <bool XCD>
static int check_ride(int gx, int H, int nride, long& xcd_taken) {
    const int gy = H + (nride > 0 ? (nride + gx - 1) / gx : 0), total = gx * gy;
    const int nextra = total - gx * H;
    std::vector<int> hit((size_t)gx * H, 0), rider((size_t)nextra + 1, 0);
    std::vector<int> first_u(8, -1), last_u(8, -1), count_u(8, 0);
    const bool xcd_branch = XCD && total % 8 == 0 && nextra % 8 == 0;
    if (xcd_branch) ++xcd_taken;
    std::vector<char> seen_transform(8, 0);
    for (int id = 0; id < total; ++id) {
        int cblk = -1, lat = -1, rid = -1;
        const bool is_rider = fft_unit_ride<XCD>(id, gx, gy, nride, cblk, lat, rid);
        const int x = id & 7;
        if (is_rider) {
            if (rid < 0 || rid >= nextra) FAIL("gx %d H %d nride %d id %d: rider index %d outside [0, %d)", gx, H, nride, id, rid, nextra);
            rider[rid] += 1;
            // riders first: in an XCD's dispatch order (ids x, x + 8, ...) no transform unit comes before a rider; in launch order
            // no transform unit has a smaller id
            if (xcd_branch ? seen_transform[x] : seen_transform[0]) FAIL("gx %d H %d nride %d id %d: a rider behind a transform unit", gx, H, nride, id);
            continue;
        }
        seen_transform[xcd_branch ? x : 0] = 1;
        if (cblk < 0 || cblk >= gx || lat < 0 || lat >= H) FAIL("gx %d H %d nride %d id %d: unit (%d, %d) out of range", gx, H, nride, id, cblk, lat);
        hit[(size_t)lat * gx + cblk] += 1;
        if (xcd_branch) {   // contiguous: the units of XCD x, in dispatch order, are consecutive
            const int u = lat * gx + cblk;
            if (first_u[x] < 0) first_u[x] = u;
            else if (u != last_u[x] + 1) FAIL("gx %d H %d nride %d: XCD %d jumps from unit %d to %d", gx, H, nride, x, last_u[x], u);
            last_u[x] = u;
            count_u[x] += 1;
        }
    }
    for (size_t q = 0; q < hit.size(); ++q)
        if (hit[q] != 1) FAIL("gx %d H %d nride %d XCD %d: unit %zu hit %d times", gx, H, nride, (int)XCD, q, hit[q]);
    for (int r = 0; r < nextra; ++r)
        if (rider[r] != 1) FAIL("gx %d H %d nride %d XCD %d: rider slot %d produced %d times", gx, H, nride, (int)XCD, r, rider[r]);
    // (slots nride .. nextra - 1 are the idle ones: the kernel returns on rid >= nride; every slot below nride exists because
    // nextra >= nride)
    if (nextra < nride) FAIL("gx %d H %d nride %d: %d rider slots", gx, H, nride, nextra);
    if (xcd_branch)
        for (int x = 0; x < 8; ++x) {
            if (count_u[x] != gx * H / 8) FAIL("gx %d H %d nride %d: XCD %d owns %d units", gx, H, nride, x, count_u[x]);
            if (first_u[x] != x * (gx * H / 8)) FAIL("gx %d H %d nride %d: XCD %d starts at unit %d", gx, H, nride, x, first_u[x]);
        }
    return 0;
}

template <bool XCD>
static int check_plain(int gx, int H, long& xcd_taken) {
    const int total = gx * H;
    std::vector<int> hit((size_t)total, 0), last_u(8, -1);
    const bool xcd_branch = XCD && total % 8 == 0;
    if (xcd_branch) ++xcd_taken;
    for (int id = 0; id < total; ++id) {
        int cblk = -1, lat = -1;
        fft_unit<XCD>(id, gx, H, cblk, lat);
        if (cblk < 0 || cblk >= gx || lat < 0 || lat >= H) FAIL("fft_unit gx %d H %d id %d: (%d, %d) out of range", gx, H, id, cblk, lat);
        const int u = lat * gx + cblk;
        hit[u] += 1;
        if (xcd_branch) {
            const int x = id & 7;
            if (last_u[x] < 0 ? u != x * (total / 8) : u != last_u[x] + 1) FAIL("fft_unit gx %d H %d: XCD %d not contiguous at unit %d", gx, H, x, u);
            last_u[x] = u;
        } else if (u != id) {
            FAIL("fft_unit gx %d H %d: launch order expected, id %d -> unit %d", gx, H, id, u);
        }
    }
    for (int q = 0; q < total; ++q)
        if (hit[q] != 1) FAIL("fft_unit gx %d H %d XCD %d: unit %d hit %d times", gx, H, (int)XCD, q, hit[q]);
    return 0;
}

// the largest byte a lane offset of the kernels reaches, +1, for a launch of this shape (fft.hip): spectral side (N1 <= 40 planes
// of H Bt 2 C floats plus an imaginary row and a channel row), grid side (R <= 32 rows of H W floats), planes input (k-group
// kg <= C / 8 - 1 of H W 16-byte entries)
static double reach(long H, long W, long Bt, long C, bool planes) {
    const double ms = (double)H * Bt * 2 * C;
    double r = (40.0 * ms + 31.0) * 4.0 + C * 4.0 + 4.0;
    const double grid = (31.0 * H * W + W) * 4.0;
    r = grid > r ? grid : r;
    if (planes) {
        const double pl = ((double)(C / 8 - 1) * H * W + W) * 16.0;
        r = pl > r ? pl : r;
    }
    return r;
}

int main() {
    long combos = 0, xcd_taken = 0;
    for (int gx = 1; gx <= 40; ++gx)
        for (int H = 1; H <= 70; ++H) {
            if (check_plain<true>(gx, H, xcd_taken) || check_plain<false>(gx, H, xcd_taken)) return 1;
            const int nrides[8] = {0, 1, gx - 1, gx, gx + 1, 8, 8 * gx, 300};
            for (int nride : nrides) {
                if (nride < 0) continue;
                if (check_ride<true>(gx, H, nride, xcd_taken) || check_ride<false>(gx, H, nride, xcd_taken)) return 1;
                ++combos;
            }
        }
    if (xcd_taken < 1000) FAIL("the XCD branch was taken %ld times only", xcd_taken);

    // ---- the offset bound.  The shapes the library runs fit; the planes input of 1040 channels on the 0.25-degree grid does not
    struct Shape { int H, W, Bt, C; bool planes, fits; };
    const Shape shapes[] = {
        {180, 360, 8, 384, false, true}, {180, 360, 8, 384, true, true}, {721, 1440, 1, 384, true, true},
        {721, 1440, 2, 1024, true, true},                  // 2 C H W = 2.126e9 bytes from the sample's base: the last k-group is in reach
        {721, 1440, 1, 1040, true, false},                 // 2.160e9: it is not
        {721, 1440, 1, 1040, false, true},                 // the same shape from fp32 input: grid rows and spectral planes only
        {721, 1440, 64, 1024, false, false},               // 42 spectral planes of H Bt 2 C floats
    };
    for (const Shape& q : shapes)
        if (fft_lane_offsets_fit(q.H, q.W, q.Bt, q.C, q.planes) != q.fits)
            FAIL("fft_lane_offsets_fit(%d, %d, %d, %d, %d) is not %d", q.H, q.W, q.Bt, q.C, (int)q.planes, (int)q.fits);
    // at the boundary of the planes term, H W = 2^20: 2 C H W crosses 2^31 between C = 1016 and C = 1024
    if (!fft_lane_offsets_fit(1024, 1024, 1, 1016, true)) FAIL("planes, C = 1016 at H W = 2^20 fits");
    if (fft_lane_offsets_fit(1024, 1024, 1, 1024, true)) FAIL("planes, C = 1024 at H W = 2^20 does not fit");
    if (!fft_lane_offsets_fit(1024, 1024, 1, 1024, false)) FAIL("fp32 input, C = 1024 at H W = 2^20 fits");
    // soundness over a sweep: whatever the predicate lets through stays below the descriptor's 2^31 - 1 bytes
    long let_through = 0, held_back = 0;
    for (long H : {1L, 8L, 180L, 721L, 1024L, 4096L, 65535L})
        for (long W : {16L, 360L, 1440L})
            for (long Bt : {1L, 3L, 64L, 4096L})
                for (long C : {8L, 40L, 384L, 1016L, 1024L, 4096L, 65536L})
                    for (int planes = 0; planes < 2; ++planes) {
                        const bool fits = fft_lane_offsets_fit((int)H, (int)W, (int)Bt, (int)C, planes != 0);
                        if (fits && reach(H, W, Bt, C, planes != 0) > 2147483647.0)
                            FAIL("H %ld W %ld Bt %ld C %ld planes %d passes the bound and reaches byte %.0f", H, W, Bt, C, planes, reach(H, W, Bt, C, planes != 0));
                        (fits ? let_through : held_back) += 1;
                    }
    if (let_through < 100 || held_back < 100) FAIL("the sweep of the bound is one-sided: %ld through, %ld held back", let_through, held_back);
    printf("fft_units: %ld (gx, H, nride) combinations ok, XCD branch taken %ld times; offset bound: %ld shapes through, %ld held back\n", combos,
           xcd_taken, let_through, held_back);
    return 0;
}
