// CPU emulation of the polar cut of the folded Legendre kernels (ace_amd/csrc/strip_fold.hip) and of the longitude FFT kernels'
// per-latitude cutoff (ace_amd/csrc/fft.hip), on the REAL tables (ace_amd/csrc/tables.cpp), packer and cut derivation
// (ace_amd/csrc/strip_pack.h: pack_legendre_fold, derive_polar_cut, fold_geom_cut).
//
// Table properties, per grid: the cut is prefix-shaped and monotone, mcut agrees with r0, every packed element inside the cut is
// zero (hi and lo) in both packs, and row r0(m) holds a live element (the cut is maximal).  At 180 x 360 legendre-gauss the dead
// share of X lies in [0.23, 0.26].
//
// Data movement: the kernel's index formulas with the cut (descriptor window based at r0 / ending r0 rows early, the table packed
// from k16-step r0 / 16 on, pairs below r0 / 32 not run, store masks [r0, Hh) / [Hh, H - r0), FFT stores and loads compared with
// min(Mm, mcut[lat])) are restated as in strip_fold_emul.cpp, arithmetic in double in the kernel's order.  With X's dead entries set
// to NaN the forward and the inverse must equal the run without the cut BIT FOR BIT, every live element written exactly once and no
// dead element written.
//
// Big form (legendre_fold_big_kernel: more than 96 folded latitudes or degrees per parity at m = 0, i.e. nlat or lmax > 192): units
// of 12, 18 or 24 k16-steps, the inverse falling through to 2 / 4 / 6 as its contraction shrinks with m; j0 = 0 (the forward table
// keeps every k16-step: no kdrop), whole 128-column groups only; the cut is the descriptor window, the store masks and the tile skip.
// Grids 194 x 48, 360 x 720, 385 x 720 legendre-gauss and 361 x 720 equiangular at N = 128, dead shares of the three 720-wide ones
// within 0.01 of 0.2850, 0.2586 and 0.2860.  Test infrastructure only (built and run by tests/test_polar_cut_cpu.py).
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("O3")   // the test builds with -O2; the contraction loops of the 720-wide grids want the vectoriser (twice as fast)
#endif
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../ace_amd/csrc/strip_pack.h"
#include "../../ace_amd/csrc/tables.h"

using namespace ace;

static int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
struct RowMap { int rbase, rstep, vlo, vhi; };

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); ++g_fail; } } while (0)

static float pow2_scale_for(const std::vector<float>& v) {   // capi.hip: max|v| scale in [2^9, 2^10)
    float mx = 0.f;
    for (float x : v) mx = std::max(mx, std::fabs(x));
    int e = 0;
    if (mx > 0.f && std::isfinite(mx)) { (void)std::frexp(mx, &e); e = 10 - e; }
    return std::ldexp(1.0f, e);
}

// a raw buffer load: base element index (may lie anywhere in `mem`), num_records in bytes, 32-bit unsigned byte offset
static double buf_load(const std::vector<float>& mem, size_t base, unsigned num_records, unsigned off, bool* fault) {
    if ((unsigned long long)off + 4ull > (unsigned long long)num_records) return 0.0;
    const size_t at = base + off / 4;
    if (at >= mem.size()) { *fault = true; return 0.0; }
    return mem[at];
}

struct Plan {
    int H, L, M;
    ShtTables t;
    StripPack fwd, fwd_cut, inv;
    PolarCut cut;
    bool kdrop = false;
    std::vector<int> kskip;
};

// one folded Legendre launch.  r0: the cut (nullptr: none); kdrop: `sp` was packed with kskip = r0 / 16 (forward)
static void run_fold(int mode, const Plan& P, const StripPack& sp, const int* r0v, bool kdrop, int N, const std::vector<float>& B,
                     std::vector<double>& C, std::vector<int>& writes, bool* fault) {
    const int H = P.H, L = P.L, M = P.M;
    const int R = mode == 0 ? L : H, K = mode == 0 ? H : L;
    const long b_kstride = mode == 0 ? N : (long)M * N, b_moff = mode == 0 ? (long)H * N : N;
    const long c_rstride = mode == 0 ? (long)M * N : N, c_moff = mode == 0 ? N : (long)H * N;
    const int G = (N + 127) / 128;
    // launch_legendre_fold: the size at m = 0 picks the kernel.  The big form takes whole 128-column groups only (legendre_fold_eligible),
    // ignores kdrop (j0 = 0, gm = fold_geom) and has bodies for 12, 18, 24 k16-steps, the inverse also for 2, 4, 6
    const bool big = fold_geom(mode, 0, R, K).nkp2 > FOLD_NKP_SMALL;
    if (big && (N % 128 != 0 || kdrop)) { std::printf("big form: N %d is not whole column groups, or kdrop is set\n", N); *fault = true; return; }
    for (int m = 0; m < M; ++m) {
        const int r0 = r0v ? r0v[m] : 0;
        const int j0 = !big && mode == 0 && kdrop ? r0 >> 4 : 0;
        const FoldGeom gm = big ? fold_geom(mode, m, R, K) : fold_geom_cut(mode, m, R, K, j0);
        const bool small_body = gm.nkp2 == 2 || gm.nkp2 == 4 || gm.nkp2 == 6, big_body = gm.nkp2 == 12 || gm.nkp2 == 18 || gm.nkp2 == 24;
        const bool has_body = big ? (big_body || (mode == 1 && small_body)) : small_body;
        if (!has_body || gm.nkp2 < gm.nkp) { std::printf("bad nkp2 %d (mode %d m %d, %s form)\n", gm.nkp2, mode, m, big ? "big" : "small"); *fault = true; return; }
        const int NKP = gm.nkp2;
        const int tp0 = mode == 1 ? r0 >> 5 : 0;
        const int npairs = gm.npairs > tp0 ? gm.npairs - tp0 : 0;
        const int nunits = 2 * npairs;
        const size_t a_at = ((size_t)sp.tile_off[m] + (size_t)tp0 * 2 * NKP) * 1024;
        if (a_at + (size_t)nunits * NKP * 1024 > sp.frags.size()) { std::printf("table stream past the end (m %d)\n", m); *fault = true; return; }
        const uint16_t* Am = sp.frags.data() + a_at;
        std::vector<double> Ad((size_t)nunits * NKP * 1024);   // this wavenumber's fragments as doubles, once for every column strip
        for (size_t q = 0; q < Ad.size(); ++q) Ad[q] = (double)f16_bits_to_f32(Am[q]);
        for (int grp = 0; grp < G; ++grp)
            for (int wave = 0; wave < 4; ++wave) {
                const int n0 = grp * 128 + wave * 32;
                if (n0 >= N) continue;   // (such a wave runs on the GPU, with clamped columns and masked stores: nothing new to check)
                std::vector<double> bf((size_t)2 * NKP * 64 * 8);
                auto BF = [&](int par, int jj, int lane, int e) -> double& { return bf[(((size_t)par * NKP + jj) * 64 + lane) * 8 + e]; };
                const long ks = b_kstride;
                const unsigned rowb = (unsigned)(ks * 4);
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = lane & 31, g = lane >> 5;
                    const int n = n0 + i, nc = n < N ? n : N - 1;
                    if (mode == 0) {
                        const int nD = gm.Hh - r0, nM = H - gm.Hh - r0;
                        const size_t baseD = (size_t)m * b_moff + (size_t)r0 * ks, baseM = (size_t)m * b_moff + (size_t)gm.Hh * ks;
                        const unsigned nrD = (unsigned)((long)(nD > 0 ? nD : 0) * rowb), nrM = (unsigned)((long)(nM > 0 ? nM : 0) * rowb);
                        for (int e = 0; e < 8; ++e) {
                            const unsigned vd = (unsigned)(((long)(16 * j0 + 8 * g + e - r0) * ks + nc) * 4);
                            const unsigned vm = (unsigned)(((long)(H - 1 - gm.Hh - (16 * j0 + 8 * g + e)) * ks + nc) * 4);
                            for (int jj = 0; jj < NKP; ++jj) {
                                const unsigned so = (unsigned)((long)(16 * jj) * rowb);
                                const double a = buf_load(B, baseD, nrD, vd + so, fault);
                                const double b = buf_load(B, baseM, nrM, vm - so, fault);
                                BF(0, jj, lane, e) = a + b;
                                BF(1, jj, lane, e) = a - b;
                            }
                        }
                    } else {
                        const size_t baseE = (size_t)m * b_moff;
                        const long span = ((long)(K - 1) * ks + N) * 4;
                        const unsigned nrE = (unsigned)(span > 0 ? span : 0);
                        for (int e = 0; e < 8; ++e) {
                            const unsigned ve = (unsigned)(((long)(m + 2 * (8 * g + e)) * ks + nc) * 4);
                            for (int jj = 0; jj < NKP; ++jj) {
                                const unsigned so = (unsigned)((long)(32 * jj) * rowb);
                                BF(0, jj, lane, e) = buf_load(B, baseE, nrE, ve + so, fault);
                                BF(1, jj, lane, e) = buf_load(B, baseE, nrE, ve + so + rowb, fault);
                            }
                        }
                    }
                }
                // a unit's contraction in the kernel's k order, the table's lo and hi fragments as separate chains (the data operand
                // stays one double here): a dropped k-step or a dead row only removes terms that are zero times a finite value
                // (the 32 columns of a row advance together, each in that k order: bt is bf with the column index innermost)
                std::vector<double> bt((size_t)2 * NKP * 16 * 32);
                for (int par = 0; par < 2; ++par)
                    for (int jj = 0; jj < NKP; ++jj)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int e = 0; e < 8; ++e)
                                bt[((((size_t)par * NKP + jj) * 2 + (lane >> 5)) * 8 + e) * 32 + (lane & 31)] = BF(par, jj, lane, e);
                auto mfma_unit = [&](int u, double D[32][32]) {
                    const int par = u & 1;
                    const double* unit = Ad.data() + (size_t)u * NKP * 1024;
                    for (int ii = 0; ii < 32; ++ii) {
                        double a0[32], a2[32];
                        for (int jc = 0; jc < 32; ++jc) a0[jc] = a2[jc] = 0.0;
                        for (int jj = 0; jj < NKP; ++jj) {
                            const double* blk = unit + (size_t)jj * 1024;
                            for (int g = 0; g < 2; ++g)
                                for (int e = 0; e < 8; ++e) {
                                    const double hi = blk[(ii + 32 * g) * 8 + e], lo = blk[512 + (ii + 32 * g) * 8 + e];
                                    const double* b = &bt[((((size_t)par * NKP + jj) * 2 + g) * 8 + e) * 32];
                                    for (int jc = 0; jc < 32; ++jc) { a0[jc] += lo * b[jc]; a2[jc] += hi * b[jc]; }
                                }
                        }
                        for (int jc = 0; jc < 32; ++jc) D[ii][jc] = a0[jc] + a2[jc];
                    }
                };
                auto store = [&](const RowMap rm, double D[32][32], bool inner) {
                    const bool fulln = N % 128 == 0;
                    const bool nomask = inner && fulln && mode == 0, nocol = inner && fulln;
                    if (N % 4 != 0) {
                        for (int lane = 0; lane < 64; ++lane)
                            for (int r = 0; r < 16; ++r) {
                                const int i = lane & 31, g = lane >> 5, n = n0 + i;
                                const int row = rm.rbase + rm.rstep * acc_row(r, g);
                                if (!(row >= rm.vlo && row < rm.vhi && n < N)) continue;
                                if (row < 0 || row >= R) { *fault = true; continue; }
                                const size_t at = (size_t)m * c_moff + (size_t)row * c_rstride + n;
                                C[at] = D[acc_row(r, g)][i];
                                writes[at]++;
                            }
                        return;
                    }
                    for (int hf = 0; hf < 2; ++hf)
                        for (int ps = 0; ps < 2; ++ps)
                            for (int lane = 0; lane < 64; ++lane) {
                                const int rl = ps * 8 + (lane >> 3), c4 = (lane & 7) * 4, ncol = n0 + c4;
                                const int row = rm.rbase + rm.rstep * (16 * hf + rl);
                                const bool ok = nomask || (row >= rm.vlo && row < rm.vhi && (nocol || ncol < N));
                                if (!ok) continue;
                                for (int q = 0; q < 4; ++q) {
                                    if (row < 0 || row >= R || ncol + q >= N) { *fault = true; continue; }
                                    const size_t at = (size_t)m * c_moff + (size_t)row * c_rstride + ncol + q;
                                    C[at] = D[16 * hf + rl][c4 + q];
                                    writes[at]++;
                                }
                            }
                };
                auto fwd_map = [&](int tp, int par) { return RowMap{m + par + 64 * tp, 2, 0, R}; };
                auto north_map = [&](int tp) { return RowMap{32 * (tp0 + tp), 1, r0, gm.Hh}; };
                auto south_map = [&](int tp) { return RowMap{H - 1 - 32 * (tp0 + tp), -1, gm.Hh, H - r0}; };
                static double Dev[32][32], Dod[32][32], Pa[32][32], Pb[32][32];
                for (int tp = 0; tp < npairs; ++tp) {
                    const bool last = tp + 1 == npairs;
                    if (mode == 0) {
                        if (tp > 0) store(fwd_map(tp - 1, 1), Pb, true);
                        mfma_unit(2 * tp, Dev);
                        if (!last) store(fwd_map(tp, 0), Dev, true);
                        mfma_unit(2 * tp + 1, Dod);
                        for (int a = 0; a < 32; ++a) for (int b = 0; b < 32; ++b) { Pb[a][b] = Dod[a][b]; if (last) Pa[a][b] = Dev[a][b]; }
                    } else {
                        if (tp > 0) { store(north_map(tp - 1), Pa, true); store(south_map(tp - 1), Pb, true); }
                        mfma_unit(2 * tp, Dev);
                        mfma_unit(2 * tp + 1, Dod);
                        for (int a = 0; a < 32; ++a) for (int b = 0; b < 32; ++b) { Pa[a][b] = Dev[a][b] + Dod[a][b]; Pb[a][b] = Dev[a][b] - Dod[a][b]; }
                    }
                }
                if (npairs > 0) {
                    const int tl = npairs - 1;
                    store(mode == 0 ? fwd_map(tl, 0) : north_map(tl), Pa, false);
                    store(mode == 0 ? fwd_map(tl, 1) : south_map(tl), Pb, false);
                }
            }
    }
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

static bool build_plan(int nlat, int nlon, Grid g, Plan& P) {
    const int lmax = g == GRID_LOBATTO ? nlat - 1 : nlat, mmax = nlon / 2 + 1;
    const std::string err = build_sht_tables(nlat, nlon, lmax, mmax, g, P.t);
    if (!err.empty()) { std::printf("tables: %s\n", err.c_str()); return false; }
    P.H = nlat; P.L = lmax; P.M = mmax;
    const float ws = pow2_scale_for(P.t.wt), ps = pow2_scale_for(P.t.pt);
    pack_legendre_fold(P.t.wt.data(), mmax, nlat, lmax, P.t.Hp, 0, ws, P.fwd);
    pack_legendre_fold(P.t.pt.data(), mmax, nlat, lmax, P.t.Lp, 1, ps, P.inv);
    P.cut = derive_polar_cut(P.fwd, P.inv, mmax, nlat, lmax);
    P.kskip.assign((size_t)mmax, 0);
    P.kdrop = P.cut.ok && fold_geom(0, 0, lmax, nlat).nkp2 <= FOLD_NKP_SMALL;
    if (P.kdrop) {
        for (int m = 0; m < mmax; ++m) P.kskip[m] = P.cut.r0[m] / 16;
        pack_legendre_fold(P.t.wt.data(), mmax, nlat, lmax, P.t.Hp, 0, ws, P.fwd_cut, P.kskip.data());
    } else {
        P.fwd_cut = P.fwd;
    }
    return true;
}

// ---- table properties (an independent walk over every packed element, in the packer's own order)
static void check_tables(const Plan& P, const char* name, double lo_share, double hi_share) {
    const int H = P.H, L = P.L, M = P.M, Hh = (H + 1) / 2;
    const PolarCut& c = P.cut;
    CHECK(c.ok, "%s: the dead rows are not a monotone prefix", name);
    if (!c.ok) return;
    CHECK((int)c.r0.size() == M && (int)c.mcut.size() == H, "%s: table sizes", name);
    for (int m = 0; m < M; ++m) {
        CHECK(c.r0[m] >= 0 && c.r0[m] <= Hh, "%s: r0[%d] = %d out of range", name, m, c.r0[m]);
        if (m > 0) CHECK(c.r0[m] >= c.r0[m - 1], "%s: r0 decreases at m %d", name, m);
    }
    CHECK(M - 1 < L || c.r0[M - 1] == Hh, "%s: the wavenumber without a degree is not wholly dead", name);
    long dead = 0;
    for (int lat = 0; lat < H; ++lat) {
        const int kf = std::min(lat, H - 1 - lat);
        CHECK(c.mcut[lat] >= 0 && c.mcut[lat] <= M, "%s: mcut[%d] out of range", name, lat);
        for (int m = 0; m < M; ++m) CHECK((m >= c.mcut[lat]) == (kf < c.r0[m]), "%s: mcut and r0 disagree at lat %d m %d", name, lat, m);
        dead += M - c.mcut[lat];
    }
    const double share = (double)dead / ((double)M * H);
    CHECK(std::fabs(share - c.dead_share) < 1e-12, "%s: dead share %.6f vs %.6f", name, share, c.dead_share);
    CHECK(share >= lo_share && share <= hi_share, "%s: dead share %.4f outside [%.4f, %.4f]", name, share, lo_share, hi_share);
    std::vector<char> live_at_r0((size_t)M, 0);
    for (int mode = 0; mode < 2; ++mode) {
        const StripPack& sp = mode == 0 ? P.fwd : P.inv;
        const int R = mode == 0 ? L : H, K = mode == 0 ? H : L;
        for (int m = 0; m < M; ++m) {
            const FoldGeom g = fold_geom(mode, m, R, K);
            for (int u = 0; u < 2 * g.npairs; ++u)
                for (int jj = 0; jj < g.nkp2; ++jj) {
                    const uint16_t* blk = sp.frags.data() + ((size_t)sp.tile_off[m] + (size_t)u * g.nkp2 + jj) * 1024;
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 8; ++e) {
                            const int i = lane & 31, gg = lane >> 5;
                            const int kf = mode == 0 ? 16 * jj + 8 * gg + e : 32 * (u >> 1) + i;
                            const bool zero = ((blk[lane * 8 + e] | blk[512 + lane * 8 + e]) & 0x7fffu) == 0;
                            if (kf < c.r0[m]) CHECK(zero, "%s: live element inside the cut (mode %d m %d kf %d)", name, mode, m, kf);
                            else if (kf == c.r0[m] && !zero) live_at_r0[m] = 1;
                        }
                }
        }
    }
    for (int m = 0; m < M; ++m)
        if (c.r0[m] < Hh) CHECK(live_at_r0[m], "%s: row r0[%d] = %d has no live element: the cut is not maximal", name, m, c.r0[m]);
    // the forward table packed from k16-step r0 / 16 on holds the elements of the full pack, shifted
    if (P.kdrop)
        for (int m = 0; m < M; ++m) {
            const FoldGeom g = fold_geom(0, m, L, H), gc = fold_geom_cut(0, m, L, H, P.kskip[m]);
            CHECK(gc.nkp + P.kskip[m] == g.nkp || (gc.nkp == 0 && P.kskip[m] >= g.nkp), "%s: k-steps of m %d", name, m);
            for (int u = 0; u < 2 * g.npairs; ++u)
                for (int jj = 0; jj < gc.nkp; ++jj)
                    CHECK(std::memcmp(P.fwd_cut.frags.data() + ((size_t)P.fwd_cut.tile_off[m] + (size_t)u * gc.nkp2 + jj) * 1024,
                                      P.fwd.frags.data() + ((size_t)P.fwd.tile_off[m] + (size_t)u * g.nkp2 + P.kskip[m] + jj) * 1024, 2048) == 0,
                          "%s: shifted table block differs (m %d unit %d step %d)", name, m, u, jj);
        }
    long steps = 0, steps_cut = 0, tiles = 0, tiles_cut = 0;
    for (int m = 0; m < M; ++m) {
        const FoldGeom g = fold_geom(0, m, L, H), gc = fold_geom_cut(0, m, L, H, P.kskip[m]), gi = fold_geom(1, m, H, L);
        steps += (long)g.npairs * g.nkp2; steps_cut += (long)gc.npairs * gc.nkp2;
        tiles += gi.npairs; tiles_cut += std::max(0, gi.npairs - c.r0[m] / 32);
    }
    std::printf("%-28s dead share %.4f  r0[M/2] %d  r0[M-2] %d  forward k16-steps %ld -> %ld  inverse tile pairs %ld -> %ld\n", name, share,
                c.r0[M / 2], c.r0[M - 2], steps, steps_cut, tiles, tiles_cut);
}

// ---- data movement: FFT store mask -> forward Legendre, inverse Legendre -> FFT load mask, cut against no cut
static void check_movement(const Plan& P, const char* name, int N) {
    const int H = P.H, L = P.L, M = P.M;
    const PolarCut& c = P.cut;
    if (!c.ok) return;
    std::mt19937 rng(977u + (unsigned)H * 131u + (unsigned)N);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    bool fault = false;
    const float qnan = std::nanf("");
    // forward: the FFT's outputs S[m][lat][n]; stored where m < min(Mm, mcut[lat]), the rest of X keeps its NaN poison
    {
        const size_t xs = (size_t)M * H * N;
        std::vector<float> S(xs), Xc(xs, qnan);
        for (auto& v : S) v = U(rng);
        long stored = 0;
        for (int m = 0; m < M; ++m)
            for (int lat = 0; lat < H; ++lat)
                if (m < std::min(M, c.mcut[lat])) { std::memcpy(&Xc[((size_t)m * H + lat) * N], &S[((size_t)m * H + lat) * N], sizeof(float) * N); stored += N; }
        const size_t ds = (size_t)L * M * N;
        std::vector<double> D0(ds, -7.0), D1(ds, -7.0);
        std::vector<int> w0(ds, 0), w1(ds, 0);
        run_fold(0, P, P.fwd, nullptr, false, N, S, D0, w0, &fault);
        run_fold(0, P, P.fwd_cut, c.r0.data(), P.kdrop, N, Xc, D1, w1, &fault);
        long bad = 0, wr = 0;
        for (int l = 0; l < L; ++l)
            for (int m = 0; m < M; ++m)
                for (int n = 0; n < N; ++n) {
                    const size_t at = ((size_t)l * M + m) * N + n;
                    const int want = l >= m ? 1 : 0;
                    if (w0[at] != want || w1[at] != want) ++wr;
                    if (want && !same_bits(D0[at], D1[at])) ++bad;
                }
        CHECK(wr == 0, "%s N %d forward: %ld elements not written exactly once", name, N, wr);
        CHECK(bad == 0, "%s N %d forward: %ld elements differ from the run without the cut", name, N, bad);
        std::printf("%-28s N %3d forward : X entries stored %.4f of all, coefficients bitwise equal\n", name, N, (double)stored / (double)xs);
    }
    // inverse: coefficients E[l][m][n] -> X; the FFT reads X where m < min(Mm, mcut[lat]) and zero elsewhere
    {
        const size_t es = (size_t)L * M * N, xs = (size_t)M * H * N;
        std::vector<float> E(es);
        for (auto& v : E) v = U(rng);
        for (int l = 0; l < L; ++l)   // never written by the producer
            for (int m = l + 1; m < M; ++m)
                for (int n = 0; n < N; ++n) E[((size_t)l * M + m) * N + n] = 1e30f;
        std::vector<double> X0(xs, -7.0), X1(xs, (double)qnan);
        std::vector<int> w0(xs, 0), w1(xs, 0);
        run_fold(1, P, P.inv, nullptr, false, N, E, X0, w0, &fault);
        run_fold(1, P, P.inv, c.r0.data(), false, N, E, X1, w1, &fault);
        long bad = 0, wr = 0, nz = 0;
        for (int m = 0; m < M; ++m)
            for (int lat = 0; lat < H; ++lat)
                for (int n = 0; n < N; ++n) {
                    const size_t at = ((size_t)m * H + lat) * N + n;
                    const bool live = m < std::min(M, c.mcut[lat]);
                    if (w0[at] != 1 || w1[at] != (live ? 1 : 0)) ++wr;
                    if (!live && !same_bits(X0[at], 0.0)) ++nz;                       // what the cut drops is an exact +0 today
                    const double f0 = X0[at], f1 = live ? X1[at] : 0.0;               // what the FFT reads
                    if (!same_bits(f0, f1)) ++bad;
                }
        CHECK(wr == 0, "%s N %d inverse: %ld elements not written exactly once (live) / never (dead)", name, N, wr);
        CHECK(nz == 0, "%s N %d inverse: %ld dead elements are not exact zeros without the cut", name, N, nz);
        CHECK(bad == 0, "%s N %d inverse: %ld elements read by the FFT differ from the run without the cut", name, N, bad);
        std::printf("%-28s N %3d inverse : live region written once, dead region untouched, FFT input bitwise equal\n", name, N);
    }
    CHECK(!fault, "%s N %d: out of bounds access", name, N);
}

int main() {
    struct Case { int nlat, nlon; Grid g; const char* name; double lo, hi; int n1, n2; } cases[] = {
        {24, 48, GRID_LEGENDRE_GAUSS, "24x48 legendre-gauss", 0.0, 1.0, 128, 20},
        {46, 92, GRID_LEGENDRE_GAUSS, "46x92 legendre-gauss", 0.0, 1.0, 128, 6},
        {45, 90, GRID_LEGENDRE_GAUSS, "45x90 legendre-gauss", 0.0, 1.0, 128, 36},
        {23, 48, GRID_LEGENDRE_GAUSS, "23x48 legendre-gauss", 0.0, 1.0, 32, 0},
        {180, 360, GRID_LEGENDRE_GAUSS, "180x360 legendre-gauss", 0.23, 0.26, 32, 0},
        {180, 360, GRID_EQUIANGULAR, "180x360 equiangular", 0.0, 1.0, 32, 0},
        {181, 360, GRID_LOBATTO, "181x360 lobatto", 0.0, 1.0, 32, 0},
        // big form: first size past the small form; 12 k16-steps at half a degree; 18 steps with an odd nlat; equiangular, odd nlat
        {194, 48, GRID_LEGENDRE_GAUSS, "194x48 legendre-gauss", 0.0, 1.0, 128, 0},
        {360, 720, GRID_LEGENDRE_GAUSS, "360x720 legendre-gauss", 0.2750, 0.2950, 128, 0},
        {385, 720, GRID_LEGENDRE_GAUSS, "385x720 legendre-gauss", 0.2486, 0.2686, 128, 0},
        {361, 720, GRID_EQUIANGULAR, "361x720 equiangular", 0.2760, 0.2960, 128, 0},
    };
    for (auto& cs : cases) {
        Plan P;
        if (!build_plan(cs.nlat, cs.nlon, cs.g, P)) return 2;
        check_tables(P, cs.name, cs.lo, cs.hi);
        check_movement(P, cs.name, cs.n1);
        if (cs.n2) check_movement(P, cs.name, cs.n2);
    }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("polar cut ok\n");
    return 0;
}
