// CPU restatement of the index algebra of dhconv_body (ace_amd/csrc/dhconv_strip.hip) on top of the launch's real work list
// (ace_amd/csrc/dhconv_units.h).  Nothing of the kernel is compiled here: what it computes per wave and lane is written out again -
//   * the A-piece source address (row clamp, XOR slot, stage window tb + t) and its LDS destination (ring slot, piece wave + 4 k,
//     16 bytes per lane), stages t >= nstages (the dummy tail) included;
//   * the fragment read address (frag_addr, key, row piece; hi plane at the address, lo plane 1024 bytes on);
//   * the B address in the dense and in the diagonal-blocks form, with kbase and the clamp of the k-group;
//   * tb, kspan, kbase, live;
//   * the accumulator's row map and the store mask
// - over operands laid out as the three producers lay them out (coefficient planes [l][(m, b)][re | im][c] as the Legendre stage and
// launch_ref_to_spec + launch_split_f16 write them, filter planes as pack_dhconv_f16c_kernel and pack_dhconv_f16g_kernel write them;
// restated below from their index arithmetic).  Values are doubles; a plane pair is two different arrays (hi, lo) and the products
// kept are the kernel's three (lo x hi, hi x lo, hi x hi), so that a fragment taken from the wrong plane shows.  Coefficients with
// m > l are NaN.  Checked:
//   1. every address lies inside its allocation (the clamped and the dummy ones too);
//   2. every filter element a unit needs is fetched by a live stage of exactly one wave of the unit, exactly once, and nothing else;
//   3. every output element with row < rows(l) is written exactly once over the launch, and none beyond;
//   4. the values, against direct complex sums over the logical operands (all units at C = 128, a spread of degrees - l = 0, 1, 4, 9, .., L - 1 - above).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ace_amd/csrc/dhconv_units.h"

namespace {

struct Cfg { int n, C, L, Mm, G, native; };

struct Rng {
    unsigned long long s;
    double next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)((s >> 11) & 0xfffffffffffffULL) / (double)0x10000000000000ULL * 2.0 - 1.0; }
};

int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad < 40) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++g_bad; } } while (0)

struct Operands {
    Cfg c;
    int cg, kstore;
    long sD, sW, sE;
    std::vector<double> Dh, Dl;        // [l][m][b][re | im][ch]
    std::vector<double> Wh, Wl;        // packed planes
    std::vector<double> wh_log, wl_log;  // logical dense filter [l][blk][i][o] (zero between groups)
};

// ---- the producers' layouts
void build(const Cfg& c, Operands& op) {
    op.c = c;
    const int C = c.C, n = c.n, L = c.L, Mm = c.Mm;
    op.cg = C / c.G;
    op.kstore = c.native ? op.cg : C;
    op.sD = (long)Mm * n * 2 * C; op.sE = op.sD; op.sW = (long)2 * op.kstore * C;
    Rng r{0x9e3779b97f4a7c15ULL ^ (unsigned long long)(C * 131 + c.G * 17 + L * 7 + n)};
    op.Dh.assign((size_t)L * op.sD, 0.0); op.Dl = op.Dh;
    for (int l = 0; l < L; ++l)
        for (int m = 0; m < Mm; ++m)
            for (int b = 0; b < n; ++b)
                for (int k = 0; k < 2 * C; ++k) {   // spec_layout_kernel: dst + (r Bt + b) 2 C + c, imaginary part C further
                    const size_t at = (((size_t)l * Mm + m) * n + b) * 2 * C + k;
                    op.Dh[at] = m <= l ? r.next() : NAN;
                    op.Dl[at] = m <= l ? 1e-3 * r.next() : NAN;
                }
    op.wh_log.assign((size_t)L * 2 * C * C, 0.0); op.wl_log = op.wh_log;
    for (size_t t = 0; t < op.wh_log.size(); ++t) {
        const int o = t % C, i = (t / C) % C;
        if (i / op.cg == o / op.cg) { op.wh_log[t] = r.next(); op.wl_log[t] = 1e-3 * r.next(); }
    }
    auto logical = [&](const std::vector<double>& w, int l, int blk, int i, int o) { return w[(((size_t)l * 2 + blk) * C + i) * C + o]; };
    const long total = (long)L * 2 * op.kstore * C;
    op.Wh.assign((size_t)total, NAN); op.Wl = op.Wh;
    for (long t = 0; t < total; ++t) {
        const int e = t % 8;
        long q = t / 8;
        const int o = q % C;
        q /= C;
        if (!c.native) {   // pack_dhconv_f16c_kernel: [l][Wr | Wi][kg < C / 8][o][8], row kg 8 + e = input channel
            const int kg = q % (C / 8);
            q /= (C / 8);
            const int blk = q % 2, l = (int)(q / 2);
            op.Wh[t] = logical(op.wh_log, l, blk, kg * 8 + e, o);
            op.Wl[t] = logical(op.wl_log, l, blk, kg * 8 + e, o);
        } else {           // pack_dhconv_f16g_kernel: [l][Wr | Wi][kg < cg / 8][o][8], row = input channel relative to o's group
            const int kg = q % (op.cg / 8);
            q /= (op.cg / 8);
            const int blk = q % 2, l = (int)(q / 2);
            const int i = (o / op.cg) * op.cg + kg * 8 + e;
            op.Wh[t] = logical(op.wh_log, l, blk, i, o);
            op.Wl[t] = logical(op.wl_log, l, blk, i, o);
        }
    }
}

struct LdsSlot { int plane; long at; bool valid; };   // 16 bytes of LDS: which plane, first of the 8 halves

// ---- one workgroup
void unit(const Operands& op, int l, int j, int row0, int rows, bool math, std::vector<int>& written, std::vector<double>& E,
          std::vector<int>& fetched) {
    const Cfg& cf = op.c;
    constexpr int PB = 2, NSTG = PB + 1;
    const int NS = (rows + 31) / 32;
    const int STAGE = NS * 8192, NA = 2 * NS;
    const int C = cf.C, K2 = 2 * C;
    const int cg = C / cf.G;
    const bool skip = cf.G > 1 && (cg % 128 == 0 || 128 % cg == 0);
    const int kspan = skip ? (cg > 128 ? cg : 128) : C;
    const int tb = skip ? ((128 * j) / kspan) * (kspan / 32) : 0;
    const int nstages = kspan / 32;
    const int kstore = op.kstore;
    const bool native = kstore != C;
    CHECK(nstages % 4 == 0 && nstages >= 4, "nstages %d", nstages);
    CHECK(NS >= 1 && NS <= ace::DH_CHUNK_STRIPS && rows >= 1, "unit rows %d", rows);
    CHECK(32 * (tb + nstages) <= C, "stage window beyond C: tb %d nstages %d", tb, nstages);

    std::vector<LdsSlot> lds((size_t)NSTG * STAGE / 16, LdsSlot{0, 0, false});
    std::fill(fetched.begin(), fetched.end(), 0);
    const long dbase = (long)l * op.sD + (long)row0 * K2;
    const long dsize = (long)op.Dh.size(), wsize = (long)op.Wh.size();

    auto issue_a = [&](int t) {
        for (int wave = 0; wave < 4; ++wave)
            for (int k = 0; k < NA; ++k)
                for (int lane = 0; lane < 64; ++lane) {
                    const int s = k >> 1, sl = k & 1, rh = wave >> 1, pl = wave & 1;
                    int row = 32 * s + 16 * rh + (lane >> 2);
                    const int ls = (lane & 3) ^ ((row >> 2) & 3);
                    row = row < rows ? row : rows - 1;
                    const int tt = tb + (t < nstages ? t : nstages - 1);
                    const long at = dbase + (long)row * K2 + sl * C + 8 * ls + 32 * tt;
                    CHECK(at >= 0 && at + 8 <= dsize, "A piece address %ld outside [0, %ld) (l %d row0 %d rows %d t %d)", at, dsize, l, row0, rows, t);
                    CHECK(at % 8 == 0, "A piece address %ld not 16-byte aligned", at);
                    const int byte = (t % NSTG) * STAGE + (wave + 4 * k) * 1024 + lane * 16;
                    CHECK(byte + 16 <= NSTG * STAGE, "LDS destination %d beyond %d", byte, NSTG * STAGE);
                    lds[byte / 16] = LdsSlot{pl, at, true};
                }
    };
    struct BAddr { long at; bool ok; };
    auto b_addr = [&](int wave, int lane, int t, int c, int blk) {
        const int i = lane & 31, g = lane >> 5;
        const int oc = 128 * j + 32 * wave;
        const int kbase = native ? (oc / cg) * cg : 0;
        const int tt = tb + (t < nstages ? t : nstages - 1);
        int kg = 4 * tt + 2 * c + g - kbase / 8;
        if (native) kg = kg < 0 ? 0 : (kg >= kstore / 8 ? kstore / 8 - 1 : kg);
        const long off = (long)blk * kstore * C + ((long)kg * C + oc + i) * 8;
        const long at = (long)l * op.sW + off;
        const bool ok = at >= 0 && at + 8 <= wsize && kg >= 0 && kg < kstore / 8;
        CHECK(ok, "B address %ld (kg %d of %d) outside [0, %ld) (l %d j %d wave %d t %d)", at, kg, kstore / 8, wsize, l, j, wave, t);
        return BAddr{at, ok};
    };
    auto is_live = [&](int wave, int t) {
        const int oc = 128 * j + 32 * wave;
        const int kbase = native ? (oc / cg) * cg : 0;
        const int k0 = 32 * (tb + t);
        return !native || (k0 >= kbase && k0 < kbase + cg);
    };

    std::vector<double> acc;   // [wave][s][tl][row 32][col 32]
    if (math) acc.assign((size_t)4 * NS * 2 * 1024, 0.0);
    issue_a(0); issue_a(1);
    for (int t = 0; t < nstages; ++t) {
        for (int wave = 0; wave < 4; ++wave) {
            const bool live = is_live(wave, t);
            double Bh[2][2][64][8], Bl[2][2][64][8];
            for (int c = 0; c < 2; ++c)
                for (int blk = 0; blk < 2; ++blk)
                    for (int lane = 0; lane < 64; ++lane) {
                        const BAddr a = b_addr(wave, lane, t, c, blk);
                        if (!a.ok) continue;
                        for (int e = 0; e < 8; ++e) {
                            Bh[c][blk][lane][e] = op.Wh[a.at + e];
                            Bl[c][blk][lane][e] = op.Wl[a.at + e];
                            if (live) ++fetched[a.at - (long)l * op.sW + e];
                        }
                    }
            if (!live) continue;
            for (int s = 0; s < NS; ++s)
                for (int ph = 0; ph < 4; ++ph) {
                    const int c = ph >> 1, sl = ph & 1;
                    double Ah[64][8], Al[64][8];
                    bool ok = true;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i = lane & 31, g = lane >> 5;
                        const int key = (i >> 2) & 3;
                        const int la = (t % NSTG) * STAGE + ((i >> 4) * 2) * 1024 + (i & 15) * 64;
                        const int addr = la + (2 * s + (ph & 1)) * 4096 + ((2 * (ph >> 1) + g) ^ key) * 16;
                        CHECK(addr % 16 == 0 && addr + 1024 + 16 <= NSTG * STAGE, "fragment address %d", addr);
                        const LdsSlot& h = lds[addr / 16];
                        const LdsSlot& lo = lds[(addr + 1024) / 16];
                        int row = 32 * s + i;
                        row = row < rows ? row : rows - 1;
                        const long want = dbase + (long)row * K2 + sl * C + 32 * (tb + t) + 16 * c + 8 * g;   // row (clamped), k = 32 (tb + t) + 16 c + 8 g ..
                        const bool good = h.valid && lo.valid && h.plane == 0 && lo.plane == 1 && h.at == want && lo.at == want;
                        CHECK(good, "fragment of l %d rows %d t %d s %d ph %d lane %d: planes %d %d, at %ld %ld, want %ld", l, rows, t, s, ph, lane, h.plane, lo.plane, h.at, lo.at, want);
                        ok = ok && good;
                        if (good && math)
                            for (int e = 0; e < 8; ++e) { Ah[lane][e] = op.Dh[h.at + e]; Al[lane][e] = op.Dl[lo.at + e]; }
                    }
                    if (!math || !ok) continue;
                    double* a0 = &acc[(((size_t)wave * NS + s) * 2 + 0) * 1024];
                    double* a1 = &acc[(((size_t)wave * NS + s) * 2 + 1) * 1024];
                    for (int ra = 0; ra < 32; ++ra)
                        for (int cb = 0; cb < 32; ++cb) {
                            double pr = 0.0, pi = 0.0;   // with Wr, with Wi: the three kept products
                            for (int g = 0; g < 2; ++g)
                                for (int e = 0; e < 8; ++e) {
                                    const double ah = Ah[ra + 32 * g][e], al = Al[ra + 32 * g][e];
                                    pr += al * Bh[c][0][cb + 32 * g][e] + ah * Bl[c][0][cb + 32 * g][e] + ah * Bh[c][0][cb + 32 * g][e];
                                    pi += al * Bh[c][1][cb + 32 * g][e] + ah * Bl[c][1][cb + 32 * g][e] + ah * Bh[c][1][cb + 32 * g][e];
                                }
                            if (sl == 0) { a0[ra * 32 + cb] += pr; a1[ra * 32 + cb] += pi; }   // D_re: real += D_re Wr, imaginary += D_re Wi
                            else { a1[ra * 32 + cb] += pr; a0[ra * 32 + cb] -= pi; }           // D_im: imaginary += D_im Wr, real -= D_im Wi
                        }
                }
        }
        issue_a(t + PB);   // requested while stage t computes, into the ring slot stage t - 1 held
        for (int wave = 0; wave < 4; ++wave)
            for (int lane = 0; lane < 64; ++lane)
                for (int q = 0; q < 4; ++q) (void)b_addr(wave, lane, t + PB, q >> 1, q & 1);   // bounds of the read-ahead, the dummy tail included
    }
    // 2. the unit's filter slice: each needed element once, nothing else
    {
        long wrong = 0;
        for (int blk = 0; blk < 2; ++blk)
            for (int kk = 0; kk < kstore; ++kk)
                for (int o = 0; o < C; ++o) {
                    const bool mine = o >= 128 * j && o < 128 * j + 128;
                    const bool need = mine && (native || (kk >= 32 * tb && kk < 32 * tb + kspan));
                    const int got = fetched[(size_t)blk * kstore * C + ((size_t)(kk / 8) * C + o) * 8 + kk % 8];
                    if (got != (need ? 1 : 0)) ++wrong;
                }
        CHECK(wrong == 0, "l %d j %d rows %d: %ld filter elements not fetched exactly once by a live stage", l, j, rows, wrong);
    }
    // epilogue: lane (i, g) holds column i; register r is row (r & 3) + 8 (r >> 2) + 4 g of the strip
    const long ebase = (long)l * op.sE + (long)row0 * K2;
    for (int wave = 0; wave < 4; ++wave)
        for (int lane = 0; lane < 64; ++lane)
            for (int s = 0; s < NS; ++s)
                for (int tl = 0; tl < 2; ++tl)
                    for (int r = 0; r < 16; ++r) {
                        const int i = lane & 31, g = lane >> 5;
                        const int oc = 128 * j + 32 * wave;
                        const int row = 32 * s + (r & 3) + 8 * (r >> 2) + 4 * g;
                        if (row >= rows) continue;
                        const long at = ebase + (long)row * K2 + tl * C + oc + i;
                        CHECK(at >= 0 && at < (long)written.size(), "store address %ld", at);
                        if (at < 0 || at >= (long)written.size()) continue;
                        ++written[at];
                        if (math) E[at] = acc[((((size_t)wave * NS + s) * 2 + tl) * 32 + (row - 32 * s)) * 32 + i];
                    }
}

double run(const Cfg& c) {
    Operands op;
    build(c, op);
    const int C = c.C;
    std::vector<int> u;
    const int per = ace::dhconv_units(c.L, c.Mm * c.n, c.n, C, u);
    std::vector<int> written((size_t)c.L * op.sE, 0);
    std::vector<double> E(written.size(), NAN);
    std::vector<int> fetched((size_t)op.sW, 0);
    std::vector<char> did_math(c.L, 0);
    auto wants_math = [&](int l) { return C <= 128 || l <= 1 || l == c.L - 1 || l % 5 == 4; };
    int nunits = 0;
    for (int x = 0; x < 8; ++x)
        for (int k = 0; k < per; ++k) {
            const int* e = &u[((size_t)x * per + k) * 4];
            if (e[3] <= 0) continue;
            unit(op, e[0], e[1], e[2], e[3], wants_math(e[0]), written, E, fetched);
            did_math[e[0]] = wants_math(e[0]);
            ++nunits;
        }
    // 3. coverage
    long wrong = 0;
    for (int l = 0; l < c.L; ++l) {
        const long want = (long)(l + 1) * c.n;
        const long rows_l = want < (long)c.Mm * c.n ? want : (long)c.Mm * c.n;
        for (long row = 0; row < (long)c.Mm * c.n; ++row)
            for (int k = 0; k < 2 * C; ++k)
                if (written[(size_t)l * op.sE + row * 2 * C + k] != (row < rows_l ? 1 : 0)) ++wrong;
    }
    CHECK(wrong == 0, "%ld output elements not written exactly once (or written beyond rows(l))", wrong);
    // 4. values
    double worst = 0.0;
    for (int l = 0; l < c.L; ++l) {
        if (!did_math[l]) continue;
        const long want = (long)(l + 1) * c.n;
        const long rows_l = want < (long)c.Mm * c.n ? want : (long)c.Mm * c.n;
        for (long row = 0; row < rows_l; ++row) {
            const double* dh = &op.Dh[(size_t)l * op.sD + row * 2 * C];
            const double* dl = &op.Dl[(size_t)l * op.sD + row * 2 * C];
            std::vector<double> re(C, 0.0), im(C, 0.0), mag(C, 0.0);
            auto p3 = [](double ah, double al, double bh, double bl) { return al * bh + ah * bl + ah * bh; };
            for (int i = 0; i < C; ++i) {   // input channel i reaches the output channels of its own group
                const double* wrh = &op.wh_log[(((size_t)l * 2 + 0) * C + i) * C];
                const double* wrl = &op.wl_log[(((size_t)l * 2 + 0) * C + i) * C];
                const double* wih = &op.wh_log[(((size_t)l * 2 + 1) * C + i) * C];
                const double* wil = &op.wl_log[(((size_t)l * 2 + 1) * C + i) * C];
                for (int o = (i / op.cg) * op.cg; o < (i / op.cg + 1) * op.cg; ++o) {
                    const double rr = p3(dh[i], dl[i], wrh[o], wrl[o]), ii = p3(dh[C + i], dl[C + i], wih[o], wil[o]);
                    const double ri = p3(dh[i], dl[i], wih[o], wil[o]), ir = p3(dh[C + i], dl[C + i], wrh[o], wrl[o]);
                    re[o] += rr - ii; im[o] += ri + ir;
                    mag[o] += std::fabs(rr) + std::fabs(ii) + std::fabs(ri) + std::fabs(ir);
                }
            }
            for (int o = 0; o < C; ++o) {
                const double gr = E[(size_t)l * op.sE + row * 2 * C + o], gi = E[(size_t)l * op.sE + row * 2 * C + C + o];
                const double err = std::fmax(std::fabs(gr - re[o]), std::fabs(gi - im[o])) / mag[o];
                if (!(err <= 1e-12)) { CHECK(false, "value at l %d row %ld o %d: (%g, %g) against (%g, %g)", l, row, o, gr, gi, re[o], im[o]); worst = 1.0; }
                else worst = std::fmax(worst, err);
            }
        }
    }
    std::printf("n %d C %3d L %2d Mm %2d G %d %-6s: %4d units, %d per XCD, worst %.2e%s\n", c.n, C, c.L, c.Mm, c.G, c.native ? "native" : "dense", nunits,
                per, worst, g_bad ? "  FAILED" : "");
    return worst;
}

}  // namespace

int main() {
    const int shapes[][3] = {{1, 96, 96}, {3, 40, 41}, {5, 40, 41}, {2, 24, 10}, {1, 1, 2}, {1, 5, 6}, {1, 8, 9}, {1, 9, 10}};   // (n, L, Mm) of the C = 128 families
    double worst = 0.0;
    for (const auto& s : shapes) worst = std::fmax(worst, run({s[0], 128, s[1], s[2], 1, 0}));
    const int tshape[3] = {5, 24, 25}, small[3] = {1, 5, 6};
    for (int C : {128, 256, 384, 512}) worst = std::fmax(worst, run({tshape[0], C, tshape[1], tshape[2], 1, 0}));
    const int gd[][2] = {{256, 4}, {256, 2}, {512, 2}, {384, 2}, {384, 4}}, gn[][2] = {{256, 8}, {256, 4}, {512, 4}, {512, 2}};
    for (const int* sh : {tshape, small}) {
        for (const auto& g : gd) worst = std::fmax(worst, run({sh[0], g[0], sh[1], sh[2], g[1], 0}));
        for (const auto& g : gn) worst = std::fmax(worst, run({sh[0], g[0], sh[1], sh[2], g[1], 1}));
    }
    if (g_bad) { std::printf("FAILED: %d checks\n", g_bad); return 1; }
    std::printf("worst: %.2e over all shapes, every address in bounds, every filter element and output element exactly once\n", worst);
    return 0;
}
