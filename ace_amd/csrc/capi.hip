// C ABI of libace_sfno.so (include/ace_sfno.h): SHT plans, building blocks and the
// SFNO forward schedule.  Host code only; the kernels live in kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/ace_sfno.h"
#include "errors.h"
#include "kernels.h"
#include "strip_pack.h"
#include "tables.h"
#include "weight_prep.h"

using namespace ace;   // fail() below is ace::fail (errors.h)

namespace ace {
Switches read_switches() {
    auto on = [](const char* name) { const char* e = std::getenv(name); return e && e[0] && !(e[0] == '0' && !e[1]); };
    Switches sw;
    sw.no_fft = on("ACE_NO_FFT");
    sw.no_strip = on("ACE_NO_STRIP");
    sw.no_fold = on("ACE_NO_FOLD");
    sw.no_dhconv_strip = on("ACE_NO_DHCONV_STRIP");
    sw.no_polar_cut = on("ACE_NO_POLAR_CUT");
    sw.polar_poison = on("ACE_POLAR_POISON");
#ifdef ACE_MEASUREMENT_SWITCHES   // historical routings: measurement builds only (tools/mkvar.sh NAME -DACE_MEASUREMENT_SWITCHES)
    sw.no_pk = on("ACE_NO_PK");
    sw.no_pk_sht = on("ACE_NO_PK_SHT");
#endif
    sw.no_enc_ws = on("ACE_NO_ENC_WS");
    sw.no_enc_pk = on("ACE_NO_ENC_PK");
    sw.no_cln_mfma = on("ACE_NO_CLN_MFMA");
    sw.no_cln_planes = on("ACE_NO_CLN_PLANES");
    sw.dense_grouped_filter = on("ACE_DENSE_GROUPED_FILTER");
    if (const char* e = std::getenv("ACE_CONV_WL")) sw.conv_wl = !(e[0] == '0' && !e[1]);
    if (const char* e = std::getenv("ACE_PLANES_STREAM")) sw.planes_stream = !(e[0] == '0' && !e[1]);
    if (const char* e = std::getenv("ACE_FUSED_PACK")) sw.fused_pack = !(e[0] == '0' && !e[1]);
    if (const char* e = std::getenv("ACE_CONV_WS")) {
        const std::string v(e);
        if (v == "all" || v == "1") sw.conv_ws_roles = 7;
        else sw.conv_ws_roles = (v.find("skip") != std::string::npos ? 1 : 0) | (v.find("fc1") != std::string::npos ? 2 : 0) |
                                (v.find("fc2") != std::string::npos ? 4 : 0);
    }
    return sw;
}
}  // namespace ace
extern "C" int ace_version(void) { return 100; }

struct DevBuf {
    float* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count, bool zero = true) {
        release();
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(float));
        if (e != hipSuccess) { p = nullptr; return e; }
        n = count;
        if (zero) e = hipMemset(p, 0, count * sizeof(float));
        return e;
    }
    hipError_t ensure(size_t count) { return count <= n ? hipSuccess : alloc(count); }
    // a spectral scratch X[m][lat][...]: zeroed, or (ACE_POLAR_POISON) quiet NaNs - once, when it is allocated.  The polar cut leaves
    // the dead entries unwritten, so a kernel that read one would show
    hipError_t alloc_x(size_t count, bool poison) {
        hipError_t e = alloc(count);
        if (e == hipSuccess && poison && count) e = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p), 0x7fc00000, count);
        return e;
    }
    hipError_t ensure_x(size_t count, bool poison) { return count <= n ? hipSuccess : alloc_x(count, poison); }
    hipError_t upload(const std::vector<float>& h) {
        hipError_t e = alloc(h.size(), false);
        if (e != hipSuccess) return e;
        return hipMemcpy(p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    }
};

// `count` floats of a device array on the host, once the stream's pending writes to it have finished
static int host_copy(const float* dev, size_t count, hipStream_t s, std::vector<float>& host) {
    host.resize(count);
    ACE_HIP_TRY(hipStreamSynchronize(s));
    ACE_HIP_TRY(hipMemcpy(host.data(), dev, count * sizeof(float), hipMemcpyDeviceToHost));
    return ACE_OK;
}
static float host_absmax(const std::vector<float>& v) {
    float mx = 0.f;
    for (float x : v) mx = std::max(mx, std::fabs(x));
    return mx;
}
// a dynamic-range slot (AMAX_SHARDS words, each the bit pattern of a non-negative float) read back as the maximum it holds
static int read_range_slot(const unsigned* slot, hipStream_t s, float* mx) {
    unsigned bits[AMAX_SHARDS];
    ACE_HIP_TRY(hipMemcpyAsync(bits, slot, sizeof(bits), hipMemcpyDeviceToHost, s));
    ACE_HIP_TRY(hipStreamSynchronize(s));
    *mx = 0.f;
    for (unsigned b : bits) { float f; std::memcpy(&f, &b, 4); *mx = std::max(*mx, f); }
    return ACE_OK;
}
// max |x| of a device array, reduced on the device (a maximum rounds nothing: the value a host loop over a copy gives)
static int device_absmax(const float* x, long count, hipStream_t s, float* mx) {
    DevBuf slot;
    ACE_HIP_TRY(slot.alloc(AMAX_SHARDS));
    ACE_HIP_TRY(launch_absmax(x, count, reinterpret_cast<unsigned*>(slot.p), s));
    return read_range_slot(reinterpret_cast<const unsigned*>(slot.p), s, mx);
}

// ---------------------------------------------------------------------------------------------
// SHT plan
// ---------------------------------------------------------------------------------------------
struct ace_sht_plan {
    int nlat = 0, nlon = 0, lmax = 0, mmax = 0, Hp = 0, Lp = 0, Kfp = 0;
    Grid grid = GRID_LEGENDRE_GAUSS;
    DevBuf wt, pt, fc, fs, gc, gs;
    DevBuf X, D;  // scratch of the standalone transforms (plan-owned, grown on demand)
    // f16x3 mode: hi/lo fp16 planes of wt / pt (same pitches, in halves) scaled by a power of two
    DevBuf wt_hi, wt_lo, pt_hi, pt_lo;
    float wt_scale = 1.f, pt_scale = 1.f;
    float wt_winf = 0.f;   // max over (m, l) of sum_k |wt[m][l][k]|: |Legendre-forward output| <= wt_winf * max|X|
    bool f16 = false;
    // strip kernels (strip.hip): wt / pt as pre-packed MFMA A fragments + per-m block offsets (nlat, lmax <= 192)
    DevBuf wt_frag, pt_frag, wt_off, pt_off;
    bool strip = false;
    // ... and in the equatorially folded form (strip_fold.hip) when the tables are mirror-symmetric about the equator
    DevBuf wt_ffrag, pt_ffrag, wt_foff, pt_foff;
    bool fold = false;
    // ... with the polar cut (strip_pack.h, PolarCut): r0[mmax] / mcut[nlat] as device int arrays; kdrop: the forward fragments start
    // at k16-step r0[m] / 16 (small form)
    DevBuf cut_r0, cut_mcut;
    bool cut = false, kdrop = false;
    double cut_share = 0.0;
    DevBuf slots;   // standalone transforms in f16x3 mode: dynamic-range slots (max|X|, max|coefficients|)
    Switches sw;    // measurement switches, read when the plan was built
    // which kernel family the last Legendre launch of each direction took (ace_sht_plan_route): 0 tile engine, 1 strip.hip,
    // 2 strip_fold.hip, 3 strip_fold.hip big form (more than 96 folded latitudes); -1 = no launch yet
    mutable int route[2] = {-1, -1};
};
static int fold_route(const LegStripArgs& f) { return legendre_fold_is_big(f) ? 3 : 2; }

static float pow2_scale_for(const std::vector<float>& v) { return pow2_scale(host_absmax(v), 10); }  // puts max|v| in [2^9, 2^10)

static int plan_build(int nlat, int nlon, int lmax, int mmax, Grid g, std::unique_ptr<ace_sht_plan>& out,
                      bool f16 = false) {
    ShtTables t;
    std::string err = build_sht_tables(nlat, nlon, lmax, mmax, g, t);
    if (!err.empty()) return fail(ACE_ERR_INVALID, err);
    auto p = std::make_unique<ace_sht_plan>();
    p->sw = read_switches();
    p->nlat = t.nlat; p->nlon = t.nlon; p->lmax = t.lmax; p->mmax = t.mmax;
    p->Hp = t.Hp; p->Lp = t.Lp; p->Kfp = t.Kfp; p->grid = g;
    ACE_HIP_TRY(p->wt.upload(t.wt));
    ACE_HIP_TRY(p->pt.upload(t.pt));
    ACE_HIP_TRY(p->fc.upload(t.fc));
    ACE_HIP_TRY(p->fs.upload(t.fs));
    ACE_HIP_TRY(p->gc.upload(t.gc));
    ACE_HIP_TRY(p->gs.upload(t.gs));
    if (f16) {
        p->f16 = true;
        p->wt_scale = pow2_scale_for(t.wt);
        for (size_t r = 0; r < (size_t)t.mmax * t.lmax; ++r) {
            double rs = 0.0;
            for (int k = 0; k < t.nlat; ++k) rs += std::fabs((double)t.wt[r * t.Hp + k]);
            p->wt_winf = std::max(p->wt_winf, (float)(rs * (1.0 + 1e-6)));
        }
        p->pt_scale = pow2_scale_for(t.pt);
        const size_t hw = (t.wt.size() + 1) / 2, hp = (t.pt.size() + 1) / 2;
        ACE_HIP_TRY(p->wt_hi.alloc(hw, false)); ACE_HIP_TRY(p->wt_lo.alloc(hw, false));
        ACE_HIP_TRY(p->pt_hi.alloc(hp, false)); ACE_HIP_TRY(p->pt_lo.alloc(hp, false));
        ACE_HIP_TRY(launch_split_f16(p->wt.p, t.Hp, p->wt_hi.p, p->wt_lo.p, t.Hp, (long)t.mmax * t.lmax, t.Hp, p->wt_scale, nullptr));
        ACE_HIP_TRY(launch_split_f16(p->pt.p, t.Lp, p->pt_hi.p, p->pt_lo.p, t.Lp, (long)t.mmax * t.nlat, t.Lp, p->pt_scale, nullptr));
        ACE_HIP_TRY(hipDeviceSynchronize());
        auto up = [](const StripPack& sp, DevBuf& frag, DevBuf& off) -> hipError_t {
            hipError_t e = frag.alloc((sp.frags.size() + 1) / 2, false);   // halves -> floats
            if (e != hipSuccess) return e;
            e = hipMemcpy(frag.p, sp.frags.data(), sp.frags.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
            if (e != hipSuccess) return e;
            e = off.alloc(sp.tile_off.size(), false);
            if (e != hipSuccess) return e;
            return hipMemcpy(off.p, sp.tile_off.data(), sp.tile_off.size() * sizeof(int), hipMemcpyHostToDevice);
        };
        if (t.nlat <= 192 && t.lmax <= 192) {
            StripPack sp;
            pack_legendre_strip(t.wt.data(), t.mmax, t.lmax, t.nlat, t.Hp, 0, p->wt_scale, sp);
            ACE_HIP_TRY(up(sp, p->wt_frag, p->wt_off));
            pack_legendre_strip(t.pt.data(), t.mmax, t.nlat, t.lmax, t.Lp, 1, p->pt_scale, sp);
            ACE_HIP_TRY(up(sp, p->pt_frag, p->pt_off));
            p->strip = true;
        }
        // P_l^m(-x) = (-1)^(l+m) P_l^m(x) on a grid that is symmetric about the equator (all three quadratures are): checked
        // on the fp32 tables themselves - mirror entries agree to the rounding of the fp64 recursion.  Folded, a parity's contraction
        // fits the strip kernels' resident operand up to 768 latitudes / degrees (strip_fold.hip: 0.25-degree grid included).
        if ((t.nlat + 1) / 2 <= 16 * FOLD_NKP_BIG && (t.lmax + 1) / 2 <= 16 * FOLD_NKP_BIG && !p->sw.no_fold &&
            fold_symmetry_error(t.wt.data(), t.mmax, t.nlat, t.lmax, t.Hp, 0) < 2e-6 &&
            fold_symmetry_error(t.pt.data(), t.mmax, t.nlat, t.lmax, t.Lp, 1) < 2e-6) {
            StripPack sp, spi;
            pack_legendre_fold(t.wt.data(), t.mmax, t.nlat, t.lmax, t.Hp, 0, p->wt_scale, sp);
            pack_legendre_fold(t.pt.data(), t.mmax, t.nlat, t.lmax, t.Lp, 1, p->pt_scale, spi);
            if (!p->sw.no_polar_cut) {
                // the (m, folded latitude) pairs whose fragments are all zero in both packs: never stored, loaded or multiplied
                const PolarCut pc = derive_polar_cut(sp, spi, t.mmax, t.nlat, t.lmax);
                if (pc.ok && pc.dead_share > 0.0) {
                    auto upi = [](const std::vector<int>& v, DevBuf& d) -> hipError_t {
                        const hipError_t e = d.alloc(v.size(), false);
                        return e != hipSuccess ? e : hipMemcpy(d.p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice);
                    };
                    ACE_HIP_TRY(upi(pc.r0, p->cut_r0));
                    ACE_HIP_TRY(upi(pc.mcut, p->cut_mcut));
                    p->cut = true;
                    p->cut_share = pc.dead_share;
                    if (fold_geom(0, 0, t.lmax, t.nlat).nkp2 <= FOLD_NKP_SMALL) {   // small form: the wholly dead leading k16-steps leave the table
                        std::vector<int> kskip(pc.r0.size());
                        for (size_t m = 0; m < kskip.size(); ++m) kskip[m] = pc.r0[m] / 16;
                        pack_legendre_fold(t.wt.data(), t.mmax, t.nlat, t.lmax, t.Hp, 0, p->wt_scale, sp, kskip.data());
                        p->kdrop = true;
                    }
                }
            }
            ACE_HIP_TRY(up(sp, p->wt_ffrag, p->wt_foff));
            ACE_HIP_TRY(up(spi, p->pt_ffrag, p->pt_foff));
            p->fold = true;
        }
    }
    out = std::move(p);
    return ACE_OK;
}

// X[m][k][b][ri][c] <- longitude DFT of x (Bt, C, H, W), optional per-(b,c) affine on load
static int run_dft_forward(const ace_sht_plan& pl, const float* x, const float* sc, const float* sh, float* X, int Bt,
                           int C, hipStream_t s, unsigned* xmax = nullptr, const _Float16* xhi = nullptr,
                           const _Float16* xlo = nullptr, long sxp = 0, const unsigned* xslot = nullptr,
                           const PackFragArgs* ride = nullptr, bool* rode = nullptr, const int* mcut = nullptr) {
    DftArgs a;
    a.mcut = mcut;   // forward_pair_mcut: only when the Legendre launch that follows honours the cut
    if (rode) *rode = false;
    if (ride && rode) { a.ride = *ride; a.nride = pack_frag_blocks(*ride); a.rode = rode; }   // a weight-packing job riding in the launch (pack_frag.h)
    a.omax = xmax;
    a.xhi = xhi; a.xlo = xlo; a.sxp = sxp; a.xslot = xslot;   // the field as P-format planes instead of fp32 (FFT form only)
    a.x = xhi ? nullptr : x; a.spec_out = X; a.tc = pl.fc.p; a.ts = pl.fs.p; a.ldt = pl.Kfp; a.sc = sc; a.sh = sh;
    a.Bt = Bt; a.C = C; a.H = pl.nlat; a.W = pl.nlon; a.Mm = pl.mmax; a.no_fft = pl.sw.no_fft;
    ACE_HIP_TRY(launch_dft_forward(a, s));
    return ACE_OK;
}
static DftArgs dft_inverse_args(const ace_sht_plan& pl, const float* X, const float* bias, float* y, int Bt, int C, unsigned* ymax) {
    DftArgs a;
    a.omax = ymax;
    a.spec = X; a.y = y; a.tc = pl.gc.p; a.ts = pl.gs.p; a.ldt = pl.Kfp; a.bias = bias;
    a.Bt = Bt; a.C = C; a.H = pl.nlat; a.W = pl.nlon; a.Mm = pl.mmax; a.no_fft = pl.sw.no_fft;
    return a;
}
static int run_dft_inverse(const ace_sht_plan& pl, const float* X, const float* bias, float* y, int Bt, int C,
                           hipStream_t s, unsigned* ymax = nullptr, const int* mcut = nullptr) {
    DftArgs a = dft_inverse_args(pl, X, bias, y, Bt, C, ymax);
    a.mcut = mcut;   // inverse_pair: only behind the folded Legendre kernel
    ACE_HIP_TRY(launch_dft_inverse(a, s));
    return ACE_OK;
}
// D[l][m][n2] = sum_k wt[m][l][k] X[m][k][n2]   (sht_fix.py:134-138), batched over m, rows l >= m only
// dry: decide the route (pl.route[0]) without launching anything
static int run_legendre_forward(const ace_sht_plan& pl, const float* X, float* D, long N2, hipStream_t s,
                                const unsigned* xmax = nullptr, unsigned* dmax = nullptr, bool planes = false, bool dry = false) {
    GemmArgs g;
    g.omax = planes ? nullptr : dmax;
    g.A = pl.wt.p; g.lda = pl.Hp; g.sA = (long)pl.lmax * pl.Hp;
    g.B = X; g.ldb = N2; g.sB = (long)pl.nlat * N2;
    g.C = D; g.ldc = (long)pl.mmax * N2; g.sC = N2;
    g.M = pl.lmax; g.N = (int)N2; g.K = pl.nlat; g.nbatch = pl.mmax; g.a_kpad = pl.Hp;
    g.tri = TRI_ROWS_GE_BATCH;
    if ((pl.strip || pl.fold) && !pl.sw.no_strip && xmax) {   // register-resident strip kernels (strip_fold.hip, strip.hip)
        LegStripArgs a;
        a.B = X; a.b_kstride = N2; a.b_moff = (long)pl.nlat * N2;
        a.A = reinterpret_cast<const _Float16*>(pl.wt_frag.p); a.tile_off = reinterpret_cast<const int*>(pl.wt_off.p);
        a.ascale = pl.wt_scale; a.bmax = xmax;
        a.c_rstride = (long)pl.mmax * N2; a.c_moff = N2;
        a.N = (int)N2; a.K = pl.nlat; a.R = pl.lmax; a.nbatch = pl.mmax; a.mode = 0;
        if (planes) {
            a.Chi = reinterpret_cast<_Float16*>(D);
            a.Clo = a.Chi + (size_t)pl.lmax * pl.mmax * N2;
            a.cw = pl.wt_winf; a.cslot = dmax;
        } else {
            a.C = D; a.omax = dmax;
        }
        if (pl.fold && !pl.sw.no_fold) {   // half the contraction: sums / differences of mirror latitudes (strip_fold.hip)
            LegStripArgs f = a;
            f.A = reinterpret_cast<const _Float16*>(pl.wt_ffrag.p); f.tile_off = reinterpret_cast<const int*>(pl.wt_foff.p);
            if (pl.cut) { f.r0 = reinterpret_cast<const int*>(pl.cut_r0.p); f.kdrop = pl.kdrop; }   // the window is safe behind any producer
            if (legendre_fold_eligible(f)) {
                if (!dry) ACE_HIP_TRY(launch_legendre_fold(f, s));
                pl.route[0] = fold_route(f);
                return ACE_OK;
            }
        }
        if (pl.strip && legendre_strip_eligible(a)) {
            if (!dry) ACE_HIP_TRY(launch_legendre_strip(a, s));
            pl.route[0] = 1;
            return ACE_OK;
        }
    }
    pl.route[0] = 0;
    if (dry) return ACE_OK;
    if (planes) {
        // D as fp16 hi/lo planes in D's own layout [l][m][n2] (the buffer holds two planes instead of one fp32 tensor):
        // the dhconv contracts over n2's channel index, so this IS the v4 engine's A operand.  dmax receives the bound.
        if (!(pl.f16 && xmax && dmax && gemm_f16x3_eligible(g))) return fail(ACE_ERR_STATE, "legendre planes path not eligible");
        _Float16* Dh = reinterpret_cast<_Float16*>(D);
        _Float16* Dl = Dh + (size_t)pl.lmax * pl.mmax * N2;
        ACE_HIP_TRY(launch_gemm_f16x3_planes(g, pl.wt_hi.p, pl.wt_lo.p, pl.wt_scale, xmax, Dh, Dl, pl.wt_winf, dmax, s));
        return ACE_OK;
    }
    if (pl.f16 && xmax && gemm_f16x3_eligible(g)) {
        ACE_HIP_TRY(launch_gemm_f16x3(g, pl.wt_hi.p, pl.wt_lo.p, pl.wt_scale, 1.f, s, xmax, dmax));
        return ACE_OK;
    }
    ACE_HIP_TRY(launch_gemm(g, s));
    return ACE_OK;
}
// X[m][k][n2] = sum_{l>=m} pt[m][k][l] E[l][m][n2]   (sht_fix.py:208-219), batched over m
// dry: decide the route (pl.route[1]) without launching anything
// skip_dead (inverse_pair): the folded kernel neither stores nor computes the entries of the polar cut
static int run_legendre_inverse(const ace_sht_plan& pl, const float* E, float* X, long N2, hipStream_t s,
                                const unsigned* emax = nullptr, bool dry = false, bool skip_dead = false) {
    GemmArgs g;
    g.A = pl.pt.p; g.lda = pl.Lp; g.sA = (long)pl.nlat * pl.Lp;
    g.B = E; g.ldb = (long)pl.mmax * N2; g.sB = N2;
    g.C = X; g.ldc = N2; g.sC = (long)pl.nlat * N2;
    g.M = pl.nlat; g.N = (int)N2; g.K = pl.lmax; g.nbatch = pl.mmax; g.a_kpad = pl.Lp;
    g.tri = TRI_K_GE_BATCH;
    if ((pl.strip || pl.fold) && !pl.sw.no_strip && emax) {   // register-resident strip kernels (strip_fold.hip, strip.hip)
        LegStripArgs a;
        a.B = E; a.b_kstride = (long)pl.mmax * N2; a.b_moff = N2;
        a.A = reinterpret_cast<const _Float16*>(pl.pt_frag.p); a.tile_off = reinterpret_cast<const int*>(pl.pt_off.p);
        a.ascale = pl.pt_scale; a.bmax = emax;
        a.C = X; a.c_rstride = N2; a.c_moff = (long)pl.nlat * N2;
        a.N = (int)N2; a.K = pl.lmax; a.R = pl.nlat; a.nbatch = pl.mmax; a.mode = 1;
        if (pl.fold && !pl.sw.no_fold) {   // even / odd degrees separately, rows and mirror rows from their sum and difference
            LegStripArgs f = a;
            f.A = reinterpret_cast<const _Float16*>(pl.pt_ffrag.p); f.tile_off = reinterpret_cast<const int*>(pl.pt_foff.p);
            if (pl.cut && skip_dead) f.r0 = reinterpret_cast<const int*>(pl.cut_r0.p);
            if (legendre_fold_eligible(f)) {
                if (!dry) ACE_HIP_TRY(launch_legendre_fold(f, s));
                pl.route[1] = fold_route(f);
                return ACE_OK;
            }
        }
        if (pl.strip && legendre_strip_eligible(a)) {
            if (!dry) ACE_HIP_TRY(launch_legendre_strip(a, s));
            pl.route[1] = 1;
            return ACE_OK;
        }
    }
    pl.route[1] = 0;
    if (dry) return ACE_OK;
    if (pl.f16 && emax && gemm_f16x3_eligible(g)) {
        ACE_HIP_TRY(launch_gemm_f16x3(g, pl.pt_hi.p, pl.pt_lo.p, pl.pt_scale, 1.f, s, emax, nullptr));
        return ACE_OK;
    }
    ACE_HIP_TRY(launch_gemm(g, s));
    return ACE_OK;
}

// ---- pairing of the polar cut -------------------------------------------------------------------------------------------------
// An entry of X that its producer does not store is only safe when the consumer does not read it.  Both halves of a pair are
// decided HERE, before the pair's first kernel is enqueued, from the predicates the launches themselves use (the dry route queries):
//   forward   the FFT drops its dead stores only when the Legendre launch that follows takes the folded kernel of the same plan (whose
//             descriptor window is on whenever the plan has a cut: reading less is safe behind any producer)
//   inverse   the folded Legendre kernel skips its dead stores and tiles only when the two-level FFT follows with the cutoff; the FFT
//             drops its dead loads whenever the Legendre launch was the folded one (exact zeros there; the tile engine and the fp32
//             path leave rounding-level values, which it keeps reading)
// Everything else - matrix DFT widths, ACE_NO_FFT / ACE_NO_FOLD / ACE_NO_STRIP, strip.hip, fp32 plans - runs as without the cut.
static const int* forward_pair_mcut(const ace_sht_plan& pl, const float* X, float* D, long N2, const unsigned* xmax, unsigned* dmax,
                                    bool planes) {
    if (!pl.cut) return nullptr;
    const int before = pl.route[0];
    const int rc = run_legendre_forward(pl, X, D, N2, nullptr, xmax, dmax, planes, true);
    const bool folded = rc == ACE_OK && pl.route[0] >= 2;
    pl.route[0] = before;
    return folded ? reinterpret_cast<const int*>(pl.cut_mcut.p) : nullptr;   // (the matrix DFT kernels do not look at it)
}
struct InversePair { bool skip_dead = false; const int* mcut = nullptr; };
static InversePair inverse_pair(const ace_sht_plan& pl, const float* E, float* X, long N2, const unsigned* emax, float* y, int Bt, int C) {
    InversePair pr;
    if (!pl.cut) return pr;
    const int before = pl.route[1];
    const int rc = run_legendre_inverse(pl, E, X, N2, nullptr, emax, true);
    const bool folded = rc == ACE_OK && pl.route[1] >= 2;
    pl.route[1] = before;
    if (!folded) return pr;
    pr.mcut = reinterpret_cast<const int*>(pl.cut_mcut.p);
    pr.skip_dead = dft_inverse_fft_takes(dft_inverse_args(pl, X, nullptr, y, Bt, C, nullptr));
    return pr;
}

extern "C" int ace_sht_plan_create_ex(int nlat, int nlon, int lmax, int mmax, const char* grid, int precision,
                                      ace_sht_plan** plan) {
    if (!plan || !grid) return fail(ACE_ERR_INVALID, "null argument");
    if (precision != 0 && precision != 1) return fail(ACE_ERR_INVALID, "precision must be 0 (fp32) or 1 (f16x3)");
    Grid g;
    if (std::string(grid) == "healpix") return fail(ACE_ERR_INVALID, "'healpix' grid not supported");
    if (!parse_grid(grid, &g)) return fail(ACE_ERR_INVALID, "Unknown quadrature mode");
    std::unique_ptr<ace_sht_plan> p;
    ACE_TRY(plan_build(nlat, nlon, lmax, mmax, g, p, precision == 1));
    if (precision == 1) ACE_HIP_TRY(p->slots.alloc((size_t)2 * AMAX_SHARDS));
    *plan = p.release();
    return ACE_OK;
}
extern "C" int ace_sht_plan_create(int nlat, int nlon, int lmax, int mmax, const char* grid, ace_sht_plan** plan) {
    return ace_sht_plan_create_ex(nlat, nlon, lmax, mmax, grid, 0, plan);
}
extern "C" void ace_sht_plan_destroy(ace_sht_plan* plan) { delete plan; }
extern "C" int ace_sht_plan_dims(const ace_sht_plan* p, int* nlat, int* nlon, int* lmax, int* mmax) {
    if (!p) return fail(ACE_ERR_INVALID, "null plan");
    if (nlat) *nlat = p->nlat;
    if (nlon) *nlon = p->nlon;
    if (lmax) *lmax = p->lmax;
    if (mmax) *mmax = p->mmax;
    return ACE_OK;
}

extern "C" int ace_sht_plan_route(const ace_sht_plan* p, int* forward, int* inverse) {
    if (!p) return fail(ACE_ERR_INVALID, "null plan");
    if (forward) *forward = p->route[0];
    if (inverse) *inverse = p->route[1];
    return ACE_OK;
}

extern "C" int ace_sht_plan_cut(const ace_sht_plan* p, double* dead_share, int* kdrop) {
    if (!p) return fail(ACE_ERR_INVALID, "null plan");
    if (dead_share) *dead_share = p->cut ? p->cut_share : 0.0;
    if (kdrop) *kdrop = p->cut && p->kdrop ? 1 : 0;
    return ACE_OK;
}

extern "C" int ace_sht_forward(ace_sht_plan* p, const float* x, float* coeffs, int n, void* stream) {
    if (!p || !x || !coeffs || n <= 0) return fail(ACE_ERR_INVALID, "ace_sht_forward: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long N2 = 2L * n;
    ACE_HIP_TRY(p->X.ensure_x(((size_t)p->mmax * p->nlat + LEG_STRIP_SLACK_ROWS) * N2, p->sw.polar_poison));
    ACE_HIP_TRY(p->D.ensure(((size_t)p->lmax + LEG_STRIP_SLACK_ROWS) * p->mmax * N2));
    // coefficients with l < m are never written by the triangular Legendre stage: the layout converter writes their zeros
    // without reading the scratch (no memset)
    unsigned* xmax = nullptr;
    if (p->f16 && p->slots.p) {
        xmax = reinterpret_cast<unsigned*>(p->slots.p);
        ACE_HIP_TRY(launch_zero_u32(xmax, 2 * AMAX_SHARDS, s));
    }
    unsigned* dmax = xmax ? xmax + AMAX_SHARDS : nullptr;
    const int* mcut = forward_pair_mcut(*p, p->X.p, p->D.p, N2, xmax, dmax, false);
    ACE_TRY(run_dft_forward(*p, x, nullptr, nullptr, p->X.p, 1, n, s, xmax, nullptr, nullptr, 0, nullptr, nullptr, nullptr, mcut));
    ACE_TRY(run_legendre_forward(*p, p->X.p, p->D.p, N2, s, xmax, dmax));
    ACE_HIP_TRY(launch_spec_to_ref(p->D.p, coeffs, 1, n, p->lmax, p->mmax, s));
    return ACE_OK;
}
extern "C" int ace_sht_inverse(ace_sht_plan* p, const float* coeffs, float* x, int n, void* stream) {
    if (!p || !x || !coeffs || n <= 0) return fail(ACE_ERR_INVALID, "ace_sht_inverse: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long N2 = 2L * n;
    ACE_HIP_TRY(p->X.ensure_x(((size_t)p->mmax * p->nlat + LEG_STRIP_SLACK_ROWS) * N2, p->sw.polar_poison));
    ACE_HIP_TRY(p->D.ensure(((size_t)p->lmax + LEG_STRIP_SLACK_ROWS) * p->mmax * N2));
    unsigned* emax = nullptr;
    if (p->f16 && p->slots.p) {   // f16x3: range of the coefficients, taken by the layout converter as it reads them (round 5: a pass
        emax = reinterpret_cast<unsigned*>(p->slots.p);   // of its own over the converted tensor, 45 us at the reference's benchmark size)
        ACE_HIP_TRY(launch_zero_u32(emax, 2 * AMAX_SHARDS, s));
    }
    // the strip kernels are exactly triangular: the converter then neither reads nor writes the entries with m > l (half the tensor)
    ACE_TRY(run_legendre_inverse(*p, p->D.p, p->X.p, N2, s, emax, true));
    ACE_HIP_TRY(launch_ref_to_spec(coeffs, p->D.p, 1, n, p->lmax, p->mmax, s, emax, p->route[1] != 0));
    const InversePair pr = inverse_pair(*p, p->D.p, p->X.p, N2, emax, x, 1, n);
    ACE_TRY(run_legendre_inverse(*p, p->D.p, p->X.p, N2, s, emax, false, pr.skip_dead));
    ACE_TRY(run_dft_inverse(*p, p->X.p, nullptr, x, 1, n, s, nullptr, pr.mcut));
    return ACE_OK;
}

extern "C" int ace_sht_tables_host(int nlat, int nlon, int lmax, int mmax, const char* grid, int which,
                                   void* out_host) {
    if (!grid || !out_host) return fail(ACE_ERR_INVALID, "null argument");
    Grid g;
    if (!parse_grid(grid, &g)) return fail(ACE_ERR_INVALID, "Unknown quadrature mode");
    if (which == 2 || which == 3) {
        std::vector<double> x, w;
        quadrature(g, nlat, x, w);
        std::memcpy(out_host, (which == 2 ? x : w).data(), sizeof(double) * nlat);
        return ACE_OK;
    }
    ShtTables t;
    std::string err = build_sht_tables(nlat, nlon, lmax, mmax, g, t);
    if (!err.empty()) return fail(ACE_ERR_INVALID, err);
    float* o = static_cast<float*>(out_host);
    for (int m = 0; m < t.mmax; ++m)
        for (int l = 0; l < t.lmax; ++l)
            for (int k = 0; k < t.nlat; ++k) {
                const size_t dst = ((size_t)m * t.lmax + l) * t.nlat + k;
                if (which == 0) o[dst] = t.wt[((size_t)m * t.lmax + l) * t.Hp + k];
                else if (which == 1) o[dst] = t.pt[((size_t)m * t.nlat + k) * t.Lp + l];
                else return fail(ACE_ERR_INVALID, "unknown table id");
            }
    return ACE_OK;
}

// ---------------------------------------------------------------------------------------------
// weight preparation for the f16x3 engines: what ace_sfno_set_weight stores once per parameter and the operator-level entries
// below build on every call
// ---------------------------------------------------------------------------------------------
// A 1x1-conv weight (rows x cols): fp16 hi / lo planes of w * ascale at `pitch` = cols rounded up to 32 halves (rows rounded up to
// 16, padding zero), row-major and / or in the packed engine's A-tile order, with the norms the output bounds are made of
struct ConvOperand {
    int pitch = 0;
    DevBuf hi, lo;      // row-major planes (the on-the-fly-split engine)
    DevBuf thi, tlo;    // the same planes in the v4 engine's A-tile order
    float ascale = 1.f; // power of two that puts max|w| in [2^9, 2^10): hi and lo parts stay in fp16's normal range
    float wabs = 0.f;   // max |w|
    float winf = 0.f;   // max row sum of |w| (bounds |W x| by winf * max|x|)
};
enum { PLANES_ROWS = 1, PLANES_TILED = 2 };
// w: device weight at pitch ld (the padded library copy or a caller's dense tensor).  Buffers `o` already owns are reused.
static int prepare_conv_operand(const float* w, int rows, int cols, long ld, int forms, hipStream_t s, ConvOperand& o) {
    std::vector<float> host;
    ACE_TRY(host_copy(w, (size_t)rows * ld, s, host));
    const WeightNorms nm = weight_norms(host.data(), rows, cols, ld);
    o.wabs = nm.absmax; o.winf = nm.winf;
    o.ascale = pow2_scale(nm.absmax, 10);
    o.pitch = (cols + 31) & ~31;
    const size_t halves = (size_t)((rows + 15) / 16 * 16) * o.pitch;
    if (forms & PLANES_ROWS) {
        if (!o.hi.p) ACE_HIP_TRY(o.hi.alloc((halves + 1) / 2, false));
        if (!o.lo.p) ACE_HIP_TRY(o.lo.alloc((halves + 1) / 2, false));
        ACE_HIP_TRY(launch_split_f16(w, ld, o.hi.p, o.lo.p, o.pitch, rows, cols, o.ascale, s));
    }
    if (forms & PLANES_TILED) {
        if (!o.thi.p) ACE_HIP_TRY(o.thi.alloc((halves + 1) / 2, false));
        if (!o.tlo.p) ACE_HIP_TRY(o.tlo.alloc((halves + 1) / 2, false));
        ACE_HIP_TRY(launch_split_f16_tiled(w, ld, o.thi.p, o.tlo.p, o.pitch, rows, cols, o.ascale, s));
    }
    return ACE_OK;
}
// The conditioning convolution (C x J, dense) of a conditional layer norm as the MFMA A fragments of cln_mfma.hip, packed on the host
// (strip_pack.h) at the scale returned in *ascale
static int prepare_cln_frags(const float* w, int C, int J, hipStream_t s, DevBuf& frag, float* ascale, WeightNorms* norms) {
    std::vector<float> host;
    ACE_TRY(host_copy(w, (size_t)C * J, s, host));
    *norms = weight_norms(host.data(), C, J, J);
    *ascale = cln_frag_scale(norms->absmax);
    std::vector<uint16_t> frags(cln_frag_halves(C, J));
    pack_cln_frags(host.data(), C, J, *ascale, frags.data());
    if (!frag.p) ACE_HIP_TRY(frag.alloc((frags.size() + 1) / 2, false));
    ACE_HIP_TRY(hipMemcpy(frag.p, frags.data(), frags.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return ACE_OK;
}

// ---------------------------------------------------------------------------------------------
// building blocks
// ---------------------------------------------------------------------------------------------
extern "C" int ace_conv1x1(const float* x, const float* weight, const float* bias, float* y, int n, int cin, int cout,
                           long hw, int act, void* stream) {
    if (!x || !weight || !y || n <= 0 || cin <= 0 || cout <= 0 || hw <= 0)
        return fail(ACE_ERR_INVALID, "ace_conv1x1: bad argument");
    GemmArgs g;
    g.A = weight; g.lda = cin; g.sA = 0;
    g.B = x; g.ldb = hw; g.sB = (long)cin * hw;
    g.C = y; g.ldc = hw; g.sC = (long)cout * hw;
    g.bias = bias; g.M = cout; g.N = (int)hw; g.K = cin; g.nbatch = n; g.act = act;
    g.a_kpad = cin;  // caller's weight is unpadded: only K % stage-depth == 0 qualifies for the direct-to-LDS engine
    ACE_HIP_TRY(launch_gemm(g, static_cast<hipStream_t>(stream)));
    return ACE_OK;
}

extern "C" int ace_conv1x1_f16x3(const float* x, const float* weight, const float* bias, float* y, int n, int cin,
                                 int cout, long hw, int act, void* stream) {
    if (!x || !weight || !y || n <= 0 || cin <= 0 || cout <= 0 || hw <= 0)
        return fail(ACE_ERR_INVALID, "ace_conv1x1_f16x3: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ConvOperand w;
    ACE_TRY(prepare_conv_operand(weight, cout, cin, cin, PLANES_ROWS, s, w));
    GemmArgs g;
    g.lda = w.pitch; g.sA = 0; g.a_kpad = w.pitch;
    g.B = x; g.ldb = hw; g.sB = (long)cin * hw;
    g.C = y; g.ldc = hw; g.sC = (long)cout * hw;
    g.bias = bias; g.M = cout; g.N = (int)hw; g.K = cin; g.nbatch = n; g.act = act;
    if (!gemm_f16x3_eligible(g)) return fail(ACE_ERR_INVALID, "ace_conv1x1_f16x3: needs 16-byte aligned x and hw % 4 == 0");
    if (g.act == ACT_GELU) g.act = ACT_GELU_FAST;
    DevBuf slotbuf;
    ACE_HIP_TRY(slotbuf.alloc(AMAX_SHARDS));
    unsigned* xslot = reinterpret_cast<unsigned*>(slotbuf.p);
    ACE_HIP_TRY(launch_absmax(x, (long)n * cin * hw, xslot, s));
    ACE_HIP_TRY(launch_gemm_f16x3(g, w.hi.p, w.lo.p, w.ascale, 1.0f, s, xslot, nullptr));
    ACE_HIP_TRY(hipStreamSynchronize(s));  // temporaries are freed on return
    return ACE_OK;
}

// Bound of one source of ace_conv1x1_fused as its producer in the network would publish it, computed on the host from a copy of the
// `planes` (sample, channel) rows of hw floats at `pitch`: max |x|, or with an affine (sc, sh per plane) the bound of x sc + sh over
// each plane from its minimum and maximum, with the rounding slack of instnorm_stats_kernel.
static int fused_source_bound(const float* x, long pitch, long hw, long planes, const float* sc, const float* sh, float* bound) {
    std::vector<float> h((size_t)planes * hw);
    ACE_HIP_TRY(hipMemcpy2D(h.data(), hw * sizeof(float), x, pitch * sizeof(float), hw * sizeof(float), planes, hipMemcpyDeviceToHost));
    float b = 0.f;
    for (long p = 0; p < planes; ++p) {
        float lo = 3.0e38f, hi = -3.0e38f;
        for (long j = 0; j < hw; ++j) { const float v = h[(size_t)p * hw + j]; lo = std::min(lo, v); hi = std::max(hi, v); }
        if (sc) {
            const float a = sc[p], c = sh[p];
            const float bd = std::max(std::fabs(std::fmaf(lo, a, c)), std::fabs(std::fmaf(hi, a, c)));
            b = std::max(b, bd + 1.1920929e-7f * std::fmaf(std::fabs(a), std::max(std::fabs(lo), std::fabs(hi)), std::fabs(c)));
        } else {
            b = std::max(b, std::max(std::fabs(lo), std::fabs(hi)));
        }
    }
    *bound = b;
    return ACE_OK;
}

extern "C" int ace_conv1x1_fused(const ace_conv1x1_fused_desc* d, ace_gemm_route* route, void* stream) {
    if (!d || !d->x || !d->weight || !d->y || d->n <= 0 || d->cin <= 0 || d->cin2 < 0 || d->cout <= 0 || d->hw <= 0 ||
        d->hw > 0x7fffffffL || d->in_pitch < d->hw || d->out_pitch < d->hw || (d->cin2 > 0) != (d->x2 != nullptr) ||
        (d->in_scale != nullptr) != (d->in_shift != nullptr) || (d->res_scale != nullptr) != (d->res_shift != nullptr) ||
        (d->res_scale && !d->res) || (d->out_scale != nullptr) != (d->out_shift != nullptr) || d->act < ACT_NONE || d->act > ACT_SILU ||
        std::isnan(d->cap) || d->engine < 0 || d->engine > 2)
        return fail(ACE_ERR_INVALID, "ace_conv1x1_fused: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int K = d->cin + d->cin2, kp = (K + 31) & ~31;
    const bool al_in = d->hw % 4 == 0 && d->in_pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(d->x) & 15) == 0 &&
                       (reinterpret_cast<uintptr_t>(d->x2) & 15) == 0;
    if (d->engine == 1 && d->in_scale) return fail(ACE_ERR_INVALID, "ace_conv1x1_fused: the direct-to-LDS engine takes no input affine");
    if (d->engine != 0 && !al_in)
        return fail(ACE_ERR_INVALID, "ace_conv1x1_fused: engines 1 and 2 need hw % 4 == 0, in_pitch % 4 == 0 and 16-byte aligned x, x2");
    if (d->engine == 2 && d->in_scale && kp > 1024)
        return fail(ACE_ERR_INVALID, "ace_conv1x1_fused: the f16x3 engine keeps an input affine of at most 1024 (padded) channels");
    GemmArgs g;
    g.B = d->x; g.ldb = d->in_pitch; g.sB = (long)d->cin * d->in_pitch;
    if (d->x2) { g.B2 = d->x2; g.ldb2 = d->in_pitch; g.sB2 = (long)d->cin2 * d->in_pitch; g.K1 = d->cin; }
    g.bsc = d->in_scale; g.bsh = d->in_shift; g.sbs = d->in_scale ? K : 0;
    g.C = d->y; g.ldc = d->out_pitch; g.sC = (long)d->cout * d->out_pitch;
    g.bias = d->bias;
    if (d->res) { g.R = d->res; g.ldr = d->in_pitch; g.sR = (long)d->cout * d->in_pitch; }
    g.rsc = d->res_scale; g.rsh = d->res_shift; g.srs = d->res_scale ? d->cout : 0;
    g.osc = d->out_scale; g.osh = d->out_shift;
    g.M = d->cout; g.N = (int)d->hw; g.K = K; g.nbatch = d->n; g.act = d->act; g.cap = d->cap;
    g.omax = d->out_absmax;
    if (d->out_absmax) ACE_HIP_TRY(launch_zero_u32(d->out_absmax, AMAX_SHARDS, s));
    DevBuf wpad, slots;
    ConvOperand w;
    GemmRoute r;
    if (d->engine == 0) {
        g.A = d->weight; g.lda = K; g.a_kpad = 0;   // a caller's unpadded weight: never the direct-to-LDS kernel
        r = gemm_route(g, false);
        ACE_HIP_TRY(launch_gemm(g, s));
    } else if (d->engine == 1) {
        ACE_HIP_TRY(wpad.alloc((size_t)d->cout * kp, true));
        ACE_HIP_TRY(hipMemcpy2DAsync(wpad.p, kp * sizeof(float), d->weight, K * sizeof(float), K * sizeof(float), d->cout,
                                 hipMemcpyDeviceToDevice, s));
        g.A = wpad.p; g.lda = kp; g.a_kpad = kp;
        r = gemm_route(g, false);
        if (r.family != 2) return fail(ACE_ERR_INVALID, "ace_conv1x1_fused: the launch does not qualify for the direct-to-LDS engine");
        ACE_HIP_TRY(launch_gemm(g, s));
    } else {
        ACE_TRY(prepare_conv_operand(d->weight, d->cout, K, K, PLANES_ROWS, s, w));
        g.lda = kp; g.sA = 0; g.a_kpad = kp;
        if (!gemm_f16x3_eligible(g)) return fail(ACE_ERR_INVALID, "ace_conv1x1_fused: the launch does not qualify for the f16x3 engine");
        // range slots of the two sources (word 0 of 64 carries the bound, the others stay zero)
        std::vector<float> sc, sh;
        if (d->in_scale) {
            sc.resize((size_t)d->n * K); sh.resize(sc.size());
            ACE_HIP_TRY(hipMemcpy(sc.data(), d->in_scale, sc.size() * sizeof(float), hipMemcpyDeviceToHost));
            ACE_HIP_TRY(hipMemcpy(sh.data(), d->in_shift, sh.size() * sizeof(float), hipMemcpyDeviceToHost));
        }
        float bound[2] = {0.f, 0.f};
        for (int b = 0; b < d->n; ++b) {   // per sample: the affine's rows of a source are not contiguous over samples
            for (int src = 0; src < (d->x2 ? 2 : 1); ++src) {
                const int c0 = src ? d->cin : 0, nc = src ? d->cin2 : d->cin;
                const float* base = (src ? d->x2 : d->x) + (long)b * nc * d->in_pitch;
                float bb = 0.f;
                ACE_TRY(fused_source_bound(base, d->in_pitch, d->hw, nc, d->in_scale ? sc.data() + (size_t)b * K + c0 : nullptr,
                                           d->in_scale ? sh.data() + (size_t)b * K + c0 : nullptr, &bb));
                bound[src] = std::max(bound[src], bb);
            }
        }
        ACE_HIP_TRY(slots.alloc(2 * AMAX_SHARDS, true));
        unsigned* xslot = reinterpret_cast<unsigned*>(slots.p);
        ACE_HIP_TRY(hipMemcpy(xslot, &bound[0], sizeof(float), hipMemcpyHostToDevice));
        ACE_HIP_TRY(hipMemcpy(xslot + AMAX_SHARDS, &bound[1], sizeof(float), hipMemcpyHostToDevice));
        if (g.act == ACT_GELU) g.act = ACT_GELU_FAST;   // as the network runs this engine
        r = gemm_route(g, true);
        g.omax = nullptr;
        ACE_HIP_TRY(launch_gemm_f16x3(g, w.hi.p, w.lo.p, w.ascale, 1.0f, s, xslot, d->out_absmax, d->x2 ? xslot + AMAX_SHARDS : nullptr));
    }
    if (route) { route->family = r.family; route->tile = r.tile; }
    ACE_HIP_TRY(hipStreamSynchronize(s));  // temporaries are freed on return
    return ACE_OK;
}

// The longitude DFT stage as an operator: fills a DftArgs from the descriptor and the plan and calls launch_dft_forward /
// launch_dft_inverse - with no_fft set for engine 0, and only after dft_*_fft_takes has said yes for engine 1, so that the launch
// takes the form the caller named or none.
extern "C" int ace_dft_stage(ace_sht_plan* plan, const ace_dft_stage_desc* d, ace_dft_route* route, void* stream) {
    if (!plan || !d) return fail(ACE_ERR_INVALID, "ace_dft_stage: null plan or descriptor");
    if (d->engine < 0 || d->engine > 1 || d->bt <= 0 || d->c <= 0 || (d->inverse != 0 && d->inverse != 1))
        return fail(ACE_ERR_INVALID, "ace_dft_stage: bad argument");
    const bool planes = d->xhi || d->xlo || d->xslot;
    if (d->inverse) {
        if (!d->spec || !d->y) return fail(ACE_ERR_INVALID, "ace_dft_stage: the inverse transform needs spec and y");
        if (d->x || planes || d->in_scale || d->in_shift || d->spec_out || d->ride_weight)
            return fail(ACE_ERR_INVALID, "ace_dft_stage: a forward operand given to the inverse transform");
    } else {
        if (!d->spec_out || (!d->x && !planes)) return fail(ACE_ERR_INVALID, "ace_dft_stage: the forward transform needs x (or the planes) and spec_out");
        if (d->spec || d->y || d->bias) return fail(ACE_ERR_INVALID, "ace_dft_stage: an inverse operand given to the forward transform");
        if ((d->in_scale != nullptr) != (d->in_shift != nullptr)) return fail(ACE_ERR_INVALID, "ace_dft_stage: in_scale and in_shift come together");
        if (planes) {
            if (d->x) return fail(ACE_ERR_INVALID, "ace_dft_stage: x and the planes are alternatives");
            if (d->engine != 1) return fail(ACE_ERR_INVALID, "ace_dft_stage: the matrix form takes no planes input");
            if (!d->xhi || !d->xlo || !d->xslot || d->c % 8 != 0 || d->sxp < (long)d->c * plan->nlat * plan->nlon)
                return fail(ACE_ERR_INVALID, "ace_dft_stage: the planes input needs xhi, xlo, xslot, c % 8 == 0 and sxp >= c H W");
        }
    }
    if (d->engine == 0 && d->mcut) return fail(ACE_ERR_INVALID, "ace_dft_stage: the matrix form does not look at mcut");
    if (d->ride_weight) {
        if (d->engine != 1) return fail(ACE_ERR_INVALID, "ace_dft_stage: the matrix form takes no rider job");
        if (!d->ride_dst || !d->ride_dst_alone) return fail(ACE_ERR_INVALID, "ace_dft_stage: a rider job needs ride_dst and ride_dst_alone");
    }
    if ((double)plan->nlat * d->bt * d->c * 2.0 * std::max(plan->mmax, plan->nlon) >= 2147483647.0)
        return fail(ACE_ERR_INVALID, "ace_dft_stage: a test entry for operands below 2^31 elements");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DftArgs a;
    a.Bt = d->bt; a.C = d->c; a.H = plan->nlat; a.W = plan->nlon; a.Mm = plan->mmax; a.ldt = plan->Kfp;
    a.no_fft = d->engine == 0;
    a.mcut = d->mcut;
    a.omax = d->out_absmax;
    bool rode = false;
    if (d->inverse) {
        a.spec = d->spec; a.y = d->y; a.bias = d->bias; a.tc = plan->gc.p; a.ts = plan->gs.p;
        if (d->engine == 1 && !dft_inverse_fft_takes(a))
            return fail(ACE_ERR_INVALID, "ace_dft_stage: the FFT form takes W in {16, 24, 48, 360, 720, 1440} and a 16-byte aligned y");
    } else {
        a.x = d->x; a.xhi = static_cast<const _Float16*>(d->xhi); a.xlo = static_cast<const _Float16*>(d->xlo); a.sxp = d->sxp; a.xslot = d->xslot;
        a.sc = d->in_scale; a.sh = d->in_shift; a.spec_out = d->spec_out; a.tc = plan->fc.p; a.ts = plan->fs.p;
        if (d->engine == 1 && !dft_forward_fft_takes(a))
            return fail(ACE_ERR_INVALID, "ace_dft_stage: the FFT form takes W in {16, 24, 48, 360, 720, 1440} and a 16-byte aligned x");
        if (d->ride_weight) {
            PackFragArgs q;
            q.W = d->ride_weight; q.ldw = d->ride_i; q.O = d->ride_o; q.I = d->ride_i; q.order = d->ride_order;
            q.scale_static = d->ride_scale; q.dst = static_cast<_Float16*>(d->ride_dst); q.nsamples = 1;
            if (d->ride_o <= 0 || d->ride_i <= 0 || !pack_frag_args_ok(q)) return fail(ACE_ERR_INVALID, "ace_dft_stage: the rider job needs ride_o % 32 == 0 and ride_i % 16 == 0 (order 1: % 32)");
            a.ride = q; a.nride = pack_frag_blocks(q); a.rode = &rode;
            ACE_HIP_TRY(launch_pack_conv_frag(q.W, q.ldw, q.O, q.I, q.order, nullptr, 0.f, q.scale_static, nullptr, d->ride_dst_alone, 0, 1, s));
        }
    }
    if (d->out_absmax) ACE_HIP_TRY(launch_zero_u32(d->out_absmax, AMAX_SHARDS, s));
    ACE_HIP_TRY(d->inverse ? launch_dft_inverse(a, s) : launch_dft_forward(a, s));
    if (route) {
        const long cols = (long)a.H * a.Bt * a.C;
        if (d->engine == 1) {
            const int R = dft_fft_rows(a.W, d->inverse != 0), gx = (a.C + R - 1) / R;
            route->form = 2; route->rows = R;
            route->units = gx * (a.H + (rode ? (a.nride + gx - 1) / gx : 0));
        } else if (d->inverse) {
            route->form = dft_inverse_matrix_vs(a) ? 1 : 0; route->rows = 0;
            route->units = (int)((cols + 127) / 128) * ((a.W / 2 + 1 + 63) / 64);
        } else {
            route->form = dft_forward_matrix_vx(a) ? 1 : 0; route->rows = 0;
            route->units = ((a.Mm + 63) / 64) * (int)((cols + 127) / 128);
        }
        route->rode = rode ? 1 : 0;
    }
    ACE_HIP_TRY(hipStreamSynchronize(s));
    return ACE_OK;
}

// The reference's MLP (fme/ace/models/modulus/layers.py:97-137: 1x1 conv -> activation -> 1x1 conv, drop_rate 0) on
// the packed-operand f16x3 engine: x is split once into P format, fc1 writes the hidden activation straight in
// P format (bound-scaled), fc2 consumes it by DMA.  Operator-level entry for tests / benchmarks.
extern "C" int ace_mlp_f16x3(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y,
                             int n, int cin, int hid, int cout, long hw, int act, void* stream) {
    if (!x || !w1 || !w2 || !y || n <= 0 || cin <= 0 || hid <= 0 || cout <= 0 || hw <= 0)
        return fail(ACE_ERR_INVALID, "ace_mlp_f16x3: bad argument");
    if (cin % 8 != 0 || hid % 8 != 0 || hw % 4 != 0)
        return fail(ACE_ERR_INVALID, "ace_mlp_f16x3: needs cin % 8 == 0, hid % 8 == 0, hw % 4 == 0");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ConvOperand p1, p2;
    ACE_TRY(prepare_conv_operand(w1, hid, cin, cin, PLANES_TILED, s, p1));
    ACE_TRY(prepare_conv_operand(w2, cout, hid, hid, PLANES_TILED, s, p2));
    float b1max = 0.f;
    if (b1) {
        std::vector<float> hb;
        ACE_TRY(host_copy(b1, (size_t)hid, s, hb));
        b1max = host_absmax(hb);
    }
    DevBuf slots, xp, up;
    ACE_HIP_TRY(slots.alloc(2 * AMAX_SHARDS, true));
    ACE_HIP_TRY(xp.alloc((size_t)n * cin * hw, true));   // two fp16 planes = one fp32 tensor's bytes
    ACE_HIP_TRY(up.alloc((size_t)n * hid * hw, true));
    unsigned* xslot = reinterpret_cast<unsigned*>(slots.p);
    unsigned* uslot = xslot + AMAX_SHARDS;
    _Float16* xh = reinterpret_cast<_Float16*>(xp.p);
    _Float16* xl = xh + (size_t)n * cin * hw;
    _Float16* uh = reinterpret_cast<_Float16*>(up.p);
    _Float16* ul = uh + (size_t)n * hid * hw;
    ACE_HIP_TRY(launch_absmax(x, (long)n * cin * hw, xslot, s));
    ACE_HIP_TRY(launch_pack_pformat(x, hw, (long)cin * hw, cin, (int)hw, n, nullptr, nullptr, 0, xslot, xh, xl, hw,
                                (long)cin * hw, s));
    Gemm4Args a;
    a.Ahi = reinterpret_cast<const _Float16*>(p1.thi.p); a.Alo = reinterpret_cast<const _Float16*>(p1.tlo.p);
    a.lda = p1.pitch; a.ascale = p1.ascale; a.a_tiled = 1;
    a.Bhi = xh; a.Blo = xl; a.ldn = hw; a.sB = (long)cin * hw; a.bmax = xslot;
    a.Chi = uh; a.Clo = ul; a.ldnc = hw; a.sCp = (long)hid * hw; a.cw = p1.winf; a.cb = b1max; a.cslot = uslot;
    a.bias = b1; a.M = hid; a.N = (int)hw; a.K = cin; a.nbatch = n;
    a.act = act == ACT_GELU ? ACT_GELU_FAST : act;
    ACE_HIP_TRY(launch_gemm_f16x3_packed(a, s));
    Gemm4Args b;
    b.Ahi = reinterpret_cast<const _Float16*>(p2.thi.p); b.Alo = reinterpret_cast<const _Float16*>(p2.tlo.p);
    b.lda = p2.pitch; b.ascale = p2.ascale; b.a_tiled = 1;
    b.Bhi = uh; b.Blo = ul; b.ldn = hw; b.sB = (long)hid * hw; b.bmax = uslot;
    b.C = y; b.ldc = hw; b.sC = (long)cout * hw;
    b.bias = b2; b.M = cout; b.N = (int)hw; b.K = hid; b.nbatch = n; b.act = ACT_NONE;
    ACE_HIP_TRY(launch_gemm_f16x3_packed(b, s));
    ACE_HIP_TRY(hipStreamSynchronize(s));  // temporaries are freed on return
    return ACE_OK;
}

// the work list of a dhconv_strip launch (dhconv_build_units) on the device
static hipError_t upload_dhconv_units(int L, int Mrows, int trimul, int C, DevBuf& buf, int* per_xcd) {
    std::vector<int> u;
    *per_xcd = dhconv_build_units(L, Mrows, trimul, C, u);
    hipError_t e = buf.alloc(u.size(), false);
    if (e != hipSuccess) return e;
    return hipMemcpy(buf.p, u.data(), u.size() * sizeof(int), hipMemcpyHostToDevice);
}

// _contract_dhconv (fme/ace/models/modulus/contractions.py:183-195): einsum("bixy,iox->boxy") on complex coefficients, on the
// kernel the network uses (dhconv_strip.hip: compensated fp16, filter streamed once).  Operator-level entry for tests and
// micro-benchmarks: converts to the internal layouts, prepares the filter planes on every call and synchronises.
extern "C" int ace_dhconv_f16x3(const float* coeffs, const float* weight, float* out, int n, int c, int L, int Mm, void* stream) {
    ace_dhconv_desc d = {};
    d.coeffs = coeffs; d.weight = weight; d.out = out;
    d.n = n; d.c = c; d.L = L; d.Mm = Mm; d.groups = 1; d.storage = 0;
    return ace_dhconv_strip_op(&d, nullptr, stream);
}

// The same contraction in every form dhconv_strip.hip has: dense or block-diagonal filter, the latter as dense planes (zero blocks
// skipped) or as the diagonal blocks alone; optional range maximum of the output.  The launch is the network's (dhconv_strip_args):
// the same planes, slots, work list and kernel - only the operands are prepared here, on every call.
extern "C" int ace_dhconv_strip_op(const ace_dhconv_desc* d, ace_dhconv_route* route, void* stream) {
    if (!d || !d->coeffs || !d->weight || !d->out || d->n <= 0 || d->c <= 0 || d->L <= 0 || d->Mm <= 0 || std::isnan(d->e_fill))
        return fail(ACE_ERR_INVALID, "ace_dhconv_strip_op: bad argument");
    const int n = d->n, c = d->c, L = d->L, Mm = d->Mm, G = d->groups;
    if (c % 128 != 0) return fail(ACE_ERR_INVALID, "ace_dhconv_strip_op: needs channels % 128 == 0");
    if (G < 1 || c % G != 0) return fail(ACE_ERR_INVALID, "ace_dhconv_strip_op: groups must divide channels");
    if (d->storage != 0 && d->storage != 1) return fail(ACE_ERR_INVALID, "ace_dhconv_strip_op: storage is 0 (dense planes) or 1 (diagonal blocks)");
    const bool native = d->storage == 1;
    if (native && !dhconv_native_groups_ok(c, G))
        return fail(ACE_ERR_INVALID, "ace_dhconv_strip_op: diagonal-block storage needs groups > 1 and channels / groups in {32, 64, 128} or a multiple of 128");
    if ((double)L * Mm * 2.0 * n * c >= 2147483647.0 || (double)L * 2.0 * c * c >= 2147483647.0)
        return fail(ACE_ERR_INVALID, "ace_dhconv_strip_op: a test entry for operands below 2^31 elements");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int cg = c / G;
    const long N2 = 2L * n * c;
    const size_t spec = (size_t)L * Mm * N2;
    const long wnumel = native || G > 1 ? (long)G * L * cg * cg * 2 : (long)c * c * L * 2;   // the caller's tensor
    DevBuf D, Dp, E, Wd, Wh, Wl, slots;
    ACE_HIP_TRY(D.alloc(spec, true));
    ACE_HIP_TRY(Dp.alloc(spec, true));          // hi | lo planes: two halves per element = one float
    ACE_HIP_TRY(E.alloc(spec, d->e_fill == 0.f));   // rows m > l are never written: they keep e_fill
    if (d->e_fill != 0.f) {
        unsigned bits;
        std::memcpy(&bits, &d->e_fill, 4);
        ACE_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(E.p), (int)bits, spec, s));
    }
    ACE_HIP_TRY(slots.alloc(2 * AMAX_SHARDS, true));
    const int kstore = native ? cg : c;
    const size_t wh = (size_t)L * 2 * kstore * c;
    ACE_HIP_TRY(Wh.alloc((wh + 1) / 2, false));
    ACE_HIP_TRY(Wl.alloc((wh + 1) / 2, false));
    unsigned* dslot = reinterpret_cast<unsigned*>(slots.p);
    unsigned* wslot = dslot + AMAX_SHARDS;
    ACE_HIP_TRY(launch_ref_to_spec(d->coeffs, D.p, n, c, L, Mm, s));
    ACE_HIP_TRY(launch_absmax(D.p, (long)spec, dslot, s));
    ACE_HIP_TRY(launch_absmax(d->weight, wnumel, wslot, s));
    float dmx = 0.f, wmx = 0.f;
    ACE_TRY(read_range_slot(dslot, s, &dmx));
    ACE_TRY(read_range_slot(wslot, s, &wmx));
    // The planes are scaled by 2^e and the kernel undoes 2^e from the slot: both from range_exponent().  (Until the range cases of
    // tests/test_gpu_dhconv_strip.py this line took pow2_scale(dmx, 12), which has no clamp where the kernel's exponent has one: beyond
    // it the result was off by a power of two.)  Where the clamp acts the planes do not hold max |coeffs| in [2^11, 2^12) and the
    // low end loses bits the 2e-6 bar needs: refused, not computed.
    bool clamped = false;
    const float dscale = std::ldexp(1.0f, range_exponent(dmx, &clamped)), wscale = pow2_scale(wmx, 10);
    if (clamped) return fail(ACE_ERR_INVALID, "ace_dhconv_strip_op: max |coeffs| outside [2^-89, 2^112): the planes' power-of-two scale is clamped there");
    ACE_HIP_TRY(launch_split_f16(D.p, N2, Dp.p, reinterpret_cast<_Float16*>(Dp.p) + spec, N2, (long)L * Mm, (int)N2, dscale, s));
    if (native) {
        ACE_HIP_TRY(launch_pack_dhconv_f16g(d->weight, Wh.p, Wl.p, c, G, L, wscale, s));
    } else if (G > 1) {
        ACE_HIP_TRY(Wd.alloc((size_t)c * c * L * 2, false));
        ACE_HIP_TRY(launch_csfno_weight_to_dense(d->weight, Wd.p, c, G, L, s));
        ACE_HIP_TRY(launch_pack_dhconv_f16c(Wd.p, Wh.p, Wl.p, c, c, L, wscale, s));
    } else {
        ACE_HIP_TRY(launch_pack_dhconv_f16c(d->weight, Wh.p, Wl.p, c, c, L, wscale, s));
    }
    DhconvStripArgs ds;
    ds.Dhi = reinterpret_cast<const _Float16*>(Dp.p); ds.Dlo = ds.Dhi + spec;
    ds.sD = (long)Mm * N2; ds.amax = dslot;
    ds.Whi = reinterpret_cast<const _Float16*>(Wh.p); ds.Wlo = reinterpret_cast<const _Float16*>(Wl.p);
    ds.sW = (long)2 * kstore * c; ds.bscale = wscale;
    ds.E = E.p; ds.sE = (long)Mm * N2; ds.omax = d->out_absmax;
    ds.C = c; ds.L = L; ds.Mrows = Mm * n; ds.trimul = n;
    ds.groups = G;
    if (native) ds.kstore = kstore;
    std::vector<int> u;
    ds.units_per_xcd = dhconv_build_units(L, Mm * n, n, c, u);
    DevBuf units;
    ACE_HIP_TRY(units.alloc(u.size(), false));
    ACE_HIP_TRY(hipMemcpy(units.p, u.data(), u.size() * sizeof(int), hipMemcpyHostToDevice));
    ds.units = reinterpret_cast<const int*>(units.p);
    if (!dhconv_strip_eligible(ds)) return fail(ACE_ERR_INVALID, "ace_dhconv_strip_op: shape not covered by dhconv_strip.hip");
    if (d->out_absmax) ACE_HIP_TRY(launch_zero_u32(d->out_absmax, AMAX_SHARDS, s));
    ACE_HIP_TRY(launch_dhconv_strip(ds, s));
    ACE_HIP_TRY(launch_spec_to_ref(E.p, d->out, n, c, L, Mm, s, true));   // entries with m > l: what E held, i.e. e_fill unless the kernel stored there
    if (route) {
        const bool skip = G > 1 && (cg % 128 == 0 || 128 % cg == 0);
        *route = ace_dhconv_route{};
        route->storage = native ? 1 : 0;
        route->kspan = skip ? std::max(cg, 128) : c;
        route->units_per_xcd = ds.units_per_xcd;
        std::map<std::pair<int, int>, int> chunks;
        for (size_t k = 0; k + 3 < u.size(); k += 4) {
            const int rows = u[k + 3];
            if (rows <= 0) continue;
            ++route->units[(rows + 31) / 32 - 1];
            route->max_chunks = std::max(route->max_chunks, ++chunks[{u[k], u[k + 1]}]);
        }
    }
    ACE_HIP_TRY(hipStreamSynchronize(s));
    return ACE_OK;
}

extern "C" int ace_instance_norm(const float* x, const float* gamma, const float* beta, float eps, float* y, int n,
                                 int c, long hw, void* stream) {
    if (!x || !y || n <= 0 || c <= 0 || hw <= 0) return fail(ACE_ERR_INVALID, "ace_instance_norm: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* st = nullptr;
    ACE_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&st), sizeof(float) * 2 * n * c));
    hipError_t e = launch_instnorm_stats(x, gamma, beta, eps, n, c, hw, st, st + (size_t)n * c, s);
    if (e == hipSuccess) e = launch_rowaffine_add(x, st, st + (size_t)n * c, nullptr, nullptr, nullptr, y, (long)n * c, hw, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(st);
    ACE_HIP_TRY(e);
    return ACE_OK;
}

extern "C" int ace_conditional_layer_norm(const float* x, const float* noise, const float* gamma, const float* beta,
                                          const float* w_scale, const float* w_bias, float eps, float* y, int n, int c,
                                          int noise_dim, long hw, void* stream) {
    if (!x || !y || n <= 0 || c <= 0 || hw <= 0 || (w_scale && (!w_bias || !noise || noise_dim <= 0)))
        return fail(ACE_ERR_INVALID, "ace_conditional_layer_norm: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DevBuf stats;
    ACE_HIP_TRY(stats.alloc((size_t)2 * n * hw, false));
    ACE_HIP_TRY(launch_cond_layer_norm(x, noise, gamma, beta, w_scale, w_bias, eps, stats.p, y, n, c, noise_dim, hw, s));
    ACE_HIP_TRY(hipStreamSynchronize(s));
    return ACE_OK;
}

extern "C" int ace_conditional_layer_norm_f16x3(const float* x, const float* noise, const float* gamma, const float* beta,
                                                const float* w_scale, const float* w_bias, float eps, float* y, int n, int c,
                                                int noise_dim, long hw, void* stream) {
    if (!x || !y || n <= 0 || c <= 0 || hw <= 0 || (w_scale && (!w_bias || !noise || noise_dim <= 0)))
        return fail(ACE_ERR_INVALID, "ace_conditional_layer_norm_f16x3: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ClnMfmaArgs a;
    a.x = x; a.y = y; a.sx = (long)c * hw; a.C = c; a.HW = hw; a.nbatch = n; a.eps = eps; a.gamma = gamma; a.beta = beta;
    DevBuf fs, fb, cslot;
    {   // the shape requirement, checked BEFORE any weight is copied or packed (same predicate as the launch: the conditioning
        // operands are stood in for by the input pointer, only their presence matters to it)
        ClnMfmaArgs probe = a;
        if (w_scale) {
            probe.cond = noise; probe.scond = (long)noise_dim * hw; probe.J = noise_dim;
            probe.As = probe.Ab = reinterpret_cast<const _Float16*>(x); probe.cslot = reinterpret_cast<const unsigned*>(x);
        }
        if (!cln_mfma_eligible(probe))
            return fail(ACE_ERR_INVALID, "ace_conditional_layer_norm_f16x3: needs c % 256 == 0 (c <= 1024), hw % 4 == 0 (c > 512: hw % 32 == 0), noise_dim <= 128");
    }
    if (w_scale) {   // the two conditioning convolutions as fragments + the conditioning field's bound
        WeightNorms nm;
        ACE_TRY(prepare_cln_frags(w_scale, c, noise_dim, s, fs, &a.ascale_s, &nm));
        ACE_TRY(prepare_cln_frags(w_bias, c, noise_dim, s, fb, &a.ascale_b, &nm));
        ACE_HIP_TRY(cslot.alloc(AMAX_SHARDS));
        ACE_HIP_TRY(launch_absmax(noise, (long)n * noise_dim * hw, reinterpret_cast<unsigned*>(cslot.p), s));
        a.cond = noise; a.scond = (long)noise_dim * hw; a.J = noise_dim; a.cslot = reinterpret_cast<const unsigned*>(cslot.p);
        a.As = reinterpret_cast<const _Float16*>(fs.p); a.Ab = reinterpret_cast<const _Float16*>(fb.p);
    }
    if (!cln_mfma_eligible(a))
        return fail(ACE_ERR_INVALID, "ace_conditional_layer_norm_f16x3: needs c % 256 == 0 (c <= 1024), hw % 4 == 0 (c > 512: hw % 32 == 0), noise_dim <= 128");
    ACE_HIP_TRY(launch_cln_mfma(a, s));
    ACE_HIP_TRY(hipStreamSynchronize(s));
    return ACE_OK;
}

extern "C" int ace_pack_normalize(const float* const* srcs, const long* strides, const float* mean, const float* std_,
                                  float* dst, int batch, int nch, long hw, void* stream) {
    if (!srcs || !strides || !mean || !std_ || !dst) return fail(ACE_ERR_INVALID, "ace_pack_normalize: null argument");
    ACE_HIP_TRY(launch_pack_normalize(srcs, strides, mean, std_, dst, batch, nch, hw, static_cast<hipStream_t>(stream)));
    return ACE_OK;
}
extern "C" int ace_unpack_denormalize(const float* src, const float* mean, const float* std_, float* const* dsts,
                                      const long* strides, int batch, int nch, long hw, void* stream) {
    if (!src || !strides || !mean || !std_ || !dsts)
        return fail(ACE_ERR_INVALID, "ace_unpack_denormalize: null argument");
    ACE_HIP_TRY(launch_unpack_denormalize(src, mean, std_, dsts, strides, batch, nch, hw, static_cast<hipStream_t>(stream)));
    return ACE_OK;
}

// global-mean removal (gmr.hip): the argument checks on the host, before the first HIP call
static bool gmr_bad_shape(int batch, int nch, int K, long hw) {
    return batch < 1 || batch > 65535 || nch < 1 || nch > 65535 || K < 1 || K > 65535 || hw < 1 || gmr_chunks(hw) > 0x7fffffffL;
}
extern "C" long ace_gmr_chunks(long hw) { return gmr_chunks(hw); }
extern "C" int ace_gmr_partials(const float* const* srcs, const long* strides, const int* plane_idx, int nsrc, double* partials,
                                int batch, int K, long hw, void* stream) {
    if (gmr_bad_shape(batch, nsrc, K, hw)) return fail(ACE_ERR_INVALID, "ace_gmr_partials: bad shape");
    if (!srcs || !strides || !plane_idx || !partials) return fail(ACE_ERR_INVALID, "ace_gmr_partials: null argument");
    ACE_HIP_TRY(launch_gmr_partials(srcs, strides, plane_idx, nsrc, partials, batch, K, hw, static_cast<hipStream_t>(stream)));
    return ACE_OK;
}
extern "C" int ace_gmr_sample_means(const float* const* srcs, const long* strides, const int* plane_idx, int nsrc,
                                    double* partials, float* means, int batch, int K, long hw, void* stream) {
    if (gmr_bad_shape(batch, nsrc, K, hw)) return fail(ACE_ERR_INVALID, "ace_gmr_sample_means: bad shape");
    if (!srcs || !strides || !plane_idx || !partials || !means)
        return fail(ACE_ERR_INVALID, "ace_gmr_sample_means: null argument");
    ACE_HIP_TRY(launch_gmr_partials(srcs, strides, plane_idx, nsrc, partials, batch, K, hw, static_cast<hipStream_t>(stream)));
    ACE_HIP_TRY(launch_gmr_sample_means(partials, means, batch, K, hw, static_cast<hipStream_t>(stream)));
    return ACE_OK;
}
extern "C" int ace_gmr_pack_normalize(const float* const* srcs, const long* strides, const float* mean, const float* std_,
                                      const int* shift_idx, const double* partials, const float* clim_mean,
                                      const int* extra_idx, const float* extra_std, float* dst, float* shift, int batch, int nin,
                                      int nextra, int K, long hw, void* stream) {
    if (gmr_bad_shape(batch, nin, K, hw) || K > nin || nextra < 0 || nin + nextra > 65535)
        return fail(ACE_ERR_INVALID, "ace_gmr_pack_normalize: bad shape (1 <= K <= nin, nextra >= 0)");
    if (!srcs || !strides || !mean || !std_ || !shift_idx || !partials || !clim_mean || !dst || !shift ||
        (nextra > 0 && (!extra_idx || !extra_std)))
        return fail(ACE_ERR_INVALID, "ace_gmr_pack_normalize: null argument");
    ACE_HIP_TRY(launch_gmr_pack_normalize(srcs, strides, mean, std_, shift_idx, partials, clim_mean, extra_idx, extra_std, dst, shift,
                                      batch, nin, nextra, K, hw, static_cast<hipStream_t>(stream)));
    return ACE_OK;
}
extern "C" int ace_gmr_unpack_denormalize(const float* src, const float* mean, const float* std_, float* const* dsts,
                                          const long* strides, const int* shift_idx, const float* shift, int batch, int nch, int K,
                                          long hw, void* stream) {
    if (gmr_bad_shape(batch, nch, K, hw)) return fail(ACE_ERR_INVALID, "ace_gmr_unpack_denormalize: bad shape");
    if (!src || !mean || !std_ || !dsts || !strides || !shift_idx || !shift)
        return fail(ACE_ERR_INVALID, "ace_gmr_unpack_denormalize: null argument");
    ACE_HIP_TRY(launch_gmr_unpack_denormalize(src, mean, std_, dsts, strides, shift_idx, shift, batch, nch, K, hw,
                                          static_cast<hipStream_t>(stream)));
    return ACE_OK;
}

// ---------------------------------------------------------------------------------------------
// the network
// ---------------------------------------------------------------------------------------------
// What a parameter is to the forward: decides which derived operands ace_sfno_set_weight stores with the library copy
enum ParamRole {
    ROLE_PLAIN,      // library copy only (the (H, W) affine fields of "layer_norm")
    ROLE_VECTOR,     // biases and per-channel norm affines: + max |value|, the bound term of the P-format producers
    ROLE_POS_EMBED,  // + its bound as a range slot (the residual of the last encoder convolution)
    ROLE_ENC_CONV, ROLE_ENC_LAST, ROLE_DEC_CONV, ROLE_SKIP, ROLE_FC1, ROLE_FC2,   // 1x1 convolutions: + planes and norms, some + fragments
    ROLE_FILTER,     // spectral filter: + the contraction's operand (native, compact or expanded)
    ROLE_CLN_COND    // conditioning convolution of a conditional layer norm: + cln_mfma.hip's fragments
};
struct Weight : ConvOperand {   // (the ConvOperand part: conv roles of an f16x3 net; ascale / wabs / winf also of ROLE_CLN_COND)
    std::string name;
    ParamRole role = ROLE_PLAIN;
    long numel = 0;
    DevBuf buf;    // library copy (reference layout; conv weights: rows zero-padded to `pitch`)
    bool set = false;
    int block = -1;
    long hw = 0;         // pixels of the grid the role's consumer runs on (block i: block_out_pixels; encoder / decoder: the data grid)
    long ext_numel = 0;  // grouped csfno filter: numel of the caller's tensor, which differs from the (dense) library copy's
    int rows = 0, cols = 0;  // conv weights (rows x cols)
    DevBuf frag0;       // packed MFMA A fragments: static weights of conv_ws.hip / conv_wl.hip, or of cln_mfma.hip (ROLE_CLN_COND)
    float absmax = 0.f; // ROLE_VECTOR: max |value|
};

struct GraphKey {
    const float* in; float* out; int batch;
    bool operator<(const GraphKey& o) const { return std::tie(in, out, batch) < std::tie(o.in, o.out, o.batch); }
};

struct ace_sfno {
    ace_sfno_config cfg;
    int H = 0, W = 0, C = 0, L = 0, Mm = 0, hid = 0, Bmax = 1;
    long HW = 0;
    // scale_factor != 1 (sfnonet.py:467-515): the blocks between the first filter's inverse transform and the last filter's work on
    // the (nlat / sf) x (nlon / sf) Gauss-Legendre grid, HWs pixels
    long HWs = 0;
    int Hs = 0, Ws = 0;
    std::unique_ptr<ace_sht_plan> plan_lg, plan_data_own;
    ace_sht_plan* plan_data = nullptr;  // == plan_lg.get() when data_grid is legendre-gauss
    std::vector<std::unique_ptr<Weight>> weights;
    std::map<std::string, int> index;
    std::vector<DevBuf> wx;  // per block: dhconv weight expanded to real [L][2C][2C] (fp32 engines)
    std::vector<DevBuf> wx_hi, wx_lo;  // per block: the same operand k-packed as fp16 hi/lo planes (f16x3 engine)
    std::vector<float> wx_scale;
    std::vector<char> wx_compact;   // per block: wx_hi/lo hold the compact (Wr | Wi) form of Gemm4Args::cplx
    std::vector<DevBuf> dh_units; std::vector<int> dh_units_per_xcd;   // work lists of the filter contraction, one per batch size 1 .. max_batch
    std::vector<char> wx_native;    // per block: ... of a grouped filter with its diagonal blocks only (1 / G of the dense form)
    // workspace
    DevBuf h0, h1, Y, T, R, U, X, D, E, stats;
    DevBuf P;  // f16x3: a C-channel activation as P-format fp16 hi/lo planes (input of the packed-operand GEMM)
    DevBuf cln_stats;    // conditional layer norm: per-pixel mean | rstd
    DevBuf inN;          // conditional layer norm of the network input (normalize_big_skip)
    // residual_filter_factor > 1 (sfnonet.py:473-497): exact-fp32 plan on the data grid with lmax = nlat / r, mmax = nlon / r / 2 + 1,
    // its scratch and the band-limited copy of the network input the decoder's big skip reads
    std::unique_ptr<ace_sht_plan> plan_res;
    DevBuf resX, resD, inF;
    DevBuf P2;           // second one: the block input h as written by the previous block's fc2 epilogue
    DevBuf part;         // per-strip row statistics from the GEMM epilogues (fused instance norm), two tensors
    DevBuf Wp0, Wp1;     // folded (norm affine) skip / fc1 weights as tiled fp16 planes, per sample
    DevBuf Wq1;          // folded (norm affine) fc1 weights as packed MFMA A fragments, per sample (conv_ws.hip)
    DevBuf Wq0;          // folded inner-skip weights likewise
    DevBuf zero_c;       // C zeros (bias of the bias-free last encoder convolution on conv_ws.hip)
    DevBuf inP;          // the network input as P-format planes (in_chans rounded up to 8 channels): operand of the first encoder convolution
    DevBuf pe_slot;      // dynamic-range slot (64 words) holding max|pos_embed|: the residual bound of that convolution
    DevBuf phys;         // fused post-step physics (ace_step_physics): fp64 global sums, parameters
    int nstrips = 0;
    DevBuf bf0, bf1;
    DevBuf amax;  // [8] uint words: bit patterns of max|X|, max|D|, max|E| of the current block (f16x3 dynamic range)  // instance-norm affine folded into inner_skip / mlp.fc1 weights, per sample
    bool taps_on = false;
    std::vector<DevBuf> taps;
    std::map<GraphKey, hipGraphExec_t> graphs;
    hipStream_t capture_stream = nullptr;
    long weights_generation = 0; // bumped by every ace_sfno_set_weight (ace_sfno_weights_generation)
    bool graphs_stale = false;   // a parameter was uploaded since the graphs were captured: re-capture lazily
    mutable int norm_batch = 0;  // samples and stream of the last forward that enqueued instance norms (ace_sfno_norm_affine)
    mutable hipStream_t norm_stream = nullptr;
    Switches sw;                 // measurement switches, read once at ace_sfno_create

    const float* w(const std::string& name) const {
        auto it = index.find(name);
        return it == index.end() ? nullptr : weights[it->second]->buf.p;
    }
    const Weight* find(const std::string& name) const {
        auto it = index.find(name);
        return it == index.end() ? nullptr : weights[it->second].get();
    }
};

static Weight& add_weight(ace_sfno* n, const std::string& name, ParamRole role, long numel, int block = -1) {
    auto w = std::make_unique<Weight>();
    w->name = name; w->role = role; w->numel = numel; w->block = block;
    n->index[name] = (int)n->weights.size();
    n->weights.push_back(std::move(w));
    return *n->weights.back();
}
// 1x1-conv weight (rows x cols) consumed on a grid of hw pixels: kept zero-padded to a multiple of 32 columns so the direct-to-LDS
// GEMM can read whole k-stages
static void add_conv_weight(ace_sfno* n, const std::string& name, ParamRole role, int rows, int cols, long hw, int block = -1) {
    Weight& w = add_weight(n, name, role, (long)rows * cols, block);
    w.rows = rows; w.cols = cols; w.pitch = (cols + 31) & ~31; w.hw = hw;
}

// Does this convolution keep static fragments (frag0) for conv_ws.hip / conv_wl.hip?  Asked by ace_sfno_set_weight with the
// weight's own consumer grid - the per-role questions of conv_roles.h that plan_route asks again per block.
static bool keeps_static_frags(const ace_sfno* n, const Weight& w) {
    const Switches& sw = n->sw;
    const int nrm = n->cfg.normalization_layer;
    switch (w.role) {
        case ROLE_SKIP: return nrm == 2 ? cln_skip_on_conv_ws(sw.conv_ws_roles, w.cols, w.rows, w.hw) : skip_on_conv_ws(sw.conv_ws_roles, w.cols, w.rows, w.hw);
        case ROLE_FC2: case ROLE_ENC_LAST: return fc2_on_conv_ws(sw.conv_ws_roles, w.cols, w.rows, w.hw);
        // fc1 without an instance norm in front of it (nothing to fold per step): static fragments for conv_wl.hip
        case ROLE_FC1: return nrm != 1 && fc1_on_conv_wl(sw.conv_wl, w.cols, w.rows, w.hw);
        default: return false;
    }
}

extern "C" int ace_sfno_create(const ace_sfno_config* cfg, ace_sfno** out) {
    if (!cfg || !out) return fail(ACE_ERR_INVALID, "null argument");
    const ace_sfno_config& c = *cfg;
    if (c.scale_factor < 1) return fail(ACE_ERR_INVALID, "scale_factor must be >= 1");
    if ((c.scale_factor != 1 || c.residual_filter_factor > 1) && c.normalization_layer == 2)
        return fail(ACE_ERR_INVALID, "scale_factor / residual_filter_factor != 1 are not built for the noise-conditioned nets");
    if (c.residual_filter_factor < 0) return fail(ACE_ERR_INVALID, "residual_filter_factor must be >= 1");
    if (c.in_chans <= 0 || c.out_chans <= 0 || c.embed_dim <= 0 || c.num_layers <= 0 || c.nlat < 2 || c.nlon < 2)
        return fail(ACE_ERR_INVALID, "non-positive dimension in ace_sfno_config");
    if (c.operator_type != 0 && c.operator_type != 1) return fail(ACE_ERR_INVALID, "Unsupported operator type");
    if (c.normalization_layer < 0 || c.normalization_layer > 3)
        return fail(ACE_ERR_INVALID, "normalization_layer must be 'none', 'instance_norm', conditional layer norm or 'layer_norm'");
    const bool cln = c.normalization_layer == 2;
    if (cln) {
        if (c.operator_type != 1) return fail(ACE_ERR_INVALID, "Only 'dhconv' operator_type is supported for NoiseConditionedSFNO models.");
        if (c.noise_embed_dim < 0 || c.noise_embed_dim > 512) return fail(ACE_ERR_INVALID, "noise_embed_dim must be in [0, 512]");
        if (c.filter_num_groups < 1 || c.embed_dim % c.filter_num_groups != 0)
            return fail(ACE_ERR_INVALID, "embed_dim must be divisible by filter_num_groups");
    }
    if (c.activation_function < 1 || c.activation_function > 3)
        return fail(ACE_ERR_INVALID, "Unknown activation function");
    // 'lobatto' is what fme.sht_fix.RealSHT defaults to and what the reference's block-level goldens were made on
    // (conditional_sfno/benchmark.py:85-86); the registered builders only ever pass the other two
    if (c.data_grid != GRID_LEGENDRE_GAUSS && c.data_grid != GRID_EQUIANGULAR && c.data_grid != GRID_LOBATTO)
        return fail(ACE_ERR_INVALID, "data_grid must be 'legendre-gauss', 'equiangular' or 'lobatto'");
    if (c.encoder_layers < 0) return fail(ACE_ERR_INVALID, "encoder_layers must be >= 0");   // 0: one bias-free convolution each side (sfnonet.py:566-577, 660-671)
    if (c.precision != 0 && c.precision != 1) return fail(ACE_ERR_INVALID, "precision must be 0 (fp32) or 1 (f16x3)");

    auto n = std::make_unique<ace_sfno>();
    n->cfg = c;
    n->sw = read_switches();
    n->H = c.nlat; n->W = c.nlon; n->C = c.embed_dim; n->HW = (long)c.nlat * c.nlon;
    n->Bmax = c.max_batch > 0 ? c.max_batch : 1;
    // sfnonet.py:467-472: the downscaled image and the modes kept
    const int sf = c.scale_factor;
    n->Hs = c.nlat / sf; n->Ws = c.nlon / sf; n->HWs = (long)n->Hs * n->Ws;
    if (n->Hs < 1 || n->Ws < 2) return fail(ACE_ERR_INVALID, "scale_factor leaves no grid");
    n->L = (int)(n->Hs * c.hard_thresholding_fraction);
    n->Mm = (int)((n->Ws / 2 + 1) * c.hard_thresholding_fraction);
    if (n->L < 1 || n->Mm < 1) return fail(ACE_ERR_INVALID, "hard_thresholding_fraction leaves no modes");
    n->hid = (int)(c.embed_dim * c.mlp_ratio);

    // trans / itrans on the inner Gauss-Legendre grid; trans_down / itrans_up on the data grid (sfnonet.py:498-515)
    ACE_TRY(plan_build(n->Hs, n->Ws, n->L, n->Mm, GRID_LEGENDRE_GAUSS, n->plan_lg, c.precision == 1));
    if (c.data_grid == GRID_LEGENDRE_GAUSS && sf == 1) {
        n->plan_data = n->plan_lg.get();
    } else {
        ACE_TRY(plan_build(c.nlat, c.nlon, n->L, n->Mm, (Grid)c.data_grid, n->plan_data_own, c.precision == 1));
        n->plan_data = n->plan_data_own.get();
    }

    if (c.residual_filter_factor > 1 && c.big_skip) {
        const int rl = c.nlat / c.residual_filter_factor, rm = c.nlon / c.residual_filter_factor / 2 + 1;
        if (rl < 1 || rm < 1) return fail(ACE_ERR_INVALID, "residual_filter_factor leaves no modes");
        ACE_TRY(plan_build(c.nlat, c.nlon, rl, rm, (Grid)c.data_grid, n->plan_res, false));
        const size_t n2 = (size_t)n->Bmax * 2 * c.in_chans;
        ACE_HIP_TRY(n->resX.alloc_x(((size_t)rm * c.nlat + LEG_STRIP_SLACK_ROWS) * n2, n->sw.polar_poison));
        ACE_HIP_TRY(n->resD.alloc(((size_t)rl + LEG_STRIP_SLACK_ROWS) * rm * n2));
        ACE_HIP_TRY(n->inF.alloc((size_t)n->Bmax * c.in_chans * n->HW));
    }

    // parameters in the reference's state_dict order
    const long C = n->C, HW = n->HW;
    if (c.pos_embed) add_weight(n.get(), "pos_embed", ROLE_POS_EMBED, C * HW);
    long cur = c.in_chans;
    for (int j = 0; j < c.encoder_layers; ++j) {
        add_conv_weight(n.get(), "encoder." + std::to_string(2 * j) + ".weight", ROLE_ENC_CONV, (int)C, (int)cur, HW);
        add_weight(n.get(), "encoder." + std::to_string(2 * j) + ".bias", ROLE_VECTOR, C);
        cur = C;
    }
    add_conv_weight(n.get(), "encoder." + std::to_string(2 * c.encoder_layers) + ".weight", ROLE_ENC_LAST, (int)C, (int)cur, HW);
    for (int i = 0; i < c.num_layers; ++i) {
        const std::string p = "blocks." + std::to_string(i) + ".";
        auto add_pair = [&](const std::string& q, ParamRole role, long len) { add_weight(n.get(), q + "weight", role, len); add_weight(n.get(), q + "bias", role, len); };
        // "layer_norm" (sfnonet.py:584-592): nn.LayerNorm over (H, W), its affine is a pair of (H, W) fields
        const long hw_n0 = i == 0 ? HW : n->HWs;                                  // sfnonet.py:616-623: norm0 sees the block's input grid,
        const long hw_n1 = (i == 0 || i + 1 < c.num_layers) ? n->HWs : HW;        // norm1 its output grid (a first block's: the inner one)
        const long hw_out = block_out_pixels(i, c.num_layers, HW, n->HWs);         // the skips and the MLP likewise (plan_route: BlockRoute::hw_out)
        auto add_cln = [&](const std::string& q, long ch) {   // ConditionalLayerNorm parameters in state_dict order
            if (c.noise_embed_dim > 0) {
                add_weight(n.get(), q + "W_scale_2d.weight", ROLE_CLN_COND, ch * c.noise_embed_dim);
                add_weight(n.get(), q + "W_bias_2d.weight", ROLE_CLN_COND, ch * c.noise_embed_dim);
            }
            if (c.affine_norms) add_pair(q + "norm.", ROLE_VECTOR, ch);
        };
        if (c.normalization_layer == 1) add_pair(p + "norm0.", ROLE_VECTOR, C);
        if (c.normalization_layer == 3) add_pair(p + "norm0.", ROLE_PLAIN, hw_n0);
        if (cln) add_cln(p + "norm0.", C);
        const long fw = c.operator_type == 1 ? C * C * n->L * 2 : C * C * (long)n->L * n->Mm * 2;
        Weight& flt = add_weight(n.get(), p + "filter.filter.weight", ROLE_FILTER, fw, i);
        if (cln) flt.ext_numel = fw / c.filter_num_groups;   // grouped: (G, L, C/G, C/G, 2)
        add_weight(n.get(), p + "filter.filter.bias", ROLE_VECTOR, C);
        add_conv_weight(n.get(), p + "inner_skip.weight", ROLE_SKIP, (int)C, (int)C, hw_out, i);
        add_weight(n.get(), p + "inner_skip.bias", ROLE_VECTOR, C);
        if (c.normalization_layer == 1) add_pair(p + "norm1.", ROLE_VECTOR, C);
        if (c.normalization_layer == 3) add_pair(p + "norm1.", ROLE_PLAIN, hw_n1);
        if (cln) add_cln(p + "norm1.", C);
        if (c.use_mlp) {
            add_conv_weight(n.get(), p + "mlp.fwd.0.weight", ROLE_FC1, n->hid, (int)C, hw_out, i);
            add_weight(n.get(), p + "mlp.fwd.0.bias", ROLE_VECTOR, n->hid);
            add_conv_weight(n.get(), p + "mlp.fwd.2.weight", ROLE_FC2, (int)C, n->hid, hw_out, i);
            add_weight(n.get(), p + "mlp.fwd.2.bias", ROLE_VECTOR, C);
        }
    }
    cur = C + (c.big_skip ? c.in_chans : 0);
    for (int j = 0; j < c.encoder_layers; ++j) {
        add_conv_weight(n.get(), "decoder." + std::to_string(2 * j) + ".weight", ROLE_DEC_CONV, (int)C, (int)cur, HW);
        add_weight(n.get(), "decoder." + std::to_string(2 * j) + ".bias", ROLE_VECTOR, C);
        cur = C;
    }
    add_conv_weight(n.get(), "decoder." + std::to_string(2 * c.encoder_layers) + ".weight", ROLE_DEC_CONV, c.out_chans, (int)cur, HW);
    if (cln && c.normalize_big_skip && c.big_skip) {
        if (c.noise_embed_dim > 0) {
            add_weight(n.get(), "norm_big_skip.W_scale_2d.weight", ROLE_CLN_COND, (long)c.in_chans * c.noise_embed_dim);
            add_weight(n.get(), "norm_big_skip.W_bias_2d.weight", ROLE_CLN_COND, (long)c.in_chans * c.noise_embed_dim);
        }
        if (c.affine_norms) { add_weight(n.get(), "norm_big_skip.norm.weight", ROLE_VECTOR, c.in_chans); add_weight(n.get(), "norm_big_skip.norm.bias", ROLE_VECTOR, c.in_chans); }
    }

    n->wx.resize(c.num_layers);
    n->wx_hi.resize(c.num_layers);
    n->wx_lo.resize(c.num_layers);
    n->wx_scale.assign(c.num_layers, 1.f);
    n->wx_compact.assign(c.num_layers, 0);
    n->wx_native.assign(c.num_layers, 0);
    for (int i = 0; i < c.num_layers; ++i) {
        // blocks whose input/output grid differs from the internal one keep D in fp32 (residual round trip) and use
        // the expanded operand
        const bool mixed = (n->plan_data != n->plan_lg.get()) && (i == 0 || i == c.num_layers - 1);
        n->wx_compact[i] = (!n->sw.no_pk_sht && c.precision == 1 && c.operator_type == 1 && n->C % 128 == 0 && !mixed &&
                            ((long)n->Bmax * 2 * n->C) % 4 == 0) ? 1 : 0;
        // grouped filter of the NoiseConditionedSFNO kept as the reference keeps it: the strip kernel is then the ONLY reader
        // (every runtime precondition of that kernel is decided HERE, from the shape: plan arithmetic = c.precision, column
        // alignment = wx_compact - a handle that stores the native form can always run it)
        n->wx_native[i] = (n->wx_compact[i] && cln && c.filter_num_groups > 1 && !n->sw.dense_grouped_filter && !n->sw.no_dhconv_strip &&
                           dhconv_native_groups_ok(n->C, c.filter_num_groups)) ? 1 : 0;
    }
    if (c.operator_type == 1 && c.precision == 1 && n->C % 128 == 0) {   // dhconv_strip.hip's work lists (depend on the batch size)
        n->dh_units.resize(n->Bmax);
        n->dh_units_per_xcd.assign(n->Bmax, 0);
        for (int b = 1; b <= n->Bmax; ++b)
            ACE_HIP_TRY(upload_dhconv_units(n->L, n->Mm * b, b, n->C, n->dh_units[b - 1], &n->dh_units_per_xcd[b - 1]));
    }
    const size_t act = (size_t)n->Bmax * C * HW;
    // + slack rows read (never used) by the strip Legendre kernels past the last contraction row
    const size_t spec_x = ((size_t)n->Mm * n->H + LEG_STRIP_SLACK_ROWS) * n->Bmax * 2 * C;
    const size_t spec_d = ((size_t)n->L + LEG_STRIP_SLACK_ROWS) * n->Mm * n->Bmax * 2 * C;
    ACE_HIP_TRY(n->h0.alloc(act));
    ACE_HIP_TRY(n->h1.alloc(act));
    ACE_HIP_TRY(n->Y.alloc(act));
    ACE_HIP_TRY(n->T.alloc(act));
    if (n->plan_data != n->plan_lg.get()) ACE_HIP_TRY(n->R.alloc(act));
    if (c.use_mlp) ACE_HIP_TRY(n->U.alloc((size_t)n->Bmax * n->hid * HW, true));
    if (c.precision == 1) {
        ACE_HIP_TRY(n->P.alloc(act, true));
        if (c.normalization_layer == 1 && c.use_mlp) {
            ACE_HIP_TRY(n->P2.alloc(act, true));
            n->nstrips = (int)((HW + 31) / 32) + 8;     // >= tilesN * WN of either tile shape and conv_ws's 32-pixel tiles
            // the per-sample fold buffers: needed when ANY block of this net runs that role on conv_ws.hip / conv_wl.hip
            auto any = [&](auto q) { return any_block(c.num_layers, HW, n->HWs, q); };
            if (any([&](long hw) { return fc1_on_conv_ws(n->sw.conv_ws_roles, (int)C, n->hid, hw) || fc1_on_conv_wl(n->sw.conv_wl, (int)C, n->hid, hw); }))
                ACE_HIP_TRY(n->Wq1.alloc((size_t)n->Bmax * n->hid * C, true));   // hi + lo halves = one float per element
            if (any([&](long hw) { return skip_on_conv_ws(n->sw.conv_ws_roles, (int)C, (int)C, hw); })) ACE_HIP_TRY(n->Wq0.alloc((size_t)n->Bmax * C * C, true));
            ACE_HIP_TRY(n->zero_c.alloc((size_t)C, true));
            ACE_HIP_TRY(n->inP.alloc((size_t)n->Bmax * ((c.in_chans + 7) / 8 * 8) * n->HW, true));   // two planes of halves = one float per element
            ACE_HIP_TRY(n->pe_slot.alloc(64, true));
            ACE_HIP_TRY(n->part.alloc((size_t)2 * n->Bmax * n->nstrips * C * 4, true));
            const size_t cp = (size_t)((C + 31) & ~31);
            ACE_HIP_TRY(n->Wp0.alloc((size_t)n->Bmax * ((C + 15) / 16 * 16) * cp, true));       // 2 planes of halves = 1 float per element
            ACE_HIP_TRY(n->Wp1.alloc((size_t)n->Bmax * ((n->hid + 15) / 16 * 16) * cp, true));
        }
    }
    ACE_HIP_TRY(n->X.alloc_x(spec_x, n->sw.polar_poison));
    ACE_HIP_TRY(n->D.alloc(spec_d));
    ACE_HIP_TRY(n->E.alloc(spec_d));
    ACE_HIP_TRY(n->stats.alloc((size_t)4 * n->Bmax * C));
    if (cln) {
        ACE_HIP_TRY(n->cln_stats.alloc((size_t)2 * n->Bmax * HW));
        if (c.normalize_big_skip && c.big_skip) ACE_HIP_TRY(n->inN.alloc((size_t)n->Bmax * c.in_chans * HW));
    }
    ACE_HIP_TRY(n->amax.alloc((size_t)(16 + 12 * c.num_layers + 1) * AMAX_SHARDS));   // + the conditioning field's slot
    if (c.normalization_layer == 1) {
        ACE_HIP_TRY(n->bf0.alloc((size_t)n->Bmax * C));
        if (c.use_mlp) {
            ACE_HIP_TRY(n->bf1.alloc((size_t)n->Bmax * n->hid));
        }
    }
    *out = n.release();
    return ACE_OK;
}

extern "C" void ace_sfno_destroy(ace_sfno* n) {
    if (!n) return;
    for (auto& kv : n->graphs) (void)hipGraphExecDestroy(kv.second);
    if (n->capture_stream) (void)hipStreamDestroy(n->capture_stream);
    delete n;
}

extern "C" long ace_sfno_weights_generation(const ace_sfno* n) { return n ? n->weights_generation : -1; }

// Device bytes the library owns for this handle at batch sizes up to `batch` (workspace + both operand forms of the weights
// + tables): SURVEY 8(b) workspace_size.  The workspace is sized by ace_sfno_config.max_batch at creation.
extern "C" long ace_sfno_workspace_size(const ace_sfno* n, int batch) {
    if (!n) { (void)fail(ACE_ERR_INVALID, "null argument"); return -1; }
    if (batch <= 0 || batch > n->Bmax) {
        (void)fail(ACE_ERR_INVALID, "batch " + std::to_string(batch) + " outside [1, max_batch=" + std::to_string(n->Bmax) + "]");
        return -1;
    }
    size_t fl = 0;
    auto add = [&](const DevBuf& b) { fl += b.n; };
    for (const DevBuf* b : {&n->h0, &n->h1, &n->Y, &n->T, &n->R, &n->U, &n->X, &n->D, &n->E, &n->stats, &n->P, &n->cln_stats, &n->inN,
                            &n->P2, &n->part, &n->Wp0, &n->Wp1, &n->Wq1, &n->Wq0, &n->zero_c, &n->inP, &n->pe_slot, &n->bf0,
                            &n->bf1, &n->amax, &n->phys})
        add(*b);
    for (const auto& t : n->taps) add(t);
    for (const auto& v : {&n->wx, &n->wx_hi, &n->wx_lo})
        for (const auto& b : *v) add(b);
    for (const auto& w : n->weights)
        for (const DevBuf* b : {&w->buf, &w->hi, &w->lo, &w->thi, &w->tlo, &w->frag0}) add(*b);
    auto plan_bytes = [&](const ace_sht_plan* p) {
        if (!p) return;
        for (const DevBuf* b : {&p->wt, &p->pt, &p->fc, &p->fs, &p->gc, &p->gs, &p->X, &p->D, &p->wt_hi, &p->wt_lo, &p->pt_hi, &p->pt_lo,
                                &p->wt_frag, &p->pt_frag, &p->wt_off, &p->pt_off, &p->slots})
            add(*b);
    };
    plan_bytes(n->plan_lg.get());
    plan_bytes(n->plan_data_own.get());
    plan_bytes(n->plan_res.get());
    for (const DevBuf* b : {&n->resX, &n->resD, &n->inF}) add(*b);
    return (long)(fl * sizeof(float));
}

extern "C" int ace_sfno_num_weights(const ace_sfno* n) { return n ? (int)n->weights.size() : 0; }
extern "C" const char* ace_sfno_weight_name(const ace_sfno* n, int i) {
    if (!n || i < 0 || i >= (int)n->weights.size()) return nullptr;
    return n->weights[i]->name.c_str();
}
extern "C" long ace_sfno_weight_numel(const ace_sfno* n, int i) {
    if (!n || i < 0 || i >= (int)n->weights.size()) return -1;
    return n->weights[i]->ext_numel ? n->weights[i]->ext_numel : n->weights[i]->numel;
}

// ---- ace_sfno_set_weight: the library copy, then the derived operands of the parameter's role - one function per stored form
// library copy: the caller's tensor in the reference layout; conv weights zero-padded to `pitch`, a grouped filter kept as it comes
// (wx_native) or expanded to the dense form
static int store_library_copy(ace_sfno* n, Weight& w, const float* src, hipStream_t s) {
    if (w.rows > 0) {
        if (!w.buf.p) ACE_HIP_TRY(w.buf.alloc((size_t)w.rows * w.pitch, true));  // zero padding columns
        ACE_HIP_TRY(hipMemcpy2DAsync(w.buf.p, sizeof(float) * w.pitch, src, sizeof(float) * w.cols, sizeof(float) * w.cols,
                                 w.rows, hipMemcpyDeviceToDevice, s));
    } else if (w.ext_numel && !n->wx_native[w.block]) {   // (G, L, C/G, C/G, 2) -> dense (Cin, Cout, L, 2), then as any dhconv weight
        if (!w.buf.p) ACE_HIP_TRY(w.buf.alloc((size_t)w.numel, false));
        ACE_HIP_TRY(launch_csfno_weight_to_dense(src, w.buf.p, n->C, n->cfg.filter_num_groups, n->L, s));
    } else {
        const long numel = w.ext_numel ? w.ext_numel : w.numel;
        if (!w.buf.p) ACE_HIP_TRY(w.buf.alloc((size_t)numel, false));
        ACE_HIP_TRY(hipMemcpyAsync(w.buf.p, src, sizeof(float) * numel, hipMemcpyDeviceToDevice, s));
    }
    return ACE_OK;
}
// dhconv filter operand.  f16x3: k-packed fp16 hi/lo planes scaled so that max|w| lands in [2^9, 2^10) - the diagonal blocks of a
// grouped filter only (native), the compact (Wr | Wi) form, or the expanded real form; fp32: the expanded real [L][2C][2C] matrix
static int store_filter_operand(ace_sfno* n, Weight& w, hipStream_t s) {
    if (n->cfg.operator_type != 1) return ACE_OK;
    const int b = w.block, C = n->C, G = n->cfg.filter_num_groups;
    const size_t cnt = (size_t)n->L * 2 * C * 2 * C;
    if (n->cfg.precision != 1 || (2 * C) % 32 != 0) {
        if (!n->wx[b].p) ACE_HIP_TRY(n->wx[b].alloc(cnt, false));
        ACE_HIP_TRY(launch_expand_dhconv_weight(w.buf.p, n->wx[b].p, C, C, n->L, s));
        return ACE_OK;
    }
    const bool native = n->wx_native[b] != 0, compact = n->wx_compact[b] != 0;
    float mx = 0.f;
    ACE_TRY(device_absmax(w.buf.p, native ? w.ext_numel : w.numel, s, &mx));
    const float sc = n->wx_scale[b] = pow2_scale(mx, 10);
    const size_t halves = native ? cnt / 2 / G : (compact ? cnt / 2 : cnt);
    if (!n->wx_hi[b].p) ACE_HIP_TRY(n->wx_hi[b].alloc((halves + 1) / 2, false));
    if (!n->wx_lo[b].p) ACE_HIP_TRY(n->wx_lo[b].alloc((halves + 1) / 2, false));
    if (native) ACE_HIP_TRY(launch_pack_dhconv_f16g(w.buf.p, n->wx_hi[b].p, n->wx_lo[b].p, C, G, n->L, sc, s));
    else if (compact) ACE_HIP_TRY(launch_pack_dhconv_f16c(w.buf.p, n->wx_hi[b].p, n->wx_lo[b].p, C, C, n->L, sc, s));
    else ACE_HIP_TRY(launch_pack_dhconv_f16(w.buf.p, n->wx_hi[b].p, n->wx_lo[b].p, C, C, n->L, sc, s));
    return ACE_OK;
}
// f16x3 conv weights: planes + norms in both orders, and the static fragments of the roles conv_ws.hip / conv_wl.hip serve
static int store_conv_operand(ace_sfno* n, Weight& w, hipStream_t s) {
    if (n->cfg.precision != 1) return ACE_OK;
    ACE_TRY(prepare_conv_operand(w.buf.p, w.rows, w.cols, w.pitch, PLANES_ROWS | PLANES_TILED, s, w));
    if (keeps_static_frags(n, w)) {
        if (!w.frag0.p) ACE_HIP_TRY(w.frag0.alloc((size_t)w.rows * w.cols, false));
        ACE_HIP_TRY(launch_pack_conv_frag(w.buf.p, w.pitch, w.rows, w.cols, 0, nullptr, 0.f, w.ascale, nullptr, w.frag0.p, 0, 1, s));
    }
    return ACE_OK;
}
// conditioning convolutions of a conditional layer norm: MFMA A fragments for cln_mfma.hip (f16x3 networks, C % 256 == 0)
static int store_cln_frags(ace_sfno* n, Weight& w, hipStream_t s) {
    const int J = n->cfg.noise_embed_dim;
    if (n->cfg.precision != 1 || J < 1 || J > 128 || w.numel != (long)n->C * J || n->C % 256 != 0 || n->C > 1024) return ACE_OK;
    WeightNorms nm;
    ACE_TRY(prepare_cln_frags(w.buf.p, n->C, J, s, w.frag0, &w.ascale, &nm));
    w.wabs = nm.absmax; w.winf = nm.winf;   // winf bounds the convolution's output by winf * max |cond|
    return ACE_OK;
}
// max |pos_embed| as a dynamic-range slot (the residual of the last encoder convolution)
static int store_pos_embed_slot(ace_sfno* n, Weight& w, hipStream_t s) {
    if (!n->pe_slot.p) return ACE_OK;
    float mx = 0.f;
    ACE_TRY(device_absmax(w.buf.p, w.numel, s, &mx));   // (C x H x W values: reduced where they are, not through a host copy)
    const std::vector<float> rep(64, mx);
    ACE_HIP_TRY(hipMemcpy(n->pe_slot.p, rep.data(), rep.size() * sizeof(float), hipMemcpyHostToDevice));
    return ACE_OK;
}
// biases and norm affines: the bound used by the P-format producers
static int store_vector_bound(Weight& w, hipStream_t s) {
    std::vector<float> host;
    ACE_TRY(host_copy(w.buf.p, (size_t)w.numel, s, host));
    w.absmax = host_absmax(host);
    return ACE_OK;
}

extern "C" int ace_sfno_set_weight(ace_sfno* n, const char* name, const float* src, long numel, void* stream) {
    if (!n || !name || !src) return fail(ACE_ERR_INVALID, "null argument");
    auto it = n->index.find(name);
    if (it == n->index.end()) return fail(ACE_ERR_INVALID, std::string("unknown parameter '") + name + "'");
    Weight& w = *n->weights[it->second];
    const long expect = w.ext_numel ? w.ext_numel : w.numel;
    if (numel != expect)
        return fail(ACE_ERR_INVALID, std::string("size mismatch for ") + name + ": expected " +
                                         std::to_string(expect) + " elements, got " + std::to_string(numel));
    hipStream_t s = static_cast<hipStream_t>(stream);
    ACE_TRY(store_library_copy(n, w, src, s));
    switch (w.role) {
        case ROLE_PLAIN: break;
        case ROLE_VECTOR: ACE_TRY(store_vector_bound(w, s)); break;
        case ROLE_POS_EMBED: ACE_TRY(store_pos_embed_slot(n, w, s)); break;
        case ROLE_FILTER: ACE_TRY(store_filter_operand(n, w, s)); break;
        case ROLE_CLN_COND: ACE_TRY(store_cln_frags(n, w, s)); break;
        default: ACE_TRY(store_conv_operand(n, w, s)); break;   // the convolutions
    }
    ACE_HIP_TRY(hipStreamSynchronize(s));
    w.set = true;
    // Captured graphs keep pointing at the same library buffers, but the host-side scalars derived from the weights
    // (ascale, winf, wabs, bias bounds, filter scale) are baked into their kernel arguments by value: drop the graphs so
    // that the next ace_sfno_forward_graph re-captures with the new scalars.
    // Marked stale here, destroyed in ace_sfno_forward_graph after a stream synchronise (an exec may still be in flight).
    n->graphs_stale = true;
    n->weights_generation += 1;
    return ACE_OK;
}

// ---------------------------------------------------------------------------------------------
// the forward schedule.  plan_route() decides which engine serves every role of every block; the enqueue_* functions below it
// fill argument structs and launch what the plan says, and decide nothing.
// ---------------------------------------------------------------------------------------------
enum FilterEngine { FLT_DHCONV_STRIP, FLT_PACKED_TILE, FLT_ADYN_F16X3, FLT_FP32, FLT_DIAGONAL };
enum ConvEngine { CONV_NONE, CONV_TILE, CONV_PACKED, CONV_WS, CONV_WL };   // v3 / fp32 tile engine, packed tile engine, conv_ws.hip, conv_wl.hip
enum BlockBody { BODY_PLAIN, BODY_PACKED, BODY_FUSED };

struct BlockRoute {
    const ace_sht_plan* fwd = nullptr; const ace_sht_plan* inv = nullptr;   // the filter's two transforms
    long hw_in = 0, hw_out = 0;      // resolution in front of / behind the filter (they differ where scale_residual)
    bool scale_residual = false;     // grids differ (s2convolutions.py:82-86): the residual is the spectrally round-tripped input
    // block input, as the producer (last encoder convolution / previous block's fc2) left it
    bool in_planes = false;          // P2 holds the RAW input as planes (bound in hslot(i)) and `part` its row statistics: norm0 finalises
    int in_nparts = 0;               // those partials (so many per row) instead of running a statistics pass
    bool in_planes_only = false;     // ... and no fp32 copy exists: the longitude FFT reads the planes
    bool n0_to_planes = false, n1_to_planes = false;   // the conditional norms are asked for P-format planes (norm1: planes only)
    bool ride_skip_pack = false;     // the inner skip's folded weights are offered to the forward FFT launch as rider workgroups
    // spectral filter
    bool dplanes = false;            // D goes from the Legendre epilogue to the contraction as fp16 planes (never fp32)
    FilterEngine filter = FLT_FP32;
    // behind the filter
    BlockBody body = BODY_PLAIN;
    ConvEngine skip = CONV_TILE, fc1 = CONV_NONE, fc2 = CONV_NONE;
    int skip_slot = -1, t_slot = -1; // range slots of the inner skip's input (-1: none, fp32 engine) and of the MLP's input
    bool pfold = false;              // fused body: fc1 folds its norm affine in the kernel's own prologue (conv_wl.hip at the ACE2 width)
    int t_nparts = 0;                // fused body: statistics partials per row the inner skip writes
    // fused body, fc2
    bool res_planes = false;         // the outer-skip residual comes from the input planes
    bool out_f32 = true;             // h' is written as fp32
    bool out_planes = false;         // ... as planes with statistics for the next block (every block but the last)
    int out_nparts = 0;
};
struct FwdRoute {
    const char* err = nullptr;       // a handle whose stored operands no engine can read for this launch (ACE_ERR_STATE)
    bool stream_ok = false;          // residual stream of the blocks as planes only where a conv_ws fc2 feeds the next block
    bool noise_range = false;        // the conditioning field's range is taken (f16x3 noise-conditioned nets)
    bool enc_hidden_planes = false;  // first encoder convolution on the packed engine: P holds the hidden activation as planes
    bool enc_planes = false;         // last encoder convolution on conv_ws.hip: h0 as planes + the statistics of block 0's norm0
    bool enc_planes_only = false;    // ... and not as fp32
    int enc_nparts = 0;
    std::vector<BlockRoute> blk;
};

// f16x3 "v4" engine: can a 1x1 convolution read a cin-channel input as P-format planes at resolution hw?
static bool packed_ok(const ace_sfno* n, int cin, long hw) {
    return !n->sw.no_pk && n->cfg.precision == 1 && n->P.p && cin % 8 == 0 && hw % 4 == 0;
}
static int ws_stat_parts(int K, int M, long HW) {   // statistics partials per row of a conv_ws.hip launch of that shape
    ConvStripArgs k;
    k.C = K; k.M = M; k.HW = (int)HW;
    return conv_ws_stat_parts(k);
}
// the filter contraction on dhconv_strip.hip (compact or native operand, coefficient planes in D)
static DhconvStripArgs dhconv_strip_args(const ace_sfno* n, int i, int B, const unsigned* dmax, unsigned* emax) {
    const int C = n->C;
    const long N2 = (long)B * 2 * C;
    DhconvStripArgs ds;
    ds.Dhi = reinterpret_cast<const _Float16*>(n->D.p);
    ds.Dlo = ds.Dhi + (size_t)n->L * n->Mm * N2;
    ds.sD = (long)n->Mm * N2; ds.amax = dmax;
    ds.Whi = reinterpret_cast<const _Float16*>(n->wx_hi[i].p);
    ds.Wlo = reinterpret_cast<const _Float16*>(n->wx_lo[i].p);
    ds.sW = (long)2 * C * C; ds.bscale = n->wx_scale[i];
    ds.E = n->E.p; ds.sE = (long)n->Mm * N2; ds.omax = emax;
    ds.C = C; ds.L = n->L; ds.Mrows = n->Mm * B; ds.trimul = B;
    ds.groups = n->cfg.normalization_layer == 2 ? n->cfg.filter_num_groups : 1;
    if (n->wx_native[i]) { ds.kstore = C / ds.groups; ds.sW = (long)2 * ds.kstore * C; }
    if ((int)n->dh_units.size() >= B) { ds.units = reinterpret_cast<const int*>(n->dh_units[B - 1].p); ds.units_per_xcd = n->dh_units_per_xcd[B - 1]; }
    return ds;
}
// dynamic-range slots of the f16x3 engine (AMAX_SHARDS words each): 0 network input, 1..7 encoder/decoder hidden,
// 8 + i % 8 block input h_i, 16 + 12 i + {0 X, 1 D, 2 E, 3 N0, 4 T, 5 N1, 6 U, 7 Y, 8 folded skip weight, 9 folded fc1 weight},
// 16 + 12 num_layers the conditioning field
static unsigned* range_slot(const ace_sfno* n, int k) {
    return n->cfg.precision == 1 && k >= 0 ? reinterpret_cast<unsigned*>(n->amax.p) + (size_t)k * AMAX_SHARDS : nullptr;
}

// Which kernel serves which role of a forward at batch size B.  Reads the configuration, the switches and which buffers / packed
// fragments exist; makes no HIP call and changes nothing.
static FwdRoute plan_route(const ace_sfno* n, int B, bool has_noise) {
    const ace_sfno_config& c = n->cfg;
    const Switches& sw = n->sw;
    const int C = n->C, hid = n->hid, nl = c.num_layers;
    const long N2 = (long)B * 2 * C;
    const bool f16 = c.precision == 1, gelu = c.activation_function == ACT_GELU;
    const bool norm = c.normalization_layer == 1, cln = c.normalization_layer == 2, lnrm = c.normalization_layer == 3;
    auto wt = [&](const std::string& name) -> const Weight& { return *n->weights[n->index.at(name)]; };
    FwdRoute r;
    r.noise_range = cln && f16 && has_noise;
    // Residual stream as planes only: once a block's fc2 (conv_ws mode 4) has written h' as P-format planes, the next block reads
    // them everywhere - longitude FFT, inner skip, outer-skip residual - and no fp32 copy of h' exists (fc2: 520 -> 420 MB)
    r.stream_ok = sw.planes_stream && f16 && !n->taps_on && n->plan_data == n->plan_lg.get() && C % 16 == 0 &&
                  !n->plan_lg->sw.no_fft && dft_fft_has_width(n->W) && dft_fft_planes_fit(n->H, n->W, B, C);
    r.blk.resize(nl);

    // ---- engines of each block (sfnonet.py:217-252): functions of the block's grids and of what was uploaded
    for (int i = 0; i < nl; ++i) {
        BlockRoute& b = r.blk[i];
        const std::string p = "blocks." + std::to_string(i) + ".";
        const int sb = 16 + 12 * i;
        b.fwd = i == 0 ? n->plan_data : n->plan_lg.get();
        b.inv = i == nl - 1 ? n->plan_data : n->plan_lg.get();
        b.scale_residual = b.fwd != b.inv;
        b.hw_in = (long)b.fwd->nlat * b.fwd->nlon;
        // everything behind the filter works on ITS output grid (the skips, norm1 and the MLP see what the inverse transform
        // produced) - the inner grid after the first block of a scale_factor != 1 net, the data grid after the last
        const long hw = b.hw_out = block_out_pixels(i, nl, n->HW, n->HWs);

        // spectral filter (s2convolutions.py:162-197)
        b.dplanes = f16 && !sw.no_pk_sht && c.operator_type == 1 && n->wx_hi[i].p && !b.scale_residual && b.fwd->f16 &&
                    N2 % 4 == 0 && (2 * C) % 32 == 0;
        if (c.operator_type != 1) {
            b.filter = FLT_DIAGONAL;
        } else {
            bool strip_ok = false;
            if (b.dplanes && n->wx_compact[i]) {
                const DhconvStripArgs ds = dhconv_strip_args(n, i, B, range_slot(n, sb + 1), range_slot(n, sb + 2));
                strip_ok = ds.units && dhconv_strip_eligible(ds);
            }
            const char* err = nullptr;
            if (n->wx_native[i] && !strip_ok) err = "grouped filter stored as diagonal blocks, but the strip kernel cannot run this launch";
            else if (strip_ok && !sw.no_dhconv_strip) b.filter = FLT_DHCONV_STRIP;
            else if (b.dplanes) b.filter = FLT_PACKED_TILE;
            else if (f16 && n->wx_hi[i].p && n->wx_compact[i]) err = "compact dhconv operand without the packed path";
            else if (f16 && n->wx_hi[i].p) b.filter = FLT_ADYN_F16X3;
            else b.filter = FLT_FP32;
            if (err && !r.err) r.err = err;
        }

        // Input of the inner skip: the normalised block input (bound from the norm statistics) or, without a norm, the raw block
        // input; the spectrally round-tripped residual of mixed-grid blocks has no range slot -> fp32 engine
        b.skip_slot = b.scale_residual ? -1 : ((norm || cln || lnrm) ? sb + 3 : 8 + i % 8);
        b.t_slot = (norm || cln || lnrm) ? sb + 5 : sb + 4;
        const bool pk = f16 && !b.scale_residual && packed_ok(n, C, hw) && (!c.use_mlp || hid % 8 == 0);
        const bool fused = pk && norm && c.use_mlp && n->P2.p;
        b.body = fused ? BODY_FUSED : pk ? BODY_PACKED : BODY_PLAIN;
        const ConvEngine other = pk ? CONV_PACKED : CONV_TILE;
        b.skip = other;
        if (c.use_mlp) b.fc1 = b.fc2 = other;
        if (fused) {
            // Instance norms fused away: every conv input is P-format planes written by its producer's epilogue, the norm affine is
            // folded into the consumer's weights.  Which of the three convolutions run on the weight-stationary kernels:
            const Weight& w1 = wt(p + "mlp.fwd.0.weight");
            if (gelu && n->Wq0.p && wt(p + "inner_skip.weight").frag0.p && skip_on_conv_ws(sw.conv_ws_roles, C, C, hw)) b.skip = CONV_WS;
            if (gelu && n->Wq1.p && fc1_on_conv_wl(sw.conv_wl, C, hid, hw)) b.fc1 = CONV_WL;
            else if (gelu && n->Wq1.p && fc1_on_conv_ws(sw.conv_ws_roles, C, hid, hw)) b.fc1 = CONV_WS;
            b.pfold = sw.fused_pack && b.fc1 == CONV_WL && C == 384 && w1.pitch % 4 == 0;
            // (C <= 1024: the fp32 output of conv_ws.hip)
            if (wt(p + "mlp.fwd.2.weight").frag0.p && C <= 1024 && fc2_on_conv_ws(sw.conv_ws_roles, hid, C, hw)) b.fc2 = CONV_WS;
            b.t_nparts = b.skip == CONV_WS ? ws_stat_parts(C, C, hw) : gemm4_strips(C, (int)hw);
        } else if (pk) {
            // conv_ws.hip mode 6: GELU(W . planes + bias + Y) -> fp32 T (the conditional norm that follows reads fp32)
            if (cln && gelu && wt(p + "inner_skip.weight").frag0.p && cln_skip_on_conv_ws(sw.conv_ws_roles, C, C, hw)) b.skip = CONV_WS;
            // conv_wl.hip: the noise-conditioned nets' fc1 (no norm affine to fold, static fragments)
            if (c.use_mlp && !norm && gelu && wt(p + "mlp.fwd.0.weight").frag0.p && fc1_on_conv_wl(sw.conv_wl, C, hid, hw)) b.fc1 = CONV_WL;
            b.n0_to_planes = cln;
            b.n1_to_planes = cln && c.use_mlp && !n->taps_on;   // followed by the packed MLP, norm1's output exists as planes only
        } else {
        }
    }

    // ---- encoder (sfnonet.py:721-733).  Its last convolution (C -> C, no bias, + pos_embed) runs on conv_ws.hip when block 0
    // takes the fused body: the epilogue then writes h0 as fp32 AND as P-format planes with the row statistics of norm0, so block 0
    // starts like every other block (no pack pass, no statistics pass over h0).
    const Weight& we = wt("encoder." + std::to_string(2 * c.encoder_layers) + ".weight");
    r.enc_planes = !sw.no_enc_ws && r.blk[0].body == BODY_FUSED && c.encoder_layers >= 1 && c.pos_embed && we.frag0.p && n->zero_c.p &&
                   n->pe_slot.p && n->part.p && fc2_on_conv_ws(sw.conv_ws_roles, C, C, n->HW);
    if (r.enc_planes) r.enc_nparts = ws_stat_parts(C, C, n->HW);
    // Then a ONE-hidden-layer encoder (the ACE2 shape) never materialises its hidden activation as fp32: the network input is packed
    // to P-format planes (in_chans rounded up to a k-group, 11 MB) and the first convolution runs on the packed-operand engine, whose
    // epilogue writes GELU(W x + b) straight as the planes the last one reads (r03: fp32 write + pack pass = 55 + 41 us per step).
    if (r.enc_planes && c.encoder_layers == 1 && n->inP.p && !sw.no_enc_pk) {
        const Weight& w0 = wt("encoder.0.weight");
        r.enc_hidden_planes = w0.thi.p && w0.pitch >= (c.in_chans + 7) / 8 * 8;
    }
    // fp32 copy of h0: only where something reads it - with the residual stream as planes and block 0's fc2 on conv_ws.hip (whose
    // residual comes from the planes) block 0 takes its input from the planes everywhere and the 100 MB write is dropped
    r.enc_planes_only = r.enc_planes && r.stream_ok && r.blk[0].fc2 == CONV_WS;

    // ---- what each block finds of its input, threaded from producer to consumer
    bool have_ph = r.enc_planes, planes_only = r.enc_planes_only;
    int nparts = r.enc_nparts;
    for (int i = 0; i < nl; ++i) {
        BlockRoute& b = r.blk[i];
        const bool last = i + 1 == nl;
        b.in_planes = have_ph; b.in_planes_only = planes_only; b.in_nparts = nparts;
        if (b.body == BODY_FUSED) {
            // The folded weights of the inner skip (W diag(a0), bs + W b0) depend on norm0's affine only: the ~300 workgroups that
            // pack them ride in the forward FFT launch instead of a dependent 7 us launch of their own
            b.ride_skip_pack = sw.fused_pack && have_ph && b.skip == CONV_WS;
            b.out_planes = !last;
            if (b.fc2 == CONV_WS) {
                // residual = a0 h + b0: from the fp32 h, or - when the block input came as planes from a producer epilogue - from
                // those planes; then a mid block writes h' as planes only
                b.res_planes = r.stream_ok && have_ph;
                b.out_f32 = last || !b.res_planes;
                nparts = ws_stat_parts(hid, C, b.hw_out);   // one partial per workgroup and row (accumulated in LDS)
            } else {
                nparts = gemm4_strips(C, (int)b.hw_out);
            }
            b.out_nparts = nparts;
            planes_only = !b.out_f32;
            have_ph = !last;
        } else if (b.body == BODY_PACKED) {
            have_ph = false;
        }
    }
    return r;
}

// hipEvent stage timer: one event after each launch group; the elapsed time between consecutive events
// is charged to the stage that just ended (the reference's CUDATimer children: fme/core/benchmark/timer.py:105-168,
// conditional_sfno/sfnonet.py:388-437, s2convolutions.py:372-431).
enum Stage {
    ST_ENCODER = 0, ST_NORM0, ST_DFT_FWD, ST_LEGENDRE_FWD, ST_CONTRACT, ST_LEGENDRE_INV, ST_DFT_INV, ST_INNER_SKIP,
    ST_NORM1, ST_MLP_FC1, ST_MLP_FC2, ST_DECODER, ST_COUNT
};
static const char* kStageNames[ST_COUNT] = {
    "encoder", "norm0_stats", "forward_transform.dft", "forward_transform.legendre", "dhconv",
    "inverse_transform.legendre", "inverse_transform.dft", "inner_skip+activation", "norm1_stats", "mlp.fc1",
    "mlp.fc2+outer_skip", "decoder"};

struct StageTimer {
    hipStream_t s;
    std::vector<hipEvent_t> ev;
    std::vector<int> stage;
    hipError_t err = hipSuccess;
    explicit StageTimer(hipStream_t st) : s(st) { push(-1); }
    void push(int st) {
        hipEvent_t e;
        hipError_t r = hipEventCreate(&e);
        if (r == hipSuccess) r = hipEventRecord(e, s);
        if (r != hipSuccess && err == hipSuccess) err = r;
        ev.push_back(e);
        stage.push_back(st);
    }
    hipError_t finish(float* ms, int* calls) {
        hipError_t r = hipStreamSynchronize(s);
        if (r != hipSuccess) return r;
        for (int i = 0; i < ST_COUNT; ++i) { ms[i] = 0.f; if (calls) calls[i] = 0; }
        for (size_t i = 1; i < ev.size(); ++i) {
            float t = 0.f;
            r = hipEventElapsedTime(&t, ev[i - 1], ev[i]);
            if (r != hipSuccess) return r;
            ms[stage[i]] += t;
            if (calls) calls[stage[i]] += 1;
        }
        return err;
    }
    ~StageTimer() { for (auto e : ev) (void)hipEventDestroy(e); }
};
#define MARK(st) do { if (f.tm) f.tm->push(st); } while (0)

// What the enqueue steps of one forward share: the handle, where to launch, views of the workspace, and the few values one step
// leaves for the next.
struct Fwd {
    const ace_sfno* n; int B; hipStream_t s; StageTimer* tm; const float* noise;
    const FwdRoute* route;
    // resolution of the launches being enqueued: the data grid, or (scale_factor != 1, between the first filter's inverse transform
    // and the last one's) the inner grid
    long HW;
    float *h, *hn;                   // block input / output
    float *sc0, *sh0, *sc1, *sh1;    // instance-norm affines of norm0 / norm1, per (sample, channel)
    _Float16 *PAh, *PAl, *PBh, *PBl; // planes of P (T / pack passes) and P2 (block input h)
    float *part_h, *part_t;          // row-statistics partials of h and T
    const float* skip_in; const unsigned* skip_in_slot;   // second source of the big-skip concat
    // left by a block's norm0 / transforms for its body
    const float *a0, *b0;            // norm0 as an affine applied on load by every consumer (never materialised)
    const float *res, *ra, *rb;      // the residual: x_norm as (h, a0, b0), or the round-tripped input of a mixed-grid block
    bool n0_planes, skip_pack_rode;  // reported by the conditional norm / the forward FFT launch

    unsigned* slot(int k) const { return range_slot(n, k); }
    unsigned* hslot(int i) const { return slot(8 + i % 8); }   // block-input slots are shared cyclically for deep nets
    long actB() const { return (long)n->C * HW; }              // per-sample stride of a C-channel activation
    const float* W(const std::string& name) const { return n->w(name); }
    const Weight& wt(const std::string& name) const { return *n->weights[n->index.at(name)]; }
    // lo planes at the resolution being enqueued (the hi plane starts the buffer)
    _Float16* Pl() const { return PAh ? PAh + (size_t)n->Bmax * n->C * HW : nullptr; }
    _Float16* Uh() const { return reinterpret_cast<_Float16*>(n->U.p); }
    _Float16* Ul() const { return Uh() + (size_t)n->Bmax * n->hid * HW; }
};

// one 1x1 convolution = one batched GEMM launch.  A operand: (ptr, pitch, per-sample stride); bias: (ptr, per-sample stride)
struct ConvW { const float* w; int pitch; long sw; const float* bias; long sbias; const float* hi; const float* lo; float ascale; };
static ConvW conv_weight(const ace_sfno* n, const std::string& wname, const std::string& bname) {
    const Weight& w = *n->weights[n->index.at(wname)];
    return ConvW{w.buf.p, w.pitch, 0, bname.empty() ? nullptr : n->w(bname), 0, w.hi.p, w.lo.p, w.ascale};
}
static int conv(const Fwd& f, const ConvW& cw, const float* in, long in_bstride, int cin, const float* in2,
                long in2_bstride, int K1, float* out, int cout, const float* R, long r_bstride, const float* rsc,
                const float* rsh, int act, const float* bsc = nullptr, const float* bsh = nullptr,
                const unsigned* bmax = nullptr, const unsigned* bmax2 = nullptr, unsigned* omax = nullptr) {
    GemmArgs g;
    g.bsc = bsc; g.bsh = bsh; g.sbs = bsc ? cin : 0;
    g.omax = omax;
    g.A = cw.w; g.lda = cw.pitch; g.sA = cw.sw; g.a_kpad = cw.pitch;
    g.B = in; g.ldb = f.HW; g.sB = in_bstride;
    g.B2 = in2; g.ldb2 = f.HW; g.sB2 = in2_bstride; g.K1 = in2 ? K1 : -1;
    g.C = out; g.ldc = f.HW; g.sC = (long)cout * f.HW;
    g.bias = cw.bias; g.sbias = cw.sbias;
    g.R = R; g.ldr = f.HW; g.sR = r_bstride;
    g.rsc = rsc; g.rsh = rsh; g.srs = rsc ? cout : 0;
    g.M = cout; g.N = (int)f.HW; g.K = cin; g.nbatch = f.B; g.act = act;
    if (f.n->cfg.precision == 1 && cw.hi && cw.sw == 0 && bmax && gemm_f16x3_eligible(g)) {
        // compensated fp16 with the B scale derived in-kernel from max|B| (slot written by B's producer)
        if (g.act == ACT_GELU) g.act = ACT_GELU_FAST;  // the epilogue is on the critical path of this engine
        ACE_HIP_TRY(launch_gemm_f16x3(g, cw.hi, cw.lo, cw.ascale, 1.0f, f.s, bmax, omax, (in2 ? bmax2 : nullptr)));
        return ACE_OK;
    }
    ACE_HIP_TRY(launch_gemm(g, f.s));
    return ACE_OK;
}

// f16x3 "v4": 1x1 convolution whose input already is in P format (fp16 hi/lo planes [cin/8][HW][8] per sample, scaled
// from the bound in `in_slot`).  Output: fp32 (+ omax) and/or P-format planes for the next convolution.
static int pack_act(const Fwd& f, const float* x, long x_bs, int cin, const float* sc, const float* sh, const unsigned* slot,
                    void* hi, void* lo) {
    ACE_HIP_TRY(launch_pack_pformat(x, f.HW, x_bs, cin, (int)f.HW, f.B, sc, sh, sc ? cin : 0, slot, hi, lo, f.HW, (long)cin * f.HW, f.s));
    return ACE_OK;
}
struct PkOpts {
    // A: static tiled planes of `w`, or per-sample folded planes (fhi/flo with scale slot fslot)
    const Weight* w = nullptr;
    const void* fhi = nullptr; const void* flo = nullptr; const unsigned* fslot = nullptr; long f_stride = 0;
    const float* bias = nullptr; long sbias = 0;
    const void* bhi = nullptr; const void* blo = nullptr; int cin = 0; const unsigned* in_slot = nullptr;
    float* out = nullptr; int cout = 0; unsigned* omax = nullptr;
    const float* R = nullptr; long r_bs = 0; const float* rsc = nullptr; const float* rsh = nullptr;
    int act = ACT_NONE;
    void* ohi = nullptr; void* olo = nullptr; float cb = 0.f; unsigned* cslot = nullptr;
    const unsigned* cinb = nullptr; const unsigned* rmax = nullptr;
    float* part = nullptr;
};
static int conv_packed(const Fwd& f, const PkOpts& o) {
    Gemm4Args a;
    if (o.fhi) {
        a.Ahi = static_cast<const _Float16*>(o.fhi); a.Alo = static_cast<const _Float16*>(o.flo);
        a.sA = o.f_stride; a.amax = o.fslot;
    } else {
        a.Ahi = reinterpret_cast<const _Float16*>(o.w->thi.p); a.Alo = reinterpret_cast<const _Float16*>(o.w->tlo.p);
        a.sA = 0; a.ascale = o.w->ascale;
    }
    a.lda = o.w->pitch; a.a_tiled = 1;
    a.Bhi = static_cast<const _Float16*>(o.bhi); a.Blo = static_cast<const _Float16*>(o.blo);
    a.ldn = f.HW; a.sB = (long)o.cin * f.HW; a.bmax = o.in_slot;
    a.C = o.out; a.ldc = f.HW; a.sC = (long)o.cout * f.HW; a.omax = o.omax;
    a.Chi = static_cast<_Float16*>(o.ohi); a.Clo = static_cast<_Float16*>(o.olo); a.ldnc = f.HW; a.sCp = (long)o.cout * f.HW;
    a.cw = o.w->winf; a.cb = o.cb; a.cslot = o.cslot; a.cinb = o.cinb; a.rmax = o.rmax;
    a.part = reinterpret_cast<float4*>(o.part);
    a.bias = o.bias; a.sbias = o.sbias;
    a.R = o.R; a.ldr = f.HW; a.sR = o.r_bs; a.rsc = o.rsc; a.rsh = o.rsh; a.srs = o.rsc ? o.cout : 0;
    a.M = o.cout; a.N = (int)f.HW; a.K = o.cin; a.nbatch = f.B;
    a.act = o.act == ACT_GELU ? ACT_GELU_FAST : o.act;
    ACE_HIP_TRY(launch_gemm_f16x3_packed(a, f.s));
    return ACE_OK;
}
// conv_ws.hip / conv_wl.hip: what every launch shares - a cin-channel input as planes at the resolution being enqueued
static ConvStripArgs strip_args(const Fwd& f, const _Float16* xhi, const _Float16* xlo, const unsigned* xslot, int cin, int cout, int act) {
    ConvStripArgs k;
    k.Xhi = xhi; k.Xlo = xlo; k.ldn = f.HW; k.sX = (long)cin * f.HW; k.xslot = xslot;
    k.C = cin; k.M = cout; k.HW = (int)f.HW; k.nbatch = f.B; k.act = act;
    return k;
}
static void static_frags(ConvStripArgs& k, const Weight& w, const float* bias) {   // ... with the fragments packed at upload
    k.A = reinterpret_cast<const _Float16*>(w.frag0.p); k.sA = 0; k.ascale = w.ascale;
    k.bias = bias; k.sbias = 0;
}

// One conditional layer norm (layers.py:245-318): a single MFMA pass (cln_mfma.hip) where the shape allows it and the
// conditioning weights were packed at upload, else statistics + apply (kernels.hip).
// planes (optional): where the single-pass kernel can, it also writes y as the P-format operand of the packed convolutions
// (scaled by a bound it publishes to omax) - *planes_done says so, the caller then skips its pack pass; with
// fp32_needed = false that is the ONLY output (y untouched).
static int cond_norm(const Fwd& f, const float* x, float* y, const std::string& q, int Cc, unsigned* omax, _Float16* phi = nullptr,
                     _Float16* plo = nullptr, bool fp32_needed = true, bool* planes_done = nullptr) {
    const ace_sfno* n = f.n;
    const int J = n->cfg.noise_embed_dim;
    const Weight* wsc = n->find(q + "W_scale_2d.weight");
    const Weight* wbi = n->find(q + "W_bias_2d.weight");
    const Weight* wga = n->find(q + "norm.weight");
    const Weight* wbe = n->find(q + "norm.bias");
    if (planes_done) *planes_done = false;
    ClnMfmaArgs a;
    a.x = x; a.y = y; a.sx = (long)Cc * f.HW; a.C = Cc; a.HW = f.HW; a.nbatch = f.B; a.eps = 1e-5f; a.omax = omax;
    a.gamma = f.W(q + "norm.weight"); a.beta = f.W(q + "norm.bias");
    if (n->cfg.precision == 1 && f.noise && wsc && wbi && wsc->frag0.p && wbi->frag0.p && !n->sw.no_cln_mfma) {
        a.cond = f.noise; a.scond = (long)J * f.HW; a.J = J; a.cslot = f.slot(16 + 12 * n->cfg.num_layers);
        a.As = reinterpret_cast<const _Float16*>(wsc->frag0.p); a.Ab = reinterpret_cast<const _Float16*>(wbi->frag0.p);
        a.ascale_s = wsc->ascale; a.ascale_b = wbi->ascale;
        if (phi && plo && omax && !n->sw.no_cln_planes && cln_mfma_planes_ok(a) && (!a.gamma || (wga && wbe))) {
            a.Phi = phi; a.Plo = plo; a.sP = (long)Cc * f.HW;
            a.gmax = a.gamma ? wga->absmax : 1.f; a.bmax = a.gamma ? wbe->absmax : 0.f;
            a.ws_inf = wsc->winf; a.wb_inf = wbi->winf;
            if (!fp32_needed) a.y = nullptr;
        }
        if (cln_mfma_eligible(a)) {
            ACE_HIP_TRY(launch_cln_mfma(a, f.s));
            if (planes_done) *planes_done = a.Phi != nullptr;
            return ACE_OK;
        }
        a.Phi = a.Plo = nullptr; a.y = y;
    }
    ACE_HIP_TRY(launch_cond_layer_norm(x, f.noise, a.gamma, a.beta, f.W(q + "W_scale_2d.weight"), f.W(q + "W_bias_2d.weight"), 1e-5f,
                                   n->cln_stats.p, y, f.B, Cc, J, f.HW, f.s, omax));
    return ACE_OK;
}

// ---- encoder (sfnonet.py:721-733): [conv+bias, act] x encoder_layers, conv (no bias), + pos_embed -> f.h
static int enqueue_encoder(Fwd& f, const float* in) {
    const ace_sfno* n = f.n;
    const ace_sfno_config& c = n->cfg;
    const FwdRoute& r = *f.route;
    const int C = n->C, Cin = c.in_chans, act = c.activation_function;
    const long HW = f.HW, actB = f.actB();
    if (c.precision == 1) {
        ACE_HIP_TRY(launch_zero_u32(f.slot(0), (long)n->amax.n, f.s));
        ACE_HIP_TRY(launch_absmax(in, (long)f.B * Cin * HW, f.slot(0), f.s));
    }
    const float* cur = in;
    long cur_bs = (long)Cin * HW;
    int curC = Cin;
    float* ping[2] = {n->Y.p, n->T.p};
    if (r.enc_hidden_planes) {   // P holds the hidden activation as planes scaled from slot(1)
        const Weight& b0 = f.wt("encoder.0.bias");
        const int cin8 = (Cin + 7) / 8 * 8;
        _Float16* Ih = reinterpret_cast<_Float16*>(n->inP.p);
        _Float16* Il = Ih + (size_t)n->Bmax * cin8 * HW;
        ACE_HIP_TRY(launch_pack_pformat(in, HW, (long)Cin * HW, Cin, (int)HW, f.B, nullptr, nullptr, 0, f.slot(0), Ih, Il, HW, (long)cin8 * HW, f.s));
        PkOpts o;
        o.w = &f.wt("encoder.0.weight"); o.bias = b0.buf.p;
        o.bhi = Ih; o.blo = Il; o.cin = cin8; o.in_slot = f.slot(0);
        o.cout = C; o.act = act;
        o.ohi = f.PAh; o.olo = f.PAl; o.cb = b0.absmax; o.cslot = f.slot(1);
        ACE_TRY(conv_packed(f, o));
    } else {
        for (int j = 0; j < c.encoder_layers; ++j) {
            const std::string p = "encoder." + std::to_string(2 * j);
            ACE_TRY(conv(f, conv_weight(n, p + ".weight", p + ".bias"), cur, cur_bs, curC, nullptr, 0, -1, ping[j & 1], C,
                         nullptr, 0, nullptr, nullptr, act, nullptr, nullptr, f.slot(j), nullptr, f.slot(1 + j)));
            cur = ping[j & 1]; cur_bs = actB; curC = C;
        }
    }
    const std::string last = "encoder." + std::to_string(2 * c.encoder_layers) + ".weight";
    if (r.enc_planes) {
        const Weight& we = f.wt(last);
        if (!r.enc_hidden_planes) ACE_TRY(pack_act(f, cur, cur_bs, C, nullptr, nullptr, f.slot(c.encoder_layers), f.PAh, f.PAl));
        ConvStripArgs k = strip_args(f, f.PAh, f.PAl, f.slot(c.encoder_layers), C, C, ACT_NONE);
        static_frags(k, we, n->zero_c.p);
        k.R = f.W("pos_embed"); k.sR = 0;
        if (!r.enc_planes_only) { k.Cf = f.h; k.sCf = actB; }
        k.Chi = f.PBh; k.Clo = f.PBl; k.sCp = (long)C * HW; k.cslot = f.hslot(0);
        k.cw = we.winf; k.cb = 0.f; k.rmax = reinterpret_cast<const unsigned*>(n->pe_slot.p);
        k.part = reinterpret_cast<float4*>(f.part_h); k.nstrips32 = r.enc_nparts;
        ACE_HIP_TRY(launch_conv_ws(k, f.s));
    } else {
        ACE_TRY(conv(f, conv_weight(n, last, ""), cur, cur_bs, curC, nullptr, 0, -1, f.h, C, c.pos_embed ? f.W("pos_embed") : nullptr, 0,
                     nullptr, nullptr, ACT_NONE, nullptr, nullptr, f.slot(c.encoder_layers), nullptr, f.hslot(0)));
    }
    MARK(ST_ENCODER);
    if (n->taps_on) ACE_HIP_TRY(hipMemcpyAsync(n->taps[0].p, f.h, sizeof(float) * f.B * actB, hipMemcpyDeviceToDevice, f.s));
    return ACE_OK;
}

// second source of the decoder's big-skip concat: the input, band-limited (residual_filter_factor) or normalised (normalize_big_skip)
static int enqueue_big_skip_source(Fwd& f, const float* in) {
    const ace_sfno* n = f.n;
    const ace_sfno_config& c = n->cfg;
    const int Cin = c.in_chans;
    f.skip_in = in;
    f.skip_in_slot = f.slot(0);
    if (f.route->noise_range)
        ACE_HIP_TRY(launch_absmax(f.noise, (long)f.B * c.noise_embed_dim * f.HW, f.slot(16 + 12 * c.num_layers), f.s));
    if (n->plan_res) {   // residual = residual_filter_up(residual_filter_down(x)) (sfnonet.py:715-716), exact fp32; its range into slot 7
        const long NR = (long)f.B * 2 * Cin;
        // (an fp32 plan: no folded kernels, so neither pair takes the polar cut - asked all the same, in the one place that decides)
        const int* mcut = forward_pair_mcut(*n->plan_res, n->resX.p, n->resD.p, NR, nullptr, nullptr, false);
        ACE_TRY(run_dft_forward(*n->plan_res, in, nullptr, nullptr, n->resX.p, f.B, Cin, f.s, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, mcut));
        ACE_TRY(run_legendre_forward(*n->plan_res, n->resX.p, n->resD.p, NR, f.s));
        const InversePair pr = inverse_pair(*n->plan_res, n->resD.p, n->resX.p, NR, nullptr, n->inF.p, f.B, Cin);
        ACE_TRY(run_legendre_inverse(*n->plan_res, n->resD.p, n->resX.p, NR, f.s, nullptr, false, pr.skip_dead));
        ACE_TRY(run_dft_inverse(*n->plan_res, n->resX.p, nullptr, n->inF.p, f.B, Cin, f.s, f.slot(7), pr.mcut));
        f.skip_in = n->inF.p;
        f.skip_in_slot = f.slot(7);
    }
    if (c.normalization_layer == 2 && c.big_skip && c.normalize_big_skip) {
        ACE_TRY(cond_norm(f, in, n->inN.p, "norm_big_skip.", Cin, f.slot(7)));
        f.skip_in = n->inN.p;
        f.skip_in_slot = f.slot(7);
    }
    return ACE_OK;
}

// norm0.  Instance norm: an affine (f.a0, f.b0) applied on load by every consumer, never materialised.  Conditional layer norm
// (NoiseConditionedSFNO) and "layer_norm" (nn.LayerNorm over (H, W) with an (H, W) affine, sfnonet.py:584-592 - a per-PIXEL affine
// does not fold into the consumers' weights): materialised in place, with their true max in the slot of the instance-norm bound.
static int enqueue_norm0(Fwd& f, int i, const BlockRoute& b) {
    const ace_sfno* n = f.n;
    const int C = n->C, sb = 16 + 12 * i, kind = n->cfg.normalization_layer;
    const std::string p = "blocks." + std::to_string(i) + ".";
    if (n->cfg.precision == 1 && i + 1 >= 8) ACE_HIP_TRY(launch_zero_u32(f.hslot(i + 1), AMAX_SHARDS, f.s));
    f.a0 = f.b0 = nullptr;
    f.n0_planes = false;
    if (kind == 0) return ACE_OK;
    if (kind == 2) {   // x_norm = CLN0(h; noise), in place: the block never needs the un-normalised h again (sfnonet.py:388-437)
        ACE_TRY(cond_norm(f, f.h, f.h, p + "norm0.", C, f.slot(sb + 3), b.n0_to_planes ? f.PAh : nullptr,
                          b.n0_to_planes ? f.Pl() : nullptr, true, &f.n0_planes));
    } else if (kind == 3) {   // x_norm = LayerNorm_(H, W)(h), in place
        ACE_HIP_TRY(launch_spatial_layer_norm(f.h, f.W(p + "norm0.weight"), f.W(p + "norm0.bias"), 1e-6f, (long)f.B * C, f.HW, f.h, f.slot(sb + 3), f.s));
    } else {
        if (b.in_planes)   // statistics of h came out of the producer's epilogue
            ACE_HIP_TRY(launch_instnorm_finalize(reinterpret_cast<const float4*>(f.part_h), b.in_nparts, f.B, C, f.HW,
                                             f.W(p + "norm0.weight"), f.W(p + "norm0.bias"), 1e-6f, f.sc0, f.sh0, f.slot(sb + 3), f.s));
        else
            ACE_HIP_TRY(launch_instnorm_stats(f.h, f.W(p + "norm0.weight"), f.W(p + "norm0.bias"), 1e-6f, f.B, C, f.HW, f.sc0, f.sh0, f.s,
                                          f.slot(sb + 3)));
        f.a0 = f.sc0; f.b0 = f.sh0;
    }
    MARK(ST_NORM0);
    return ACE_OK;
}

// spectral filter, first half (s2convolutions.py:162-197): longitude DFT and Legendre transform of x_norm; on a mixed-grid block
// also the residual = inverse(forward(x_norm)) on the output grid
static int enqueue_forward_transform(Fwd& f, int i, const BlockRoute& b) {
    const ace_sfno* n = f.n;
    const int C = n->C, sb = 16 + 12 * i, B = f.B;
    const long N2 = (long)B * 2 * C;
    unsigned *xmax = f.slot(sb + 0), *dmax = f.slot(sb + 1);
    // (Round 4 tried packing the inner skip's folded weights on a side stream beside the SHT chain - they depend on norm0's
    // statistics only.  Same box, whole step in a hipGraph: 5.76 -> 5.86 ms; the fork / join edges cost more than the 7 us
    // kernel they hide.  profiles/r04_s3_kdur_side_pack_*.txt)
    PackFragArgs skip_pack;
    if (b.ride_skip_pack) {
        const std::string p = "blocks." + std::to_string(i) + ".";
        const Weight& wsk = f.wt(p + "inner_skip.weight");
        skip_pack.W = wsk.buf.p; skip_pack.ldw = wsk.pitch; skip_pack.O = C; skip_pack.I = C; skip_pack.order = 0;
        skip_pack.a = f.a0; skip_pack.wmax = wsk.wabs; skip_pack.scale_static = 1.f; skip_pack.wslot = f.slot(sb + 8);
        skip_pack.dst = reinterpret_cast<_Float16*>(n->Wq0.p); skip_pack.sDst = (long)C * C * 2;
        skip_pack.b = f.b0; skip_pack.bias = f.wt(p + "inner_skip.bias").buf.p; skip_pack.bf = n->bf0.p; skip_pack.nsamples = B;
    }
    const PackFragArgs* ride = b.ride_skip_pack ? &skip_pack : nullptr;
    const int* mcut = forward_pair_mcut(*b.fwd, n->X.p, n->D.p, N2, xmax, dmax, b.dplanes);
    if (b.in_planes_only)
        ACE_TRY(run_dft_forward(*b.fwd, nullptr, f.a0, f.b0, n->X.p, B, C, f.s, xmax, f.PBh, f.PBl, (long)C * f.HW, f.hslot(i), ride, &f.skip_pack_rode, mcut));
    else
        ACE_TRY(run_dft_forward(*b.fwd, f.h, f.a0, f.b0, n->X.p, B, C, f.s, xmax, nullptr, nullptr, 0, nullptr, ride, &f.skip_pack_rode, mcut));
    MARK(ST_DFT_FWD);
    ACE_TRY(run_legendre_forward(*b.fwd, n->X.p, n->D.p, N2, f.s, xmax, dmax, b.dplanes));
    MARK(ST_LEGENDRE_FWD);
    f.res = f.h; f.ra = f.a0; f.rb = f.b0;
    if (b.scale_residual) {
        const InversePair pr = inverse_pair(*b.inv, n->D.p, n->X.p, N2, dmax, n->R.p, B, C);
        ACE_TRY(run_legendre_inverse(*b.inv, n->D.p, n->X.p, N2, f.s, dmax, false, pr.skip_dead));
        MARK(ST_LEGENDRE_INV);
        ACE_TRY(run_dft_inverse(*b.inv, n->X.p, nullptr, n->R.p, B, C, f.s, nullptr, pr.mcut));
        MARK(ST_DFT_INV);
        f.res = n->R.p; f.ra = nullptr; f.rb = nullptr;
    }
    return ACE_OK;
}

// the filter itself.  dhconv (contractions.py:183-195): per l, (m,b) x 2C times real 2C x 2C
static int enqueue_contraction(Fwd& f, int i, const BlockRoute& b) {
    const ace_sfno* n = f.n;
    const int C = n->C, sb = 16 + 12 * i, B = f.B;
    const long N2 = (long)B * 2 * C;
    unsigned *dmax = f.slot(sb + 1), *emax = f.slot(sb + 2);
    switch (b.filter) {
    case FLT_DHCONV_STRIP:
        ACE_HIP_TRY(launch_dhconv_strip(dhconv_strip_args(n, i, B, dmax, emax), f.s));
        break;
    case FLT_PACKED_TILE: {
        Gemm4Args a;
        a.Ahi = reinterpret_cast<const _Float16*>(n->D.p);
        a.Alo = a.Ahi + (size_t)n->L * n->Mm * N2;
        a.lda = 2 * C; a.sA = (long)n->Mm * N2; a.amax = dmax;
        a.Bhi = reinterpret_cast<const _Float16*>(n->wx_hi[i].p);
        a.Blo = reinterpret_cast<const _Float16*>(n->wx_lo[i].p);
        a.ldn = 2 * C; a.sB = (long)2 * C * 2 * C; a.bscale = n->wx_scale[i];
        if (n->wx_compact[i]) { a.cplx = C; a.ldn = C; a.sB = (long)2 * C * C; a.tile = 1; }
        a.C = n->E.p; a.ldc = 2 * C; a.sC = (long)n->Mm * N2; a.omax = emax;
        a.M = n->Mm * B; a.N = 2 * C; a.K = 2 * C; a.nbatch = n->L;
        a.tri = TRI_ROWS_LE_BATCH; a.trimul = B;
        ACE_HIP_TRY(launch_gemm_f16x3_packed(a, f.s));
        break;
    }
    case FLT_ADYN_F16X3:
    case FLT_FP32: {
        GemmArgs g;
        g.A = n->D.p; g.lda = 2 * C; g.sA = (long)n->Mm * N2;
        g.B = n->wx[i].p; g.ldb = 2 * C; g.sB = (long)2 * C * 2 * C;
        g.C = n->E.p; g.ldc = 2 * C; g.sC = (long)n->Mm * N2;
        g.M = n->Mm * B; g.N = 2 * C; g.K = 2 * C; g.nbatch = n->L; g.a_kpad = 2 * C;
        g.tri = TRI_ROWS_LE_BATCH; g.trimul = B;
        g.omax = emax;
        if (b.filter == FLT_ADYN_F16X3)
            ACE_HIP_TRY(launch_gemm_f16x3_adyn(g, n->wx_hi[i].p, n->wx_lo[i].p, 2 * C, (long)2 * C * 2 * C, n->wx_scale[i], dmax, emax, f.s));
        else
            ACE_HIP_TRY(launch_gemm(g, f.s));
        break;
    }
    case FLT_DIAGONAL:
        ACE_HIP_TRY(launch_contract_diagonal(n->D.p, f.W("blocks." + std::to_string(i) + ".filter.filter.weight"), n->E.p, B, C, C, n->L, n->Mm, f.s, emax));
        break;
    }
    MARK(ST_CONTRACT);
    return ACE_OK;
}

// spectral filter, second half: inverse transforms + bias -> Y.  What follows works on the filter's OUTPUT grid.
static int enqueue_inverse_transform(Fwd& f, int i, const BlockRoute& b) {
    const ace_sfno* n = f.n;
    const int sb = 16 + 12 * i;
    const InversePair pr = inverse_pair(*b.inv, n->E.p, n->X.p, (long)f.B * 2 * n->C, f.slot(sb + 2), n->Y.p, f.B, n->C);
    ACE_TRY(run_legendre_inverse(*b.inv, n->E.p, n->X.p, (long)f.B * 2 * n->C, f.s, f.slot(sb + 2), false, pr.skip_dead));
    MARK(ST_LEGENDRE_INV);
    ACE_TRY(run_dft_inverse(*b.inv, n->X.p, f.W("blocks." + std::to_string(i) + ".filter.filter.bias"), n->Y.p, f.B, n->C, f.s, f.slot(sb + 7), pr.mcut));
    MARK(ST_DFT_INV);
    f.HW = b.hw_out;
    return ACE_OK;
}

// Body of a block with the instance norms fused away: x = act(filter + inner_skip(residual)), norm1 -> MLP -> + residual
// (sfnonet.py:229-250).  Every conv input is P-format planes written by its producer's epilogue, the norm affine is folded into the
// consumer's weights, the norm statistics come out of the producer's epilogue: no pass over an activation other than the GEMMs.
static int enqueue_fused_body(Fwd& f, int i, const BlockRoute& b) {
    const ace_sfno* n = f.n;
    const int C = n->C, hid = n->hid, B = f.B, act = n->cfg.activation_function, sb = 16 + 12 * i;
    const long HW = f.HW, actB = f.actB();
    hipStream_t s = f.s;
    const std::string p = "blocks." + std::to_string(i) + ".";
    const Weight &ws = f.wt(p + "inner_skip.weight"), &bsw = f.wt(p + "inner_skip.bias");
    const Weight &w1 = f.wt(p + "mlp.fwd.0.weight"), &b1w = f.wt(p + "mlp.fwd.0.bias");
    const Weight &w2 = f.wt(p + "mlp.fwd.2.weight"), &b2w = f.wt(p + "mlp.fwd.2.bias");
    const long cp = ws.pitch;
    _Float16* F0h = reinterpret_cast<_Float16*>(n->Wp0.p);
    const long f0s = (long)((C + 15) / 16 * 16) * cp;
    _Float16* F0l = F0h + (size_t)n->Bmax * f0s;
    _Float16* F1h = reinterpret_cast<_Float16*>(n->Wp1.p);
    const long f1s = (long)((hid + 15) / 16 * 16) * cp;
    _Float16* F1l = F1h + (size_t)n->Bmax * f1s;
    _Float16 *Uh = f.Uh(), *Ul = f.Ul();

    // inner skip: T = act(Y + Ws norm0(h) + bs), written as P-format planes only (+ its row statistics)
    const float* skip_bias = bsw.buf.p;
    long skip_sbias = 0;
    const unsigned* in_slot = f.slot(b.skip_slot);
    if (b.in_planes) {   // h planes from the producer; the affine goes into the weights
        if (b.skip != CONV_WS)
            ACE_HIP_TRY(launch_fold_affine_f16(ws.buf.p, ws.pitch, ws.wabs, f.ra, f.rb, bsw.buf.p, F0h, F0l, n->bf0.p, B, C, C, cp, f0s, f.slot(sb + 8), s));
        skip_bias = n->bf0.p; skip_sbias = C; in_slot = f.hslot(i);
    } else {             // first block: normalise + split h in one pass
        ACE_TRY(pack_act(f, f.res, actB, C, f.ra, f.rb, in_slot, f.PBh, f.PBl));
    }
    if (b.skip == CONV_WS) {
        ConvStripArgs k = strip_args(f, f.PBh, f.PBl, in_slot, C, C, ACT_GELU);
        if (b.in_planes) {
            _Float16* Q0 = reinterpret_cast<_Float16*>(n->Wq0.p);
            if (!f.skip_pack_rode)   // (packed by rider workgroups of this block's forward FFT otherwise)
                ACE_HIP_TRY(launch_pack_conv_frag(ws.buf.p, ws.pitch, C, C, 0, f.ra, ws.wabs, 1.f, f.slot(sb + 8), Q0, (long)C * C * 2, B, s,
                                              f.rb, bsw.buf.p, n->bf0.p));
            k.A = Q0; k.sA = (long)C * C * 2; k.aslot = f.slot(sb + 8);
        } else {
            k.A = reinterpret_cast<const _Float16*>(ws.frag0.p); k.sA = 0; k.ascale = ws.ascale;
        }
        k.bias = skip_bias; k.sbias = skip_sbias;
        k.R = n->Y.p; k.sR = actB;
        k.cw = ws.winf; k.cb = bsw.absmax; k.cinb = f.slot(sb + 3); k.rmax = f.slot(sb + 7);
        k.Chi = f.PAh; k.Clo = f.PAl; k.sCp = (long)C * HW; k.cslot = f.slot(sb + 4);
        k.part = reinterpret_cast<float4*>(f.part_t); k.nstrips32 = b.t_nparts;   // one partial per pixel group (accumulated in registers)
        ACE_HIP_TRY(launch_conv_ws(k, s));
    } else {
        PkOpts o;
        o.w = &ws; o.cin = C; o.cout = C; o.act = act;
        if (b.in_planes) { o.fhi = F0h; o.flo = F0l; o.fslot = f.slot(sb + 8); o.f_stride = f0s; }
        o.bias = skip_bias; o.sbias = skip_sbias;
        o.bhi = f.PBh; o.blo = f.PBl; o.in_slot = in_slot;
        o.R = n->Y.p; o.r_bs = actB;
        o.ohi = f.PAh; o.olo = f.PAl; o.cb = bsw.absmax; o.cslot = f.slot(sb + 4); o.cinb = f.slot(sb + 3); o.rmax = f.slot(sb + 7);
        o.part = f.part_t;
        ACE_TRY(conv_packed(f, o));
    }
    MARK(ST_INNER_SKIP);

    // norm1 statistics -> affine -> folded fc1 weights; fc1 writes U = act(.) as planes
    ACE_HIP_TRY(launch_instnorm_finalize(reinterpret_cast<const float4*>(f.part_t), b.t_nparts, B, C, HW, f.W(p + "norm1.weight"),
                                     f.W(p + "norm1.bias"), 1e-6f, f.sc1, f.sh1, f.slot(sb + 5), s));
    if (b.fc1 == CONV_WS || b.fc1 == CONV_WL) {
        _Float16* Q1 = reinterpret_cast<_Float16*>(n->Wq1.p);
        const long q1s = (long)hid * C * 2;
        // (pfold: W1 diag(a1), b1 + W1 b1' folded in the convolution's own prologue: +1.4 us against a 6.7 us launch)
        if (!b.pfold)
            ACE_HIP_TRY(launch_pack_conv_frag(w1.buf.p, w1.pitch, hid, C, 0, f.sc1, w1.wabs, 1.f, f.slot(sb + 9), Q1, q1s, B, s, f.sh1,
                                          b1w.buf.p, n->bf1.p));
        MARK(ST_NORM1);
        ConvStripArgs k = strip_args(f, f.PAh, f.PAl, f.slot(sb + 4), C, hid, ACT_GELU);
        if (b.pfold) {
            k.Wraw = w1.buf.p; k.ldw = w1.pitch; k.wabs = w1.wabs; k.fa = f.sc1; k.fb = f.sh1; k.sfa = C;
            k.bias = b1w.buf.p; k.sbias = 0;
        } else {
            k.A = Q1; k.sA = q1s; k.aslot = f.slot(sb + 9);
            k.bias = n->bf1.p; k.sbias = hid;
        }
        k.cw = w1.winf; k.cb = b1w.absmax; k.cinb = f.slot(sb + 5);
        k.Chi = Uh; k.Clo = Ul; k.sCp = (long)hid * HW; k.cslot = f.slot(sb + 6);
        ACE_HIP_TRY(b.fc1 == CONV_WL ? launch_conv_wl(k, s) : launch_conv_ws(k, s));
    } else {
        ACE_HIP_TRY(launch_fold_affine_f16(w1.buf.p, w1.pitch, w1.wabs, f.sc1, f.sh1, b1w.buf.p, F1h, F1l, n->bf1.p, B, hid, C, cp, f1s,
                                       f.slot(sb + 9), s));
        MARK(ST_NORM1);
        PkOpts f1;
        f1.w = &w1; f1.fhi = F1h; f1.flo = F1l; f1.fslot = f.slot(sb + 9); f1.f_stride = f1s;
        f1.bias = n->bf1.p; f1.sbias = hid;
        f1.bhi = f.PAh; f1.blo = f.PAl; f1.cin = C; f1.in_slot = f.slot(sb + 4);
        f1.cout = hid; f1.act = act;
        f1.ohi = Uh; f1.olo = Ul; f1.cb = b1w.absmax; f1.cslot = f.slot(sb + 6); f1.cinb = f.slot(sb + 5);
        ACE_TRY(conv_packed(f, f1));
    }
    MARK(ST_MLP_FC1);

    // fc2 + outer skip: h' as fp32 and / or as planes with statistics for the next block (then a bound instead of the true max
    // goes into the h slot)
    if (b.fc2 == CONV_WS) {
        ConvStripArgs k = strip_args(f, Uh, Ul, f.slot(sb + 6), hid, C, ACT_NONE);
        static_frags(k, w2, b2w.buf.p);
        k.rsc = f.ra; k.rsh = f.rb; k.srs = C;
        if (b.res_planes) { k.Rhi = f.PBh; k.Rlo = f.PBl; k.sRp = (long)C * HW; k.rslot = f.hslot(i); }
        else { k.R = f.res; k.sR = actB; }
        if (b.out_f32) { k.Cf = f.hn; k.sCf = actB; }
        if (b.out_planes) {
            k.Chi = f.PBh; k.Clo = f.PBl; k.sCp = (long)C * HW; k.cslot = f.hslot(i + 1);
            k.cw = w2.winf; k.cb = b2w.absmax; k.rmax = f.slot(sb + 3);
            k.part = reinterpret_cast<float4*>(f.part_h); k.nstrips32 = b.out_nparts;
        } else {
            k.omax = f.hslot(i + 1);
        }
        ACE_HIP_TRY(launch_conv_ws(k, s));
    } else {
        PkOpts f2;
        f2.w = &w2; f2.bias = b2w.buf.p;
        f2.bhi = Uh; f2.blo = Ul; f2.cin = hid; f2.in_slot = f.slot(sb + 6);
        f2.out = f.hn; f2.cout = C; f2.act = ACT_NONE;
        f2.R = f.res; f2.r_bs = actB; f2.rsc = f.ra; f2.rsh = f.rb;
        if (b.out_planes) {
            f2.ohi = f.PBh; f2.olo = f.PBl; f2.cb = b2w.absmax; f2.cslot = f.hslot(i + 1); f2.rmax = f.slot(sb + 3);
            f2.part = f.part_h;
        } else {
            f2.omax = f.hslot(i + 1);
        }
        ACE_TRY(conv_packed(f, f2));
    }
    return ACE_OK;
}

// norm1 of the other two bodies, on T: materialised in place (conditional norm / "layer_norm"; *planes: the conditional norm wrote
// the MLP's operand planes, and only them) or left as an affine (*a1, *b1) for the consumer (instance norm)
static int enqueue_norm1(Fwd& f, int i, const BlockRoute& b, const float** a1, const float** b1, bool* planes) {
    const ace_sfno* n = f.n;
    const int C = n->C, sb = 16 + 12 * i, kind = n->cfg.normalization_layer;
    const std::string p = "blocks." + std::to_string(i) + ".";
    *a1 = *b1 = nullptr;
    *planes = false;
    if (kind == 0) return ACE_OK;
    if (kind == 2) {
        ACE_TRY(cond_norm(f, n->T.p, n->T.p, p + "norm1.", C, f.slot(sb + 5), b.n1_to_planes ? f.PAh : nullptr,
                          b.n1_to_planes ? f.Pl() : nullptr, false, planes));
    } else if (kind == 3) {
        ACE_HIP_TRY(launch_spatial_layer_norm(n->T.p, f.W(p + "norm1.weight"), f.W(p + "norm1.bias"), 1e-6f, (long)f.B * C, f.HW, n->T.p, f.slot(sb + 5), f.s));
    } else {
        ACE_HIP_TRY(launch_instnorm_stats(n->T.p, f.W(p + "norm1.weight"), f.W(p + "norm1.bias"), 1e-6f, f.B, C, f.HW, f.sc1, f.sh1, f.s,
                                      f.slot(sb + 5)));
        *a1 = f.sc1; *b1 = f.sh1;
    }
    MARK(ST_NORM1);
    return ACE_OK;
}

// Body of a block on the packed-operand engine with materialised norms (conditional / layer norm, or none): one pack pass per conv
// input unless the norm wrote the planes itself; fc1's epilogue writes U = act(.) straight in P format (bound-scaled), which fc2
// consumes by DMA - the hidden activation never exists in fp32
static int enqueue_packed_body(Fwd& f, int i, const BlockRoute& b) {
    const ace_sfno* n = f.n;
    const int C = n->C, hid = n->hid, act = n->cfg.activation_function, sb = 16 + 12 * i;
    const long HW = f.HW, actB = f.actB();
    const std::string p = "blocks." + std::to_string(i) + ".";
    const Weight& ws = f.wt(p + "inner_skip.weight");
    const unsigned* skip_max = f.slot(b.skip_slot);
    _Float16 *Ph = f.PAh, *Pl = f.Pl();
    if (!f.n0_planes) ACE_TRY(pack_act(f, f.res, actB, C, f.ra, f.rb, skip_max, Ph, Pl));
    if (b.skip == CONV_WS) {
        ConvStripArgs k = strip_args(f, Ph, Pl, skip_max, C, C, act);
        static_frags(k, ws, f.W(p + "inner_skip.bias"));
        k.R = n->Y.p; k.sR = actB;
        k.Cf = n->T.p; k.sCf = actB; k.omax = f.slot(sb + 4);
        ACE_HIP_TRY(launch_conv_ws(k, f.s));
    } else {
        PkOpts o;
        o.w = &ws; o.bias = f.W(p + "inner_skip.bias");
        o.bhi = Ph; o.blo = Pl; o.cin = C; o.in_slot = skip_max;
        o.out = n->T.p; o.cout = C; o.omax = f.slot(sb + 4);
        o.R = n->Y.p; o.r_bs = actB; o.act = act;
        ACE_TRY(conv_packed(f, o));
    }
    MARK(ST_INNER_SKIP);
    const float *a1, *b1;
    bool n1_planes;
    ACE_TRY(enqueue_norm1(f, i, b, &a1, &b1, &n1_planes));
    if (b.fc1 == CONV_NONE) {
        ACE_HIP_TRY(launch_rowaffine_add(n->T.p, a1, b1, f.res, f.ra, f.rb, f.hn, (long)f.B * C, HW, f.s));
        return ACE_OK;
    }
    const Weight &w1 = f.wt(p + "mlp.fwd.0.weight"), &b1w = f.wt(p + "mlp.fwd.0.bias");
    const unsigned* tmax = f.slot(b.t_slot);
    _Float16 *Uh = f.Uh(), *Ul = f.Ul();
    if (!n1_planes) ACE_TRY(pack_act(f, n->T.p, actB, C, a1, b1, tmax, Ph, Pl));
    if (b.fc1 == CONV_WL) {   // weights in LDS, unsynchronised waves
        ConvStripArgs k = strip_args(f, Ph, Pl, tmax, C, hid, ACT_GELU);
        static_frags(k, w1, b1w.buf.p);
        k.cw = w1.winf; k.cb = b1w.absmax;
        k.Chi = Uh; k.Clo = Ul; k.sCp = (long)hid * HW; k.cslot = f.slot(sb + 6);
        ACE_HIP_TRY(launch_conv_wl(k, f.s));
    } else {
        PkOpts o;
        o.w = &w1; o.bias = b1w.buf.p;
        o.bhi = Ph; o.blo = Pl; o.cin = C; o.in_slot = tmax;
        o.cout = hid; o.act = act;
        o.ohi = Uh; o.olo = Ul; o.cb = b1w.absmax; o.cslot = f.slot(sb + 6);
        ACE_TRY(conv_packed(f, o));
    }
    MARK(ST_MLP_FC1);
    PkOpts o;
    o.w = &f.wt(p + "mlp.fwd.2.weight"); o.bias = f.W(p + "mlp.fwd.2.bias");
    o.bhi = Uh; o.blo = Ul; o.cin = hid; o.in_slot = f.slot(sb + 6);
    o.out = f.hn; o.cout = C; o.omax = f.hslot(i + 1);
    o.R = f.res; o.r_bs = actB; o.rsc = f.ra; o.rsh = f.rb;
    ACE_TRY(conv_packed(f, o));
    return ACE_OK;
}

// Body of a block on the tile engines (fp32 mode, mixed-grid blocks, shapes the packed engine does not take): the convolutions
// read fp32 and apply the instance-norm affine on load.  (The fp32 mode used to fold it into a per-sample weight W diag(a),
// bias + W b for the direct-to-LDS engine: the products W a x then carry the mean of x through the fp32 accumulation, and at
// mean / std = 300 a block's output missed twice the fp32 reference's own error - tests/test_gpu_norm_dc.py (c).)
static int enqueue_plain_body(Fwd& f, int i, const BlockRoute& b) {
    const ace_sfno* n = f.n;
    const int C = n->C, hid = n->hid, act = n->cfg.activation_function, sb = 16 + 12 * i;
    const long actB = f.actB();
    const std::string p = "blocks." + std::to_string(i) + ".";
    ConvW wskip = conv_weight(n, p + "inner_skip.weight", p + "inner_skip.bias");
    ACE_TRY(conv(f, wskip, f.res, actB, C, nullptr, 0, -1, n->T.p, C, n->Y.p, actB, nullptr, nullptr, act,
                 f.ra, f.rb, f.slot(b.skip_slot), nullptr, f.slot(sb + 4)));
    MARK(ST_INNER_SKIP);
    const float *a1, *b1;
    bool n1_planes;
    ACE_TRY(enqueue_norm1(f, i, b, &a1, &b1, &n1_planes));
    if (b.fc1 == CONV_NONE) {
        ACE_HIP_TRY(launch_rowaffine_add(n->T.p, a1, b1, f.res, f.ra, f.rb, f.hn, (long)f.B * C, f.HW, f.s));
        return ACE_OK;
    }
    ConvW wfc1 = conv_weight(n, p + "mlp.fwd.0.weight", p + "mlp.fwd.0.bias");
    ACE_TRY(conv(f, wfc1, n->T.p, actB, C, nullptr, 0, -1, n->U.p, hid, nullptr, 0, nullptr, nullptr, act,
                 a1, b1, f.slot(b.t_slot), nullptr, f.slot(sb + 6)));
    MARK(ST_MLP_FC1);
    ACE_TRY(conv(f, conv_weight(n, p + "mlp.fwd.2.weight", p + "mlp.fwd.2.bias"), n->U.p, (long)hid * f.HW, hid, nullptr, 0, -1, f.hn,
                 C, f.res, actB, f.ra, f.rb, ACT_NONE, nullptr, nullptr, f.slot(sb + 6), nullptr, f.hslot(i + 1)));
    return ACE_OK;
}

// ---- decoder on cat(x, input) (sfnonet.py:741-747); the concat is two row sources of one GEMM
static int enqueue_decoder(Fwd& f, float* out) {
    const ace_sfno* n = f.n;
    const ace_sfno_config& c = n->cfg;
    const int C = n->C, Cin = c.in_chans;
    const long actB = f.actB();
    float* ping[2] = {n->Y.p, n->T.p};
    const float* cur = f.h;
    const unsigned* h_slot = c.use_mlp ? f.hslot(c.num_layers) : nullptr;   // the last block's range slot
    for (int j = 0; j < c.encoder_layers; ++j) {
        const std::string p = "decoder." + std::to_string(2 * j);
        const bool cat = (j == 0 && c.big_skip);
        ACE_TRY(conv(f, conv_weight(n, p + ".weight", p + ".bias"), cur, actB, cat ? C + Cin : C, cat ? f.skip_in : nullptr,
                     (long)Cin * f.HW, C, ping[j & 1], C, nullptr, 0, nullptr, nullptr, c.activation_function, nullptr, nullptr,
                     j == 0 ? h_slot : f.slot(3 + j), f.skip_in_slot, f.slot(4 + j)));
        cur = ping[j & 1];
    }
    // without hidden decoder layers the last convolution is the one that sees cat(x, input) and the last block's range slot
    const bool first = c.encoder_layers == 0, cat = first && c.big_skip;
    ACE_TRY(conv(f, conv_weight(n, "decoder." + std::to_string(2 * c.encoder_layers) + ".weight", ""), cur, actB, cat ? C + Cin : C,
                 cat ? f.skip_in : nullptr, (long)Cin * f.HW, cat ? C : -1, out, c.out_chans, nullptr, 0, nullptr, nullptr, ACT_NONE,
                 nullptr, nullptr, first ? h_slot : f.slot(3 + c.encoder_layers), cat ? f.skip_in_slot : nullptr, nullptr));
    MARK(ST_DECODER);
    return ACE_OK;
}

static int forward_impl(const ace_sfno* n, const float* in, float* out, int B, hipStream_t s, StageTimer* tm = nullptr,
                        const float* noise = nullptr) {
    const FwdRoute route = plan_route(n, B, noise != nullptr);
    if (route.err) return fail(ACE_ERR_STATE, route.err);
    const size_t bc = (size_t)n->Bmax * n->C;
    Fwd f{};
    f.n = n; f.B = B; f.s = s; f.tm = tm; f.noise = noise; f.route = &route;
    f.HW = n->HW;
    f.h = n->h0.p; f.hn = n->h1.p;
    f.sc0 = n->stats.p; f.sh0 = f.sc0 + bc; f.sc1 = f.sh0 + bc; f.sh1 = f.sc1 + bc;
    f.PAh = reinterpret_cast<_Float16*>(n->P.p);  f.PAl = f.PAh ? f.PAh + bc * n->HW : nullptr;
    f.PBh = reinterpret_cast<_Float16*>(n->P2.p); f.PBl = f.PBh ? f.PBh + bc * n->HW : nullptr;
    f.part_h = n->part.p;
    f.part_t = n->part.p ? n->part.p + (size_t)n->Bmax * n->nstrips * n->C * 4 : nullptr;

    ACE_TRY(enqueue_encoder(f, in));
    ACE_TRY(enqueue_big_skip_source(f, in));
    for (int i = 0; i < n->cfg.num_layers; ++i) {   // sfnonet.py:217-252
        const BlockRoute& b = route.blk[i];
        ACE_TRY(enqueue_norm0(f, i, b));
        ACE_TRY(enqueue_forward_transform(f, i, b));
        ACE_TRY(enqueue_contraction(f, i, b));
        ACE_TRY(enqueue_inverse_transform(f, i, b));
        if (b.body == BODY_FUSED) ACE_TRY(enqueue_fused_body(f, i, b));
        else if (b.body == BODY_PACKED) ACE_TRY(enqueue_packed_body(f, i, b));
        else ACE_TRY(enqueue_plain_body(f, i, b));
        MARK(ST_MLP_FC2);
        std::swap(f.h, f.hn);
        if (n->taps_on)
            ACE_HIP_TRY(hipMemcpyAsync(n->taps[i + 1].p, f.h, sizeof(float) * B * f.actB(), hipMemcpyDeviceToDevice, s));
    }
    if (n->cfg.normalization_layer == 1 && n->cfg.num_layers > 0) { n->norm_batch = B; n->norm_stream = s; }
    return enqueue_decoder(f, out);
}

static int check_ready(ace_sfno* n, const float* in, float* out, int batch) {
    if (!n || !in || !out) return fail(ACE_ERR_INVALID, "null argument");
    if (batch <= 0 || batch > n->Bmax)
        return fail(ACE_ERR_INVALID, "batch " + std::to_string(batch) + " outside [1, max_batch=" +
                                         std::to_string(n->Bmax) + "]");
    for (auto& w : n->weights)
        if (!w->set) return fail(ACE_ERR_STATE, "parameter '" + w->name + "' has not been set");
    return ACE_OK;
}

extern "C" int ace_sfno_forward(ace_sfno* n, const float* in, float* out, int batch, void* stream) {
    ACE_TRY(check_ready(n, in, out, batch));
    if (n->cfg.normalization_layer == 2)
        return fail(ACE_ERR_STATE, "this net is noise conditioned: call ace_sfno_forward_conditioned");
    return forward_impl(n, in, out, batch, static_cast<hipStream_t>(stream));
}

extern "C" int ace_sfno_forward_conditioned(ace_sfno* n, const float* in, const float* noise, float* out, int batch,
                                            void* stream) {
    ACE_TRY(check_ready(n, in, out, batch));
    if (n->cfg.normalization_layer != 2)
        return fail(ACE_ERR_STATE, "ace_sfno_forward_conditioned needs a net created with conditional layer norms");
    if (!noise && n->cfg.noise_embed_dim > 0) return fail(ACE_ERR_INVALID, "null noise");
    return forward_impl(n, in, out, batch, static_cast<hipStream_t>(stream), nullptr, noise);
}

#ifdef ACE_DEBUG_WS   // debugging builds only (tools/mkvar.sh dbg -DACE_DEBUG_WS): copy of an internal workspace after a forward
extern "C" long ace_debug_read_workspace(ace_sfno* n, const char* which, void* dst, long max_bytes) {
    const std::string w(which);
    DevBuf* b = w == "U" ? &n->U : w == "P" ? &n->P : w == "P2" ? &n->P2 : w == "part" ? &n->part : w == "Y" ? &n->Y : nullptr;
    if (!b || !b->p) return -1;
    const long bytes = std::min<long>((long)(b->n * sizeof(float)), max_bytes);
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    if (hipMemcpy(dst, b->p, bytes, hipMemcpyDeviceToHost) != hipSuccess) return -3;
    return bytes;
}
#endif

extern "C" int ace_sfno_sht_route(const ace_sfno* n, int* forward, int* inverse) {
    if (!n || !n->plan_lg) return fail(ACE_ERR_INVALID, "null argument");
    return ace_sht_plan_route(n->plan_lg.get(), forward, inverse);
}
extern "C" int ace_sfno_sht_cut(const ace_sfno* n, double* dead_share, int* kdrop) {
    if (!n || !n->plan_lg) return fail(ACE_ERR_INVALID, "null argument");
    return ace_sht_plan_cut(n->plan_lg.get(), dead_share, kdrop);
}
// The instance-norm affine the last forward applied: tables (batch, C) of norm0 (which = 0) or norm1 (which = 1) of the LAST block
// (the tables are shared by all blocks) and the range bound that norm published (maximum over the words of its slot; -1 where the
// precision publishes none).  Synchronises the stream of that forward, launches nothing.
extern "C" int ace_sfno_norm_affine(const ace_sfno* n, int which, float* scale, float* shift, float* bound) {
    if (!n || !scale || !shift || !bound || which < 0 || which > 1) return fail(ACE_ERR_INVALID, "null argument / which outside {0, 1}");
    if (n->norm_batch <= 0 || !n->stats.p) return fail(ACE_ERR_INVALID, "no instance-norm forward has run on this handle");
    ACE_HIP_TRY(hipStreamSynchronize(n->norm_stream));
    const size_t bc = (size_t)n->Bmax * n->C, nb = sizeof(float) * n->norm_batch * n->C;
    const float* sc = n->stats.p + (which ? 2 * bc : 0);
    ACE_HIP_TRY(hipMemcpy(scale, sc, nb, hipMemcpyDeviceToHost));
    ACE_HIP_TRY(hipMemcpy(shift, sc + bc, nb, hipMemcpyDeviceToHost));
    *bound = -1.f;
    if (const unsigned* slot = range_slot(n, 16 + 12 * (n->cfg.num_layers - 1) + (which ? 5 : 3))) {
        unsigned words[AMAX_SHARDS];
        ACE_HIP_TRY(hipMemcpy(words, slot, sizeof(words), hipMemcpyDeviceToHost));
        unsigned m = 0;   // bit patterns of non-negative floats order like the floats
        for (unsigned wd : words) m = wd > m ? wd : m;
        std::memcpy(bound, &m, sizeof(float));
    }
    return ACE_OK;
}
extern "C" int ace_sfno_num_stages(void) { return ST_COUNT; }
extern "C" const char* ace_sfno_stage_name(int i) { return (i >= 0 && i < ST_COUNT) ? kStageNames[i] : nullptr; }
extern "C" int ace_sfno_forward_timed(ace_sfno* n, const float* in, float* out, int batch, void* stream, float* ms_host,
                                      int* calls_host) {
    ACE_TRY(check_ready(n, in, out, batch));
    if (n->cfg.normalization_layer == 2) return fail(ACE_ERR_STATE, "this net is noise conditioned: call ace_sfno_forward_conditioned");
    if (!ms_host) return fail(ACE_ERR_INVALID, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    StageTimer tm(s);
    ACE_TRY(forward_impl(n, in, out, batch, s, &tm));
    ACE_HIP_TRY(tm.finish(ms_host, calls_host));
    return ACE_OK;
}

extern "C" int ace_sfno_forward_conditioned_timed(ace_sfno* n, const float* in, const float* noise, float* out, int batch,
                                                  void* stream, float* ms_host, int* calls_host) {
    ACE_TRY(check_ready(n, in, out, batch));
    if (n->cfg.normalization_layer != 2)
        return fail(ACE_ERR_STATE, "ace_sfno_forward_conditioned_timed needs a net created with conditional layer norms");
    if (!ms_host || (!noise && n->cfg.noise_embed_dim > 0)) return fail(ACE_ERR_INVALID, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    StageTimer tm(s);
    ACE_TRY(forward_impl(n, in, out, batch, s, &tm, noise));
    ACE_HIP_TRY(tm.finish(ms_host, calls_host));
    return ACE_OK;
}

extern "C" int ace_sfno_set_taps(ace_sfno* n, int enable) {
    if (!n) return fail(ACE_ERR_INVALID, "null argument");
    if (enable && n->cfg.scale_factor != 1)   // the taps are (batch, C, nlat, nlon) copies: the inner blocks of such a net live on another grid
        return fail(ACE_ERR_STATE, "per-block taps are not available for scale_factor != 1");
    if (enable && n->taps.empty()) {
        n->taps = std::vector<DevBuf>(n->cfg.num_layers + 1);
        for (auto& t : n->taps) ACE_HIP_TRY(t.alloc((size_t)n->Bmax * n->C * n->HW));
    }
    n->taps_on = enable != 0;
    return ACE_OK;
}
extern "C" int ace_sfno_get_tap(ace_sfno* n, int i, float* dst, int batch, void* stream) {
    if (!n || !dst) return fail(ACE_ERR_INVALID, "null argument");
    if (n->taps.empty() || i < -1 || i >= n->cfg.num_layers) return fail(ACE_ERR_STATE, "taps not enabled / bad index");
    ACE_HIP_TRY(hipMemcpyAsync(dst, n->taps[i + 1].p, sizeof(float) * batch * n->C * n->HW, hipMemcpyDeviceToDevice,
                           static_cast<hipStream_t>(stream)));
    return ACE_OK;
}

extern "C" int ace_sfno_forward_graph(ace_sfno* n, const float* in, float* out, int batch, void* stream) {
    ACE_TRY(check_ready(n, in, out, batch));
    if (n->cfg.normalization_layer == 2) return fail(ACE_ERR_STATE, "this net is noise conditioned: call ace_sfno_forward_conditioned");
    if (n->taps_on) return fail(ACE_ERR_STATE, "disable taps before using the graph path");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n->graphs_stale) {   // parameters changed since capture: the scalars baked into the kernel arguments are out of date
        ACE_HIP_TRY(hipStreamSynchronize(s));   // no exec of this handle may be in flight when it is destroyed
        for (auto& kv : n->graphs) (void)hipGraphExecDestroy(kv.second);
        n->graphs.clear();
        n->graphs_stale = false;
    }
    GraphKey key{in, out, batch};
    auto it = n->graphs.find(key);
    if (it == n->graphs.end()) {
        if (!n->capture_stream) ACE_HIP_TRY(hipStreamCreateWithFlags(&n->capture_stream, hipStreamNonBlocking));
        // everything queued on the caller's stream must be visible to the first replay; capture itself runs nothing
        hipGraph_t graph = nullptr;
        ACE_HIP_TRY(hipStreamBeginCapture(n->capture_stream, hipStreamCaptureModeThreadLocal));
        int rc = forward_impl(n, in, out, batch, n->capture_stream);
        hipError_t e = hipStreamEndCapture(n->capture_stream, &graph);
        if (rc != ACE_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        ACE_HIP_TRY(e);
        hipGraphExec_t exec = nullptr;
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        ACE_HIP_TRY(e);
        it = n->graphs.emplace(key, exec).first;
    }
    ACE_HIP_TRY(hipGraphLaunch(it->second, s));
    return ACE_OK;
}
