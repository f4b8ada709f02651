// Inference diagnostics (fme/ace/aggregator/inference: reduced.py, time_mean.py, spectrum.py) as deterministic reductions over
// the output planes of a rollout window, read in place through a pointer table.
//   diag_window    one pass over the (plane j, sample b, step t) fields of a window.  Workgroup (chunk, j) owns 1024 pixels
//                  (4 per thread) of plane j and walks every (b, t) in order; per (b, t) each wave reduces its 256 pixels to
//                  (sum w, weighted mean, sum w (x - mean)^2) - two passes over registers, fp64 - and stores them as one
//                  partial; pixels of zero weight are skipped (NaN included).  The same loads feed the per-pixel time sums,
//                  which each thread adds to the persistent fp64 accumulator of its own pixels (no two threads share one).
//   diag_combine   one wave per (t, j): the partials of each sample merged by Chan's parallel update in a fixed order (lane
//                  strides, then a butterfly), the per-sample weighted mean and std averaged over the batch in sample order and
//                  added to the fp64 series at i_time_start + t.  A plane whose accumulator row or weight row is out of range
//                  is skipped by both kernels: it contributes to nothing.
//   diag_spectrum  one workgroup per (l, name): sum over (plane, m) of |c_lm|^2 in fp64 from the complex64 output of the
//                  forward SHT, a fixed-order block sum, added to the fp64 spectrum accumulator.
// No float atomics, no host synchronisation, no allocation: two identical runs are bitwise identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "diag_common.h"

namespace {

constexpr int NMOM = 3;              // sum of weights, weighted mean, second central moment

// Chan et al.'s parallel update of (weight, mean, M2) with the partial (wb, mb, Mb); empty partials are skipped
__device__ __forceinline__ void chan(double& w, double& m, double& M, double wb, double mb, double Mb) {
    if (wb == 0.0) return;
    if (w == 0.0) { w = wb; m = mb; M = Mb; return; }
    const double n = w + wb, d = mb - m;
    m += d * (wb / n);
    M += Mb + d * d * (w * wb / n);
    w = n;
}

__global__ __launch_bounds__(NT) void diag_window_kernel(const float* const* srcs, const long* __restrict__ strides,
                                                         const int* __restrict__ rows, const int* __restrict__ wrows,
                                                         const float* __restrict__ weights, int nw, double* __restrict__ partial,
                                                         double* __restrict__ tsum, int nrows, int B, int T, int t_begin,
                                                         int do_tsum, long HW, int nchunk) {
    const int chunk = blockIdx.x, j = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wrows[j];
    if (wr < 0 || wr >= nw) return;
    const long p = (long)chunk * CHUNK + (long)threadIdx.x * PIX;
    const float* base = srcs[j];
    const long sb = strides[2 * j], st = strides[2 * j + 1];
    const bool vec = DIAG_VEC4_OK(base, HW, sb, st);
    const float* wrow = weights + (long)wr * HW;
    const float4 w4 = load4(wrow, p, HW, DIAG_VEC4_ROW_OK(wrow, HW));
    const float wv[PIX] = {w4.x, w4.y, w4.z, w4.w};
    double acc[PIX] = {0.0, 0.0, 0.0, 0.0};
    const long nparts = (long)nchunk * WAVES;
    const int n = B * T;
    float4 nx = load4(base, p, HW, vec);
    for (int i = 0; i < n; ++i) {
        const int b = i / T, t = i - b * T;
        const float4 x4 = nx;
        if (i + 1 < n) {                               // the next plane's load is in flight during this plane's reductions
            const int b1 = (i + 1) / T, t1 = (i + 1) - b1 * T;
            nx = load4(base + (long)b1 * sb + (long)t1 * st, p, HW, vec);
        }
        const float xv[PIX] = {x4.x, x4.y, x4.z, x4.w};
        double W = 0.0, S = 0.0;
#pragma unroll
        for (int k = 0; k < PIX; ++k)
            if (wv[k] != 0.0f) { W += (double)wv[k]; S += (double)wv[k] * (double)xv[k]; }
        W = wave_sum(W);
        S = wave_sum(S);
        const double m = W > 0.0 ? S / W : 0.0;
        double M = 0.0;
#pragma unroll
        for (int k = 0; k < PIX; ++k)
            if (wv[k] != 0.0f) { const double d = (double)xv[k] - m; M += (double)wv[k] * d * d; }
        M = wave_sum(M);
        if (lane == 0) {
            double* q = partial + ((((long)j * B + b) * T + t) * nparts + (long)chunk * WAVES + wave) * NMOM;
            q[0] = W;
            q[1] = m;
            q[2] = M;
        }
        if (do_tsum && t >= t_begin) {
#pragma unroll
            for (int k = 0; k < PIX; ++k) acc[k] += (double)xv[k];
        }
    }
    const int r = rows[j];
    if (do_tsum && r >= 0 && r < nrows) {
        double* a = tsum + (long)r * HW;
#pragma unroll
        for (int k = 0; k < PIX; ++k)
            if (p + k < HW) a[p + k] += acc[k];
    }
}

__global__ __launch_bounds__(64) void diag_combine_kernel(const double* __restrict__ partial, const int* __restrict__ rows,
                                                          const int* __restrict__ wrows, int nw, double* __restrict__ series,
                                                          int nrows, int n_time, int B, int T, int t0, long nparts) {
    const int t = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
    const int r = rows[j], wr = wrows[j];
    // a plane without a weight row has no partials (diag_window_kernel skipped it): it contributes to nothing
    if (r < 0 || r >= nrows || wr < 0 || wr >= nw || t0 + t < 0 || t0 + t >= n_time) return;
    double sm = 0.0, ss = 0.0;
    for (int b = 0; b < B; ++b) {
        const double* q = partial + (((long)j * B + b) * T + t) * nparts * NMOM;
        double w = 0.0, m = 0.0, M = 0.0;
        for (long i = lane; i < nparts; i += 64) chan(w, m, M, q[i * NMOM], q[i * NMOM + 1], q[i * NMOM + 2]);
        for (int o = 1; o < 64; o <<= 1) {
            const double wo = __shfl_xor(w, o, 64), mo = __shfl_xor(m, o, 64), Mo = __shfl_xor(M, o, 64);
            chan(w, m, M, wo, mo, Mo);
        }
        // no valid pixel: 0 / 0 as the reference's weighted mean gives
        sm += w > 0.0 ? m : NAN;
        ss += w > 0.0 ? sqrt(M / w) : NAN;
    }
    if (lane == 0) {
        series[(long)r * n_time + t0 + t] += sm / B;
        series[((long)nrows + r) * n_time + t0 + t] += ss / B;
    }
}

__global__ __launch_bounds__(NT) void diag_spectrum_kernel(const float2* __restrict__ coeffs, const int* __restrict__ rows,
                                                           double* __restrict__ spec, int nrows, long planes, int L, int M) {
    const int l = blockIdx.x, j = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float2* c = coeffs + (long)j * planes * L * M + (long)l * M;
    double s = 0.0;
    const long n = planes * M;
    for (long i = threadIdx.x; i < n; i += NT) {
        const long pl = i / M, m = i - pl * M;
        const float2 v = c[pl * L * M + m];
        s += (double)v.x * (double)v.x + (double)v.y * (double)v.y;
    }
    s = wave_sum(s);
    __shared__ double red[WAVES];
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const int r = rows[j];
    if (threadIdx.x == 0 && r >= 0 && r < nrows) {
        double tot = 0.0;
        for (int w = 0; w < WAVES; ++w) tot += red[w];
        spec[(long)r * L + l] += tot;
    }
}

// ---- the paired pass (inference evaluator) -------------------------------------------------------------------------------------
//   diag_paired    one pass over the generated and the target (plane j, sample b, step t) fields of a window.  Workgroup (band, j)
//                  owns R full latitude rows of name j (R * nlon <= 256 * K pixels, K per thread in registers) and walks every
//                  (b, t) in order with the next plane's loads in flight.  Per (b, t) both fields go to LDS with the band's two halo
//                  rows, and from that one read come, in fp64: the generated field's (sum w, mean, M2) per wave (two passes over
//                  registers), the per-wave sums of w y, w d, w d^2 (d = gen - target) and of w |grad| and w over the pixels whose
//                  gradient is not NaN (torch.gradient stencils: central inside, one-sided at the four edges, no wrap), and per row
//                  the nan-mean over longitude (one wave per row, lanes stride the row, a butterfly), which that wave adds to the
//                  zonal accumulator.  Each thread adds its own pixels to the two per-pixel time sums.
//   paired_combine one wave per (t, j): per sample the partials merged in a fixed order (Chan for the moments, plain fp64 sums for
//                  the rest), the six per-sample values averaged over the batch in sample order and added to the series.
constexpr int NQ = 10;               // per-wave partial: sum w, mean, M2, sum w y, sum w d, sum w d^2, (sum w g, sum w) gen, target
constexpr int NSERIES = 6;

struct PairedArgs {
    const float* const* gen; const long* gstr; const float* const* tgt; const long* tstr;
    const int* rows; const int* wrows; const float* weights; int nw;
    double* partial; double* tsum; double* zonal; int nrows, B, T, t_begin, do_maps, zt0, factor, nslots, H, W, R, nband;
};

__device__ __forceinline__ double grad_mag(const float* f, int li, int W, float x, bool top, bool bot, bool left, bool right) {
    // torch.gradient, unit spacing, edge_order 1; differences of fp32 values are exact in fp64
    const double c = (double)x;
    const double gy = top ? (double)f[li + W] - c : bot ? c - (double)f[li - W] : ((double)f[li + W] - (double)f[li - W]) * 0.5;
    const double gx = left ? (double)f[li + 1] - c : right ? c - (double)f[li - 1] : ((double)f[li + 1] - (double)f[li - 1]) * 0.5;
    return sqrt(gy * gy + gx * gx);
}

template <int K>
__global__ __launch_bounds__(NT) void diag_paired_kernel(PairedArgs a) {
    extern __shared__ float lds[];
    const int band = blockIdx.x, j = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = a.rows[j], wr = a.wrows[j];
    if (r < 0 || r >= a.nrows || wr < 0 || wr >= a.nw) return;
    const int H = a.H, W = a.W;
    const int r0 = band * a.R, Rb = min(a.R, H - r0), npix = Rb * W;
    const long HW = (long)H * W, p0 = (long)r0 * W;
    const float* gbase = a.gen[j];
    const float* tbase = a.tgt[j];
    const bool paired = tbase != nullptr;
    const long gsb = a.gstr[2 * j], gst = a.gstr[2 * j + 1];
    const long tsb = paired ? a.tstr[2 * j] : 0, tst = paired ? a.tstr[2 * j + 1] : 0;
    float* fg = lds;                               // (R + 2) rows of the generated field: halo above, the band, halo below
    float* ft = lds + (long)(a.R + 2) * W;         // the same of the target
    const float* wrow = a.weights + (long)wr * HW + p0;

    float wv[K];
    unsigned edge[K];                              // bit 0 valid, 1 first row, 2 last row, 3 first column, 4 last column
    double Wsum = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int p = threadIdx.x + k * NT;
        const bool ok = p < npix;
        const int rr = ok ? p / W : 0, c = p - rr * W;
        wv[k] = ok ? wrow[p] : 0.0f;
        edge[k] = (ok ? 1u : 0u) | (r0 + rr == 0 ? 2u : 0u) | (r0 + rr == H - 1 ? 4u : 0u) | (c == 0 ? 8u : 0u) | (c == W - 1 ? 16u : 0u);
        if (wv[k] != 0.0f) Wsum += (double)wv[k];
    }
    Wsum = wave_sum(Wsum);

    double accg[K], acct[K];
#pragma unroll
    for (int k = 0; k < K; ++k) accg[k] = acct[k] = 0.0;
    float nxg[K], nxt[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int p = threadIdx.x + k * NT;
        nxg[k] = p < npix ? gbase[p0 + p] : 0.0f;
        nxt[k] = paired && p < npix ? tbase[p0 + p] : 0.0f;
    }
    const long nparts = (long)a.nband * WAVES;
    const int n = a.B * a.T;
    const double zdiv = (double)a.B * (double)a.factor;
    for (int i = 0; i < n; ++i) {
        const int b = i / a.T, t = i - b * a.T;
        const float* gp = gbase + (long)b * gsb + (long)t * gst;
        const float* tp = paired ? tbase + (long)b * tsb + (long)t * tst : nullptr;
        float xg[K], xt[K];
#pragma unroll
        for (int k = 0; k < K; ++k) { xg[k] = nxg[k]; xt[k] = nxt[k]; }
        if (i + 1 < n) {                           // the next plane's loads are in flight during this plane's work
            const int b1 = (i + 1) / a.T, t1 = (i + 1) - b1 * a.T;
            const float* g1 = gbase + (long)b1 * gsb + (long)t1 * gst + p0;
            const float* q1 = paired ? tbase + (long)b1 * tsb + (long)t1 * tst + p0 : nullptr;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int p = threadIdx.x + k * NT;
                nxg[k] = p < npix ? g1[p] : 0.0f;
                nxt[k] = paired && p < npix ? q1[p] : 0.0f;
            }
        }
        // the band and its halo rows to LDS
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int p = threadIdx.x + k * NT;
            if (p < npix) { fg[W + p] = xg[k]; if (paired) ft[W + p] = xt[k]; }
        }
        for (int c = threadIdx.x; c < W; c += NT) {
            if (r0 > 0) { fg[c] = gp[p0 - W + c]; if (paired) ft[c] = tp[p0 - W + c]; }
            if (r0 + Rb < H) { fg[W + npix + c] = gp[p0 + npix + c]; if (paired) ft[W + npix + c] = tp[p0 + npix + c]; }
        }
        __syncthreads();

        // the generated field's moments, two passes over registers
        double S = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (wv[k] != 0.0f) S += (double)wv[k] * (double)xg[k];
        S = wave_sum(S);
        const double m = Wsum > 0.0 ? S / Wsum : 0.0;
        double M = 0.0, Sy = 0.0, Sd = 0.0, Sd2 = 0.0, gn = 0.0, gd = 0.0, tn = 0.0, td = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (wv[k] == 0.0f) continue;
            const double w = (double)wv[k];
            const double dm = (double)xg[k] - m;
            M += w * dm * dm;
            const int li = W + threadIdx.x + k * NT;
            const bool top = edge[k] & 2u, bot = edge[k] & 4u, left = edge[k] & 8u, right = edge[k] & 16u;
            const double g = grad_mag(fg, li, W, xg[k], top, bot, left, right);
            if (g == g) { gn += w * g; gd += w; }
            if (paired) {
                const double y = (double)xt[k], d = (double)xg[k] - y;
                Sy += w * y;
                Sd += w * d;
                Sd2 += w * d * d;
                const double h = grad_mag(ft, li, W, xt[k], top, bot, left, right);
                if (h == h) { tn += w * h; td += w; }
            }
        }
        M = wave_sum(M);
        gn = wave_sum(gn);
        gd = wave_sum(gd);
        if (paired) {
            Sy = wave_sum(Sy); Sd = wave_sum(Sd); Sd2 = wave_sum(Sd2); tn = wave_sum(tn); td = wave_sum(td);
        }
        if (lane == 0) {
            double* q = a.partial + ((((long)j * a.B + b) * a.T + t) * nparts + (long)band * WAVES + wave) * NQ;
            q[0] = Wsum; q[1] = m; q[2] = M; q[3] = Sy; q[4] = Sd; q[5] = Sd2; q[6] = gn; q[7] = gd; q[8] = tn; q[9] = td;
        }
        if (a.do_maps) {
            if (t >= a.t_begin) {
#pragma unroll
                for (int k = 0; k < K; ++k) { accg[k] += (double)xg[k]; acct[k] += (double)xt[k]; }
            }
            // zonal means: wave w owns rows w, w + 4, ... of the band
            const int zt = a.zt0 + t;
            const int slot = zt >= 0 ? zt / a.factor : -1;
            if (slot >= 0 && slot < a.nslots) {
                for (int rr = wave; rr < Rb; rr += WAVES) {
                    for (int side = 0; side < (paired ? 2 : 1); ++side) {
                        const float* f = (side ? ft : fg) + (long)(1 + rr) * W;
                        double s = 0.0, cnt = 0.0;
                        for (int c = lane; c < W; c += 64) {
                            const float v = f[c];
                            if (v == v) { s += (double)v; cnt += 1.0; }
                        }
                        s = wave_sum(s);
                        cnt = wave_sum(cnt);
                        if (lane == 0) {
                            double* z = a.zonal + (((long)side * a.nrows + r) * a.nslots + slot) * H + r0 + rr;
                            *z += (s / cnt) / zdiv;            // an all-NaN row: 0 / 0
                        }
                    }
                }
            }
        }
        __syncthreads();                           // the next plane overwrites the LDS rows
    }
    if (a.do_maps) {
        double* ag = a.tsum + (long)r * HW + p0;
        double* at = a.tsum + ((long)a.nrows + r) * HW + p0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int p = threadIdx.x + k * NT;
            if (p < npix) { ag[p] += accg[k]; if (paired) at[p] += acct[k]; }
        }
    }
}

__global__ __launch_bounds__(64) void paired_combine_kernel(const double* __restrict__ partial, const float* const* tgt,
                                                            const int* __restrict__ rows, const int* __restrict__ wrows, int nw,
                                                            double* __restrict__ series, int nrows, int n_time, int B, int T, int t0,
                                                            long nparts) {
    const int t = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
    const int r = rows[j], wr = wrows[j];
    if (r < 0 || r >= nrows || wr < 0 || wr >= nw || t0 + t < 0 || t0 + t >= n_time) return;
    const bool paired = tgt[j] != nullptr;
    double out[NSERIES] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < B; ++b) {
        const double* q = partial + (((long)j * B + b) * T + t) * nparts * NQ;
        double w = 0.0, m = 0.0, M = 0.0, s[NQ - 3] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (long i = lane; i < nparts; i += 64) {
            chan(w, m, M, q[i * NQ], q[i * NQ + 1], q[i * NQ + 2]);
#pragma unroll
            for (int k = 0; k < NQ - 3; ++k) s[k] += q[i * NQ + 3 + k];
        }
        for (int o = 1; o < 64; o <<= 1) {
            const double wo = __shfl_xor(w, o, 64), mo = __shfl_xor(m, o, 64), Mo = __shfl_xor(M, o, 64);
            chan(w, m, M, wo, mo, Mo);
        }
#pragma unroll
        for (int k = 0; k < NQ - 3; ++k) s[k] = wave_sum(s[k]);
        // no valid pixel: 0 / 0 as the reference's weighted mean gives
        out[0] += w > 0.0 ? m : NAN;
        out[1] += w > 0.0 ? sqrt(M / w) : NAN;
        if (paired) {
            const double gg = s[3] / s[4], gt = s[5] / s[6];
            out[2] += s[0] / w;
            out[3] += s[1] / w;
            out[4] += sqrt(s[2] / w);
            out[5] += 100.0 * (gg - gt) / gt;
        }
    }
    if (lane == 0) {
        for (int k = 0; k < (paired ? NSERIES : 2); ++k) series[((long)k * nrows + r) * n_time + t0 + t] += out[k] / B;
    }
}

constexpr int PAIRED_K_SMALL = 6, PAIRED_K_LARGE = 12;
constexpr long PAIRED_LDS_MAX = 65536;

// rows per band: as many full rows as 256 * K pixels hold (4 at nlon = 360, 1 at 1440 with K = 6); K = 12 past nlon = 1536
int paired_k_for(int nlon) { return nlon <= NT * PAIRED_K_SMALL ? PAIRED_K_SMALL : PAIRED_K_LARGE; }
int paired_rows_for(int nlat, int nlon) {
    const int r = (NT * paired_k_for(nlon)) / nlon;
    return r < 1 ? 1 : (r > nlat ? nlat : r);
}
long paired_lds_bytes(int nlat, int nlon) { return 2L * (paired_rows_for(nlat, nlon) + 2) * nlon * (long)sizeof(float); }
bool paired_shape_ok(int nlat, int nlon) {
    return nlat >= 2 && nlon >= 2 && nlon <= NT * PAIRED_K_LARGE && paired_lds_bytes(nlat, nlon) <= PAIRED_LDS_MAX;
}
long paired_nband(int nlat, int nlon) { const int r = paired_rows_for(nlat, nlon); return (nlat + r - 1) / r; }

}  // namespace

extern "C" long ace_diag_partial_doubles(int nplanes, int batch, int steps, long hw) {
    if (nplanes < 0 || batch < 1 || steps < 1 || hw < 1) return -1;
    return (long)nplanes * batch * steps * nchunk_for(hw) * WAVES * NMOM;
}

extern "C" int ace_diag_window(const float* const* srcs, const long* strides, const int* rows, const int* wrows,
                               const float* weights, int nw, double* partial, double* tsum, double* series, int nrows, int n_time,
                               int t0, int t_begin, int do_tsum, int nplanes, int batch, int steps, long hw, void* stream) {
    if (nplanes < 0 || nplanes > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_window: need 0 <= nplanes <= 65535");
    if (steps < 1 || steps > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_window: need 1 <= steps <= 65535");
    if (batch < 1 || hw < 1 || nw < 1 || nrows < 1)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_window: need batch >= 1, hw >= 1, nw >= 1, nrows >= 1");
    if (t0 < 0 || t0 + (long)steps > n_time || t_begin < 0)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_window: need 0 <= t0, t0 + steps <= n_time, 0 <= t_begin");
    if (nplanes == 0) return ACE_OK;
    if (!srcs || !strides || !rows || !wrows || !weights || !partial || !series || (do_tsum && !tsum))
        return ace::fail(ACE_ERR_INVALID, "ace_diag_window: null argument");
    const long nchunk = nchunk_for(hw);
    if (nchunk > 2147483647L) return ace::fail(ACE_ERR_INVALID, "ace_diag_window: plane too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(diag_window_kernel, dim3((unsigned)nchunk, nplanes), dim3(NT), 0, s, srcs, strides, rows, wrows, weights, nw,
                       partial, tsum, nrows, batch, steps, t_begin, do_tsum, hw, (int)nchunk);
    ACE_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(diag_combine_kernel, dim3(steps, nplanes), dim3(64), 0, s, partial, rows, wrows, nw, series, nrows, n_time, batch,
                       steps, t0, nchunk * WAVES);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_diag_spectrum(const void* coeffs, const int* rows, double* spec, int nrows, int nnames, long planes, int lmax,
                                 int mmax, void* stream) {
    if (nnames < 0 || nnames > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_spectrum: need 0 <= nnames <= 65535");
    if (planes < 1 || lmax < 1 || mmax < 1 || nrows < 1)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_spectrum: need planes >= 1, lmax >= 1, mmax >= 1, nrows >= 1");
    if (nnames == 0) return ACE_OK;
    if (!coeffs || !rows || !spec) return ace::fail(ACE_ERR_INVALID, "ace_diag_spectrum: null argument");
    hipLaunchKernelGGL(diag_spectrum_kernel, dim3(lmax, nnames), dim3(NT), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float2*>(coeffs), rows, spec, nrows, planes, lmax, mmax);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}

extern "C" long ace_diag_paired_partial_doubles(int nplanes, int batch, int steps, int nlat, int nlon) {
    if (nplanes < 0 || batch < 1 || steps < 1 || !paired_shape_ok(nlat, nlon)) return -1;
    return (long)nplanes * batch * steps * paired_nband(nlat, nlon) * WAVES * NQ;
}

extern "C" int ace_diag_paired_window(const float* const* gen, const long* gen_strides, const float* const* target,
                                      const long* target_strides, const int* rows, const int* wrows, const float* weights, int nw,
                                      double* partial, double* tsum, double* zonal, double* series, int nrows, int n_time, int t0,
                                      int t_begin, int do_maps, int zt0, int factor, int nslots, int nplanes, int batch, int steps,
                                      int nlat, int nlon, void* stream) {
    if (nplanes < 0 || nplanes > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_paired_window: need 0 <= nplanes <= 65535");
    if (steps < 1 || steps > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_paired_window: need 1 <= steps <= 65535");
    if (batch < 1 || nw < 1 || nrows < 1)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_paired_window: need batch >= 1, nw >= 1, nrows >= 1");
    if (!paired_shape_ok(nlat, nlon))
        return ace::fail(ACE_ERR_INVALID, "ace_diag_paired_window: need nlat >= 2 and 2 <= nlon <= 2730 (the gradient's stencils; three "
                                      "rows of both fields in 64 KiB of LDS)");
    if (t0 < 0 || t0 + (long)steps > n_time || t_begin < 0)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_paired_window: need 0 <= t0, t0 + steps <= n_time, 0 <= t_begin");
    if (do_maps && (factor < 1 || nslots < 1 || zt0 < 0))
        return ace::fail(ACE_ERR_INVALID, "ace_diag_paired_window: need factor >= 1, nslots >= 1, zt0 >= 0 with do_maps");
    if (nplanes == 0) return ACE_OK;
    if (!gen || !gen_strides || !target || !target_strides || !rows || !wrows || !weights || !partial || !series ||
        (do_maps && (!tsum || !zonal)))
        return ace::fail(ACE_ERR_INVALID, "ace_diag_paired_window: null argument");
    PairedArgs a{gen, gen_strides, target, target_strides, rows, wrows, weights, nw, partial, tsum, zonal, nrows, batch, steps, t_begin,
                 do_maps, zt0, do_maps ? factor : 1, nslots, nlat, nlon, paired_rows_for(nlat, nlon), (int)paired_nband(nlat, nlon)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)a.nband, nplanes);
    const size_t lds = (size_t)paired_lds_bytes(nlat, nlon);
    if (paired_k_for(nlon) == PAIRED_K_SMALL)
        hipLaunchKernelGGL(diag_paired_kernel<PAIRED_K_SMALL>, grid, dim3(NT), lds, s, a);
    else
        hipLaunchKernelGGL(diag_paired_kernel<PAIRED_K_LARGE>, grid, dim3(NT), lds, s, a);
    ACE_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(paired_combine_kernel, dim3(steps, nplanes), dim3(64), 0, s, partial, target, rows, wrows, nw, series, nrows,
                       n_time, batch, steps, t0, (long)a.nband * WAVES);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}
