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
#include <cstdint>
#include <string>

#include "../../include/ace_sfno.h"

static thread_local std::string g_derr;
static int dfail(int code, const std::string& m) { g_derr = m; return code; }
extern "C" const char* ace_diag_last_error(void) { return g_derr.c_str(); }
#define DIAG_TRY(expr)                                                                                      \
    do {                                                                                                    \
        hipError_t e__ = (expr);                                                                            \
        if (e__ != hipSuccess) return dfail(ACE_ERR_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

namespace {

constexpr int NT = 256;              // four wave64s
constexpr int WAVES = NT / 64;
constexpr int PIX = 4;               // pixels per thread
constexpr int CHUNK = NT * PIX;      // pixels per workgroup
constexpr int NMOM = 3;              // sum of weights, weighted mean, second central moment

__device__ __forceinline__ double wave_sum(double v) {
    // xor butterfly: every lane ends with the same sum (fp add is commutative)
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Chan et al.'s parallel update of (weight, mean, M2) with the partial (wb, mb, Mb); empty partials are skipped
__device__ __forceinline__ void chan(double& w, double& m, double& M, double wb, double mb, double Mb) {
    if (wb == 0.0) return;
    if (w == 0.0) { w = wb; m = mb; M = Mb; return; }
    const double n = w + wb, d = mb - m;
    m += d * (wb / n);
    M += Mb + d * d * (w * wb / n);
    w = n;
}

__device__ __forceinline__ float4 load4(const float* s, long p, long HW, bool vec) {
    if (vec && p + 3 < HW) return *reinterpret_cast<const float4*>(s + p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p < HW) v.x = s[p];
    if (p + 1 < HW) v.y = s[p + 1];
    if (p + 2 < HW) v.z = s[p + 2];
    if (p + 3 < HW) v.w = s[p + 3];
    return v;
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
    const bool vec = (HW & 3) == 0 && (reinterpret_cast<uintptr_t>(base) & 15u) == 0 && (sb & 3) == 0 && (st & 3) == 0;
    const float* wrow = weights + (long)wr * HW;
    const float4 w4 = load4(wrow, p, HW, (HW & 3) == 0 && (reinterpret_cast<uintptr_t>(wrow) & 15u) == 0);
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

long nchunk_for(long hw) { return (hw + CHUNK - 1) / CHUNK; }

}  // namespace

extern "C" long ace_diag_partial_doubles(int nplanes, int batch, int steps, long hw) {
    if (nplanes < 0 || batch < 1 || steps < 1 || hw < 1) return -1;
    return (long)nplanes * batch * steps * nchunk_for(hw) * WAVES * NMOM;
}

extern "C" int ace_diag_window(const float* const* srcs, const long* strides, const int* rows, const int* wrows,
                               const float* weights, int nw, double* partial, double* tsum, double* series, int nrows, int n_time,
                               int t0, int t_begin, int do_tsum, int nplanes, int batch, int steps, long hw, void* stream) {
    if (nplanes < 0 || nplanes > 65535) return dfail(ACE_ERR_INVALID, "ace_diag_window: need 0 <= nplanes <= 65535");
    if (steps < 1 || steps > 65535) return dfail(ACE_ERR_INVALID, "ace_diag_window: need 1 <= steps <= 65535");
    if (batch < 1 || hw < 1 || nw < 1 || nrows < 1)
        return dfail(ACE_ERR_INVALID, "ace_diag_window: need batch >= 1, hw >= 1, nw >= 1, nrows >= 1");
    if (t0 < 0 || t0 + (long)steps > n_time || t_begin < 0)
        return dfail(ACE_ERR_INVALID, "ace_diag_window: need 0 <= t0, t0 + steps <= n_time, 0 <= t_begin");
    if (nplanes == 0) return ACE_OK;
    if (!srcs || !strides || !rows || !wrows || !weights || !partial || !series || (do_tsum && !tsum))
        return dfail(ACE_ERR_INVALID, "ace_diag_window: null argument");
    const long nchunk = nchunk_for(hw);
    if (nchunk > 2147483647L) return dfail(ACE_ERR_INVALID, "ace_diag_window: plane too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(diag_window_kernel, dim3((unsigned)nchunk, nplanes), dim3(NT), 0, s, srcs, strides, rows, wrows, weights, nw,
                       partial, tsum, nrows, batch, steps, t_begin, do_tsum, hw, (int)nchunk);
    DIAG_TRY(hipGetLastError());
    hipLaunchKernelGGL(diag_combine_kernel, dim3(steps, nplanes), dim3(64), 0, s, partial, rows, wrows, nw, series, nrows, n_time, batch,
                       steps, t0, nchunk * WAVES);
    DIAG_TRY(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_diag_spectrum(const void* coeffs, const int* rows, double* spec, int nrows, int nnames, long planes, int lmax,
                                 int mmax, void* stream) {
    if (nnames < 0 || nnames > 65535) return dfail(ACE_ERR_INVALID, "ace_diag_spectrum: need 0 <= nnames <= 65535");
    if (planes < 1 || lmax < 1 || mmax < 1 || nrows < 1)
        return dfail(ACE_ERR_INVALID, "ace_diag_spectrum: need planes >= 1, lmax >= 1, mmax >= 1, nrows >= 1");
    if (nnames == 0) return ACE_OK;
    if (!coeffs || !rows || !spec) return dfail(ACE_ERR_INVALID, "ace_diag_spectrum: null argument");
    hipLaunchKernelGGL(diag_spectrum_kernel, dim3(lmax, nnames), dim3(NT), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float2*>(coeffs), rows, spec, nrows, planes, lmax, mmax);
    DIAG_TRY(hipGetLastError());
    return ACE_OK;
}
