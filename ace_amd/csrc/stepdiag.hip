// Corrector step diagnostics (fme/core/step/step_diagnostics.py, fme/ace/aggregator/inference/step_diagnostics.py): the per-step
// delta = corrected - network output of the variables the corrector wrote, and the correction metrics of a window of deltas.
//   stepdiag_snapshot      workgroup (chunk, plane k, sample b) copies its 1024 pixels of the uncorrected output plane into the
//                          recorder's buffer, ahead of the in-place physics kernels; 16-byte accesses when both planes allow them,
//                          4-byte ones otherwise, chosen once per workgroup.
//   stepdiag_delta_window  workgroup (chunk, plane k, (b, t)): snap = fl32(out - snap) in place over the snapshot buffer, once per
//                          window, after the last step's physics.
//   correction_window      the structure of diag_window (diag.hip).  Workgroup (chunk, plane j) owns 1024 pixels (4 per thread) of
//                          delta plane j and walks every (b, t) in order with the next plane's load in flight; per element
//                          n = fl32(d / std_j), widened to fp64.  Per (b, t) each wave reduces its 256 pixels to (sum w, weighted
//                          mean of n, sum w (n - mean)^2, weighted mean of |n|) - two passes over registers - and stores them as
//                          one partial; pixels of zero weight are skipped (NaN included).  The same loads feed the per-pixel sums of
//                          n and |n| over (b, t), which each thread adds to the persistent fp64 accumulators of its own pixels.
//   correction_combine     one wave per (t, j): the partials of each sample merged by Chan's parallel update in a fixed order (lane
//                          strides, then a butterfly), the per-sample weighted mean of |n| and the weighted std of n averaged over
//                          the batch in sample order and added to the fp64 series at t0 + t.
// No atomics, no workgroup waits for another, no host synchronisation, no allocation: two identical runs are bitwise identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "diag_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NMOM = 4;              // sum of weights, weighted mean of n, second central moment of n, weighted mean of |n|

__device__ __forceinline__ void store4(float* d, long p, long HW, bool vec, const float4& v) {
    if (vec && p + 3 < HW) { *reinterpret_cast<float4*>(d + p) = v; return; }
    if (p < HW) d[p] = v.x;
    if (p + 1 < HW) d[p + 1] = v.y;
    if (p + 2 < HW) d[p + 2] = v.z;
    if (p + 3 < HW) d[p + 3] = v.w;
}

__global__ __launch_bounds__(NT) void stepdiag_snapshot_kernel(const float* const* srcs, const long* __restrict__ src_strides,
                                                               float* const* dsts, const long* __restrict__ dst_strides, long HW) {
    const int chunk = blockIdx.x, k = blockIdx.y, b = blockIdx.z;
    const long p = (long)chunk * CHUNK + (long)threadIdx.x * PIX;
    const long ss = src_strides[k], ds = dst_strides[k];
    const float* src = srcs[k];
    float* dst = dsts[k];
    const bool vec = DIAG_VEC4_ROW_OK(src, HW) && (ss & 3) == 0 && DIAG_VEC4_ROW_OK(dst, HW) && (ds & 3) == 0;
    if (p >= HW) return;
    store4(dst + (long)b * ds, p, HW, vec, load4(src + (long)b * ss, p, HW, vec));
}

__global__ __launch_bounds__(NT) void stepdiag_delta_kernel(const float* const* outs, const long* __restrict__ out_strides,
                                                            float* const* snaps, const long* __restrict__ snap_strides, int T,
                                                            long HW) {
    const int chunk = blockIdx.x, k = blockIdx.y;
    const int b = blockIdx.z / T, t = blockIdx.z - b * T;
    const long p = (long)chunk * CHUNK + (long)threadIdx.x * PIX;
    const float* out = outs[k];
    float* snap = snaps[k];
    const long osb = out_strides[2 * k], ost = out_strides[2 * k + 1];
    const long ssb = snap_strides[2 * k], sst = snap_strides[2 * k + 1];
    const bool vec = DIAG_VEC4_OK(out, HW, osb, ost) && DIAG_VEC4_OK(snap, HW, ssb, sst);
    if (p >= HW) return;
    float* q = snap + (long)b * ssb + (long)t * sst;
    const float4 o = load4(out + (long)b * osb + (long)t * ost, p, HW, vec);
    const float4 s = load4(q, p, HW, vec);
    store4(q, p, HW, vec, make_float4(o.x - s.x, o.y - s.y, o.z - s.z, o.w - s.w));
}

// Chan et al.'s parallel update of (weight, mean, M2) and of the weighted mean of |n| with a partial; empty partials are skipped
__device__ __forceinline__ void chan4(double& w, double& m, double& M, double& a, double wb, double mb, double Mb, double ab) {
    if (wb == 0.0) return;
    if (w == 0.0) { w = wb; m = mb; M = Mb; a = ab; return; }
    const double n = w + wb, d = mb - m, f = wb / n;
    m += d * f;
    M += Mb + d * d * (w * wb / n);
    a += (ab - a) * f;
    w = n;
}

__global__ __launch_bounds__(NT) void correction_window_kernel(const float* const* srcs, const long* __restrict__ strides,
                                                               const float* __restrict__ stds, const int* __restrict__ rows,
                                                               const int* __restrict__ wrows, const float* __restrict__ weights,
                                                               int nw, double* __restrict__ partial, double* __restrict__ sgn,
                                                               double* __restrict__ mag, int nrows, int B, int T, long HW,
                                                               int nchunk) {
    const int chunk = blockIdx.x, j = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = rows[j], wr = wrows[j];
    if (r < 0 || r >= nrows || wr < 0 || wr >= nw) return;
    const long p = (long)chunk * CHUNK + (long)threadIdx.x * PIX;
    const float* base = srcs[j];
    const long sb = strides[2 * j], st = strides[2 * j + 1];
    const bool vec = DIAG_VEC4_OK(base, HW, sb, st);
    const float sd = stds[j];
    const float* wrow = weights + (long)wr * HW;
    const float4 w4 = load4(wrow, p, HW, DIAG_VEC4_ROW_OK(wrow, HW));
    const float wv[PIX] = {w4.x, w4.y, w4.z, w4.w};
    double W = 0.0;
#pragma unroll
    for (int k = 0; k < PIX; ++k)
        if (wv[k] != 0.0f) W += (double)wv[k];
    W = wave_sum(W);
    double accs[PIX] = {0.0, 0.0, 0.0, 0.0}, acca[PIX] = {0.0, 0.0, 0.0, 0.0};
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
        // the correctly rounded fp32 quotient, as torch forms delta / std; fp64 from here on
        const double xv[PIX] = {(double)__fdiv_rn(x4.x, sd), (double)__fdiv_rn(x4.y, sd), (double)__fdiv_rn(x4.z, sd),
                                (double)__fdiv_rn(x4.w, sd)};
        double S = 0.0, A = 0.0;
#pragma unroll
        for (int k = 0; k < PIX; ++k)
            if (wv[k] != 0.0f) { S += (double)wv[k] * xv[k]; A += (double)wv[k] * fabs(xv[k]); }
        S = wave_sum(S);
        A = wave_sum(A);
        const double m = W > 0.0 ? S / W : 0.0;
        double M = 0.0;
#pragma unroll
        for (int k = 0; k < PIX; ++k)
            if (wv[k] != 0.0f) { const double d = xv[k] - m; M += (double)wv[k] * d * d; }
        M = wave_sum(M);
        if (lane == 0) {
            double* q = partial + ((((long)j * B + b) * T + t) * nparts + (long)chunk * WAVES + wave) * NMOM;
            q[0] = W;
            q[1] = m;
            q[2] = M;
            q[3] = W > 0.0 ? A / W : 0.0;
        }
#pragma unroll
        for (int k = 0; k < PIX; ++k) { accs[k] += xv[k]; acca[k] += fabs(xv[k]); }
    }
    double* s = sgn + (long)r * HW;
    double* a = mag + (long)r * HW;
#pragma unroll
    for (int k = 0; k < PIX; ++k)
        if (p + k < HW) { s[p + k] += accs[k]; a[p + k] += acca[k]; }
}

__global__ __launch_bounds__(64) void correction_combine_kernel(const double* __restrict__ partial, const int* __restrict__ rows,
                                                                const int* __restrict__ wrows, int nw, double* __restrict__ series,
                                                                int nrows, int n_time, int B, int T, int t0, long nparts) {
    const int t = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
    const int r = rows[j], wr = wrows[j];
    // a plane without a row or a weight row has no partials (correction_window_kernel skipped it): it contributes to nothing
    if (r < 0 || r >= nrows || wr < 0 || wr >= nw || t0 + t < 0 || t0 + t >= n_time) return;
    double sa = 0.0, ss = 0.0;
    for (int b = 0; b < B; ++b) {
        const double* q = partial + (((long)j * B + b) * T + t) * nparts * NMOM;
        double w = 0.0, m = 0.0, M = 0.0, a = 0.0;
        for (long i = lane; i < nparts; i += 64) chan4(w, m, M, a, q[i * NMOM], q[i * NMOM + 1], q[i * NMOM + 2], q[i * NMOM + 3]);
        for (int o = 1; o < 64; o <<= 1) {
            const double wo = __shfl_xor(w, o, 64), mo = __shfl_xor(m, o, 64), Mo = __shfl_xor(M, o, 64), ao = __shfl_xor(a, o, 64);
            chan4(w, m, M, a, wo, mo, Mo, ao);
        }
        // no weighted pixel: 0 / 0 as the reference's weighted mean gives
        sa += w > 0.0 ? a : NAN;
        ss += w > 0.0 ? sqrt(M / w) : NAN;
    }
    if (lane == 0) {
        series[(long)r * n_time + t0 + t] += sa / B;
        series[((long)nrows + r) * n_time + t0 + t] += ss / B;
    }
}

}  // namespace

extern "C" int ace_stepdiag_snapshot(const float* const* srcs, const long* src_strides, float* const* dsts, const long* dst_strides,
                                     int nplanes, int batch, long hw, void* stream) {
    if (nplanes < 0 || nplanes > 65535) return ace::fail(ACE_ERR_INVALID, "ace_stepdiag_snapshot: need 0 <= nplanes <= 65535 (a grid dimension)");
    if (batch < 1 || batch > 65535) return ace::fail(ACE_ERR_INVALID, "ace_stepdiag_snapshot: need 1 <= batch <= 65535 (a grid dimension)");
    if (hw < 1 || nchunk_for(hw) > 2147483647L) return ace::fail(ACE_ERR_INVALID, "ace_stepdiag_snapshot: need 1 <= hw <= 1024 * (2^31 - 1)");
    if (nplanes == 0) return ACE_OK;
    if (!srcs || !src_strides || !dsts || !dst_strides) return ace::fail(ACE_ERR_INVALID, "ace_stepdiag_snapshot: null argument");
    hipLaunchKernelGGL(stepdiag_snapshot_kernel, dim3((unsigned)nchunk_for(hw), nplanes, batch), dim3(NT), 0,
                       static_cast<hipStream_t>(stream), srcs, src_strides, dsts, dst_strides, hw);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_stepdiag_delta_window(const float* const* outs, const long* out_strides, float* const* snaps,
                                         const long* snap_strides, int nplanes, int batch, int steps, long hw, void* stream) {
    if (nplanes < 0 || nplanes > 65535) return ace::fail(ACE_ERR_INVALID, "ace_stepdiag_delta_window: need 0 <= nplanes <= 65535 (a grid dimension)");
    if (batch < 1 || steps < 1 || (long)batch * steps > 65535)
        return ace::fail(ACE_ERR_INVALID, "ace_stepdiag_delta_window: need batch >= 1, steps >= 1, batch * steps <= 65535 (a grid dimension)");
    if (hw < 1 || nchunk_for(hw) > 2147483647L) return ace::fail(ACE_ERR_INVALID, "ace_stepdiag_delta_window: need 1 <= hw <= 1024 * (2^31 - 1)");
    if (nplanes == 0) return ACE_OK;
    if (!outs || !out_strides || !snaps || !snap_strides) return ace::fail(ACE_ERR_INVALID, "ace_stepdiag_delta_window: null argument");
    hipLaunchKernelGGL(stepdiag_delta_kernel, dim3((unsigned)nchunk_for(hw), nplanes, batch * steps), dim3(NT), 0,
                       static_cast<hipStream_t>(stream), outs, out_strides, snaps, snap_strides, steps, hw);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}

extern "C" long ace_diag_correction_partial_doubles(int nplanes, int batch, int steps, long hw) {
    if (nplanes < 0 || batch < 1 || steps < 1 || hw < 1) return -1;
    return (long)nplanes * batch * steps * nchunk_for(hw) * WAVES * NMOM;
}

extern "C" int ace_diag_correction_window(const float* const* deltas, const long* strides, const float* stds, const int* rows,
                                          const int* wrows, const float* weights, int nw, double* partial, double* signed_sum,
                                          double* magnitude_sum, double* series, int nrows, int n_time, int t0, int nplanes, int batch,
                                          int steps, long hw, void* stream) {
    if (nplanes < 0 || nplanes > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_correction_window: need 0 <= nplanes <= 65535");
    if (steps < 1 || steps > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_correction_window: need 1 <= steps <= 65535");
    if (batch < 1 || hw < 1 || nw < 1 || nrows < 1)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_correction_window: need batch >= 1, hw >= 1, nw >= 1, nrows >= 1");
    if (t0 < 0 || t0 + (long)steps > n_time)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_correction_window: need 0 <= t0, t0 + steps <= n_time");
    if (nplanes == 0) return ACE_OK;
    if (!deltas || !strides || !stds || !rows || !wrows || !weights || !partial || !signed_sum || !magnitude_sum || !series)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_correction_window: null argument");
    const long nchunk = nchunk_for(hw);
    if (nchunk > 2147483647L) return ace::fail(ACE_ERR_INVALID, "ace_diag_correction_window: plane too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(correction_window_kernel, dim3((unsigned)nchunk, nplanes), dim3(NT), 0, s, deltas, strides, stds, rows, wrows,
                       weights, nw, partial, signed_sum, magnitude_sum, nrows, batch, steps, hw, (int)nchunk);
    ACE_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(correction_combine_kernel, dim3(steps, nplanes), dim3(64), 0, s, partial, rows, wrows, nw, series, nrows, n_time,
                       batch, steps, t0, nchunk * WAVES);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}
