// The evaluator's per-pixel sums over time (fme/ace/aggregator/inference: trend.py:104-147, enso/enso_coefficient.py:118-168 and
// 418-437, near_zero_fraction.py:147-186): acc[pixel] += sum over samples b and steps t of c[b][t] * f(x[b][t][pixel]), f the
// identity (the regression sums: sum y, sum t y, sum index y) or the indicator x <= eps (the near-zero counts).  The reference forms
// them per name - and the ENSO covariance per sample - with torch ops that each read the window again; here one call covers both
// sides and all names of a window, and every plane is read once.
//   regress_window  workgroup (chunk, plane j, side) owns 1024 pixels (4 per thread) of plane j and walks every sample and every
//                   step >= t_begin in order, the next plane's load in flight.  A thread keeps the fp64 accumulators of its own four
//                   pixels for up to NM maps in registers (NM = 4 or 8, chosen by the host from nmaps; the map a term feeds is
//                   uniform over the grid, so the select is a scalar branch, not a register index) and the 32-bit below-eps counts
//                   of the same pixels; at the end it adds them to the persistent maps and int64 counts - no two threads share a
//                   pixel.  With the indicator on each wave also reduces sum w[p] below[p] of every (b, t) to one partial, and
//                   sum w[p] once.
//   regress_frac    one wave per (plane, side): the partials of each (b, t) summed in a fixed order (lane strides, then a
//                   butterfly), divided by the sum of weights and added up over b and t in order, then added to below_frac.
// No float atomics, no host synchronisation, no allocation: two identical runs are bitwise identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "diag_common.h"

namespace {

constexpr int MAX_MAPS = ACE_DIAG_REGRESS_MAX_MAPS;     // 8 maps x 4 pixels x fp64 = 64 VGPRs of accumulators: no spill
constexpr int MAX_TERMS = 64;

struct RegArgs {
    const float* const* src[2];
    const long* strides[2];
    const int* rows;
    const int* wrows;
    const float* weights;
    const double* coef;
    const int* slot;
    const float* eps;
    double* maps;
    long long* below_count;
    double* below_frac;
    double* partial;         // [2][nplanes][B][T][nparts] sum w below, then [2][nplanes][nparts] sum w
    int nw, nrows, nterms, nmaps, t_begin, nplanes, B, T;
    long HW;
    int nchunk;
};

template <int NM, bool IND>
__global__ __launch_bounds__(NT) void regress_window_kernel(RegArgs a) {
#pragma clang fp contract(off)
    const int chunk = blockIdx.x, j = blockIdx.y, side = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* base = a.src[side][j];
    const int r = a.rows[j];
    if (base == nullptr || r < 0 || r >= a.nrows) return;
    const long HW = a.HW, p = (long)chunk * CHUNK + (long)threadIdx.x * PIX;
    const long sb = a.strides[side][2 * j], st = a.strides[side][2 * j + 1];
    const bool vec = DIAG_VEC4_OK(base, HW, sb, st);
    const int B = a.B, T = a.T, t_begin = a.t_begin, span = T - t_begin, n = B * span;
    const long nparts = (long)a.nchunk * WAVES, part = (long)chunk * WAVES + wave;
    double acc[NM > 0 ? NM : 1][PIX];
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int k = 0; k < PIX; ++k) acc[m][k] = 0.0;
    int cnt[PIX] = {0, 0, 0, 0};
    float wv[PIX] = {0.f, 0.f, 0.f, 0.f};
    float eps = 0.f;
    bool ind = false;                // uniform over the workgroup
    double* q = nullptr;
    if (IND) {
        const int wr = a.wrows[j];
        ind = wr >= 0 && wr < a.nw;
        if (ind) {
            const float* wrow = a.weights + (long)wr * HW;
            const float4 w4 = load4(wrow, p, HW, DIAG_VEC4_ROW_OK(wrow, HW));
            wv[0] = w4.x; wv[1] = w4.y; wv[2] = w4.z; wv[3] = w4.w;
            eps = a.eps[j];
            q = a.partial + ((long)side * a.nplanes + j) * B * T * nparts + part;
            double W = 0.0;
#pragma unroll
            for (int k = 0; k < PIX; ++k)
                if (wv[k] != 0.0f) W += (double)wv[k];       // pixels past the plane loaded a weight of 0
            W = wave_sum(W);
            if (lane == 0) a.partial[2L * a.nplanes * B * T * nparts + ((long)side * a.nplanes + j) * nparts + part] = W;
        }
    }
    if (n > 0) {
        float4 nx = load4(base + (long)t_begin * st, p, HW, vec);
        for (int i = 0; i < n; ++i) {
            const int b = i / span, t = t_begin + (i - b * span);
            const float4 x4 = nx;
            if (i + 1 < n) {                           // the next plane's load is in flight during this plane's sums
                const int b1 = (i + 1) / span, t1 = t_begin + ((i + 1) - b1 * span);
                nx = load4(base + (long)b1 * sb + (long)t1 * st, p, HW, vec);
            }
            const float xv[PIX] = {x4.x, x4.y, x4.z, x4.w};
            if (NM > 0) {
                for (int k = 0; k < a.nterms; ++k) {
                    const int s = a.slot[k * B + b];
                    if (s < 0 || s >= a.nmaps) continue;
                    const double c = a.coef[((long)k * B + b) * T + t];
#pragma unroll
                    for (int m = 0; m < NM; ++m)
                        if (s == m) {
#pragma unroll
                            for (int e = 0; e < PIX; ++e) acc[m][e] += c * (double)xv[e];      // product rounded, then added
                        }
                }
            }
            if (IND && ind) {
                double S = 0.0;
#pragma unroll
                for (int e = 0; e < PIX; ++e) {
                    const bool below = xv[e] <= eps;       // NaN: not below; pixels past the plane have weight 0 and are not stored
                    cnt[e] += below ? 1 : 0;
                    if (below && wv[e] != 0.0f) S += (double)wv[e];
                }
                S = wave_sum(S);
                if (lane == 0) q[((long)b * T + t) * nparts] = S;
            }
        }
    }
    if (NM > 0) {
        double* out = a.maps + (((long)side * a.nrows + r) * a.nmaps) * HW;
#pragma unroll
        for (int m = 0; m < NM; ++m)
            if (m < a.nmaps) {
#pragma unroll
                for (int e = 0; e < PIX; ++e)
                    if (p + e < HW) out[(long)m * HW + p + e] += acc[m][e];
            }
    }
    if (IND && ind) {
        long long* c = a.below_count + ((long)side * a.nrows + r) * HW;
#pragma unroll
        for (int e = 0; e < PIX; ++e)
            if (p + e < HW) c[p + e] += (long long)cnt[e];
    }
}

// one wave per (plane, side)
__global__ __launch_bounds__(64) void regress_frac_kernel(RegArgs a) {
#pragma clang fp contract(off)
    const int j = blockIdx.x, side = blockIdx.y, lane = threadIdx.x;
    const int r = a.rows[j], wr = a.wrows[j];
    if (a.src[side][j] == nullptr || r < 0 || r >= a.nrows || wr < 0 || wr >= a.nw) return;
    const long nparts = (long)a.nchunk * WAVES;
    const int B = a.B, T = a.T;
    const double* den = a.partial + 2L * a.nplanes * B * T * nparts + ((long)side * a.nplanes + j) * nparts;
    double W = 0.0;
    for (long i = lane; i < nparts; i += 64) W += den[i];
    W = wave_sum(W);
    double frac = 0.0;
    for (int b = 0; b < B; ++b)
        for (int t = a.t_begin; t < T; ++t) {
            const double* q = a.partial + ((((long)side * a.nplanes + j) * B + b) * T + t) * nparts;
            double S = 0.0;
            for (long i = lane; i < nparts; i += 64) S += q[i];
            S = wave_sum(S);
            frac += S / W;
        }
    if (lane == 0) a.below_frac[(long)side * a.nrows + r] += frac;
}

bool shape_ok(int nplanes, int batch, int steps, long hw) {
    return nplanes >= 0 && nplanes <= 65535 && batch >= 1 && steps >= 1 && (long)batch * steps <= 2147483647L && hw >= 1 &&
           nchunk_for(hw) <= 2147483647L;
}

template <int NM>
void launch(const RegArgs& a, bool ind, dim3 grid, hipStream_t s) {
    if (ind) hipLaunchKernelGGL((regress_window_kernel<NM, true>), grid, dim3(NT), 0, s, a);
    else hipLaunchKernelGGL((regress_window_kernel<NM, false>), grid, dim3(NT), 0, s, a);
}

}  // namespace

extern "C" long ace_diag_regress_partial_doubles(int nplanes, int batch, int steps, long hw) {
    if (!shape_ok(nplanes, batch, steps, hw)) return -1;
    return 2L * nplanes * nchunk_for(hw) * WAVES * ((long)batch * steps + 1);
}

extern "C" int ace_diag_regress_window(const float* const* gen, const long* gen_strides, const float* const* target,
                                       const long* target_strides, const int* rows, const double* coef, const int* slot,
                                       double* maps, const float* eps, const int* wrows, const float* weights, int nw,
                                       double* partial, long long* below_count, double* below_frac, int nrows, int nterms,
                                       int nmaps, int t_begin, int nplanes, int batch, int steps, long hw, void* stream) {
    if (nplanes < 0 || nplanes > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_regress_window: need 0 <= nplanes <= 65535");
    if (nmaps < 0 || nmaps > MAX_MAPS)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_regress_window: need 0 <= nmaps <= " + std::to_string(MAX_MAPS) +
                                               " (the accumulators of a pixel stay in registers); split the maps over several calls");
    if (nterms < 0 || nterms > MAX_TERMS || (nterms > 0 && nmaps == 0))
        return ace::fail(ACE_ERR_INVALID, "ace_diag_regress_window: need 0 <= nterms <= 64, and nmaps >= 1 when nterms > 0");
    if (batch < 1 || steps < 1 || (long)batch * steps > 2147483647L)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_regress_window: need batch >= 1, steps >= 1, batch * steps < 2^31 (32-bit "
                                               "counters per thread)");
    if (hw < 1 || nchunk_for(hw) > 2147483647L || nrows < 1)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_regress_window: need 1 <= hw <= 1024 * (2^31 - 1), nrows >= 1");
    if (t_begin < 0) return ace::fail(ACE_ERR_INVALID, "ace_diag_regress_window: need t_begin >= 0");
    if (nplanes == 0) return ACE_OK;
    if (!gen || !gen_strides || !target || !target_strides || !rows)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_regress_window: null argument");
    if (nterms > 0 && (!coef || !slot || !maps))
        return ace::fail(ACE_ERR_INVALID, "ace_diag_regress_window: null argument (coef, slot and maps are needed when nterms > 0)");
    const bool ind = eps != nullptr;
    if (ind && (!wrows || !weights || !partial || !below_count || !below_frac || nw < 1))
        return ace::fail(ACE_ERR_INVALID, "ace_diag_regress_window: null argument (wrows, weights, partial, below_count and "
                                               "below_frac are needed when eps is given)");
    if ((nterms == 0 && !ind) || t_begin >= steps) return ACE_OK;
    RegArgs a;
    a.src[0] = gen; a.src[1] = target;
    a.strides[0] = gen_strides; a.strides[1] = target_strides;
    a.rows = rows; a.wrows = wrows; a.weights = weights; a.coef = coef; a.slot = slot; a.eps = eps;
    a.maps = maps; a.below_count = below_count; a.below_frac = below_frac; a.partial = partial;
    a.nw = nw; a.nrows = nrows; a.nterms = nterms; a.nmaps = nterms > 0 ? nmaps : 0; a.t_begin = t_begin;
    a.nplanes = nplanes; a.B = batch; a.T = steps; a.HW = hw;
    a.nchunk = (int)nchunk_for(hw);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)a.nchunk, nplanes, 2);
    if (a.nmaps == 0) launch<0>(a, ind, grid, s);
    else if (a.nmaps <= 4) launch<4>(a, ind, grid, s);
    else launch<MAX_MAPS>(a, ind, grid, s);
    ACE_HIP_TRY(hipGetLastError());
    if (ind) {
        hipLaunchKernelGGL(regress_frac_kernel, dim3(nplanes, 2), dim3(64), 0, s, a);
        ACE_HIP_TRY(hipGetLastError());
    }
    return ACE_OK;
}
