// The evaluator's video metric (fme/ace/aggregator/inference/video.py:33-255): per time slot of the whole inference and per pixel,
// the means over the samples of the generated and the target field and, for the extended videos, of their squares and of the
// squared error, with the smallest and the largest error.  The reference forms each per name with separate torch ops on the whole
// window and adds every result into host fp64 buffers; here one call covers all names and both sides of a window, every plane is
// read once, and the (n_time, H W) accumulators stay in device memory.
//   video_window  workgroup (chunk, plane j, step t) owns 1024 pixels (4 per thread, one 16-byte load per side and sample) of step
//                 t of plane j.  A thread keeps the five fp64 sums and the two fp32 extrema of each of its four pixels in
//                 registers and loops over the samples; the loads of DEPTH samples of both sides are issued before the adds that
//                 consume them (2 x 4 x 16 bytes x 256 threads = 32 KiB in flight per workgroup), the adds stay in sample order,
//                 so the result does not depend on the depth.  Then one read-modify-write of its slots, or with assign one write.
// Each slot is owned by one thread: no atomics, no scratch, no LDS, no host synchronisation, no allocation; two identical runs
// are bitwise identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "diag_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int DEPTH = 4;                                   // samples whose loads are in flight ahead of the adds

struct VideoArgs {
    const float* const* gen;
    const long* gen_strides;
    const float* const* target;
    const long* target_strides;
    const int* rows;
    double* mean;
    double* sq;
    float* err;
    int nrows, n_time, t0, B;
    long HW;
};

struct PixAcc {
    double sg[PIX], st[PIX], sgg[PIX], stt[PIX], sdd[PIX];
    float mn[PIX], mx[PIX];
};

template <bool EXT>
__device__ __forceinline__ void add_sample(PixAcc& a, const float4& g4, const float4& y4, bool paired) {
    const float g[PIX] = {g4.x, g4.y, g4.z, g4.w}, y[PIX] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
    for (int k = 0; k < PIX; ++k) {
        const double gd = (double)g[k];
        a.sg[k] += gd;
        if (EXT) a.sgg[k] += gd * gd;
        if (paired) {
            const double yd = (double)y[k];
            a.st[k] += yd;
            if (EXT) {
                a.stt[k] += yd * yd;
                const float d = g[k] - y[k];               // the error in fp32, as the reference forms its error tensor
                const double dd = (double)d;
                a.sdd[k] += dd * dd;
                // a NaN error makes the extremum NaN, and a NaN extremum stays: d < NaN is false
                if (d < a.mn[k] || d != d) a.mn[k] = d;
                if (d > a.mx[k] || d != d) a.mx[k] = d;
            }
        }
    }
}

// q[0..3] (+)= v[0..3] for the pixels that exist; whole 16-byte accesses where vec
template <bool ASSIGN>
__device__ __forceinline__ void put_sums(double* q, const double (&v)[PIX], double B, bool vec, long p, long HW) {
    double w[PIX];
#pragma unroll
    for (int k = 0; k < PIX; ++k) w[k] = v[k] / B;
    if (vec) {
        double2* q2 = reinterpret_cast<double2*>(q);
        if (!ASSIGN) {
            const double2 o0 = q2[0], o1 = q2[1];
            w[0] = o0.x + w[0]; w[1] = o0.y + w[1]; w[2] = o1.x + w[2]; w[3] = o1.y + w[3];
        }
        q2[0] = make_double2(w[0], w[1]);
        q2[1] = make_double2(w[2], w[3]);
    } else {
#pragma unroll
        for (int k = 0; k < PIX; ++k)
            if (p + k < HW) q[k] = ASSIGN ? w[k] : q[k] + w[k];
    }
}

// the stored extremum joined with the window's: NaN on either side gives NaN
template <bool IS_MIN>
__device__ __forceinline__ float join(float old, float v) {
    return ((IS_MIN ? v < old : v > old) || v != v) ? v : old;
}

template <bool ASSIGN, bool IS_MIN>
__device__ __forceinline__ void put_ext(float* q, const float (&v)[PIX], bool vec, long p, long HW) {
    if (vec) {
        float4* q4 = reinterpret_cast<float4*>(q);
        float4 w = make_float4(v[0], v[1], v[2], v[3]);
        if (!ASSIGN) {
            const float4 o = *q4;
            w = make_float4(join<IS_MIN>(o.x, v[0]), join<IS_MIN>(o.y, v[1]), join<IS_MIN>(o.z, v[2]), join<IS_MIN>(o.w, v[3]));
        }
        *q4 = w;
    } else {
#pragma unroll
        for (int k = 0; k < PIX; ++k)
            if (p + k < HW) q[k] = ASSIGN ? v[k] : join<IS_MIN>(q[k], v[k]);
    }
}

template <bool EXT, bool ASSIGN>
__global__ __launch_bounds__(NT) void video_window_kernel(VideoArgs a) {
    const int chunk = blockIdx.x, j = blockIdx.y, t = blockIdx.z;
    const float* gbase = a.gen[j];
    const int r = a.rows[j];
    if (gbase == nullptr || r < 0 || r >= a.nrows) return;
    const long HW = a.HW, p = (long)chunk * CHUNK + (long)threadIdx.x * PIX;
    if (p >= HW) return;                                   // no thread of this kernel waits for another
    const float* ybase = a.target[j];
    const bool paired = ybase != nullptr;
    const long gsb = a.gen_strides[2 * j], gst = a.gen_strides[2 * j + 1];
    const long ysb = paired ? a.target_strides[2 * j] : 0, yst = paired ? a.target_strides[2 * j + 1] : 0;
    const bool gvec = DIAG_VEC4_OK(gbase, HW, gsb, gst);
    const bool yvec = paired && DIAG_VEC4_OK(ybase, HW, ysb, yst);
    const float* gx = gbase + (long)t * gst;
    const float* yx = paired ? ybase + (long)t * yst : nullptr;
    const int B = a.B;

    PixAcc acc;
#pragma unroll
    for (int k = 0; k < PIX; ++k) {
        acc.sg[k] = acc.st[k] = acc.sgg[k] = acc.stt[k] = acc.sdd[k] = 0.0;
        acc.mn[k] = INFINITY;
        acc.mx[k] = -INFINITY;
    }
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    int b = 0;
    for (; b + DEPTH <= B; b += DEPTH) {
        float4 g[DEPTH], y[DEPTH];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) {
            g[k] = load4(gx + (long)(b + k) * gsb, p, HW, gvec);
            y[k] = paired ? load4(yx + (long)(b + k) * ysb, p, HW, yvec) : zero;
        }
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) add_sample<EXT>(acc, g[k], y[k], paired);
    }
    if (b < B) {                                           // the remainder: its loads issued together too, the adds in order
        const int rem = B - b;                             // 1 .. DEPTH - 1, uniform over the grid
        float4 g[DEPTH - 1], y[DEPTH - 1];
#pragma unroll
        for (int k = 0; k < DEPTH - 1; ++k)
            if (k < rem) {
                g[k] = load4(gx + (long)(b + k) * gsb, p, HW, gvec);
                y[k] = paired ? load4(yx + (long)(b + k) * ysb, p, HW, yvec) : zero;
            }
#pragma unroll
        for (int k = 0; k < DEPTH - 1; ++k)
            if (k < rem) add_sample<EXT>(acc, g[k], y[k], paired);
    }

    // every index into the accumulators in 64-bit: nrows * n_time * hw passes 2^31 in real use
    const long plane = (long)a.nrows * a.n_time * HW;
    const long o = ((long)r * a.n_time + (a.t0 + t)) * HW + p;
    const bool full = p + 3 < HW;
    const bool dvec = full && (HW & 1) == 0;               // the bases are checked below, per buffer
    const double Bd = (double)B;
    const bool mvec = dvec && (reinterpret_cast<uintptr_t>(a.mean) & 15u) == 0;
    put_sums<ASSIGN>(a.mean + o, acc.sg, Bd, mvec, p, HW);
    if (paired) put_sums<ASSIGN>(a.mean + plane + o, acc.st, Bd, mvec, p, HW);
    if (EXT) {
        const bool svec = dvec && (reinterpret_cast<uintptr_t>(a.sq) & 15u) == 0;
        put_sums<ASSIGN>(a.sq + o, acc.sgg, Bd, svec, p, HW);
        if (paired) {
            put_sums<ASSIGN>(a.sq + plane + o, acc.stt, Bd, svec, p, HW);
            put_sums<ASSIGN>(a.sq + 2 * plane + o, acc.sdd, Bd, svec, p, HW);
            const bool evec = full && (HW & 3) == 0 && (reinterpret_cast<uintptr_t>(a.err) & 15u) == 0;
            put_ext<ASSIGN, true>(a.err + o, acc.mn, evec, p, HW);
            put_ext<ASSIGN, false>(a.err + plane + o, acc.mx, evec, p, HW);
        }
    }
}

}  // namespace

extern "C" int ace_diag_video_window(const float* const* gen, const long* gen_strides, const float* const* target,
                                     const long* target_strides, const int* rows, double* mean, double* sq, float* err, int nrows,
                                     int n_time, int t0, int assign, int nplanes, int batch, int steps, long hw, void* stream) {
    if (nplanes < 0 || nplanes > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_video_window: need 0 <= nplanes <= 65535 (a grid dimension)");
    if (batch < 1 || steps < 1 || steps > 65535)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_video_window: need batch >= 1 and 1 <= steps <= 65535 (a grid dimension)");
    if (hw < 1 || nchunk_for(hw) > 2147483647L || nrows < 1 || n_time < 1)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_video_window: need 1 <= hw <= 1024 * (2^31 - 1), nrows >= 1, n_time >= 1");
    if (t0 < 0 || (long)t0 + steps > n_time)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_video_window: need t0 >= 0 and t0 + steps <= n_time");
    if (!mean) return ace::fail(ACE_ERR_INVALID, "ace_diag_video_window: null argument (mean)");
    if ((sq == nullptr) != (err == nullptr))
        return ace::fail(ACE_ERR_INVALID, "ace_diag_video_window: sq and err are given together (the extended videos) or not at all");
    if (nplanes == 0) return ACE_OK;
    if (!gen || !gen_strides || !target || !target_strides || !rows)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_video_window: null argument");
    VideoArgs a;
    a.gen = gen; a.gen_strides = gen_strides; a.target = target; a.target_strides = target_strides; a.rows = rows;
    a.mean = mean; a.sq = sq; a.err = err; a.nrows = nrows; a.n_time = n_time; a.t0 = t0; a.B = batch; a.HW = hw;
    const dim3 grid((unsigned)nchunk_for(hw), nplanes, steps);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (sq) {
        if (assign) hipLaunchKernelGGL((video_window_kernel<true, true>), grid, dim3(NT), 0, s, a);
        else hipLaunchKernelGGL((video_window_kernel<true, false>), grid, dim3(NT), 0, s, a);
    } else {
        if (assign) hipLaunchKernelGGL((video_window_kernel<false, true>), grid, dim3(NT), 0, s, a);
        else hipLaunchKernelGGL((video_window_kernel<false, false>), grid, dim3(NT), 0, s, a);
    }
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}
