// The data writers' reductions over time (fme/ace/inference/data_writer: time_coarsen.py:187-196, the block means of coarsen_factor
// steps; monthly.py:339-382, the sums over the steps of each calendar month): per-pixel sums over runs of consecutive steps of a
// window.  The reference forms them per name with torch / numpy ops on the whole window, the monthly ones after a copy of every step
// to the host; here one call covers all names of a window, every plane is read once, and what leaves the device is the reduced
// record.
//   time_segments  workgroup (chunk, plane j, sample b) owns 1024 pixels (4 per thread, one 16-byte load) of the fields of sample b
//                  of plane j.  A thread keeps the fp64 sums of its four pixels in registers, walks the segments of its sample in
//                  order and stores each segment's sum and mean as the segment closes: no scratch, no second pass.  The step loop
//                  depends on itself through the adds only, so the loads of UNROLL steps are issued before the adds that consume
//                  them (8 x 16 bytes x 256 threads = 32 KiB in flight per workgroup); the adds stay in step order, so the result
//                  does not depend on the unroll.
// No atomics, no host synchronisation, no allocation: two identical runs are bitwise identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "diag_common.h"

namespace {

constexpr int UNROLL = 8;

struct SegArgs {
    const float* const* srcs;
    const long* strides;
    const int* rows;
    const int* edges;
    double* sums;
    float* means;
    int nrows, nseg, B, T;
    long HW;
};

__device__ __forceinline__ int clamp_edge(int e, int T) { return e < 0 ? 0 : (e > T ? T : e); }

__device__ __forceinline__ void add4(double (&acc)[PIX], const float4& v) {
    acc[0] += (double)v.x;
    acc[1] += (double)v.y;
    acc[2] += (double)v.z;
    acc[3] += (double)v.w;
}

__global__ __launch_bounds__(NT) void time_segments_kernel(SegArgs a) {
#pragma clang fp contract(off)
    const int chunk = blockIdx.x, j = blockIdx.y, b = blockIdx.z;
    const float* base = a.srcs[j];
    const int r = a.rows[j];
    if (base == nullptr || r < 0 || r >= a.nrows) return;
    const long HW = a.HW, p = (long)chunk * CHUNK + (long)threadIdx.x * PIX;
    if (p >= HW) return;                                   // no thread of this kernel waits for another
    const long sb = a.strides[2 * j], st = a.strides[2 * j + 1];
    const bool vec = DIAG_VEC4_OK(base, HW, sb, st);
    const int T = a.T, nseg = a.nseg;
    const float* x = base + (long)b * sb;
    const int* e = a.edges + (long)b * (nseg + 1);
    const long out0 = (((long)r * a.B + b) * nseg) * HW + p;
    // whole 16-byte stores where the four pixels exist and every row of the outputs starts aligned
    const bool full = p + 3 < HW;
    const bool svec = full && (HW & 1) == 0 && (reinterpret_cast<uintptr_t>(a.sums) & 15u) == 0;
    const bool mvec = full && (HW & 3) == 0 && (reinterpret_cast<uintptr_t>(a.means) & 15u) == 0;
    int lo = clamp_edge(e[0], T);
    for (int s = 0; s < nseg; ++s) {
        const int hi = clamp_edge(e[s + 1], T);
        double acc[PIX] = {0.0, 0.0, 0.0, 0.0};
        int t = lo;
        for (; t + UNROLL <= hi; t += UNROLL) {
            float4 v[UNROLL];
#pragma unroll
            for (int k = 0; k < UNROLL; ++k) v[k] = load4(x + (long)(t + k) * st, p, HW, vec);
#pragma unroll
            for (int k = 0; k < UNROLL; ++k) add4(acc, v[k]);
        }
        if (t < hi) {                                      // the remainder: its loads issued together too, the adds in order
            const int rem = hi - t;                        // 1 .. UNROLL - 1, uniform over the workgroup
            float4 v[UNROLL - 1];
#pragma unroll
            for (int k = 0; k < UNROLL - 1; ++k)
                if (k < rem) v[k] = load4(x + (long)(t + k) * st, p, HW, vec);
#pragma unroll
            for (int k = 0; k < UNROLL - 1; ++k)
                if (k < rem) add4(acc, v[k]);
        }
        const int n = hi > lo ? hi - lo : 0;
        const long o = out0 + (long)s * HW;
        if (a.sums) {
            double* q = a.sums + o;
            if (svec) {
                *reinterpret_cast<double2*>(q) = make_double2(acc[0], acc[1]);
                *reinterpret_cast<double2*>(q + 2) = make_double2(acc[2], acc[3]);
            } else {
#pragma unroll
                for (int k = 0; k < PIX; ++k)
                    if (p + k < HW) q[k] = acc[k];
            }
        }
        if (a.means) {
            float m[PIX];
            const double dn = (double)n;                   // 0 for an empty segment: 0.0 / 0.0, NaN
#pragma unroll
            for (int k = 0; k < PIX; ++k) m[k] = (float)(acc[k] / dn);
            float* q = a.means + o;
            if (mvec) {
                *reinterpret_cast<float4*>(q) = make_float4(m[0], m[1], m[2], m[3]);
            } else {
#pragma unroll
                for (int k = 0; k < PIX; ++k)
                    if (p + k < HW) q[k] = m[k];
            }
        }
        lo = hi;
    }
}

}  // namespace

extern "C" int ace_diag_time_segments(const float* const* srcs, const long* strides, const int* rows, const int* edges,
                                      double* sums, float* means, int nrows, int nseg, int nplanes, int batch, int steps,
                                      long hw, void* stream) {
    if (nplanes < 0 || nplanes > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_time_segments: need 0 <= nplanes <= 65535");
    if (batch < 1 || batch > 65535 || steps < 1)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_time_segments: need 1 <= batch <= 65535 (a grid dimension), steps >= 1");
    if (hw < 1 || nchunk_for(hw) > 2147483647L || nrows < 1)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_time_segments: need 1 <= hw <= 1024 * (2^31 - 1), nrows >= 1");
    if (nseg < 0 || nseg > 2147483646) return ace::fail(ACE_ERR_INVALID, "ace_diag_time_segments: need 0 <= nseg < 2^31 - 1");
    if (nplanes == 0 || nseg == 0) return ACE_OK;
    if (!srcs || !strides || !rows || !edges) return ace::fail(ACE_ERR_INVALID, "ace_diag_time_segments: null argument");
    if (!sums && !means)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_time_segments: null argument (at least one of sums and means is needed)");
    SegArgs a;
    a.srcs = srcs; a.strides = strides; a.rows = rows; a.edges = edges; a.sums = sums; a.means = means;
    a.nrows = nrows; a.nseg = nseg; a.B = batch; a.T = steps; a.HW = hw;
    const dim3 grid((unsigned)nchunk_for(hw), nplanes, batch);
    hipLaunchKernelGGL(time_segments_kernel, grid, dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}
