// The regional file writers' reduction (fme/ace/inference/data_writer/file_writer.py:505-551: a latitude / longitude box, a
// selection of steps, optionally after block means over time): per-pixel sums over runs of steps of a window, of the pixels of one
// rectangle of the plane only, written as a compact record.  The reference copies every step of every field to the host and cuts
// there with xarray; here one call covers all names of a window, only the box and only the steps of some segment are read, and
// what leaves the device is the kept record.
//   region_segments  the compact record of a (plane, sample, segment) is nlat_r * nlon_r pixels, row-major; workgroup (chunk, plane
//                  j, sample b) owns 1024 consecutive pixels of it, thread i the four from chunk * 1024 + 4 i.  Compact pixel q is
//                  the source pixel (lat0 + q / nlon_r) * nlon + lon0 + q % nlon_r: the four source offsets are formed once per
//                  thread, before the loops.  When nlon_r, lon0, nlon, the base and both strides are all multiples of 4 floats the
//                  four pixels lie in one region row, 16-byte aligned, and are one 16-byte load (the workgroup takes the vector
//                  path as a whole: the predicate depends on the plane, not on the thread); otherwise they may lie in two rows
//                  and are loaded one by one.  The rest is time_segments' (timeseg.hip): the fp64 sums of the four pixels stay in
//                  registers across a segment, the loads of UNROLL steps are issued ahead of the adds, the adds stay in step order.
// No atomics, no host synchronisation, no allocation: two identical runs are bitwise identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "diag_common.h"

namespace {

constexpr int UNROLL = 8;

struct RegionArgs {
    const float* const* srcs;
    const long* strides;
    const int* rows;
    const int* bounds;
    double* sums;
    float* means;
    int nrows, nseg, B, T;
    int nlon, lat0, lon0, nlon_r;
    long R;                               // nlat_r * nlon_r, the pixels of the region
};

__device__ __forceinline__ int clamp_step(int e, int T) { return e < 0 ? 0 : (e > T ? T : e); }

__device__ __forceinline__ void add4(double (&acc)[PIX], const float4& v) {
    acc[0] += (double)v.x;
    acc[1] += (double)v.y;
    acc[2] += (double)v.z;
    acc[3] += (double)v.w;
}

// the four pixels of a thread from the plane at s: one 16-byte load at off[0], or four loads at off[0 .. 3]
template <bool VEC>
__device__ __forceinline__ float4 fetch4(const float* s, const long (&off)[PIX]) {
    if (VEC) return *reinterpret_cast<const float4*>(s + off[0]);
    return make_float4(s[off[0]], s[off[1]], s[off[2]], s[off[3]]);
}

template <bool VEC>
__device__ __forceinline__ void region_segments_body(const RegionArgs& a, const float* x, long st, int r, int b, long p) {
#pragma clang fp contract(off)
    const long R = a.R;
    // source offsets of the compact pixels p .. p + 3; a pixel past the end of the region reads the last one and is never stored
    long off[PIX];
#pragma unroll
    for (int k = 0; k < PIX; ++k) {
        const long q = p + k < R ? p + k : R - 1;
        off[k] = ((long)a.lat0 + q / a.nlon_r) * a.nlon + a.lon0 + q % a.nlon_r;
    }
    const int T = a.T, nseg = a.nseg;
    const int* bd = a.bounds + (long)b * nseg * 2;
    const long out0 = (((long)r * a.B + b) * nseg) * R + p;
    // whole 16-byte stores where the four pixels exist and every record of the outputs starts aligned
    const bool full = p + 3 < R;
    const bool svec = full && (R & 1) == 0 && (reinterpret_cast<uintptr_t>(a.sums) & 15u) == 0;
    const bool mvec = full && (R & 3) == 0 && (reinterpret_cast<uintptr_t>(a.means) & 15u) == 0;
    for (int s = 0; s < nseg; ++s) {
        const int lo = clamp_step(bd[2 * (long)s], T), hi = clamp_step(bd[2 * (long)s + 1], T);
        double acc[PIX] = {0.0, 0.0, 0.0, 0.0};
        int t = lo;
        for (; t + UNROLL <= hi; t += UNROLL) {
            float4 v[UNROLL];
#pragma unroll
            for (int k = 0; k < UNROLL; ++k) v[k] = fetch4<VEC>(x + (long)(t + k) * st, off);
#pragma unroll
            for (int k = 0; k < UNROLL; ++k) add4(acc, v[k]);
        }
        if (t < hi) {                                      // the remainder: its loads issued together too, the adds in order
            const int rem = hi - t;                        // 1 .. UNROLL - 1, uniform over the workgroup
            float4 v[UNROLL - 1];
#pragma unroll
            for (int k = 0; k < UNROLL - 1; ++k)
                if (k < rem) v[k] = fetch4<VEC>(x + (long)(t + k) * st, off);
#pragma unroll
            for (int k = 0; k < UNROLL - 1; ++k)
                if (k < rem) add4(acc, v[k]);
        }
        const int n = hi > lo ? hi - lo : 0;
        const long o = out0 + (long)s * R;
        if (a.sums) {
            double* q = a.sums + o;
            if (svec) {
                *reinterpret_cast<double2*>(q) = make_double2(acc[0], acc[1]);
                *reinterpret_cast<double2*>(q + 2) = make_double2(acc[2], acc[3]);
            } else {
#pragma unroll
                for (int k = 0; k < PIX; ++k)
                    if (p + k < R) q[k] = acc[k];
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
                    if (p + k < R) q[k] = m[k];
            }
        }
    }
}

__global__ __launch_bounds__(NT) void region_segments_kernel(RegionArgs a) {
    const int chunk = blockIdx.x, j = blockIdx.y, b = blockIdx.z;
    const float* base = a.srcs[j];
    const int r = a.rows[j];
    if (base == nullptr || r < 0 || r >= a.nrows) return;
    const long p = (long)chunk * CHUNK + (long)threadIdx.x * PIX;
    if (p >= a.R) return;                                  // no thread of this kernel waits for another
    const long sb = a.strides[2 * j], st = a.strides[2 * j + 1];
    // one decision for the workgroup: with all of these multiples of 4 floats a thread's four pixels are 16 aligned bytes of one row
    const bool vec = ((a.nlon_r | a.lon0 | a.nlon) & 3) == 0 && ((sb | st) & 3) == 0 && (reinterpret_cast<uintptr_t>(base) & 15u) == 0;
    const float* x = base + (long)b * sb;
    if (vec)
        region_segments_body<true>(a, x, st, r, b, p);
    else
        region_segments_body<false>(a, x, st, r, b, p);
}

}  // namespace

extern "C" int ace_diag_region_segments(const float* const* srcs, const long* strides, const int* rows, const int* bounds,
                                        double* sums, float* means, int nrows, int nseg, int nplanes, int batch, int steps,
                                        int nlat, int nlon, int lat0, int nlat_r, int lon0, int nlon_r, void* stream) {
    if (nplanes < 0 || nplanes > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_region_segments: need 0 <= nplanes <= 65535");
    if (batch < 1 || batch > 65535 || steps < 1)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_region_segments: need 1 <= batch <= 65535 (a grid dimension), steps >= 1");
    if (nlat < 1 || nlon < 1 || nrows < 1)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_region_segments: need nlat >= 1, nlon >= 1, nrows >= 1");
    if (lat0 < 0 || nlat_r < 1 || (long)lat0 + nlat_r > nlat)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_region_segments: need 0 <= lat0, 1 <= nlat_r, lat0 + nlat_r <= nlat");
    if (lon0 < 0 || nlon_r < 1 || (long)lon0 + nlon_r > nlon)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_region_segments: need 0 <= lon0, 1 <= nlon_r, lon0 + nlon_r <= nlon");
    const long R = (long)nlat_r * nlon_r;
    if (nchunk_for(R) > 2147483647L)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_region_segments: need nlat_r * nlon_r <= 1024 * (2^31 - 1)");
    if (nseg < 0 || nseg > 2147483646) return ace::fail(ACE_ERR_INVALID, "ace_diag_region_segments: need 0 <= nseg < 2^31 - 1");
    if (nplanes == 0 || nseg == 0) return ACE_OK;
    if (!srcs || !strides || !rows || !bounds) return ace::fail(ACE_ERR_INVALID, "ace_diag_region_segments: null argument");
    if (!sums && !means)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_region_segments: null argument (at least one of sums and means is needed)");
    RegionArgs a;
    a.srcs = srcs; a.strides = strides; a.rows = rows; a.bounds = bounds; a.sums = sums; a.means = means;
    a.nrows = nrows; a.nseg = nseg; a.B = batch; a.T = steps;
    a.nlon = nlon; a.lat0 = lat0; a.lon0 = lon0; a.nlon_r = nlon_r; a.R = R;
    const dim3 grid((unsigned)nchunk_for(R), nplanes, batch);
    hipLaunchKernelGGL(region_segments_kernel, grid, dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}
