// Static spatial masking of the stepper (fme/core/spatial_masking.py:98-150) as single launches over every plane of a step:
//   data[name] = fill where round(mask) == mask_value
// The comparison itself is not evaluated here.  The caller computes one uint8 hit plane per distinct 2-D mask with exactly the
// torch expression of the reference (torch.round(mask).to(torch.int64) == mask_value, on the device), so NaN masks, halves and
// the int64 conversion behave as they do in torch; the kernels only select between the fill and the source value, and their
// output is bitwise the torch path's.
//   mask_planes          one pass per plane: dst = hit ? fill : src (in place allowed; an unmasked in-place plane is skipped)
//   mask_pack_normalize  the stepper's pack_normalize_kernel with the input masking folded in: the masked value is optionally
//                        staged (the corrector reads the masked input) and normalised into the packed network input with the
//                        same two roundings; planes past `npack` are masked and staged only (the corrector's next-step data)
// Both are memory bound: one read of each source and of its hit plane, one write per destination.  float4 accesses per
// (plane, sample) when hw % 4 == 0 and every address of the plane is 16-byte aligned; scalar otherwise.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ace_sfno.h"
#include "errors.h"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ float sel(unsigned char hit, float fill, float v) { return hit ? fill : v; }

__device__ __forceinline__ float4 sel4(uchar4 h, float fill, float4 v) {
    return make_float4(sel(h.x, fill, v.x), sel(h.y, fill, v.y), sel(h.z, fill, v.z), sel(h.w, fill, v.w));
}

// normalizer.py:221: (t - means[k]) / stds[k], two roundings (as pack_normalize_kernel)
__device__ __forceinline__ float norm(float v, float mu, float sd) { return __fdiv_rn(__fsub_rn(v, mu), sd); }

// the hit plane of plane j (nullptr: unmasked); an index outside [0, nmask) counts as unmasked
__device__ __forceinline__ const unsigned char* hit_plane(const int* mask_idx, const unsigned char* hits, int nmask, int j, long HW) {
    const int m = mask_idx[j];
    return (m >= 0 && m < nmask) ? hits + (long)m * HW : nullptr;
}

// src and dst may be the same plane: no __restrict__ on them
__global__ __launch_bounds__(NT) void mask_planes_kernel(const float* const* srcs, const long* __restrict__ src_strides,
                                                         float* const* dsts, const long* __restrict__ dst_strides,
                                                         const int* __restrict__ mask_idx, const unsigned char* __restrict__ hits,
                                                         int nmask, const float* __restrict__ fill, long HW) {
    const int j = blockIdx.y, b = blockIdx.z;
    const float* s = srcs[j] + (long)b * src_strides[j];
    float* d = dsts[j] + (long)b * dst_strides[j];
    const unsigned char* h = hit_plane(mask_idx, hits, nmask, j, HW);
    if (!h && s == d) return;     // unmasked, in place: nothing to do
    const float f = fill[j];
    const long t0 = (long)blockIdx.x * NT + threadIdx.x, dt = (long)gridDim.x * NT;
    if ((HW & 3) == 0 && aligned16(s) && aligned16(d) && (!h || (reinterpret_cast<uintptr_t>(h) & 3u) == 0)) {
        const long n4 = HW >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(s);
        float4* d4 = reinterpret_cast<float4*>(d);
        if (h) {
            const uchar4* h4 = reinterpret_cast<const uchar4*>(h);
            for (long t = t0; t < n4; t += dt) d4[t] = sel4(h4[t], f, s4[t]);
        } else {
            for (long t = t0; t < n4; t += dt) d4[t] = s4[t];
        }
        return;
    }
    if (h) {
        for (long t = t0; t < HW; t += dt) d[t] = sel(h[t], f, s[t]);
    } else {
        for (long t = t0; t < HW; t += dt) d[t] = s[t];
    }
}

// src and stage may be the same plane; x is never a source
__global__ __launch_bounds__(NT) void mask_pack_normalize_kernel(const float* const* srcs, const long* __restrict__ src_strides,
                                                                 const int* __restrict__ mask_idx,
                                                                 const unsigned char* __restrict__ hits, int nmask,
                                                                 const float* __restrict__ fill, float* const* stage,
                                                                 const long* __restrict__ stage_strides,
                                                                 const float* __restrict__ mean, const float* __restrict__ stdv,
                                                                 float* __restrict__ x, int npack, long HW) {
    const int j = blockIdx.y, b = blockIdx.z;
    const float* s = srcs[j] + (long)b * src_strides[j];
    float* st = stage ? stage[j] : nullptr;
    if (st) st += (long)b * stage_strides[j];
    const bool pack = j < npack;
    if (!pack && !st) return;
    float* d = pack ? x + ((long)b * npack + j) * HW : nullptr;
    const unsigned char* h = hit_plane(mask_idx, hits, nmask, j, HW);
    const float f = fill[j];
    const float mu = pack ? mean[j] : 0.0f, sd = pack ? stdv[j] : 1.0f;
    const long t0 = (long)blockIdx.x * NT + threadIdx.x, dt = (long)gridDim.x * NT;
    const bool vec = (HW & 3) == 0 && aligned16(s) && (!st || aligned16(st)) && (!d || aligned16(d)) &&
                     (!h || (reinterpret_cast<uintptr_t>(h) & 3u) == 0);
    if (vec) {
        const long n4 = HW >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(s);
        const uchar4* h4 = reinterpret_cast<const uchar4*>(h);
        for (long t = t0; t < n4; t += dt) {
            float4 v = s4[t];
            if (h) v = sel4(h4[t], f, v);
            if (st) reinterpret_cast<float4*>(st)[t] = v;
            if (d) reinterpret_cast<float4*>(d)[t] = make_float4(norm(v.x, mu, sd), norm(v.y, mu, sd), norm(v.z, mu, sd),
                                                                 norm(v.w, mu, sd));
        }
        return;
    }
    for (long t = t0; t < HW; t += dt) {
        float v = s[t];
        if (h) v = sel(h[t], f, v);
        if (st) st[t] = v;
        if (d) d[t] = norm(v, mu, sd);
    }
}

// the grid of launch_pack_normalize: up to 64 workgroups of 256 threads per (plane, sample), grid-stride beyond
dim3 grid_for(long HW, int nplanes, int batch) {
    unsigned gx = (unsigned)((HW + 1023) / 1024);
    if (gx > 64) gx = 64;
    if (gx < 1) gx = 1;
    return dim3(gx, nplanes, batch);
}

bool bad_shape(int nplanes, int batch, long hw) { return nplanes < 0 || nplanes > 65535 || batch < 1 || batch > 65535 || hw < 1; }

}  // namespace

extern "C" int ace_mask_planes(const float* const* srcs, const long* src_strides, float* const* dsts, const long* dst_strides,
                               const int* mask_idx, const unsigned char* hits, int nmask, const float* fill, int nplanes, int batch,
                               long hw, void* stream) {
    if (bad_shape(nplanes, batch, hw) || nmask < 0) return ace::fail(ACE_ERR_INVALID, "ace_mask_planes: bad shape");
    if (nplanes == 0) return ACE_OK;
    if (!srcs || !src_strides || !dsts || !dst_strides || !mask_idx || !fill || (nmask > 0 && !hits))
        return ace::fail(ACE_ERR_INVALID, "ace_mask_planes: null argument");
    hipLaunchKernelGGL(mask_planes_kernel, grid_for(hw, nplanes, batch), dim3(NT), 0, static_cast<hipStream_t>(stream), srcs,
                       src_strides, dsts, dst_strides, mask_idx, hits, nmask, fill, hw);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_mask_pack_normalize(const float* const* srcs, const long* src_strides, const int* mask_idx,
                                       const unsigned char* hits, int nmask, const float* fill, float* const* stage,
                                       const long* stage_strides, const float* mean, const float* std_, float* dst, int npack,
                                       int nplanes, int batch, long hw, void* stream) {
    if (bad_shape(nplanes, batch, hw) || nmask < 0 || npack < 0 || npack > nplanes)
        return ace::fail(ACE_ERR_INVALID, "ace_mask_pack_normalize: bad shape (0 <= npack <= nplanes)");
    if (nplanes == 0) return ACE_OK;
    if (!srcs || !src_strides || !mask_idx || !fill || (nmask > 0 && !hits) || (stage && !stage_strides) ||
        (npack > 0 && (!mean || !std_ || !dst)))
        return ace::fail(ACE_ERR_INVALID, "ace_mask_pack_normalize: null argument");
    hipLaunchKernelGGL(mask_pack_normalize_kernel, grid_for(hw, nplanes, batch), dim3(NT), 0, static_cast<hipStream_t>(stream),
                       srcs, src_strides, mask_idx, hits, nmask, fill, stage, stage_strides, mean, std_, dst, npack, hw);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}
