// Global-mean removal of the single-module step (fme/core/step/global_mean_removal.py, applied by step_with_adjustments,
// fme/core/step/single_module.py:650-668) folded into the stepper's pack and unpack launches:
//   gmr_partials            fp64 partial sums of the K reduced planes over fixed chunks of GMR_CHUNK pixels
//   gmr_pack_normalize      pack_normalize_kernel with the shift of a listed channel added in front of the normaliser, the
//                           synthetic channels (-shift / std, broadcast) written behind the in_names, the shifts published
//   gmr_unpack_denormalize  unpack_denormalize_kernel with the shift of a listed channel subtracted behind the de-normaliser
//   gmr_sample_means        the same chunk-ordered finisher on its own (the host transform of ace_amd/global_mean_removal.py)
// The reduction order is the contract of include/ace_sfno.h ("Global-mean removal"), restated in tests/_gmr_ref.py: a chunk's
// sum depends on the pixel values and on hw only - not on the alignment of the plane (the 16-byte and the 4-byte load paths feed
// the same accumulators in the same order), the batch, or the number of planes - and every consumer of the partials adds them
// in chunk order, so there is one sample mean per (sample, plane) whoever computes it.  No atomics, no workgroup waits for
// another: the pack launch reads what the partials launch wrote, in stream order.
// The reduction is latency bound (K x B x hw x 4 bytes, 259 KB per plane at 1 degree); pack and unpack move the bytes of the
// plain kernels plus the synthetic channels.  float4 accesses per (plane, sample) when hw % 4 == 0 and every address of the
// plane is 16-byte aligned, chosen once per workgroup; scalar otherwise.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "kernels.h"

namespace ace {

namespace {

constexpr int NT = 256;
constexpr int GMR_CHUNK = 4096;                 // pixels per partial sum
constexpr int ROUNDS = GMR_CHUNK / (4 * NT);    // float4 loads per thread and chunk, all in flight
static_assert(ROUNDS * 4 * NT == GMR_CHUNK, "a chunk is a whole number of float4 rounds of the workgroup");

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Pixel i of a chunk goes to accumulator i % 4 of thread (i / 4) % NT, in round i / (4 NT): rounds ascending.  Pixels past the
// end of the plane add +0.0, which changes no accumulator (they start at +0.0).
__global__ __launch_bounds__(NT) void gmr_partials_kernel(const float* const* __restrict__ srcs, const long* __restrict__ strides,
                                                          const int* __restrict__ plane_idx, int nsrc,
                                                          double* __restrict__ partials, int K, long HW, long nchunks) {
    const int c = blockIdx.x, k = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    double* out = partials + ((long)b * K + k) * nchunks + c;
    const int j = plane_idx[k];
    if (j < 0 || j >= nsrc) {       // an index outside the table row: no read, the mean of this (sample, plane) is NaN
        if (t == 0) *out = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const float* plane = srcs[j] + (long)b * strides[j];
    const long e0 = (long)c * GMR_CHUNK;
    const float* x = plane + e0;
    const long left = HW - e0;
    const int n = left < GMR_CHUNK ? (int)left : GMR_CHUNK;
    float4 v[ROUNDS];
    if ((HW & 3) == 0 && aligned16(plane)) {        // e0 % 4 == 0 and n % 4 == 0: every quad is whole and aligned
        const float4* x4 = reinterpret_cast<const float4*>(x);
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int g = r * NT + t;
            v[r] = 4 * g < n ? x4[g] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    } else {
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int i = 4 * (r * NT + t);
            v[r].x = i < n ? x[i] : 0.0f;
            v[r].y = i + 1 < n ? x[i + 1] : 0.0f;
            v[r].z = i + 2 < n ? x[i + 2] : 0.0f;
            v[r].w = i + 3 < n ? x[i + 3] : 0.0f;
        }
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        a0 += (double)v[r].x;
        a1 += (double)v[r].y;
        a2 += (double)v[r].z;
        a3 += (double)v[r].w;
    }
    double s = (a0 + a1) + (a2 + a3);
    // lanes of a wave: s[l] += s[l + off], off = 32, 16, 8, 4, 2, 1 (lane 0 holds the wave's sum)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    __shared__ double wave_sum[NT / 64];
    if ((t & 63) == 0) wave_sum[t >> 6] = s;
    __syncthreads();
    if (t == 0) *out = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// the partials of (b, k) added in chunk order, divided by hw in fp64, rounded to fp32 once
__device__ __forceinline__ float sample_mean(const double* __restrict__ partials, int b, int k, int K, long nchunks, long HW) {
    const double* p = partials + ((long)b * K + k) * nchunks;
    double s = p[0];
    for (long c = 1; c < nchunks; ++c) s += p[c];
    return (float)(s / (double)HW);
}

// global_mean_removal.py:231 / :316: means[field] - sample_mean, an fp32 subtraction
__device__ __forceinline__ float sample_shift(const double* __restrict__ partials, const float* __restrict__ clim_mean, int b,
                                              int k, int K, long nchunks, long HW) {
    return __fsub_rn(clim_mean[k], sample_mean(partials, b, k, K, nchunks, HW));
}

__global__ __launch_bounds__(NT) void gmr_sample_means_kernel(const double* __restrict__ partials, float* __restrict__ means,
                                                              int Bt, int K, long nchunks, long HW) {
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i < (long)Bt * K) means[i] = sample_mean(partials, (int)(i / K), (int)(i % K), K, nchunks, HW);
}

// global_mean_removal.py:247 / :322 then normalizer.py:221: ((t + shift) - means[k]) / stds[k], three roundings
__device__ __forceinline__ float shift_norm(float v, float sh, float mu, float sd) {
    return __fdiv_rn(__fsub_rn(__fadd_rn(v, sh), mu), sd);
}
__device__ __forceinline__ float norm(float v, float mu, float sd) { return __fdiv_rn(__fsub_rn(v, mu), sd); }

__global__ __launch_bounds__(NT) void gmr_pack_normalize_kernel(const float* const* __restrict__ srcs, const long* __restrict__ strides,
                                                                const float* __restrict__ mean, const float* __restrict__ stdv,
                                                                const int* __restrict__ shift_idx,
                                                                const double* __restrict__ partials,
                                                                const float* __restrict__ clim_mean,
                                                                const int* __restrict__ extra_idx,
                                                                const float* __restrict__ extra_std, float* __restrict__ dst,
                                                                float* __restrict__ shift, int nin, int nextra, int K, long HW,
                                                                long nchunks) {
    const int j = blockIdx.y, b = blockIdx.z;
    float* d = dst + ((long)b * (nin + nextra) + j) * HW;
    // the shift of (b, k) is published by the first workgroup of channel k (K <= nin): the bits every user of it computes
    if (blockIdx.x == 0 && j < K && threadIdx.x == 0) shift[(long)b * K + j] = sample_shift(partials, clim_mean, b, j, K, nchunks, HW);
    const long t0 = (long)blockIdx.x * NT + threadIdx.x, dt = (long)gridDim.x * NT;
    const bool quads = (HW & 3) == 0 && aligned16(d);
    if (j >= nin) {     // synthetic channel (global_mean_removal.py:236 / :329): (-shift) / std, broadcast over the plane
        const int k = extra_idx[j - nin];
        const float v = (k >= 0 && k < K) ? __fdiv_rn(-sample_shift(partials, clim_mean, b, k, K, nchunks, HW), extra_std[j - nin])
                                          : __int_as_float(0x7fc00000);
        if (quads) {
            const float4 v4 = make_float4(v, v, v, v);
            for (long t = t0; t < (HW >> 2); t += dt) reinterpret_cast<float4*>(d)[t] = v4;
        } else {
            for (long t = t0; t < HW; t += dt) d[t] = v;
        }
        return;
    }
    const float* s = srcs[j] + (long)b * strides[j];
    const float mu = mean[j], sd = stdv[j];
    const int k = shift_idx[j];
    const bool vec = quads && aligned16(s);
    if (k >= 0 && k < K) {
        const float sh = sample_shift(partials, clim_mean, b, k, K, nchunks, HW);
        if (vec) {
            const float4* s4 = reinterpret_cast<const float4*>(s);
            for (long t = t0; t < (HW >> 2); t += dt) {
                const float4 v = s4[t];
                reinterpret_cast<float4*>(d)[t] = make_float4(shift_norm(v.x, sh, mu, sd), shift_norm(v.y, sh, mu, sd),
                                                              shift_norm(v.z, sh, mu, sd), shift_norm(v.w, sh, mu, sd));
            }
        } else {
            for (long t = t0; t < HW; t += dt) d[t] = shift_norm(s[t], sh, mu, sd);
        }
        return;
    }
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(s);
        for (long t = t0; t < (HW >> 2); t += dt) {
            const float4 v = s4[t];
            reinterpret_cast<float4*>(d)[t] = make_float4(norm(v.x, mu, sd), norm(v.y, mu, sd), norm(v.z, mu, sd), norm(v.w, mu, sd));
        }
    } else {
        for (long t = t0; t < HW; t += dt) d[t] = norm(s[t], mu, sd);
    }
}

// normalizer.py:236 as torch evaluates it (the product rounded before the sum, kernels.hip's denormalize), then
// global_mean_removal.py:265 / :347: one fp32 subtraction
__device__ __forceinline__ float denorm(float y, float sd, float mu) {
#pragma clang fp contract(off)
    const float p = y * sd;
    return p + mu;
}
__device__ __forceinline__ float denorm_unshift(float y, float sd, float mu, float sh) {
#pragma clang fp contract(off)
    const float p = y * sd;
    const float q = p + mu;
    return q - sh;
}

__global__ __launch_bounds__(NT) void gmr_unpack_denormalize_kernel(const float* __restrict__ src, const float* __restrict__ mean,
                                                                    const float* __restrict__ stdv, float* const* __restrict__ dsts,
                                                                    const long* __restrict__ strides,
                                                                    const int* __restrict__ shift_idx,
                                                                    const float* __restrict__ shift, int nch, int K, long HW) {
    const int j = blockIdx.y, b = blockIdx.z;
    const float* s = src + ((long)b * nch + j) * HW;
    float* d = dsts[j] + (long)b * strides[j];
    const float mu = mean[j], sd = stdv[j];
    const int k = shift_idx[j];
    const long t0 = (long)blockIdx.x * NT + threadIdx.x, dt = (long)gridDim.x * NT;
    const bool vec = (HW & 3) == 0 && aligned16(s) && aligned16(d);
    if (k >= 0 && k < K) {
        const float sh = shift[(long)b * K + k];
        if (vec) {
            const float4* s4 = reinterpret_cast<const float4*>(s);
            for (long t = t0; t < (HW >> 2); t += dt) {
                const float4 v = s4[t];
                reinterpret_cast<float4*>(d)[t] = make_float4(denorm_unshift(v.x, sd, mu, sh), denorm_unshift(v.y, sd, mu, sh),
                                                              denorm_unshift(v.z, sd, mu, sh), denorm_unshift(v.w, sd, mu, sh));
            }
        } else {
            for (long t = t0; t < HW; t += dt) d[t] = denorm_unshift(s[t], sd, mu, sh);
        }
        return;
    }
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(s);
        for (long t = t0; t < (HW >> 2); t += dt) {
            const float4 v = s4[t];
            reinterpret_cast<float4*>(d)[t] = make_float4(denorm(v.x, sd, mu), denorm(v.y, sd, mu), denorm(v.z, sd, mu), denorm(v.w, sd, mu));
        }
    } else {
        for (long t = t0; t < HW; t += dt) d[t] = denorm(s[t], sd, mu);
    }
}

// the grid of launch_pack_normalize: up to 64 workgroups of 256 threads per (channel, sample), grid-stride beyond
dim3 glue_grid(long HW, int nch, int Bt) {
    unsigned gx = (unsigned)((HW + 1023) / 1024);
    if (gx > 64) gx = 64;
    if (gx < 1) gx = 1;
    return dim3(gx, nch, Bt);
}

}  // namespace

long gmr_chunks(long HW) { return HW < 1 ? 0 : (HW + GMR_CHUNK - 1) / GMR_CHUNK; }

hipError_t launch_gmr_partials(const float* const* srcs, const long* strides, const int* plane_idx, int nsrc, double* partials,
                               int Bt, int K, long HW, hipStream_t s) {
    const long nchunks = gmr_chunks(HW);
    hipLaunchKernelGGL(gmr_partials_kernel, dim3((unsigned)nchunks, K, Bt), dim3(NT), 0, s, srcs, strides, plane_idx, nsrc,
                       partials, K, HW, nchunks);
    return hipGetLastError();
}

hipError_t launch_gmr_sample_means(const double* partials, float* means, int Bt, int K, long HW, hipStream_t s) {
    const long n = (long)Bt * K;
    hipLaunchKernelGGL(gmr_sample_means_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, s, partials, means, Bt, K,
                       gmr_chunks(HW), HW);
    return hipGetLastError();
}

hipError_t launch_gmr_pack_normalize(const float* const* srcs, const long* strides, const float* mean, const float* stdv,
                                     const int* shift_idx, const double* partials, const float* clim_mean,
                                     const int* extra_idx, const float* extra_std, float* dst, float* shift, int Bt, int nin,
                                     int nextra, int K, long HW, hipStream_t s) {
    hipLaunchKernelGGL(gmr_pack_normalize_kernel, glue_grid(HW, nin + nextra, Bt), dim3(NT), 0, s, srcs, strides, mean, stdv,
                       shift_idx, partials, clim_mean, extra_idx, extra_std, dst, shift, nin, nextra, K, HW, gmr_chunks(HW));
    return hipGetLastError();
}

hipError_t launch_gmr_unpack_denormalize(const float* src, const float* mean, const float* stdv, float* const* dsts,
                                         const long* strides, const int* shift_idx, const float* shift, int Bt, int nch, int K,
                                         long HW, hipStream_t s) {
    hipLaunchKernelGGL(gmr_unpack_denormalize_kernel, glue_grid(HW, nch, Bt), dim3(NT), 0, s, src, mean, stdv, dsts, strides,
                       shift_idx, shift, nch, K, HW);
    return hipGetLastError();
}

}  // namespace ace
