// Lat-lon UNet glue (the Samudra ocean emulator, fme/ace/models/ocean/m2lines/): the memory-bound operators around the packed
// compensated-fp16 convolution engine of healpix.hip, on an equiangular latitude x longitude grid.
//   * halo padding: circular (or zero) in longitude, zero in latitude, written straight into the engine's P-format operand planes
//     [img][cpad / 8][(H + 2p) x pitch_p cells][8], optionally through a per-(image, channel) affine (instance norm / batch norm in
//     eval) and CappedGELU - so neither the normalised nor the activated tensor ever exists in fp32;
//   * instance-norm statistics of pitched planes: two passes over each plane, fp64 accumulation of (x - mean)^2 (no E[x^2] - mean^2);
//   * 2 x 2 average pooling with floor at odd sizes;
//   * bilinear x 2 upsampling (align_corners false; plain, or periodic in longitude) fused with the reference's pad-to-skip-shape
//     and the skip addition.
// Every fp32 tensor carries a 64-word bound slot (bits of a bound on max|x|, zeroed by the caller) and keeps its gap columns
// [W, pitch) defined (zeros written here; finite values from convolutions).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/ace_sfno.h"
#include "errors.h"
#include "kernels.h"
#include "strip_common.h"

using namespace ace;

#define ACE_LL_SLACK 16   // zero entries behind a padded operand (the last taps of the last row read past the end)

namespace {

// one atomicMax per workgroup (256 threads) into the 64-shard bound slot
__device__ __forceinline__ void ll_block_amax(float vmax, unsigned* __restrict__ amax) {
    __shared__ float wmax[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = vmax;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(amax + (blockIdx.x & 63), __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
}

// GELU's minimum is -0.16997 (at x = -0.7518): a bound on |CappedGELU| whatever its input
#define LL_GELU_MIN_BOUND 0.17f

// bound of act(scale x + shift) from the bound b of scale x + shift: |gelu(v)| <= |v| and gelu(v) >= -0.17, then min(., cap)
__device__ __forceinline__ float ll_act_bound(float b, int act, float cap) {
    if (act != ACT_GELU) return b;
    return cap >= 0.f ? fmaxf(fminf(cap, b), LL_GELU_MIN_BOUND) : fmaxf(-cap, LL_GELU_MIN_BOUND);
}

// y (P-format, entries of 8 channels) = pad( act( ss ? scale x + shift : x ) ); see ace_ll_pad_planes
__global__ __launch_bounds__(256) void ll_pad_planes_kernel(const float* __restrict__ x, long x_img_stride, long x_chan_stride, int x_pitch,
                                                            int c, int H, int W, int p, int circular, _Float16* __restrict__ hi,
                                                            _Float16* __restrict__ lo, int pitch_p, int imgs, const float* __restrict__ ss,
                                                            long ss_img_stride, int act, float cap, const unsigned* __restrict__ xmax,
                                                            float bscale, float boff, unsigned* __restrict__ pmax, int slack) {
    const int lane = threadIdx.x & 63;
    const float bound = ll_act_bound(bscale * wave_max_bits(slot_load(xmax + lane)) + boff, act, cap);
    const float scale = ldexpf(1.0f, pow2_exponent_for(bound));
    if (blockIdx.x == 0 && threadIdx.x < 64) pmax[threadIdx.x] = __float_as_uint(bound);
    const int cg8 = (c + 7) / 8, rows = H + 2 * p, wp = W + 2 * p;
    const long cells = (long)rows * pitch_p;
    const long total = (long)imgs * cg8 * cells;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int cellp = (int)(t % cells);
        const int r = cellp / pitch_p, col = cellp % pitch_p;
        const long q = t / cells;
        const int cg = (int)(q % cg8), img = (int)(q / cg8);
        half8 hh, ll;
#pragma unroll
        for (int e = 0; e < 8; ++e) { hh[e] = (_Float16)0.f; ll[e] = (_Float16)0.f; }
        const int sr = r - p;
        int sc = col - p;
        bool inside = col < wp && sr >= 0 && sr < H;
        if (inside) {
            if (sc < 0 || sc >= W) {
                if (circular) sc = sc < 0 ? sc + W : sc - W;   // p <= W: one wrap at most
                else inside = false;
            }
        }
        if (inside) {
            const float* src = x + (long)img * x_img_stride + (long)sr * x_pitch + sc;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int ch = 8 * cg + e;
                if (ch >= c) break;
                float v = src[(long)ch * x_chan_stride];
                if (ss) {
                    const float* sp = ss + 2 * ((long)img * ss_img_stride + ch);
                    v = fmaf(sp[0], v, sp[1]);
                }
                if (act == ACT_GELU) v = fminf(0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)), cap);
                v = __builtin_amdgcn_fmed3f(v * scale, -65504.f, 65504.f);
                const _Float16 h = (_Float16)v;
                hh[e] = h;
                ll[e] = (_Float16)(v - (float)h);
            }
        }
        const long eo = (((long)img * cg8 + cg) * cells + cellp) * 8;
        *reinterpret_cast<half8*>(hi + eo) = hh;
        *reinterpret_cast<half8*>(lo + eo) = ll;
    }
    if (slack > 0 && blockIdx.x == gridDim.x - 1 && (int)threadIdx.x < slack) {
        half8 z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (_Float16)0.f;
        const long eo = ((long)imgs * cg8 * cells + threadIdx.x) * 8;
        *reinterpret_cast<half8*>(hi + eo) = z;
        *reinterpret_cast<half8*>(lo + eo) = z;
    }
}

// block-wide sum of a double (256 threads); every thread gets the result
__device__ __forceinline__ double ll_block_sum(double v, double* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// one workgroup per (image, channel) plane: mean, then the biased variance as the mean of (x - mean)^2, both in fp64
__global__ __launch_bounds__(256) void ll_norm_stats_kernel(const float* __restrict__ x, long img_stride, long chan_stride, int pitch, int c,
                                                            int H, int W, float eps, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ ss,
                                                            float* __restrict__ mv, unsigned* __restrict__ amax) {
    __shared__ double sh[4];
    __shared__ float shf[8];
    const long plane = blockIdx.x;
    const int ch = (int)(plane % c);
    const float* base = x + (plane / c) * img_stride + (long)ch * chan_stride;
    const int n = H * W;
    double s = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = base[(long)(i / W) * pitch + i % W];
        s += (double)v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    const double mean = ll_block_sum(s, sh) / (double)n;
    double s2 = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double d = (double)base[(long)(i / W) * pitch + i % W] - mean;
        s2 = fma(d, d, s2);
    }
    const double var = ll_block_sum(s2, sh) / (double)n;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off, 64));
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { shf[threadIdx.x >> 6] = mn; shf[4 + (threadIdx.x >> 6)] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = fminf(fminf(shf[0], shf[1]), fminf(shf[2], shf[3]));
        mx = fmaxf(fmaxf(shf[4], shf[5]), fmaxf(shf[6], shf[7]));
        const double g = gamma ? (double)gamma[ch] : 1.0, b = beta ? (double)beta[ch] : 0.0;
        const double sc = g / sqrt(var + (double)eps);
        const double sf = b - mean * sc;
        ss[2 * plane] = (float)sc;
        ss[2 * plane + 1] = (float)sf;
        if (mv) { mv[2 * plane] = (float)mean; mv[2 * plane + 1] = (float)var; }
        // the affine is applied in fp32 (one fma): a relative margin covers its rounding
        const double bd = fmax(fabs(sc * (double)mn + sf), fabs(sc * (double)mx + sf));
        atomicMax(amax + (plane & 63), __float_as_uint((float)(bd * (1.0 + 1e-5) + 1e-30)));
    }
}

// nn.AvgPool2d(2) (floor): x [planes][H][px] -> y [planes][H / 2][py], gap columns of y zeroed; amax: bound of y
__global__ __launch_bounds__(256) void ll_pool2_kernel(const float* __restrict__ x, float* __restrict__ y, long planes, int H, int W, int px,
                                                       long sx, int py, long sy, unsigned* __restrict__ amax) {
    const int Ho = H / 2, Wo = W / 2;
    const long total = planes * Ho * py;
    float vmax = 0.f;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int xo = (int)(t % py), yo = (int)((t / py) % Ho);
        const long pl = t / ((long)py * Ho);
        float v = 0.f;
        if (xo < Wo) {
            const float* s = x + pl * sx + (long)(2 * yo) * px + 2 * xo;
            v = (((s[0] + s[1]) + s[px]) + s[px + 1]) * 0.25f;
        }
        y[pl * sy + (long)yo * py + xo] = v;
        vmax = fmaxf(vmax, fabsf(v));
    }
    ll_block_amax(vmax, amax);
}

// torch's bilinear source index at scale 2 (align_corners false): max(0.5 (o + 0.5) - 0.5, 0), the upper neighbour clamped
__device__ __forceinline__ void ll_src(int o, int n, int& i0, int& i1, float& l1) {
    const float f = fmaxf(0.5f * ((float)o + 0.5f) - 0.5f, 0.f);
    i0 = (int)f;
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l1 = f - (float)i0;
}

// y = pad_to_skip( upsample2(x) ) + skip; see ace_ll_upsample2_add
__global__ __launch_bounds__(256) void ll_upsample2_add_kernel(const float* __restrict__ x, long planes, int h, int w, int px, long sx,
                                                               const float* __restrict__ skip, int ps, long sk, float* __restrict__ y, int H,
                                                               int W, int py, long sy, int pad_top, int pad_left, int circular, int periodic,
                                                               unsigned* __restrict__ amax) {
    const long total = planes * H * py;
    const int h2 = 2 * h, w2 = 2 * w;
    float vmax = 0.f;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int X = (int)(t % py), Y = (int)((t / py) % H);
        const long pl = t / ((long)py * H);
        float v = 0.f;
        if (X < W) {
            const int yy = Y - pad_top;
            int xx = X - pad_left;
            bool in = yy >= 0 && yy < h2;
            if (in && (xx < 0 || xx >= w2)) {
                if (circular) xx = xx < 0 ? xx + w2 : xx - w2;
                else in = false;
            }
            float u = 0.f;
            if (in) {
                int y0, y1, x0, x1;
                float ly1, lx1;
                ll_src(yy, h, y0, y1, ly1);
                if (periodic) {
                    // the reference pads one column circularly, interpolates the (w + 2)-wide plane, drops 2 columns each side
                    ll_src(xx + 2, w + 2, x0, x1, lx1);
                    x0 = x0 == 0 ? w - 1 : (x0 == w + 1 ? 0 : x0 - 1);
                    x1 = x1 == 0 ? w - 1 : (x1 == w + 1 ? 0 : x1 - 1);
                } else {
                    ll_src(xx, w, x0, x1, lx1);
                }
                const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
                const float* s = x + pl * sx;
                u = ly0 * (lx0 * s[(long)y0 * px + x0] + lx1 * s[(long)y0 * px + x1]) +
                    ly1 * (lx0 * s[(long)y1 * px + x0] + lx1 * s[(long)y1 * px + x1]);
            }
            v = u + skip[pl * sk + (long)Y * ps + X];
        }
        y[pl * sy + (long)Y * py + X] = v;
        vmax = fmaxf(vmax, fabsf(v));
    }
    ll_block_amax(vmax, amax);
}

unsigned ll_grid(long total) {
    long g = (total + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

}  // namespace

extern "C" int ace_ll_pad_planes(const float* x, long x_img_stride, long x_chan_stride, int x_pitch, int c, int H, int W, int p, int circular,
                                 void* hi, void* lo, int pitch_p, int imgs, const float* ss, long ss_img_stride, int act, float cap,
                                 const unsigned* xmax, float bscale, float boff, unsigned* pmax, void* stream) {
    if (!x || !hi || !lo || !xmax || !pmax || imgs < 1 || c < 1 || H < 1 || W < 1 || p < 0 || x_pitch < W || pitch_p < W + 2 * p ||
        (pitch_p & 3) || (circular && p > W) || !(bscale >= 0.f) || !(boff >= 0.f) || x_chan_stride < (long)H * x_pitch ||
        x_img_stride < (long)c * x_chan_stride)
        return fail(ACE_ERR_INVALID, "ace_ll_pad_planes: bad argument (pitch_p >= W + 2p, pitch_p % 4 == 0, a circular halo p <= W)");
    if (!(act == ACT_NONE || act == ACT_GELU) || std::isnan(cap))
        return fail(ACE_ERR_INVALID, "ace_ll_pad_planes: activation must be none or (capped) gelu");
    const long total = (long)imgs * ((c + 7) / 8) * (H + 2 * p) * pitch_p;
    hipLaunchKernelGGL(ll_pad_planes_kernel, dim3(ll_grid(total)), dim3(256), 0, static_cast<hipStream_t>(stream), x, x_img_stride,
                       x_chan_stride, x_pitch, c, H, W, p, circular, static_cast<_Float16*>(hi), static_cast<_Float16*>(lo), pitch_p, imgs,
                       ss, ss_img_stride, act, cap, xmax, bscale, boff, pmax, ACE_LL_SLACK);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_ll_norm_stats(const float* x, long img_stride, long chan_stride, int pitch, int imgs, int c, int H, int W, float eps,
                                 const float* gamma, const float* beta, float* ss, float* mean_var, unsigned* amax, void* stream) {
    if (!x || !ss || !amax || imgs < 1 || c < 1 || H < 1 || W < 1 || pitch < W || chan_stride < (long)H * pitch ||
        img_stride < (long)c * chan_stride || !(eps >= 0.f) || (long)H * W > (1L << 30))
        return fail(ACE_ERR_INVALID, "ace_ll_norm_stats: bad argument");
    hipLaunchKernelGGL(ll_norm_stats_kernel, dim3((unsigned)((long)imgs * c)), dim3(256), 0, static_cast<hipStream_t>(stream), x, img_stride,
                       chan_stride, pitch, c, H, W, eps, gamma, beta, ss, mean_var, amax);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_ll_pool2(const float* x, float* y, long planes, int H, int W, int pitch_in, long plane_stride_in, int pitch_out,
                            long plane_stride_out, unsigned* amax, void* stream) {
    if (!x || !y || !amax || planes < 1 || H < 2 || W < 2 || pitch_in < W || pitch_out < W / 2 || plane_stride_in < (long)H * pitch_in ||
        plane_stride_out < (long)(H / 2) * pitch_out)
        return fail(ACE_ERR_INVALID, "ace_ll_pool2: bad argument (H, W >= 2)");
    const long total = planes * (H / 2) * pitch_out;
    hipLaunchKernelGGL(ll_pool2_kernel, dim3(ll_grid(total)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, planes, H, W, pitch_in,
                       plane_stride_in, pitch_out, plane_stride_out, amax);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_ll_upsample2_add(const float* x, long planes, int h, int w, int pitch_x, long plane_stride_x, const float* skip,
                                    int pitch_skip, long plane_stride_skip, float* y, int H, int W, int pitch_y, long plane_stride_y,
                                    int circular, int periodic, unsigned* amax, void* stream) {
    if (!x || !skip || !y || !amax || planes < 1 || h < 1 || w < 1 || H < 2 * h || W < 2 * w || pitch_x < w || pitch_skip < W ||
        pitch_y < W || plane_stride_x < (long)h * pitch_x || plane_stride_skip < (long)H * pitch_skip || plane_stride_y < (long)H * pitch_y ||
        (circular && W - 2 * w > 2 * w))
        return fail(ACE_ERR_INVALID, "ace_ll_upsample2_add: bad argument (skip at least 2h x 2w, a circular pad at most one wrap)");
    const int pad_top = (H - 2 * h) / 2, pad_left = (W - 2 * w) / 2;
    const long total = planes * H * pitch_y;
    hipLaunchKernelGGL(ll_upsample2_add_kernel, dim3(ll_grid(total)), dim3(256), 0, static_cast<hipStream_t>(stream), x, planes, h, w, pitch_x,
                       plane_stride_x, skip, pitch_skip, plane_stride_skip, y, H, W, pitch_y, plane_stride_y, pad_top, pad_left, circular,
                       periodic, amax);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}
