// The smooth flood fill of masked fields ahead of the power spectrum (fme/core/fill.py: SmoothFloodFill(num_steps=4), wired in
// fme/ace/aggregator/inference/spectrum.py:331), fused with the stacking of a spectrum chunk: one call builds the SHT's whole
// (nnames, B, T, H, W) input, filling the planes of masked names and copying the others, in place of a torch.stack followed, on
// the torch path, by about 30 launches and a dozen full-size temporaries per name.  The arithmetic contract is the
// diag_fill_planes entry of include/ace_sfno.h.
//   fill_mean   one workgroup per plane of a name whose layer table holds an interior (layer 5) pixel: the fp64 mean over the valid
//               pixels, per-thread strided sums, a wave butterfly, then the four waves in order.  Planes of other names return
//               after a scan of their layer table and read no data.
//   fill_tile   workgroup (tile, plane) owns TILE_H x TILE_W output pixels and holds them with a halo of 6 in LDS: 4 pixels of
//               expansion cone plus 2 of blur.  The region is loaded once (masked pixels as 0, interior pixels as the plane mean,
//               rows beyond the poles marked as never known, longitude modular), the four expansion sweeps run in LDS with "outside
//               the region is unknown" - a layer-k pixel k or more pixels inside the region only reads pixels that are right by then,
//               so the outer 4 rings come out wrong and rings 5 and 6, which the blur of the tile reads, right - then the latitude
//               pass of the blur (replicate rows), the longitude pass and the blend, and one coalesced store.  Sweep k reads only
//               pixels of layer < k or 5 and writes only pixels of layer k, so one barrier per sweep is enough.  The pixels of
//               each layer are listed while the region is loaded (LDS counters; the lists lie in the latitude pass's buffer), so
//               a sweep runs densely over its own pixels and not, divergent, over the whole region.  A tile whose
//               blurred valid values are all 1 has no masked pixel within the blur's reach: it stores its source pixels and
//               skips sweeps and blur (open ocean, most tiles of an ocean field).
//               A plane whose tab entry names no table is copied, every workgroup a contiguous share of it.
// Each output pixel is written by one thread from a fixed sequence of operations: no atomics, bitwise repeatable.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "diag_common.h"

namespace {

constexpr int STEPS = ACE_DIAG_FILL_STEPS;
constexpr int BLUR = 2;                              // half width of the 5-tap Gaussian
constexpr int HALO = STEPS + BLUR;
constexpr int TH = ACE_DIAG_FILL_TILE_H, TW = ACE_DIAG_FILL_TILE_W;
constexpr int RH = TH + 2 * HALO, RW = TW + 2 * HALO;      // the region a workgroup holds
constexpr int VW = TW + 2 * BLUR;                    // columns of the latitude pass
constexpr unsigned char INTERIOR = STEPS + 1;        // layer of a pixel the expansion does not reach: it takes the plane mean
constexpr unsigned char NOROW = 255;                 // a region row beyond a pole: never known
constexpr int UNROLL = 8;                            // independent loads a thread of fill_mean keeps in flight
constexpr int REGION_PER = (RH * RW + NT - 1) / NT;  // region pixels per thread
constexpr int OUT_PER = TH * TW / NT;                // output pixels per thread
static_assert(TH * TW % NT == 0, "every thread owns the same number of output pixels");
static_assert(ACE_DIAG_FILL_STEPS == 4 && HALO == 6, "the header states the constants of the contract");

struct FillArgs {
    const float* const* srcs;
    const long* strides;
    const int* tab;
    const unsigned char* layers;
    const float* blurred;
    double* mean;
    float* dst;
    double g[BLUR + 1];                               // the normalised taps at distance 0, 1, 2
    int nmasks, T, H, W, tilesx, ntiles;
    long BT, HW;
};

__global__ __launch_bounds__(NT) void fill_mean_kernel(FillArgs a) {
    const long plane = blockIdx.x;
    const int n = (int)(plane / a.BT);
    const long i = plane - (long)n * a.BT;
    const int t = a.tab[n];
    if (t < 0 || t >= a.nmasks) return;
    const unsigned char* lay = a.layers + (long)t * a.HW;
    // both loops keep UNROLL independent loads in flight; a thread still adds its pixels in ascending order
    int any = 0;
    for (long p0 = threadIdx.x; p0 < a.HW; p0 += (long)UNROLL * NT) {
        unsigned char l[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) l[u] = p0 + (long)u * NT < a.HW ? lay[p0 + (long)u * NT] : 0;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) any |= l[u] == INTERIOR;
    }
    if (!__syncthreads_or(any)) return;               // uniform over the workgroup
    const long b = i / a.T, tt = i - b * a.T;
    const float* s = a.srcs[n] + b * a.strides[2 * n] + tt * a.strides[2 * n + 1];
    double sum = 0.0, cnt = 0.0;
    for (long p0 = threadIdx.x; p0 < a.HW; p0 += (long)UNROLL * NT) {
        unsigned char l[UNROLL];
        float x[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const long p = p0 + (long)u * NT;
            l[u] = p < a.HW ? lay[p] : NOROW;
            x[u] = p < a.HW ? s[p] : 0.0f;            // loaded whatever the layer, added only at a valid pixel
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
            if (l[u] == 0) { sum += (double)x[u]; cnt += 1.0; }
    }
    sum = wave_sum(sum);
    cnt = wave_sum(cnt);
    __shared__ double s_sum[WAVES], s_cnt[WAVES];
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = sum; s_cnt[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < WAVES; ++w) { sum += s_sum[w]; cnt += s_cnt[w]; }
        a.mean[plane] = sum / cnt;                    // no valid pixel: 0 / 0, the plane comes out NaN
    }
}

__global__ __launch_bounds__(NT) void fill_tile_kernel(FillArgs a) {
#pragma clang fp contract(off)
    __shared__ float s_x[RH * RW];
    __shared__ float s_v[TH * VW];
    __shared__ unsigned char s_l[RH * RW];
    __shared__ int s_cnt[STEPS + 1];
    // the pixels of each layer 1..4, listed so that a sweep runs densely over its own; in s_v, which the sweeps do not use
    unsigned short* s_list = reinterpret_cast<unsigned short*>(s_v);
    static_assert(RH * RW <= 65535 && RH * RW * sizeof(unsigned short) <= TH * VW * sizeof(float), "the lists fit in s_v");
    const long plane = blockIdx.x / a.ntiles;
    const int tile = (int)(blockIdx.x - plane * a.ntiles);
    const int n = (int)(plane / a.BT);
    const long i = plane - (long)n * a.BT;
    const long b = i / a.T, tt = i - b * a.T;
    const float* s = a.srcs[n] + b * a.strides[2 * n] + tt * a.strides[2 * n + 1];
    float* d = a.dst + plane * a.HW;
    const int t = a.tab[n];
    const int H = a.H, W = a.W;
    if (t < 0 || t >= a.nmasks) {
        const long per = (a.HW + a.ntiles - 1) / a.ntiles, p0 = (long)tile * per;
        const long p1 = p0 + per < a.HW ? p0 + per : a.HW;
        for (long p = p0 + threadIdx.x; p < p1; p += NT) d[p] = s[p];
        return;
    }
    const unsigned char* lay = a.layers + (long)t * a.HW;
    const float* bvp = a.blurred + (long)t * a.HW;
    const int r0 = (tile / a.tilesx) * TH, c0 = (tile % a.tilesx) * TW;
    int cb = (c0 - HALO) % W;                         // the region's first column
    if (cb < 0) cb += W;
    // Every load of the tile is issued before the first is used: the blurred valid values of this thread's output pixels, then
    // layer and source of its region pixels.  The source is loaded whatever the layer and kept only at a valid pixel.
    float bv[OUT_PER];
    int blend = 0;
#pragma unroll
    for (int q = 0; q < OUT_PER; ++q) {
        const int idx = threadIdx.x + q * NT, ti = idx / TW, j = idx - ti * TW;
        const int r = r0 + ti, c = c0 + j;
        bv[q] = r < H && c < W ? bvp[(long)r * W + c] : 1.0f;
        blend |= bv[q] != 1.0f;
    }
    const float mean = (float)a.mean[plane];          // written when the table has an interior pixel, used only at one
    if (threadIdx.x <= STEPS) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    int rank[REGION_PER], layer[REGION_PER];
#pragma unroll
    for (int q = 0; q < REGION_PER; ++q) rank[q] = -1;
#pragma unroll
    for (int q = 0; q < REGION_PER; ++q) {
        const int idx = threadIdx.x + q * NT;
        if (idx >= RH * RW) break;
        const int ri = idx / RW, ci = idx - ri * RW;
        const int r = r0 - HALO + ri;
        int c = cb + ci;
        if (c >= W) c -= W;
        if (c >= W) c %= W;                           // a region more than twice as wide as the grid
        const bool row = r >= 0 && r < H;
        const long p = row ? (long)r * W + c : 0;
        unsigned char l = lay[p];
        const float v = s[p];
        if (!row || l > INTERIOR) l = NOROW;          // beyond a pole, or not a layer: never known, never updated
        s_l[idx] = l;
        s_x[idx] = l == 0 ? v : (l == INTERIOR ? mean : 0.0f);
        // A layer-k pixel fewer than k pixels inside the region would come out wrong, and no pixel that comes out right reads
        // it (its readers are of a higher layer and at most one pixel further in): it is not listed and keeps 0.
        int in = ri < RH - 1 - ri ? ri : RH - 1 - ri;
        in = ci < in ? ci : in;
        in = RW - 1 - ci < in ? RW - 1 - ci : in;
        layer[q] = l;
        rank[q] = l >= 1 && l <= STEPS && l <= in ? atomicAdd(&s_cnt[l], 1) : -1;
    }
    if (!__syncthreads_or(blend)) {
        // bv == 1 on the whole tile: every pixel within the blur's reach is valid and out = x, the source
#pragma unroll
        for (int q = 0; q < OUT_PER; ++q) {
            const int idx = threadIdx.x + q * NT, ti = idx / TW, j = idx - ti * TW;
            const int r = r0 + ti, c = c0 + j;
            if (r < H && c < W) d[(long)r * W + c] = s_x[(ti + HALO) * RW + (j + HALO)];
        }
        return;
    }
    int first[STEPS + 2];                             // where the list of layer k starts
    first[1] = 0;
#pragma unroll
    for (int k = 1; k <= STEPS; ++k) first[k + 1] = first[k] + s_cnt[k];
#pragma unroll
    for (int q = 0; q < REGION_PER; ++q)
        if (rank[q] >= 0) s_list[first[layer[q]] + rank[q]] = (unsigned short)(threadIdx.x + q * NT);
    __syncthreads();
    // The order of a list depends on the order of the atomics; the value of a pixel does not.
#pragma unroll
    for (int k = 1; k <= STEPS; ++k) {
        for (int e = first[k] + threadIdx.x; e < first[k + 1]; e += NT) {
            const int idx = s_list[e];                // a listed pixel has all nine neighbours inside the region
            double sum = 0.0;
            int cnt = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int nb = idx + dy * RW + dx;
                    const unsigned char l = s_l[nb];
                    if (l < k || l == INTERIOR) { sum += (double)s_x[nb]; ++cnt; }
                }
            if (cnt) s_x[idx] = (float)(sum / (double)cnt);
        }
        __syncthreads();
    }
    for (int idx = threadIdx.x; idx < TH * VW; idx += NT) {
        const int ti = idx / VW, j = idx - ti * VW;
        const int r = r0 + ti;
        double acc = 0.0;
        if (r < H) {
            for (int q = -BLUR; q <= BLUR; ++q) {
                int rq = r + q;
                rq = rq < 0 ? 0 : (rq > H - 1 ? H - 1 : rq);
                acc += a.g[q < 0 ? -q : q] * (double)s_x[(rq - r0 + HALO) * RW + (HALO - BLUR + j)];
            }
        }
        s_v[idx] = (float)acc;
    }
    __syncthreads();
#pragma unroll
    for (int o = 0; o < OUT_PER; ++o) {
        const int idx = threadIdx.x + o * NT, ti = idx / TW, j = idx - ti * TW;
        const int r = r0 + ti, c = c0 + j;
        if (r >= H || c >= W) continue;
        const float x = s_x[(ti + HALO) * RW + (j + HALO)];
        float out = x;
        if (bv[o] != 1.0f) {                          // at 1 the blend is x * 1 + blur * 0
            double acc = 0.0;
            for (int q = -BLUR; q <= BLUR; ++q) acc += a.g[q < 0 ? -q : q] * (double)s_v[ti * VW + (j + BLUR + q)];
            const float bl = (float)acc;
            out = (float)((double)x * (double)bv[o] + (double)bl * (1.0 - (double)bv[o]));
        }
        d[(long)r * W + c] = out;
    }
}

const char* fill_refusal(int nmasks, int nnames, int batch, int steps, int nlat, int nlon) {
    if (nnames < 0 || nmasks < 0) return "need nnames >= 0 and nmasks >= 0";
    if (batch < 1 || steps < 1) return "need batch >= 1 and steps >= 1";
    if (nlat < ACE_DIAG_FILL_MIN_NLAT || nlon < ACE_DIAG_FILL_MIN_NLON) return "need nlat >= 2 and nlon >= 8";
    const long tiles = (long)((nlat + TH - 1) / TH) * ((nlon + TW - 1) / TW);
    const long samples = (long)nnames * batch;        // < 2^62: the product below cannot overflow once this is < 2^31
    if (samples > 2147483647L || samples * steps > 2147483647L / tiles)
        return "need nnames * batch * steps * tiles < 2^31 (one workgroup per tile and plane)";
    return nullptr;
}

}  // namespace

extern "C" long ace_diag_fill_scratch_doubles(int nnames, int batch, int steps, int nlat, int nlon) {
    if (fill_refusal(0, nnames, batch, steps, nlat, nlon)) return -1;
    return (long)nnames * batch * steps;
}

extern "C" int ace_diag_fill_planes(const float* const* srcs, const long* strides, const int* tab, const unsigned char* layers,
                                    const float* blurred, int nmasks, double* scratch, float* dst, int nnames, int batch, int steps,
                                    int nlat, int nlon, void* stream) {
    if (const char* why = fill_refusal(nmasks, nnames, batch, steps, nlat, nlon))
        return ace::fail(ACE_ERR_INVALID, std::string("ace_diag_fill_planes: ") + why);
    if (nnames == 0) return ACE_OK;
    if (!srcs || !strides || !tab || !dst || (nmasks > 0 && (!layers || !blurred || !scratch)))
        return ace::fail(ACE_ERR_INVALID, "ace_diag_fill_planes: null argument");
    if ((reinterpret_cast<uintptr_t>(dst) & 3u) || (reinterpret_cast<uintptr_t>(scratch) & 7u) ||
        (reinterpret_cast<uintptr_t>(blurred) & 3u))
        return ace::fail(ACE_ERR_INVALID, "ace_diag_fill_planes: dst and blurred must be 4-byte, scratch 8-byte aligned");
    FillArgs a;
    a.srcs = srcs; a.strides = strides; a.tab = tab; a.layers = layers; a.blurred = blurred; a.mean = scratch; a.dst = dst;
    const double e1 = std::exp(-0.5), e2 = std::exp(-2.0), norm = 1.0 + 2.0 * e1 + 2.0 * e2;      // sigma 1
    a.g[0] = 1.0 / norm; a.g[1] = e1 / norm; a.g[2] = e2 / norm;
    a.nmasks = nmasks; a.T = steps; a.H = nlat; a.W = nlon;
    a.tilesx = (nlon + TW - 1) / TW;
    a.ntiles = a.tilesx * ((nlat + TH - 1) / TH);
    a.BT = (long)batch * steps;
    a.HW = (long)nlat * nlon;
    const long planes = (long)nnames * a.BT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nmasks > 0) {
        hipLaunchKernelGGL(fill_mean_kernel, dim3((unsigned)planes), dim3(NT), 0, s, a);
        ACE_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(fill_tile_kernel, dim3((unsigned)(planes * a.ntiles)), dim3(NT), 0, s, a);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}
