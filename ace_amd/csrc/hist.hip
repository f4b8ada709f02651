// The inference evaluator's histogram metric (fme/ace/aggregator/inference/histogram.py on fme/core/histogram.py:74-225): a
// dynamic histogram of every paired variable for prediction and target, kept on the device.  The reference reads each variable's
// minimum and maximum back to the host, doubles its numpy bin range until the window fits and calls torch.bincount per variable;
// here one call covers both sides and all names of a window in three stream-ordered launches, and nothing is read back.
//   hist_range    workgroup (chunk, plane j, side) owns 1024 pixels (4 per thread) of plane j and walks every (sample, step):
//                 minimum, maximum and a "non-finite seen" flag over its unmasked pixels, a wave butterfly then one partial per
//                 workgroup.  min and max are exact and order-independent.
//   hist_update   one wave per (plane j, side): combines the partials, decides whether the window is recorded, grows the
//                 device-resident fp64 range by the reference's doublings (pairs of bins merged into the far half) and leaves
//                 (float)lo, (float)bin and a skip flag for the binning pass.
//   hist_bin      the same partition as hist_range.  Each wave owns a sub-histogram of 32-bit counters in LDS.  Before a value
//                 touches LDS the wave peels, twice, the bin of its first pending lane: every lane holding that bin is counted
//                 with one ballot and added once.  A zero-inflated plane (precipitation: most of a wave in one bin) therefore
//                 costs one or two LDS adds per 64 values in place of a 64-way same-address conflict; what is left after the two
//                 rounds goes through LDS atomics, which spread-out bins serve without conflict.  The sub-histograms are summed
//                 and added to the int64 counts with one 64-bit atomic per non-empty bin and workgroup.
// Integer adds commute, so the counts are bitwise repeatable whatever order the workgroups run in.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "diag_common.h"

namespace {

constexpr int MAX_BINS = 1024;
constexpr int MAX_PLANES_PER_CALL = 1 << 21;    // batch * steps: 1024 pixels of each fit a 32-bit LDS counter
constexpr int PEEL = 2;              // rounds of wave-level combining before the LDS atomics

struct Partial { float mn, mx; int bad, pad; };       // one per (side, plane, chunk)
struct BinParam { float lo, bin; int skip, pad; };    // one per (side, plane), after the partials

// which of this thread's four pixels are inside the plane and not masked out
__device__ __forceinline__ void live_pixels(const unsigned char* mask, long p, long HW, bool live[PIX]) {
#pragma unroll
    for (int k = 0; k < PIX; ++k) live[k] = p + k < HW && (mask == nullptr || mask[p + k] == 0);
}

struct HistArgs {
    const float* const* src[2];
    const long* strides[2];
    const int* rows;
    const unsigned char* const* masks;
    Partial* partial;
    BinParam* param;
    double* range;
    long long* counts;
    int* dropped;
    int nrows, n_bins, nplanes, B, T;
    long HW;
    int nchunk;
};

__global__ __launch_bounds__(NT) void hist_range_kernel(HistArgs a) {
    const int chunk = blockIdx.x, j = blockIdx.y, side = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* base = a.src[side][j];
    const int r = a.rows[j];
    if (base == nullptr || r < 0 || r >= a.nrows) return;
    const long HW = a.HW, p = (long)chunk * CHUNK + (long)threadIdx.x * PIX;
    const long sb = a.strides[side][2 * j], st = a.strides[side][2 * j + 1];
    const bool vec = DIAG_VEC4_OK(base, HW, sb, st);
    bool live[PIX];
    live_pixels(a.masks ? a.masks[j] : nullptr, p, HW, live);
    float mn = INFINITY, mx = -INFINITY;
    int bad = 0;
    const int n = a.B * a.T;
    float4 nx = load4(base, p, HW, vec);
    for (int i = 0; i < n; ++i) {
        const float4 x4 = nx;
        if (i + 1 < n) {
            const int b1 = (i + 1) / a.T, t1 = (i + 1) - b1 * a.T;
            nx = load4(base + (long)b1 * sb + (long)t1 * st, p, HW, vec);
        }
        const float xv[PIX] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
        for (int k = 0; k < PIX; ++k)
            if (live[k]) {
                if (!isfinite(xv[k])) bad = 1;
                else { mn = fminf(mn, xv[k]); mx = fmaxf(mx, xv[k]); }
            }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        bad |= __shfl_xor(bad, o, 64);
    }
    __shared__ float s_mn[WAVES], s_mx[WAVES];
    __shared__ int s_bad[WAVES];
    if (lane == 0) { s_mn[wave] = mn; s_mx[wave] = mx; s_bad[wave] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < WAVES; ++w) { mn = fminf(mn, s_mn[w]); mx = fmaxf(mx, s_mx[w]); bad |= s_bad[w]; }
        Partial* q = a.partial + ((long)side * a.nplanes + j) * a.nchunk + chunk;
        q->mn = mn;
        q->mx = mx;
        q->bad = bad;
    }
}

// one wave per (plane, side)
__global__ __launch_bounds__(64) void hist_update_kernel(HistArgs a) {
#pragma clang fp contract(off)
    const int j = blockIdx.x, side = blockIdx.y, lane = threadIdx.x;
    BinParam* out = a.param + (long)side * a.nplanes + j;
    const int r = a.rows[j];
    if (a.src[side][j] == nullptr || r < 0 || r >= a.nrows) {
        if (lane == 0) out->skip = 1;
        return;
    }
    const Partial* q = a.partial + ((long)side * a.nplanes + j) * a.nchunk;
    float mn = INFINITY, mx = -INFINITY;
    int bad = 0;
    for (int c = lane; c < a.nchunk; c += 64) { mn = fminf(mn, q[c].mn); mx = fmaxf(mx, q[c].mx); bad |= q[c].bad; }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        bad |= __shfl_xor(bad, o, 64);
    }
    // every lane holds the same values from here on and takes the same branches
    const int nb = a.n_bins;
    double* rg = a.range + ((long)side * a.nrows + r) * 2;
    long long* cnt = a.counts + ((long)side * a.nrows + r) * nb;
    const double vmin = (double)(mn - 1.0e-6f), vmax = (double)(mx + 1.0e-6f);      // the epsilon in fp32, as torch adds it
    double lo = rg[0], hi = rg[1];
    int nleft = 0, nright = 0;
    bool skip = bad != 0 || !isfinite(vmin) || !isfinite(vmax);      // an empty selection leaves min = +inf
    if (!skip) {
        if (lo != lo) { lo = vmin; hi = vmax; }                     // NaN: no window yet
        else {
            // each doubling doubles hi - lo > 0, so both loops end; the bound only keeps a corrupted state from spinning
            for (; vmin < lo && nleft < 4096; ++nleft) lo = hi - 2.0 * (hi - lo);
            for (; vmax > hi && nright < 4096; ++nright) hi = lo + 2.0 * (hi - lo);
        }
    }
    const double step = (hi - lo) / (double)nb;
    const float flo = (float)lo, fbin = (float)((lo + step) - lo);
    skip = skip || !(fbin > 0.0f) || !isfinite(fbin) || !isfinite(flo);
    if (skip) {
        if (lane == 0) { out->skip = 1; a.dropped[(long)side * a.nrows + r] += 1; }
        return;
    }
    const int half = nb / 2;
    for (int d = 0; d < nleft + nright; ++d) {
        long long c[MAX_BINS / 2 / 64];
#pragma unroll
        for (int k = 0; k < MAX_BINS / 2 / 64; ++k) {
            const int i = lane + 64 * k;
            c[k] = i < half ? cnt[2 * i] + cnt[2 * i + 1] : 0;
        }
        __syncthreads();
        const int off = d < nleft ? half : 0, zero = d < nleft ? 0 : half;
#pragma unroll
        for (int k = 0; k < MAX_BINS / 2 / 64; ++k) {
            const int i = lane + 64 * k;
            if (i < half) { cnt[off + i] = c[k]; cnt[zero + i] = 0; }
        }
        __syncthreads();
    }
    if (lane == 0) {
        rg[0] = lo;
        rg[1] = hi;
        out->lo = flo;
        out->bin = fbin;
        out->skip = 0;
    }
}

__global__ __launch_bounds__(NT) void hist_bin_kernel(HistArgs a) {
#pragma clang fp contract(off)
    extern __shared__ unsigned int s_hist[];           // [WAVES][n_bins]
    const int chunk = blockIdx.x, j = blockIdx.y, side = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const BinParam prm = a.param[(long)side * a.nplanes + j];
    if (prm.skip) return;                               // uniform over the workgroup; covers NULL planes and bad rows
    const int nb = a.n_bins;
    for (int i = threadIdx.x; i < WAVES * nb; i += NT) s_hist[i] = 0u;
    __syncthreads();
    unsigned int* h = s_hist + wave * nb;
    const float* base = a.src[side][j];
    const long HW = a.HW, p = (long)chunk * CHUNK + (long)threadIdx.x * PIX;
    const long sb = a.strides[side][2 * j], st = a.strides[side][2 * j + 1];
    const bool vec = DIAG_VEC4_OK(base, HW, sb, st);
    bool live[PIX];
    live_pixels(a.masks ? a.masks[j] : nullptr, p, HW, live);
    const float flo = prm.lo, fbin = prm.bin, top = (float)nb;
    const int n = a.B * a.T;
    float4 nx = load4(base, p, HW, vec);
    for (int i = 0; i < n; ++i) {
        const float4 x4 = nx;
        if (i + 1 < n) {
            const int b1 = (i + 1) / a.T, t1 = (i + 1) - b1 * a.T;
            nx = load4(base + (long)b1 * sb + (long)t1 * st, p, HW, vec);
        }
        const float xv[PIX] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
        for (int k = 0; k < PIX; ++k) {
            const float q = __fdiv_rn(xv[k] - flo, fbin);             // IEEE division: a reciprocal multiply moves values across edges
            const int bin = !(q < top) ? nb - 1 : (q < 0.0f ? 0 : (int)q);
            bool todo = live[k];
#pragma unroll
            for (int round = 0; round < PEEL; ++round) {
                const unsigned long long pending = __ballot(todo);
                if (pending == 0ull) break;
                const int leader = __ffsll((long long)pending) - 1;
                const int b0 = __shfl(bin, leader, 64);
                const bool same = todo && bin == b0;
                const unsigned long long m = __ballot(same);
                if (lane == leader) atomicAdd(&h[b0], (unsigned int)__popcll(m));
                todo = todo && !same;
            }
            if (todo) atomicAdd(&h[bin], 1u);
        }
    }
    __syncthreads();
    const int r = a.rows[j];
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(a.counts) + ((long)side * a.nrows + r) * nb;
    for (int i = threadIdx.x; i < nb; i += NT) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += s_hist[w * nb + i];
        if (s) atomicAdd(&cnt[i], s);
    }
}

}  // namespace

extern "C" long ace_diag_hist_scratch_bytes(int nplanes, int batch, int steps, long hw) {
    if (nplanes < 0 || nplanes > 65535 || batch < 1 || steps < 1 || (long)batch * steps > MAX_PLANES_PER_CALL || hw < 1 ||
        nchunk_for(hw) > 2147483647L)
        return -1;
    return 2L * nplanes * (nchunk_for(hw) * (long)sizeof(Partial) + (long)sizeof(BinParam));
}

extern "C" int ace_diag_hist_window(const float* const* gen, const long* gen_strides, const float* const* target,
                                    const long* target_strides, const int* rows, const unsigned char* const* masks, void* scratch,
                                    double* range, long long* counts, int* dropped, int nrows, int n_bins, int nplanes, int batch,
                                    int steps, long hw, void* stream) {
    if (nplanes < 0 || nplanes > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_hist_window: need 0 <= nplanes <= 65535");
    if (n_bins < 2 || n_bins > MAX_BINS || (n_bins & 1))
        return ace::fail(ACE_ERR_INVALID, "ace_diag_hist_window: need an even n_bins, 2 <= n_bins <= 1024");
    if (batch < 1 || steps < 1 || (long)batch * steps > MAX_PLANES_PER_CALL)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_hist_window: need batch >= 1, steps >= 1, batch * steps <= 2097152 (32-bit "
                                               "counters per workgroup)");
    if (hw < 1 || nchunk_for(hw) > 2147483647L || nrows < 1)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_hist_window: need 1 <= hw <= 1024 * (2^31 - 1), nrows >= 1");
    if (nplanes == 0) return ACE_OK;
    if (!gen || !gen_strides || !target || !target_strides || !rows || !scratch || !range || !counts || !dropped)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_hist_window: null argument");
    if (reinterpret_cast<uintptr_t>(scratch) & 15u)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_hist_window: scratch must be 16-byte aligned");
    HistArgs a;
    a.src[0] = gen; a.src[1] = target;
    a.strides[0] = gen_strides; a.strides[1] = target_strides;
    a.rows = rows; a.masks = masks;
    a.nchunk = (int)nchunk_for(hw);
    a.partial = static_cast<Partial*>(scratch);
    a.param = reinterpret_cast<BinParam*>(a.partial + 2L * nplanes * a.nchunk);
    a.range = range; a.counts = counts; a.dropped = dropped;
    a.nrows = nrows; a.n_bins = n_bins; a.nplanes = nplanes; a.B = batch; a.T = steps; a.HW = hw;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)a.nchunk, nplanes, 2);
    hipLaunchKernelGGL(hist_range_kernel, grid, dim3(NT), 0, s, a);
    ACE_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hist_update_kernel, dim3(nplanes, 2), dim3(64), 0, s, a);
    ACE_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hist_bin_kernel, grid, dim3(NT), (size_t)WAVES * n_bins * sizeof(unsigned int), s, a);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}
