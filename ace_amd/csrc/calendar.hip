// The evaluator's calendar metrics (fme/ace/aggregator/inference: seasonal.py:40-69, annual.py:181-208, enso/dynamic_index.py:65-92,
// ipo/ipo_index.py:43-58 and 109-131): per-pixel sums of the steps of each calendar bin (the seasons), and per (sample, step) the
// weighted means of a plane over a few regions (the globe, the Nino 3.4 box, the three tripole boxes).  The reference copies every
// field to the host and groups it with xarray for the first, and runs one torch reduction per name and region followed by a .cpu()
// for the second; here one call covers both sides and all names of a window, and every plane is read once for both outputs.
//   calendar_window  workgroup (chunk, plane j, side) owns 1024 pixels (4 per thread) of plane j and walks every sample and every
//                    step >= t_begin in order, the next plane's load in flight.  A thread keeps the fp64 sums of its own four pixels
//                    for up to NB bins in registers (NB = 4 or 8; the bin of a step is uniform over the grid, so the select is a
//                    scalar branch, not a register index, and a step is only ever ADDED to its own bin: nothing is multiplied, a
//                    NaN stays where it is) and the fp32 weights of the same pixels for up to NR regions (the region loop is
//                    unrolled, the set of regions a plane feeds a scalar mask).  Each wave reduces sum w x and sum w of every
//                    (region, b, t) to one partial pair.  At the end a thread adds its sums to the persistent bins - no two threads
//                    share a pixel.
//   calendar_series  one workgroup per (region, plane, side), a wave per (b, t) in turn: the partial pairs summed in a fixed order
//                    (lane strides, then a butterfly), divided and ASSIGNED to the series.
// No float atomics, no host synchronisation, no allocation: two identical runs are bitwise identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "diag_common.h"

namespace {

constexpr int MAX_BINS = ACE_DIAG_CALENDAR_MAX_BINS;        // 8 bins x 4 pixels x fp64 = 64 VGPRs of accumulators: no spill
constexpr int MAX_REG = ACE_DIAG_CALENDAR_MAX_REGIONS;      // 8 regions x 4 pixels x fp32 = 32 VGPRs of weights

struct CalArgs {
    const float* const* src[2];
    const long* strides[2];
    const int* rows;
    const int* bin;
    double* bins;
    const float* regions;
    const int* srow;
    const int* mode;
    const int* wrows;
    const float* weights;
    double* series;
    double* partial;         // [2][nplanes][nreg][B][T][nparts][2]: sum w x, sum w
    int nw, nrows, nbins, nreg, nsrows, n_time, t0, t_begin, nplanes, B, T;
    long HW;
    int nchunk;
};

// the regions plane j feeds, as a bit mask (uniform over the workgroup): a valid weight row and a valid series row
__device__ __forceinline__ unsigned region_mask(const CalArgs& a, int j) {
    const int wr = a.wrows[j];
    if (wr < 0 || wr >= a.nw) return 0u;
    unsigned m = 0u;
    for (int r = 0; r < a.nreg; ++r) {
        const int s = a.srow[(long)j * a.nreg + r];
        if (s >= 0 && s < a.nsrows) m |= 1u << r;
    }
    return m;
}

template <int NB, int NR>
__global__ __launch_bounds__(NT) void calendar_window_kernel(CalArgs a) {
#pragma clang fp contract(off)
    const int chunk = blockIdx.x, j = blockIdx.y, side = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* base = a.src[side][j];
    const int r0 = a.rows[j];
    if (base == nullptr || r0 < 0 || r0 >= a.nrows) return;
    const long HW = a.HW, p = (long)chunk * CHUNK + (long)threadIdx.x * PIX;
    const long sb = a.strides[side][2 * j], st = a.strides[side][2 * j + 1];
    const bool vec = DIAG_VEC4_OK(base, HW, sb, st);
    const int B = a.B, T = a.T, t_begin = a.t_begin, span = T - t_begin, n = B * span;
    const long nparts = (long)a.nchunk * WAVES, part = (long)chunk * WAVES + wave;
    double acc[NB > 0 ? NB : 1][PIX];
#pragma unroll
    for (int m = 0; m < NB; ++m)
#pragma unroll
        for (int k = 0; k < PIX; ++k) acc[m][k] = 0.0;
    float wv[NR > 0 ? NR : 1][PIX];
    unsigned live = 0u, nanaware = 0u;         // uniform over the workgroup
    if (NR > 0) {
        live = region_mask(a, j);
        if (live) {
            const float* wrow = a.weights + (long)a.wrows[j] * HW;
            const float4 a4 = load4(wrow, p, HW, DIAG_VEC4_ROW_OK(wrow, HW));
            const float av[PIX] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
            for (int r = 0; r < NR; ++r) {
#pragma unroll
                for (int e = 0; e < PIX; ++e) wv[r][e] = 0.f;
                if (live >> r & 1u) {
                    const float* rrow = a.regions + (long)r * HW;
                    const float4 g4 = load4(rrow, p, HW, DIAG_VEC4_ROW_OK(rrow, HW));
                    const float gv[PIX] = {g4.x, g4.y, g4.z, g4.w};
                    const bool m1 = a.mode[r] == 1;
                    if (m1) nanaware |= 1u << r;
#pragma unroll
                    for (int e = 0; e < PIX; ++e) wv[r][e] = m1 ? gv[e] : gv[e] * av[e];      // the fp32 product; 0 past the plane
                }
            }
        }
    }
    double* q = a.partial + (((long)side * a.nplanes + j) * a.nreg) * B * T * nparts * 2 + part * 2;
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
            if (NB > 0) {
                const int m = a.bin[(long)b * T + t];
#pragma unroll
                for (int k = 0; k < NB; ++k)
                    if (m == k && k < a.nbins) {
#pragma unroll
                        for (int e = 0; e < PIX; ++e) acc[k][e] += (double)xv[e];
                    }
            }
            if (NR > 0 && live) {
#pragma unroll
                for (int r = 0; r < NR; ++r)
                    if (live >> r & 1u) {
                        const bool skipnan = nanaware >> r & 1u;
                        double N = 0.0, D = 0.0;
#pragma unroll
                        for (int e = 0; e < PIX; ++e) {
                            const float w = wv[r][e];
                            if (w != 0.0f && !(skipnan && xv[e] != xv[e])) {
                                N += (double)w * (double)xv[e];        // exact in fp64: two 24-bit significands
                                D += (double)w;
                            }
                        }
                        N = wave_sum(N);
                        D = wave_sum(D);
                        if (lane == 0) {
                            double* o = q + (((long)r * B + b) * T + t) * nparts * 2;
                            o[0] = N;
                            o[1] = D;
                        }
                    }
            }
        }
    }
    if (NB > 0) {
        double* out = a.bins + (((long)side * a.nrows + r0) * a.nbins) * HW;
#pragma unroll
        for (int m = 0; m < NB; ++m)
            if (m < a.nbins) {
#pragma unroll
                for (int e = 0; e < PIX; ++e)
                    if (p + e < HW) out[(long)m * HW + p + e] += acc[m][e];
            }
    }
}

// workgroup (region r, plane j, side), its four waves taking the (b, t) entries in turn
__global__ __launch_bounds__(NT) void calendar_series_kernel(CalArgs a) {
#pragma clang fp contract(off)
    const int r = blockIdx.x, j = blockIdx.y, side = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = a.rows[j];
    if (a.src[side][j] == nullptr || r0 < 0 || r0 >= a.nrows) return;
    if (!(region_mask(a, j) >> r & 1u)) return;
    const int s = a.srow[(long)j * a.nreg + r];
    const long nparts = (long)a.nchunk * WAVES;
    const int B = a.B, T = a.T, span = T - a.t_begin, n = B * span;
    const double* q = a.partial + ((((long)side * a.nplanes + j) * a.nreg + r) * B) * T * nparts * 2;
    double* out = a.series + (((long)side * a.nsrows + s) * B) * a.n_time + a.t0;
    for (int i = wave; i < n; i += WAVES) {
        const int b = i / span, t = a.t_begin + (i - b * span);
        const double* e = q + ((long)b * T + t) * nparts * 2;
        double N = 0.0, D = 0.0;
        for (long k = lane; k < nparts; k += 64) {
            N += e[2 * k];
            D += e[2 * k + 1];
        }
        N = wave_sum(N);
        D = wave_sum(D);
        if (lane == 0) out[(long)b * a.n_time + t] = N / D;
    }
}

bool shape_ok(int nplanes, int nreg, int batch, int steps, long hw) {
    return nplanes >= 0 && nplanes <= 65535 && nreg >= 0 && nreg <= MAX_REG && batch >= 1 && steps >= 1 &&
           (long)batch * steps <= 2147483647L && hw >= 1 && nchunk_for(hw) <= 2147483647L;
}

template <int NB>
void launch(const CalArgs& a, bool ser, dim3 grid, hipStream_t s) {
    if (ser) hipLaunchKernelGGL((calendar_window_kernel<NB, MAX_REG>), grid, dim3(NT), 0, s, a);
    else hipLaunchKernelGGL((calendar_window_kernel<NB, 0>), grid, dim3(NT), 0, s, a);
}

}  // namespace

extern "C" long ace_diag_calendar_partial_doubles(int nplanes, int nreg, int batch, int steps, long hw) {
    if (!shape_ok(nplanes, nreg, batch, steps, hw)) return -1;
    return 2L * nplanes * nreg * batch * steps * nchunk_for(hw) * WAVES * 2;
}

extern "C" int ace_diag_calendar_window(const float* const* gen, const long* gen_strides, const float* const* target,
                                        const long* target_strides, const int* rows, const int* bin, double* bins,
                                        const float* regions, const int* srow, const int* mode, const int* wrows,
                                        const float* weights, int nw, double* partial, double* series, int nrows, int nbins,
                                        int nreg, int nsrows, int n_time, int t0, int t_begin, int nplanes, int batch, int steps,
                                        long hw, void* stream) {
    if (nplanes < 0 || nplanes > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_calendar_window: need 0 <= nplanes <= 65535");
    if (nbins < 0 || nbins > MAX_BINS)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_calendar_window: need 0 <= nbins <= " + std::to_string(MAX_BINS) +
                                               " (the sums of a pixel stay in registers); split the bins over several calls");
    if (nreg < 0 || nreg > MAX_REG)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_calendar_window: need 0 <= nreg <= " + std::to_string(MAX_REG) +
                                               " (the weights of a pixel stay in registers)");
    if (batch < 1 || steps < 1 || (long)batch * steps > 2147483647L)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_calendar_window: need batch >= 1, steps >= 1, batch * steps < 2^31");
    if (hw < 1 || nchunk_for(hw) > 2147483647L || nrows < 1)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_calendar_window: need 1 <= hw <= 1024 * (2^31 - 1), nrows >= 1");
    if (t_begin < 0) return ace::fail(ACE_ERR_INVALID, "ace_diag_calendar_window: need t_begin >= 0");
    const bool ser = series != nullptr;
    if (ser && (nsrows < 1 || t0 < 0 || (long)t0 + steps > n_time))
        return ace::fail(ACE_ERR_INVALID, "ace_diag_calendar_window: with series need nsrows >= 1, t0 >= 0 and t0 + steps <= "
                                               "n_time");
    if (nplanes == 0) return ACE_OK;
    if (!gen || !gen_strides || !target || !target_strides || !rows)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_calendar_window: null argument");
    if (bins && nbins > 0 && !bin)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_calendar_window: null argument (bin is needed when bins is given)");
    if (ser && (nw < 1 || !wrows || !weights || !partial || (nreg > 0 && (!regions || !srow || !mode))))
        return ace::fail(ACE_ERR_INVALID, "ace_diag_calendar_window: null argument (regions, srow, mode, wrows, weights and "
                                               "partial are needed when series is given)");
    const bool do_bins = bins != nullptr && nbins > 0, do_ser = ser && nreg > 0;
    if ((!do_bins && !do_ser) || t_begin >= steps) return ACE_OK;
    CalArgs a;
    a.src[0] = gen; a.src[1] = target;
    a.strides[0] = gen_strides; a.strides[1] = target_strides;
    a.rows = rows; a.bin = bin; a.bins = bins; a.regions = regions; a.srow = srow; a.mode = mode; a.wrows = wrows;
    a.weights = weights; a.series = series; a.partial = partial;
    a.nw = nw; a.nrows = nrows; a.nbins = do_bins ? nbins : 0; a.nreg = do_ser ? nreg : 0; a.nsrows = nsrows; a.n_time = n_time;
    a.t0 = t0; a.t_begin = t_begin; a.nplanes = nplanes; a.B = batch; a.T = steps; a.HW = hw;
    a.nchunk = (int)nchunk_for(hw);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)a.nchunk, nplanes, 2);
    if (a.nbins == 0) launch<0>(a, do_ser, grid, s);
    else if (a.nbins <= 4) launch<4>(a, do_ser, grid, s);
    else launch<MAX_BINS>(a, do_ser, grid, s);
    ACE_HIP_TRY(hipGetLastError());
    if (do_ser) {
        hipLaunchKernelGGL(calendar_series_kernel, dim3(a.nreg, nplanes, 2), dim3(NT), 0, s, a);
        ACE_HIP_TRY(hipGetLastError());
    }
    return ACE_OK;
}
