// The exchange of the coupled atmosphere-ocean stepper (fme/coupled/stepper.py:986-1148) as two launches per coupled step:
//   ocean_to_atmosphere   the ocean's state as the atmosphere's forcings over the n_inner + 1 time levels of its window
//                         (_get_atmosphere_forcings, _forcings_from_ocean_with_ocean_fraction) and the prescribed initial surface
//                         temperature (_prescribe_ic_sst): every value a selection or a chain of single fp32 operations in the
//                         reference's order, so the output is bitwise the torch path's
//   atmosphere_to_ocean   the time mean of n_inner atmosphere planes per name into the name's slot of a two-level ocean forcing
//                         window, NaN in the other slot (_get_ocean_forcings); the sum runs in t order in fp64 and is rounded to
//                         fp32 once - the one place that differs (by rounding only) from the reference's fp32 mean
// ocean_to_atmosphere_window is the first of these for a rollout on static windows (ace_amd/coupled_rollout.py): the same kernel
// body, every destination a window of the n_inner + 1 levels inside the atmosphere engine's own buffers, a one-level product
// stored to each of them.
// Both are memory bound streaming kernels: a thread owns four consecutive pixels, every source is read once and every
// destination written once.  16-byte accesses on a row (one plane of one sample at one time level) whose hw % 4 == 0 and whose
// address is 16-byte aligned, scalar otherwise, decided per row.  A (job, sample) gets hw / 1024 workgroups of 256 threads in
// atmosphere_to_ocean (one job per name) and hw / 256 single-wave workgroups in ocean_to_atmosphere, whose fraction job is alone
// at B = 1 and has to reach every CU by itself; both are capped at 65536 pixels per (job, sample) and grid-stride beyond.
#include "diag_common.h"

#include <cfloat>

#pragma clang fp contract(off)

namespace {

constexpr long MAX_PIXELS = 65536;      // per (job, sample) and grid-stride trip
constexpr int O2A_NT = 64;

__device__ __forceinline__ float4 ld(const float* row, long p, long HW) { return load4(row, p, HW, DIAG_VEC4_ROW_OK(row, HW)); }

__device__ __forceinline__ void st(float* row, long p, long HW, float4 v) {
    if (DIAG_VEC4_ROW_OK(row, HW) && p + 3 < HW) {
        *reinterpret_cast<float4*>(row + p) = v;
        return;
    }
    if (p < HW) row[p] = v.x;
    if (p + 1 < HW) row[p + 1] = v.y;
    if (p + 2 < HW) row[p + 2] = v.z;
    if (p + 3 < HW) row[p + 3] = v.w;
}

// tensor.where(mask != 0, 0) (stepper.py:1053-1058); no mask: the value itself
__device__ __forceinline__ float keep(float m, float v) { return m != 0.0f ? v : 0.0f; }
__device__ __forceinline__ float4 ldmask(const float* mask, long p, long HW) {
    return mask ? ld(mask, p, HW) : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
}
__device__ __forceinline__ float4 keep4(float4 m, float4 v) {
    return make_float4(keep(m.x, v.x), keep(m.y, v.y), keep(m.z, v.z), keep(m.w, v.w));
}

// torch.nan_to_num: NaN -> 0, +-inf -> +-FLT_MAX
__device__ __forceinline__ float nan_to_num(float x) { return isnan(x) ? 0.0f : (isinf(x) ? copysignf(FLT_MAX, x) : x); }

// torch.clip(x, min=0): NaN stays NaN
__device__ __forceinline__ float clip0(float x) { return x < 0.0f ? 0.0f : x; }

// Prescriber (fme/core/prescriber.py:54-117): mask * target + (1 - mask) * gen, or target where round(mask) == 1
__device__ __forceinline__ float prescribe(float m, float target, float gen, int interpolate) {
    if (interpolate) return __fadd_rn(__fmul_rn(m, target), __fmul_rn(__fsub_rn(1.0f, m), gen));
    return rintf(m) == 1.0f ? target : gen;
}

#define EACH4(out, expr_x, expr_y, expr_z, expr_w) const float4 out = make_float4(expr_x, expr_y, expr_z, expr_w)

// one value of one time level stored to the first n levels of a destination window (step stride st); the 16-byte decision is
// st()'s, per level row
__device__ __forceinline__ void st_levels(float* row, long step, int n, long p, long HW, float4 v) {
    for (int t = 0; t < n; ++t) st(row + t * step, p, HW, v);
}

// slots: 0 sst, 1 initial surface temperature, 2 ocean fraction (mode 0: source the atmosphere's own; else source the land
// fraction), modes 1, 2: 3 sea-ice fraction, 4 the ocean's sea-ice field under its own name; pass-through fields after these.
// blockIdx.y == 0: slots below `first`; blockIdx.y = 1 + k: pass-through field k
// WINDOW: every destination but slot 1's is a window of T levels and a one-level product is stored to each of them (L levels);
// otherwise L = 1 and the step stride of a one-level destination is not read.  Slot 2's window may be its own source (mode 0):
// a thread reads a level's four pixels before it stores them and nobody else touches them.
template <bool WINDOW>
__global__ __launch_bounds__(O2A_NT) void o2a_kernel(const float* const* srcs, const long* __restrict__ ss, float* const* dsts,
                                                 const long* __restrict__ ds, const float* const* masks, int first, int mode,
                                                 int interpolate, int T, long HW) {
    const long b = blockIdx.z;
    constexpr long CHUNK = O2A_NT * PIX;          // (shadows diag_common.h's: single-wave workgroups here)
    const long nchunk = (HW + CHUNK - 1) / CHUNK;
    const int L = WINDOW ? T : 1;
    if (blockIdx.y > 0) {
        const int j = first + (int)blockIdx.y - 1;
        const float* s = srcs[j] + b * ss[2 * j];
        float* d = dsts[j] + b * ds[2 * j];
        const long d_st = WINDOW ? ds[2 * j + 1] : 0;
        const float* m = masks[j];
        for (long c = blockIdx.x; c < nchunk; c += gridDim.x) {
            const long p = c * CHUNK + (long)threadIdx.x * PIX;
            if (p < HW) st_levels(d, d_st, L, p, HW, keep4(ldmask(m, p, HW), ld(s, p, HW)));
        }
        return;
    }
    const float* sst_s = srcs[0] + b * ss[0];
    float* sst_d = dsts[0] + b * ds[0];
    const long sst_st = WINDOW ? ds[1] : 0;
    const float* ic_s = srcs[1] + b * ss[2];
    float* ic_d = dsts[1] + b * ds[2];
    const float* f_s = srcs[2] + b * ss[4];                           // ocean fraction (mode 0) or land fraction, T levels
    const long f_st = ss[5];
    float* of_d = dsts[2] ? dsts[2] + b * ds[4] : nullptr;
    const long of_st = ds[5];
    const float* sif_s = mode ? srcs[3] + b * ss[6] : nullptr;
    float* si_d = mode ? dsts[3] + b * ds[6] : nullptr;
    const long si_st = mode ? ds[7] : 0;
    float* raw_d = (mode && dsts[4]) ? dsts[4] + b * ds[8] : nullptr;
    const long raw_st = (WINDOW && mode) ? ds[9] : 0;
    const float *m_sst = masks[0], *m_of = masks[2], *m_si = mode ? masks[3] : nullptr, *m_raw = mode ? masks[4] : nullptr;
    for (long c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const long p = c * CHUNK + (long)threadIdx.x * PIX;
        if (p >= HW) continue;
        const float4 sst = keep4(ldmask(m_sst, p, HW), ld(sst_s, p, HW));
        const float4 mask_of = ldmask(m_of, p, HW);          // read once for all time levels
        st_levels(sst_d, sst_st, L, p, HW, sst);
        float4 of0;
        if (mode == 0) {
            // carried over from the atmosphere forcing; written only where the ocean's masks change it
            const int nt = of_d ? T : 1;
            for (int t = 0; t < nt; ++t) {
                const float4 v = keep4(mask_of, ld(f_s + t * f_st, p, HW));
                if (of_d) st(of_d + t * of_st, p, HW, v);
                if (t == 0) of0 = v;
            }
        } else {
            const float4 raw = ld(sif_s, p, HW);
            if (raw_d) st_levels(raw_d, raw_st, L, p, HW, keep4(ldmask(m_raw, p, HW), raw));
            const float4 mask_si = ldmask(m_si, p, HW);
            EACH4(sif, nan_to_num(raw.x), nan_to_num(raw.y), nan_to_num(raw.z), nan_to_num(raw.w));
            if (mode == 1) st_levels(si_d, si_st, L, p, HW, keep4(mask_si, sif));          // a sea_ice_fraction: no time dependence
            for (int t = 0; t < T; ++t) {
                const float4 land = ld(f_s + t * f_st, p, HW);
                EACH4(sea, __fsub_rn(1.0f, land.x), __fsub_rn(1.0f, land.y), __fsub_rn(1.0f, land.z), __fsub_rn(1.0f, land.w));
                float4 si = sif;
                if (mode == 2) {                                              // an ocean_sea_ice_fraction: sif0 * (1 - land)
                    si = make_float4(__fmul_rn(sif.x, sea.x), __fmul_rn(sif.y, sea.y), __fmul_rn(sif.z, sea.z), __fmul_rn(sif.w, sea.w));
                    st(si_d + t * si_st, p, HW, keep4(mask_si, si));
                }
                EACH4(of, clip0(__fsub_rn(sea.x, si.x)), clip0(__fsub_rn(sea.y, si.y)), clip0(__fsub_rn(sea.z, si.z)),
                      clip0(__fsub_rn(sea.w, si.w)));
                const float4 v = keep4(mask_of, of);
                st(of_d + t * of_st, p, HW, v);
                if (t == 0) of0 = v;
            }
        }
        const float4 gen = ld(ic_s, p, HW);
        st(ic_d, p, HW, make_float4(prescribe(of0.x, sst.x, gen.x, interpolate), prescribe(of0.y, sst.y, gen.y, interpolate),
                                    prescribe(of0.z, sst.z, gen.z, interpolate), prescribe(of0.w, sst.w, gen.w, interpolate)));
    }
}

// srcs [N][T] planes with their sample strides ss [N][T]; dsts [N] windows with (sample, step) strides ds [N][2]
__global__ __launch_bounds__(NT) void a2o_kernel(const float* const* srcs, const long* __restrict__ ss, float* const* dsts,
                                                 const long* __restrict__ ds, const int* __restrict__ slot, int T, long HW) {
    const int j = blockIdx.y;
    const long b = blockIdx.z;
    const long nchunk = (HW + CHUNK - 1) / CHUNK;
    const int sl = slot[j] ? 1 : 0;
    float* base = dsts[j] + b * ds[2 * j];
    float* mean_d = base + sl * ds[2 * j + 1];
    float* nan_d = base + (1 - sl) * ds[2 * j + 1];
    const float qnan = __int_as_float(0x7fc00000);
    const double n = (double)T;
    for (long c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const long p = c * CHUNK + (long)threadIdx.x * PIX;
        if (p >= HW) continue;
        double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0;
        for (int t = 0; t < T; ++t) {
            const long k = (long)j * T + t;
            const float4 v = ld(srcs[k] + b * ss[k], p, HW);
            ax += (double)v.x;
            ay += (double)v.y;
            az += (double)v.z;
            aw += (double)v.w;
        }
        st(mean_d, p, HW, make_float4((float)(ax / n), (float)(ay / n), (float)(az / n), (float)(aw / n)));
        st(nan_d, p, HW, make_float4(qnan, qnan, qnan, qnan));
    }
}

unsigned grid_x(long hw, long chunk) {
    const long n = (hw < MAX_PIXELS ? hw : MAX_PIXELS);
    return (unsigned)((n + chunk - 1) / chunk);
}


// the argument checks and the launch of both forms of the ocean -> atmosphere exchange; `name`: the entry, for its messages
template <bool WINDOW>
int launch_o2a(const std::string& name, const float* const* srcs, const long* src_strides, float* const* dsts, const long* dst_strides,
               const float* const* masks, int npass, int mode, int interpolate, int n_inner, int batch, long hw, void* stream) {
    if (npass < 0 || npass > ACE_COUPLE_MAX_NAMES) return ace::fail(ACE_ERR_INVALID, name + ": npass outside 0 .. ACE_COUPLE_MAX_NAMES");
    if (mode < ACE_COUPLE_OFRAC_CARRIED || mode > ACE_COUPLE_OFRAC_FROM_OCEAN_SIF)
        return ace::fail(ACE_ERR_INVALID, name + ": unknown mode");
    if (interpolate != 0 && interpolate != 1) return ace::fail(ACE_ERR_INVALID, name + ": interpolate must be 0 or 1");
    if (n_inner <= 0 || n_inner > ACE_COUPLE_MAX_INNER)
        return ace::fail(ACE_ERR_INVALID, name + ": n_inner outside 1 .. ACE_COUPLE_MAX_INNER");
    if (batch < 1 || batch > 65535) return ace::fail(ACE_ERR_INVALID, name + ": batch outside 1 .. 65535");
    if (hw <= 0) return ace::fail(ACE_ERR_INVALID, name + ": hw must be positive");
    if (!srcs || !src_strides || !dsts || !dst_strides || !masks) return ace::fail(ACE_ERR_INVALID, name + ": null argument");
    const int first = mode == ACE_COUPLE_OFRAC_CARRIED ? 3 : 5;
    hipLaunchKernelGGL(o2a_kernel<WINDOW>, dim3(grid_x(hw, O2A_NT * PIX), 1 + npass, batch), dim3(O2A_NT), 0,
                       static_cast<hipStream_t>(stream), srcs, src_strides, dsts, dst_strides, masks, first, mode, interpolate,
                       n_inner + 1, hw);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}

}  // namespace

extern "C" int ace_couple_ocean_to_atmosphere(const float* const* srcs, const long* src_strides, float* const* dsts,
                                              const long* dst_strides, const float* const* masks, int npass, int mode,
                                              int interpolate, int n_inner, int batch, long hw, void* stream) {
    return launch_o2a<false>("ace_couple_ocean_to_atmosphere", srcs, src_strides, dsts, dst_strides, masks, npass, mode, interpolate,
                             n_inner, batch, hw, stream);
}

extern "C" int ace_couple_ocean_to_atmosphere_window(const float* const* srcs, const long* src_strides, float* const* dsts,
                                                     const long* dst_strides, const float* const* masks, int npass, int mode,
                                                     int interpolate, int n_inner, int batch, long hw, void* stream) {
    return launch_o2a<true>("ace_couple_ocean_to_atmosphere_window", srcs, src_strides, dsts, dst_strides, masks, npass, mode,
                            interpolate, n_inner, batch, hw, stream);
}

extern "C" int ace_couple_atmosphere_to_ocean(const float* const* srcs, const long* src_strides, float* const* dsts,
                                              const long* dst_strides, const int* slot, int nnames, int n_inner, int batch,
                                              long hw, void* stream) {
    if (nnames < 0 || nnames > ACE_COUPLE_MAX_NAMES)
        return ace::fail(ACE_ERR_INVALID, "ace_couple_atmosphere_to_ocean: nnames outside 0 .. ACE_COUPLE_MAX_NAMES");
    if (n_inner <= 0 || n_inner > ACE_COUPLE_MAX_INNER)
        return ace::fail(ACE_ERR_INVALID, "ace_couple_atmosphere_to_ocean: n_inner outside 1 .. ACE_COUPLE_MAX_INNER");
    if (batch < 1 || batch > 65535) return ace::fail(ACE_ERR_INVALID, "ace_couple_atmosphere_to_ocean: batch outside 1 .. 65535");
    if (hw <= 0) return ace::fail(ACE_ERR_INVALID, "ace_couple_atmosphere_to_ocean: hw must be positive");
    if (nnames == 0) return ACE_OK;
    if (!srcs || !src_strides || !dsts || !dst_strides || !slot)
        return ace::fail(ACE_ERR_INVALID, "ace_couple_atmosphere_to_ocean: null argument");
    hipLaunchKernelGGL(a2o_kernel, dim3(grid_x(hw, CHUNK), nnames, batch), dim3(NT), 0, static_cast<hipStream_t>(stream), srcs,
                       src_strides, dsts, dst_strides, slot, n_inner, hw);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}
