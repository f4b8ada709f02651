// The ocean's derived variables (fme/core/ocean_derived_variables.py, the OceanData properties of fme/core/ocean_data.py they
// read) over one window, in one launch: any subset of
//   ocean_heat_content, ocean_heat_content_tendency, implied_tendency_of_ocean_heat_content_due_to_advection,
//   net_energy_flux_into_ocean_column, sea_ice_fraction, HI, hfds
// for batch x steps x hw pixels.  The reference stacks every thetao level (a full copy), multiplies three times at full size, takes
// a nansum, a where and a diff, and a dozen elementwise passes over the surface fields - after concatenating the initial condition
// onto every field of the window.  Here every input plane is read once and every output written once; the time level before the
// window's first step is read where it lies (the `head` planes), nothing is concatenated.
//   work split   workgroup (chunk, time chunk, sample) owns 1024 consecutive pixels over t_chunk steps, thread i the four pixels
//                from chunk * 1024 + 4 i: one 16-byte load per plane when hw, every base and every stride are multiples of 4
//                floats (decided once per launch, on the host: the predicate depends on the descriptor only), four loads
//                otherwise.  The column sum keeps the loads of UNROLL levels (thetao and dz) in flight ahead of the adds; the adds
//                stay in level order.  The dz table is re-read every step and stays in cache.
//   time chunks  a chunk's first step needs the column sum of the step before it: it is recomputed (from the head planes for the
//                window's first step), so chunks are independent and the result does not depend on t_chunk, bit for bit.
// All fp64 work is in a fixed order; no atomics, no scratch buffer, no allocation, no host synchronisation: two identical calls
// are bitwise identical.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/ace_sfno.h"
#include "errors.h"

// the reference's torch ops round after every multiply and add: no fused multiply-adds in the fp32 arithmetic
#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int PIX = 4;               // pixels per thread
constexpr int CHUNK = NT * PIX;      // pixels per workgroup
constexpr int UNROLL = 8;            // levels whose loads are issued together
constexpr int TARGET_GROUPS = 512;   // t_chunk = 0: the longest chunks that still give about two workgroups per compute unit

// fme/core/constants.py: SPECIFIC_HEAT_OF_SEA_WATER_CM4 * DENSITY_OF_SEA_WATER_CM4, one double
constexpr double CP_RHO = 3992.0 * 1035.0;

constexpr unsigned W_OHC = 1u << ACE_OCEAN_DERIVE_OHC, W_TEND = 1u << ACE_OCEAN_DERIVE_OHC_TENDENCY,
                   W_ADV = 1u << ACE_OCEAN_DERIVE_ADVECTION, W_NET = 1u << ACE_OCEAN_DERIVE_NET_FLUX,
                   W_SIF = 1u << ACE_OCEAN_DERIVE_SEA_ICE_FRACTION, W_HI = 1u << ACE_OCEAN_DERIVE_HI,
                   W_HFDS = 1u << ACE_OCEAN_DERIVE_HFDS;

// pixels p .. p + 3 of a plane of hw pixels: one 16-byte load, or four loads (a pixel past the end reads the last one and is never
// stored)
template <bool VEC>
__device__ __forceinline__ float4 ld4(const float* s, long p, long hw) {
    if (VEC) return *reinterpret_cast<const float4*>(s + p);
    const long last = hw - 1;
    return make_float4(s[p], s[p + 1 < hw ? p + 1 : last], s[p + 2 < hw ? p + 2 : last], s[p + 3 < hw ? p + 3 : last]);
}

template <bool VEC>
__device__ __forceinline__ void st4(float* d, long p, long hw, const float (&v)[PIX]) {
    if (VEC) {
        *reinterpret_cast<float4*>(d + p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < PIX; ++i)
            if (p + i < hw) d[p + i] = v[i];
    }
}

template <bool VEC>
__device__ __forceinline__ void field4(const ace_ocean_derive_field& f, int b, int t, long p, long hw, float (&v)[PIX]) {
    const float4 x = ld4<VEC>(f.base + (long)b * f.bstride + (long)t * f.tstride, p, hw);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
}

// the planes of level k at step t of sample b, or its head plane (HEAD; NULL where the initial condition has no such level)
template <bool HEAD>
__device__ __forceinline__ const float* level_plane(const ace_ocean_derive_level& L, int b, int t) {
    if (HEAD) return L.head ? L.head + (long)b * L.head_bstride : nullptr;
    return L.f.base + (long)b * L.f.bstride + (long)t * L.f.tstride;
}

__device__ __forceinline__ void add_level(double (&acc)[PIX], const float4& th, const float4& dz) {
    // (double) thetao * (double) dz is exact in fp64 (24 + 24 significand bits), so the fused multiply-add rounds once, as the
    // separate add would; a NaN thetao contributes nothing (nansum)
    if (!isnan(th.x)) acc[0] = __builtin_fma((double)th.x, (double)dz.x, acc[0]);
    if (!isnan(th.y)) acc[1] = __builtin_fma((double)th.y, (double)dz.y, acc[1]);
    if (!isnan(th.z)) acc[2] = __builtin_fma((double)th.z, (double)dz.z, acc[2]);
    if (!isnan(th.w)) acc[3] = __builtin_fma((double)th.w, (double)dz.w, acc[3]);
}

// S(b, t, p .. p + 3) = CP_RHO * sum_k thetao_k dz_k, k ascending
template <bool VEC, bool HEAD>
__device__ __forceinline__ void column_sum(const ace_ocean_derive_desc& d, int b, int t, long p, long hw, double (&S)[PIX]) {
    const float4 nan4 = make_float4(NAN, NAN, NAN, NAN);
    double acc[PIX] = {0.0, 0.0, 0.0, 0.0};
    const int L = d.nlev;
    int k = 0;
    for (; k + UNROLL <= L; k += UNROLL) {
        float4 th[UNROLL], dz[UNROLL];
#pragma unroll
        for (int j = 0; j < UNROLL; ++j) {
            const float* s = level_plane<HEAD>(d.thetao[k + j], b, t);
            th[j] = s ? ld4<VEC>(s, p, hw) : nan4;
            dz[j] = ld4<VEC>(d.dz + (long)(k + j) * hw, p, hw);
        }
#pragma unroll
        for (int j = 0; j < UNROLL; ++j) add_level(acc, th[j], dz[j]);
    }
    if (k < L) {                                           // the remainder: its loads issued together too, the adds in order
        const int rem = L - k;                             // 1 .. UNROLL - 1, uniform over the launch
        float4 th[UNROLL - 1], dz[UNROLL - 1];
#pragma unroll
        for (int j = 0; j < UNROLL - 1; ++j)
            if (j < rem) {
                const float* s = level_plane<HEAD>(d.thetao[k + j], b, t);
                th[j] = s ? ld4<VEC>(s, p, hw) : nan4;
                dz[j] = ld4<VEC>(d.dz + (long)(k + j) * hw, p, hw);
            }
#pragma unroll
        for (int j = 0; j < UNROLL - 1; ++j)
            if (j < rem) add_level(acc, th[j], dz[j]);
    }
#pragma unroll
    for (int i = 0; i < PIX; ++i) S[i] = acc[i] * CP_RHO;
}

// vol * 1e9 / (area * frac) in fp64, rounded to fp32, with the value of where(isnan(vol), NaN, nan_to_num(exp(9 ln 10 + ln vol -
// ln area - ln frac))) on the extended reals at every special input (the table of include/ace_sfno.h)
__device__ __forceinline__ float sea_ice_thickness(float vol_f, float area_f, float frac_f) {
    const double vol = (double)vol_f, area = (double)area_f, frac = (double)frac_f;
    if (isnan(vol)) return NAN;
    if (isnan(frac) || isnan(area)) return 0.0f;                       // a NaN logarithm: nan_to_num gives 0
    if (vol < 0.0 || frac < 0.0 || area < 0.0) return 0.0f;            // the logarithm of a negative number is NaN
    if (vol == 0.0) return 0.0f;                                       // -inf, or -inf + inf = NaN
    if (isinf(frac) || isinf(area)) return 0.0f;                       // -inf, or inf - inf = NaN
    if (isinf(vol)) return FLT_MAX;
    const double den = area * frac;                                    // exact: 24 + 24 significand bits
    if (den == 0.0) return FLT_MAX;                                    // + inf
    const float q = (float)((vol * 1e9) / den);                        // vol * 1e9 is exact too: one rounding in fp64, one to fp32
    return q > FLT_MAX ? FLT_MAX : q;
}

template <bool VEC>
__global__ __launch_bounds__(NT) void ocean_derive_kernel(ace_ocean_derive_desc d, int t_chunk) {
    const long hw = d.hw;
    const long p = (long)blockIdx.x * CHUNK + (long)threadIdx.x * PIX;
    if (p >= hw) return;                                   // no thread of this kernel waits for another
    const int b = blockIdx.z;
    const int t0 = blockIdx.y * t_chunk;
    const int t1 = t0 + t_chunk < d.steps ? t0 + t_chunk : d.steps;
    const unsigned want = d.want;
    const bool need_S = (want & (W_OHC | W_TEND | W_ADV)) != 0, need_tend = (want & (W_TEND | W_ADV)) != 0;
    const bool need_net = (want & (W_NET | W_ADV)) != 0;
    const bool need_ssf = need_net || (want & W_HI) != 0 || ((want & W_HFDS) != 0);
    const bool need_hfds = need_net || (want & W_HFDS) != 0;
    const bool need_land = (want & W_SIF) != 0 || (need_ssf && !d.sea_surface_fraction.base) ||
                           ((want & W_HI) != 0 && !d.ocean_sea_ice_fraction.base);

    float ocean[PIX] = {0.f, 0.f, 0.f, 0.f}, area[PIX] = {0.f, 0.f, 0.f, 0.f};
    if (need_S) {
        const float4 m = ld4<VEC>(d.mask0, p, hw);
        ocean[0] = m.x; ocean[1] = m.y; ocean[2] = m.z; ocean[3] = m.w;
    }
    if (want & W_HI) {
        const float4 a = ld4<VEC>(d.area_m2, p, hw);
        area[0] = a.x; area[1] = a.y; area[2] = a.z; area[3] = a.w;
    }
    double prev[PIX] = {0.0, 0.0, 0.0, 0.0};
    bool have_prev = false;
    if (need_tend) {
        if (t0 > 0) {
            column_sum<VEC, false>(d, b, t0 - 1, p, hw, prev);
            have_prev = true;
        } else if (d.has_head) {
            column_sum<VEC, true>(d, b, 0, p, hw, prev);
            have_prev = true;
        }
    }
    for (int t = t0; t < t1; ++t) {
        const long at = (long)b * d.out_bstride + (long)t * d.out_tstride;
        float tend[PIX] = {0.f, 0.f, 0.f, 0.f};
        if (need_S) {
            double S[PIX];
            column_sum<VEC, false>(d, b, t, p, hw, S);
            if (want & W_OHC) {
                float v[PIX];
#pragma unroll
                for (int i = 0; i < PIX; ++i) v[i] = ocean[i] > 0.0f ? (float)S[i] : NAN;
                st4<VEC>(d.out[ACE_OCEAN_DERIVE_OHC] + at, p, hw, v);
            }
            if (need_tend) {
#pragma unroll
                for (int i = 0; i < PIX; ++i) {
                    // the window's first step without a head: the reference's zeros_like row, land included
                    tend[i] = !have_prev ? 0.0f : (ocean[i] > 0.0f ? (float)((S[i] - prev[i]) / d.dt_seconds) : NAN);
                    prev[i] = S[i];
                }
                have_prev = true;
                if (want & W_TEND) st4<VEC>(d.out[ACE_OCEAN_DERIVE_OHC_TENDENCY] + at, p, hw, tend);
            }
        }
        float land[PIX] = {0.f, 0.f, 0.f, 0.f}, ssf[PIX] = {0.f, 0.f, 0.f, 0.f}, hf[PIX] = {0.f, 0.f, 0.f, 0.f};
        if (need_land) field4<VEC>(d.land_fraction, b, t, p, hw, land);
        if (need_ssf) {
            if (d.sea_surface_fraction.base) {
                field4<VEC>(d.sea_surface_fraction, b, t, p, hw, ssf);
            } else {
#pragma unroll
                for (int i = 0; i < PIX; ++i) ssf[i] = 1.0f - land[i];
            }
        }
        if (need_hfds) {
            if (d.hfds.base) {
                field4<VEC>(d.hfds, b, t, p, hw, hf);
            } else {
                float total[PIX];
                field4<VEC>(d.hfds_total_area, b, t, p, hw, total);
#pragma unroll
                for (int i = 0; i < PIX; ++i) hf[i] = total[i] / ssf[i];
            }
            if (want & W_HFDS) st4<VEC>(d.out[ACE_OCEAN_DERIVE_HFDS] + at, p, hw, hf);
        }
        if (need_net) {
            float geo[PIX] = {0.f, 0.f, 0.f, 0.f}, net[PIX];
            if (d.hfgeou.base) field4<VEC>(d.hfgeou, b, t, p, hw, geo);
#pragma unroll
            for (int i = 0; i < PIX; ++i) net[i] = (hf[i] + geo[i]) * ssf[i];
            if (want & W_NET) st4<VEC>(d.out[ACE_OCEAN_DERIVE_NET_FLUX] + at, p, hw, net);
            if (want & W_ADV) {
                float adv[PIX];
#pragma unroll
                for (int i = 0; i < PIX; ++i) adv[i] = tend[i] - net[i];
                st4<VEC>(d.out[ACE_OCEAN_DERIVE_ADVECTION] + at, p, hw, adv);
            }
        }
        if (want & (W_SIF | W_HI)) {
            float osif[PIX] = {0.f, 0.f, 0.f, 0.f};
            if (d.ocean_sea_ice_fraction.base) field4<VEC>(d.ocean_sea_ice_fraction, b, t, p, hw, osif);
            if (want & W_SIF) {
                float v[PIX];
#pragma unroll
                for (int i = 0; i < PIX; ++i) v[i] = osif[i] * (1.0f - land[i]);
                st4<VEC>(d.out[ACE_OCEAN_DERIVE_SEA_ICE_FRACTION] + at, p, hw, v);
            }
            if (want & W_HI) {
                float vol[PIX], frac[PIX], v[PIX];
                field4<VEC>(d.sea_ice_volume, b, t, p, hw, vol);
                if (d.ocean_sea_ice_fraction.base) {
#pragma unroll
                    for (int i = 0; i < PIX; ++i) frac[i] = osif[i] * ssf[i];
                } else {
                    float sif[PIX];
                    field4<VEC>(d.sea_ice_fraction, b, t, p, hw, sif);
#pragma unroll
                    for (int i = 0; i < PIX; ++i) frac[i] = (sif[i] * ssf[i]) / (1.0f - land[i]);
                }
#pragma unroll
                for (int i = 0; i < PIX; ++i) v[i] = sea_ice_thickness(vol[i], area[i], frac[i]);
                st4<VEC>(d.out[ACE_OCEAN_DERIVE_HI] + at, p, hw, v);
            }
        }
    }
}

int refuse(const std::string& m) { return ace::fail(ACE_ERR_INVALID, "ace_ocean_derive_window: " + m); }

bool aligned4(const void* p, long s0 = 0, long s1 = 0) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && ((s0 | s1) & 3) == 0; }
bool field_aligned(const ace_ocean_derive_field& f) { return !f.base || aligned4(f.base, f.bstride, f.tstride); }

}  // namespace

extern "C" int ace_ocean_derive_window(const ace_ocean_derive_desc* desc, void* stream) {
    if (!desc) return refuse("null argument");
    const ace_ocean_derive_desc& d = *desc;
    const unsigned want = d.want;
    if (want >> ACE_OCEAN_DERIVE_NOUT) return refuse("unknown bits in want");
    if (d.batch < 1 || d.batch > 65535 || d.steps < 1 || d.hw < 1) return refuse("need 1 <= batch <= 65535 (a grid dimension), steps >= 1, hw >= 1");
    const long nchunk = (d.hw + CHUNK - 1) / CHUNK;
    if (nchunk > 2147483647L) return refuse("need hw <= 1024 * (2^31 - 1)");
    if (d.t_chunk < 0) return refuse("need t_chunk >= 0");
    if (d.nlev < 0 || d.nlev > ACE_OCEAN_MAX_LEVELS) return refuse("nlev outside 0 .. " + std::to_string(ACE_OCEAN_MAX_LEVELS));
    if (want == 0) return ACE_OK;
    for (int i = 0; i < ACE_OCEAN_DERIVE_NOUT; ++i)
        if (((want >> i) & 1u) && !d.out[i]) return refuse("a wanted output has no destination");
    const bool need_S = (want & (W_OHC | W_TEND | W_ADV)) != 0, need_net = (want & (W_NET | W_ADV)) != 0;
    if (need_S) {
        if (d.nlev < 1) return refuse("the heat content needs 1 .. " + std::to_string(ACE_OCEAN_MAX_LEVELS) + " levels");
        if (!d.dz || !d.mask0) return refuse("the heat content needs dz and mask0");
        for (int k = 0; k < d.nlev; ++k)
            if (!d.thetao[k].f.base) return refuse("the heat content needs every thetao level: level " + std::to_string(k) + " is absent");
        if ((want & (W_TEND | W_ADV)) && !(d.dt_seconds > 0)) return refuse("the tendency needs dt_seconds > 0");
    }
    const bool has_ssf = d.sea_surface_fraction.base || d.land_fraction.base;
    if ((want & W_HFDS) && d.hfds.base) return refuse("hfds is wanted but its plane exists: there is nothing to derive");
    if ((want & W_SIF) && d.sea_ice_fraction.base) return refuse("sea_ice_fraction is wanted but its plane exists: there is nothing to derive");
    if ((want & W_HFDS) && !(d.hfds_total_area.base && has_ssf)) return refuse("hfds needs hfds_total_area and the sea-surface or land fraction");
    if (need_net && !((d.hfds.base || d.hfds_total_area.base) && has_ssf))
        return refuse("the net flux needs hfds or hfds_total_area, and the sea-surface or land fraction");
    if ((want & W_SIF) && !(d.ocean_sea_ice_fraction.base && d.land_fraction.base))
        return refuse("sea_ice_fraction needs ocean_sea_ice_fraction and land_fraction");
    if (want & W_HI) {
        if (!d.sea_ice_volume.base || !d.area_m2 || !has_ssf) return refuse("HI needs sea_ice_volume, area_m2 and the sea-surface or land fraction");
        if (!d.ocean_sea_ice_fraction.base && !(d.sea_ice_fraction.base && d.land_fraction.base))
            return refuse("HI needs ocean_sea_ice_fraction, or sea_ice_fraction and land_fraction");
    }
    int t_chunk = d.t_chunk;
    if (t_chunk == 0) {
        const long groups_per_step = nchunk * d.batch;
        long c = (long)d.steps * groups_per_step / TARGET_GROUPS;
        c = c < 1 ? 1 : (c > d.steps ? d.steps : c);
        if (((long)d.steps + c - 1) / c > 65535) c = ((long)d.steps + 65534) / 65535;
        t_chunk = (int)c;
    }
    if (t_chunk > d.steps) t_chunk = d.steps;
    const long ntc = ((long)d.steps + t_chunk - 1) / t_chunk;
    if (ntc > 65535) return refuse("need ceil(steps / t_chunk) <= 65535 (a grid dimension)");

    // one decision for the launch: every plane it may touch starts 16-byte aligned at every (sample, step)
    bool vec = (d.hw & 3) == 0 && field_aligned(d.hfds) && field_aligned(d.hfds_total_area) && field_aligned(d.hfgeou) &&
               field_aligned(d.sea_surface_fraction) && field_aligned(d.land_fraction) && field_aligned(d.ocean_sea_ice_fraction) &&
               field_aligned(d.sea_ice_fraction) && field_aligned(d.sea_ice_volume) && aligned4(d.dz) && aligned4(d.mask0) &&
               aligned4(d.area_m2);
    for (int k = 0; vec && k < d.nlev; ++k)
        vec = field_aligned(d.thetao[k].f) && aligned4(d.thetao[k].head, d.thetao[k].head_bstride);
    for (int i = 0; vec && i < ACE_OCEAN_DERIVE_NOUT; ++i)
        if ((want >> i) & 1u) vec = aligned4(d.out[i], d.out_bstride, d.out_tstride);

    const dim3 grid((unsigned)nchunk, (unsigned)ntc, (unsigned)d.batch);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(ocean_derive_kernel<true>, grid, dim3(NT), 0, s, d, t_chunk);
    else
        hipLaunchKernelGGL(ocean_derive_kernel<false>, grid, dim3(NT), 0, s, d, t_chunk);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ace::fail(ACE_ERR_RUNTIME, std::string("ace_ocean_derive_window: launch failed: ") + hipGetErrorString(e));
    return ACE_OK;
}
