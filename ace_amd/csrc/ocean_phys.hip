// Ocean corrector of the stepper as gfx950 kernels: what OceanCorrectorConfig (fme/core/corrector/ocean.py) builds, applied
// to the denormalised output planes of one step, in place, in the reference's order:
//   force positive -> sea-ice fraction (clamp to [0, 1], rebalance against the input's land, zero where ice free)
//   -> surface energy flux (hfds) -> ocean heat content (one ratio per sample scales every thetao level and the SST in C)
// Every correction but the last is column-local, and the last needs three masked area-weighted global means of quantities
// the earlier links produce.  So two launches:
//   O1  one column per thread (grid-stride): the column-local corrections, written in place; then the column's heat
//       content of output and input (depth integral, NaN counted as zero, NaN where the top level is masked) and its net
//       flux into the ocean -> per-workgroup fp64 partial sums (fixed tree, no atomics) of w * OHC_gen, w * OHC_in, w * F
//       and w, w = area weight times the mask for "ocean_heat_content"
//   O2  each workgroup re-sums its sample's partials in one fixed order, forms the ratio in fp64, scales thetao_k and sst
// A column reads ~2 L + 15 fields once: at 1 degree and 19 levels ~14 MB per sample; the passes are launch-, not
// bandwidth-bound.  Two calls on the same inputs give bitwise-identical outputs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ace_sfno.h"
#include "errors.h"

// the reference's torch ops round after every multiply and add: no fused multiply-adds in the per-column arithmetic
#pragma clang fp contract(off)

namespace {

constexpr int MAXL = ACE_OCEAN_MAX_LEVELS;
constexpr int NQ = 4;            // partial-sum slots: OHC of output, OHC of input, net flux, weight
constexpr int NBLK_MAX = 512;    // workgroups per sample (grid-stride beyond)
constexpr int NT = 256;

// fme/core/constants.py
constexpr float LATENT_HEAT_OF_VAPORIZATION = 2.5e6f;
constexpr float LATENT_HEAT_OF_FREEZING = 334000.0f;
constexpr float CP_SEA = 3992.0f;     // SPECIFIC_HEAT_OF_SEA_WATER_CM4
constexpr float RHO_SEA = 1035.0f;    // DENSITY_OF_SEA_WATER_CM4
constexpr float T_FREEZE = 273.15f;   // FREEZING_TEMPERATURE_KELVIN

struct OceanParams {           // static per handle
    int H, W, L, max_batch;
    int sea_ice, remove_negative, hfds, ohc;
    float dt, heating;
    const float* wlat;         // [H] area weight per row
    const float* mask_ohc;     // [H * W] or null
    const float* mask0;        // [H * W]
    const float* dz;           // [L][H * W]
    double* part;              // [max_batch][NQ][NBLK_MAX]
};

__device__ __forceinline__ float ld(const ace_phys_plane& f, int b, long px) { return f.p[(long)b * f.stride + px]; }
__device__ __forceinline__ void st(const ace_phys_plane& f, int b, long px, float v) { f.p[(long)b * f.stride + px] = v; }

// torch.clamp semantics: NaN passes through
__device__ __forceinline__ float clamp_min0(float v) { return v < 0.0f ? 0.0f : v; }
__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// DepthCoordinate.depth_integral(thetao * 3992 * 1035) of one column (coordinates.py:412-440)
__device__ __forceinline__ double column_heat(const OceanParams& P, const ace_phys_plane* T, int b, long px, long HW) {
    if (P.mask0[px] <= 0.0f) return (double)NAN;
    double s = 0.0;
    for (int k = 0; k < P.L; ++k) {
        const float x = ((ld(T[k], b, px) * CP_SEA) * RHO_SEA) * P.dz[(long)k * HW + px];
        if (!isnan(x)) s += (double)x;
    }
    return s;
}

__device__ __forceinline__ float frozen_rate(const ace_ocean_fields& F, int b, long px) {
    if (F.frozen.p) return ld(F.frozen, b, px);
    if (F.frozen_parts[0].p) return (ld(F.frozen_parts[0], b, px) + ld(F.frozen_parts[1], b, px)) + ld(F.frozen_parts[2], b, px);
    return 0.0f;
}

// fixed-order workgroup reduction of NQ doubles; thread q < NQ of the workgroup stores slot q
__device__ __forceinline__ void block_store_partials(double (&v)[NQ], double* dst /* [NQ][NBLK_MAX] */, int blk) {
    __shared__ double red[NQ][NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = 0; q < NQ; ++q) {
        double x = v[q];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
        if (lane == 0) red[q][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        const int q = threadIdx.x;
        dst[(long)q * NBLK_MAX + blk] = ((red[q][0] + red[q][1]) + (red[q][2] + red[q][3]));
    }
}

// ---- O1 -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void ocean_o1(OceanParams P, ace_ocean_fields F, int nblk) {
    const int b = blockIdx.y;
    const long HW = (long)P.H * P.W;
    double acc[NQ] = {0.0, 0.0, 0.0, 0.0};
    for (long px = (long)blockIdx.x * NT + threadIdx.x; px < HW; px += (long)nblk * NT) {
        for (int i = 0; i < F.npositive; ++i) st(F.positive[i], b, px, clamp_min0(ld(F.positive[i], b, px)));   // utils.py:26-44
        if (P.sea_ice) {   // ocean.py:55-93
            float sif = clamp01(ld(F.sif, b, px));
            if (P.remove_negative) {
                float neg = (1.0f - sif) - ld(F.reb_land, b, px);
                neg = neg > 0.0f ? 0.0f : neg;            // clip(max=0), NaN passes
                sif = sif + neg;
            }
            st(F.sif, b, px, sif);
            const float keep = sif > 0.0f ? 1.0f : 0.0f;
            for (int i = 0; i < F.nzero; ++i) st(F.zero[i], b, px, ld(F.zero[i], b, px) * keep);
        }
        if (P.hfds) {      // ocean.py:369-428
            const float land = ld(F.in_land, b, px);
            const float sif_in = F.in_sif_is_ocean_sif ? ld(F.in_sif, b, px) * (1.0f - land) : ld(F.in_sif, b, px);
            const float ofrac = (1.0f - land) - sif_in;
            const float net_sfc = (((ld(F.dsw, b, px) - ld(F.usw, b, px)) + ld(F.dlw, b, px)) - ld(F.ulw, b, px))
                                  + (-ld(F.lhf, b, px) - ld(F.shf, b, px)) - frozen_rate(F, b, px) * LATENT_HEAT_OF_FREEZING;
            const float lhf = ld(F.lhf, b, px);
            const float mass = (CP_SEA * ((ld(F.precip, b, px) + frozen_rate(F, b, px)) - lhf / LATENT_HEAT_OF_VAPORIZATION))
                               * (ld(F.in_sst, b, px) - T_FREEZE);
            float net = net_sfc + mass;
            if (F.hfds_total_area) {
                const float fs = ld(F.f_ssf, b, px);
                net = net * (F.f_ssf_is_land ? 1.0f - fs : fs);
            }
            const float g = ld(F.hfds, b, px);
            st(F.hfds, b, px, P.hfds == 1 ? net * ofrac + g : net * ofrac + g * (1.0f - ofrac));
        }
        if (P.ohc) {       // ocean.py:431-486: the column's share of the three means
            const float w = P.wlat[px / P.W] * (P.mask_ohc ? P.mask_ohc[px] : 1.0f);
            if (w != 0.0f) {
                const double gen = column_heat(P, F.thetao, b, px, HW);
                const double inp = column_heat(P, F.thetao_in, b, px, HW);
                const float fs = ld(F.f_ssf, b, px);
                const float ssf = F.f_ssf_is_land ? 1.0f - fs : fs;
                const float geo = F.hfgeou.p ? ld(F.hfgeou, b, px) : 0.0f;
                float flux;
                if (F.flux_source == 0) {
                    flux = ld(F.hfds, b, px) + geo * ssf;
                } else if (F.flux_source == 1) {
                    flux = (ld(F.hfds, b, px) + geo) * ssf;
                } else if (F.flux_source == 2) {
                    flux = (ld(F.in_flux, b, px) + geo) * ssf;
                } else {
                    const float is = ld(F.in_ssf, b, px);
                    flux = (ld(F.in_flux, b, px) / (F.in_ssf_is_land ? 1.0f - is : is) + geo) * ssf;
                }
                // metrics.weighted_mean in fp32: (x * w) rounded, then summed; here the sum is fp64
                acc[0] += (double)((float)gen * w);
                acc[1] += (double)((float)inp * w);
                acc[2] += (double)(flux * w);
                acc[3] += (double)w;
            }
        }
    }
    if (P.ohc) block_store_partials(acc, P.part + (long)b * NQ * NBLK_MAX, blockIdx.x);
}

// ---- O2 -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void ocean_o2(OceanParams P, ace_ocean_fields F, int nblk) {
    const int b = blockIdx.y;
    const long HW = (long)P.H * P.W;
    __shared__ double red[NQ][NT / 64];
    __shared__ float ratio_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* src = P.part + (long)b * NQ * NBLK_MAX;
    for (int q = 0; q < NQ; ++q) {   // thread t adds partials t, t + NT, ...; then the same tree as O1
        double x = 0.0;
        for (int i = threadIdx.x; i < nblk; i += NT) x += src[(long)q * NBLK_MAX + i];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
        if (lane == 0) red[q][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s[NQ];
        for (int q = 0; q < NQ; ++q) s[q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
        const double gen = s[0] / s[3], inp = s[1] / s[3], flux = s[2] / s[3];
        ratio_s = (float)((inp + (flux + (double)P.heating) * (double)P.dt) / gen);
    }
    __syncthreads();
    const float r = ratio_s;
    for (long px = (long)blockIdx.x * NT + threadIdx.x; px < HW; px += (long)nblk * NT) {
        for (int k = 0; k < P.L; ++k) st(F.thetao[k], b, px, ld(F.thetao[k], b, px) * r);
        if (F.sst.p) st(F.sst, b, px, (ld(F.sst, b, px) - T_FREEZE) * r + T_FREEZE);
    }
}

}  // namespace

struct ace_ocean_phys {
    OceanParams P;
    void* dev = nullptr;       // one allocation: wlat | mask_ohc | mask0 | dz | part
    long o1 = 0, o2 = 0;       // launches made (route query)
};

extern "C" int ace_ocean_phys_create(const ace_ocean_config* c, const float* wlat_host, const float* dz_host, const float* mask_ohc_host,
                                     const float* mask0_host, ace_ocean_phys** out) {
    if (!c || !out) return ace::fail(ACE_ERR_INVALID, "null argument");
    if (c->nlat < 1 || c->nlon < 1 || c->max_batch < 1) return ace::fail(ACE_ERR_INVALID, "bad grid / batch");
    if (c->hfds < 0 || c->hfds > 2 || c->ohc < 0 || c->ohc > 1) return ace::fail(ACE_ERR_INVALID, "unknown correction variant");
    if (c->ohc) {
        if (!wlat_host || !dz_host || !mask0_host) return ace::fail(ACE_ERR_INVALID, "the heat-content correction needs area weights, dz and the top-level mask");
        if (c->nlev < 1 || c->nlev > MAXL) return ace::fail(ACE_ERR_INVALID, "the heat-content correction supports 1 .. " + std::to_string(MAXL) + " levels");
        if (!(c->timestep_seconds > 0)) return ace::fail(ACE_ERR_INVALID, "timestep required");
    }
    auto h = std::make_unique<ace_ocean_phys>();
    OceanParams& P = h->P;
    std::memset(&P, 0, sizeof(P));
    P.H = c->nlat; P.W = c->nlon; P.L = c->ohc ? c->nlev : 0; P.max_batch = c->max_batch;
    P.sea_ice = c->sea_ice; P.remove_negative = c->remove_negative_ocean_fraction; P.hfds = c->hfds; P.ohc = c->ohc;
    P.dt = (float)c->timestep_seconds; P.heating = (float)c->unaccounted_heating;
    const size_t HW = (size_t)c->nlat * c->nlon;
    auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
    const size_t b_w = up((size_t)c->nlat * 4), b_m = c->ohc ? up(HW * 4) : 0, b_dz = up(HW * 4 * P.L);
    const size_t b_part = c->ohc ? (size_t)c->max_batch * NQ * NBLK_MAX * 8 : 0;
    const size_t total = b_w + 2 * b_m + b_dz + b_part + 256;
    if (hipMalloc(&h->dev, total) != hipSuccess) return ace::fail(ACE_ERR_RUNTIME, "hipMalloc failed");
    char* d = static_cast<char*>(h->dev);
    bool ok = hipMemset(d, 0, total) == hipSuccess;
    if (ok && c->ohc) {
        ok = hipMemcpy(d, wlat_host, (size_t)c->nlat * 4, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(d + b_w + b_m, mask0_host, HW * 4, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(d + b_w + 2 * b_m, dz_host, HW * 4 * P.L, hipMemcpyHostToDevice) == hipSuccess;
        if (ok && mask_ohc_host) ok = hipMemcpy(d + b_w, mask_ohc_host, HW * 4, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        (void)hipFree(h->dev);
        return ace::fail(ACE_ERR_RUNTIME, "device initialisation failed");
    }
    P.wlat = reinterpret_cast<const float*>(d);
    P.mask_ohc = (c->ohc && mask_ohc_host) ? reinterpret_cast<const float*>(d + b_w) : nullptr;
    P.mask0 = reinterpret_cast<const float*>(d + b_w + b_m);
    P.dz = reinterpret_cast<const float*>(d + b_w + 2 * b_m);
    P.part = reinterpret_cast<double*>(d + b_w + 2 * b_m + b_dz);
    *out = h.release();
    return ACE_OK;
}

extern "C" void ace_ocean_phys_destroy(ace_ocean_phys* h) {
    if (!h) return;
    if (h->dev) (void)hipFree(h->dev);
    delete h;
}

extern "C" int ace_ocean_phys_launches(const ace_ocean_phys* h, long* o1, long* o2) {
    if (!h || !o1 || !o2) return ace::fail(ACE_ERR_INVALID, "null argument");
    *o1 = h->o1;
    *o2 = h->o2;
    return ACE_OK;
}

extern "C" int ace_ocean_phys_apply(ace_ocean_phys* h, const ace_ocean_fields* f, int batch, void* stream) {
    if (!h || !f) return ace::fail(ACE_ERR_INVALID, "null argument");
    const OceanParams& P = h->P;
    if (batch < 1 || batch > P.max_batch) return ace::fail(ACE_ERR_INVALID, "batch outside [1, max_batch]");
    if (f->npositive < 0 || f->npositive > ACE_OCEAN_MAX_POSITIVE || f->nzero < 0 || f->nzero > ACE_OCEAN_MAX_ZERO)
        return ace::fail(ACE_ERR_INVALID, "too many force-positive / zero-where-ice-free fields");
    auto has = [](const ace_phys_plane& p) { return p.p != nullptr; };
    for (int i = 0; i < f->npositive; ++i) if (!has(f->positive[i])) return ace::fail(ACE_ERR_INVALID, "a force-positive field is missing");
    if (P.sea_ice) {
        if (!has(f->sif) || (P.remove_negative && !has(f->reb_land))) return ace::fail(ACE_ERR_INVALID, "sea-ice fraction correction: a required field is missing");
        for (int i = 0; i < f->nzero; ++i) if (!has(f->zero[i])) return ace::fail(ACE_ERR_INVALID, "a zero-where-ice-free field is missing");
    }
    if (P.hfds && !(has(f->hfds) && has(f->in_land) && has(f->in_sif) && has(f->in_sst) && has(f->dlw) && has(f->ulw) && has(f->dsw) &&
                    has(f->usw) && has(f->lhf) && has(f->shf) && has(f->precip) && (!f->hfds_total_area || has(f->f_ssf))))
        return ace::fail(ACE_ERR_INVALID, "surface energy flux correction: a required field is missing");
    if (P.ohc) {
        for (int k = 0; k < P.L; ++k)
            if (!has(f->thetao[k]) || !has(f->thetao_in[k])) return ace::fail(ACE_ERR_INVALID, "heat-content correction: a thetao level is missing");
        if (!has(f->f_ssf) || f->flux_source < 0 || f->flux_source > 3) return ace::fail(ACE_ERR_INVALID, "heat-content correction: bad flux source");
        if (f->flux_source <= 1 && !has(f->hfds)) return ace::fail(ACE_ERR_INVALID, "heat-content correction: the output heat flux is missing");
        if (f->flux_source >= 2 && !has(f->in_flux)) return ace::fail(ACE_ERR_INVALID, "heat-content correction: the input heat flux is missing");
        if (f->flux_source == 3 && !has(f->in_ssf)) return ace::fail(ACE_ERR_INVALID, "heat-content correction: the input sea-surface fraction is missing");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long HW = (long)P.H * P.W;
    int nblk = (int)((HW + NT - 1) / NT);
    if (nblk > NBLK_MAX) nblk = NBLK_MAX;
    dim3 grid((unsigned)nblk, (unsigned)batch), block(NT);
    const bool o1 = f->npositive > 0 || P.sea_ice || P.hfds || P.ohc;
    if (o1) {
        hipLaunchKernelGGL(ocean_o1, grid, block, 0, s, P, *f, nblk);
        if (hipGetLastError() != hipSuccess) return ace::fail(ACE_ERR_RUNTIME, "ocean O1 launch failed");
        ++h->o1;
    }
    if (P.ohc) {
        hipLaunchKernelGGL(ocean_o2, grid, block, 0, s, P, *f, nblk);
        if (hipGetLastError() != hipSuccess) return ace::fail(ACE_ERR_RUNTIME, "ocean O2 launch failed");
        ++h->o2;
    }
    return ACE_OK;
}
