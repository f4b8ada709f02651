// The evaluator's ensemble metrics at one step of a window (fme/ace/aggregator/one_step/ensemble.py:74-173 on fme/core/ensemble.py:4-44):
// per pixel the almost-fair CRPS, the ensemble-mean squared error and the ensemble variance of every name, averaged over the initial
// conditions, added to four persistent fp64 maps.  The reference materialises a (B, E (E - 1) / 2, H, W) tensor of member pairs per
// name and then runs three reductions over it and the window, per name; here one call covers all names and every plane is read once.
//   ensemble_step  workgroup (chunk, plane j) owns NT * NPIX pixels of plane j, thread i the NPIX pixels from (chunk * NT + i) * NPIX.
//                  For each initial condition a thread loads the E member values of its pixels into registers (the kernel is
//                  instantiated per member-count bucket EMAX and fully unrolled over it; n_members is uniform over the grid, so
//                  the e < E predicates are scalar branches and the register array is never indexed at run time), forms the mean,
//                  streams the E target planes past it for |g - y| and (m - y)^2, then walks the member pairs in registers.  The
//                  largest bucket holds 2 pixels per thread (8-byte loads where the planes allow), the others 4 (16-byte loads).
// Each pixel is owned by one thread: no atomics, no host synchronisation, no allocation; two identical runs are bitwise identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "diag_common.h"

namespace {

constexpr int MAX_MEMBERS = ACE_DIAG_ENSEMBLE_MAX_MEMBERS;

struct EnsArgs {
    const float* const* gen;
    const long* gen_strides;
    const float* const* target;
    const long* target_strides;
    const int* rows;
    double* maps;            // this slot's [4][nrows][hw]
    int* seen;               // this slot's [nrows]
    double pair_weight;
    int nrows, t, n_ic, E;
    long HW;
};

// Whether load_pix<2> may read 8 bytes at once: every plane of a field with sample stride sb and step stride st starts 8-byte aligned
// and holds an even number of pixels (p is even, so p + 1 < HW wherever p < HW).
#define ENS_VEC2_OK(base, HW, sb, st) \
    (((HW) & 1) == 0 && (reinterpret_cast<uintptr_t>(base) & 7u) == 0 && ((sb) & 1) == 0 && ((st) & 1) == 0)

// NPIX consecutive pixels from p < HW of a plane of HW pixels; 0 past its end.  vec: one 16-byte (NPIX 4) or 8-byte (NPIX 2) load
template <int NPIX>
__device__ __forceinline__ void load_pix(float (&v)[NPIX], const float* s, long p, long HW, bool vec) {
    if constexpr (NPIX == 4) {
        const float4 x = load4(s, p, HW, vec);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
        static_assert(NPIX == 2, "4 or 2 pixels per thread");
        if (vec) {
            const float2 x = *reinterpret_cast<const float2*>(s + p);
            v[0] = x.x; v[1] = x.y;
        } else {
            v[0] = s[p];
            v[1] = p + 1 < HW ? s[p + 1] : 0.f;
        }
    }
}

template <int EMAX, int NPIX>
__global__ __launch_bounds__(NT) void ensemble_step_kernel(EnsArgs a) {
#pragma clang fp contract(off)
    const int j = blockIdx.y;
    const float* gb = a.gen[j];
    const float* tb = a.target[j];
    const int r = a.rows[j];
    if (gb == nullptr || tb == nullptr || r < 0 || r >= a.nrows) return;
    const long HW = a.HW, p = ((long)blockIdx.x * NT + threadIdx.x) * NPIX;
    if (p >= HW) return;
    const long gsb = a.gen_strides[2 * j], gst = a.gen_strides[2 * j + 1];
    const long tsb = a.target_strides[2 * j], tst = a.target_strides[2 * j + 1];
    const bool gvec = NPIX == 4 ? DIAG_VEC4_OK(gb, HW, gsb, gst) : ENS_VEC2_OK(gb, HW, gsb, gst);
    const bool tvec = NPIX == 4 ? DIAG_VEC4_OK(tb, HW, tsb, tst) : ENS_VEC2_OK(tb, HW, tsb, tst);
    const int E = a.E;
    const double dE = (double)E, npairs = (double)(E * (E - 1) / 2);
    gb += (long)a.t * gst;
    tb += (long)a.t * tst;
    double crps[NPIX], mse[NPIX], var[NPIX];
#pragma unroll
    for (int k = 0; k < NPIX; ++k) crps[k] = mse[k] = var[k] = 0.0;
    bool any = false;
    for (int i = 0; i < a.n_ic; ++i) {
        const long b0 = (long)i * E;
        float g[EMAX][NPIX];
#pragma unroll
        for (int e = 0; e < EMAX; ++e) {
            if (e < E) {
                load_pix<NPIX>(g[e], gb + (b0 + e) * gsb, p, HW, gvec);
            } else {
#pragma unroll
                for (int k = 0; k < NPIX; ++k) g[e][k] = 0.f;
            }
        }
        double m[NPIX], ab[NPIX], q[NPIX], v[NPIX], s[NPIX];
#pragma unroll
        for (int k = 0; k < NPIX; ++k) m[k] = ab[k] = q[k] = v[k] = s[k] = 0.0;
#pragma unroll
        for (int e = 0; e < EMAX; ++e)
            if (e < E) {
#pragma unroll
                for (int k = 0; k < NPIX; ++k) m[k] += (double)g[e][k];
            }
#pragma unroll
        for (int k = 0; k < NPIX; ++k) m[k] = m[k] / dE;
#pragma unroll
        for (int e = 0; e < EMAX; ++e)
            if (e < E) {
                float y[NPIX];                           // the target planes are streamed, not held
                load_pix<NPIX>(y, tb + (b0 + e) * tsb, p, HW, tvec);
#pragma unroll
                for (int k = 0; k < NPIX; ++k) {
                    const double gd = (double)g[e][k], yd = (double)y[k];
                    ab[k] += fabs(gd - yd);
                    const double dq = m[k] - yd, dv = gd - m[k];
                    q[k] += dq * dq;
                    v[k] += dv * dv;
                    any = any || (p + k < HW && y[k] == y[k]);
                }
            }
#pragma unroll
        for (int e = 0; e < EMAX; ++e)
            if (e + 1 < E) {
#pragma unroll
                for (int f = e + 1; f < EMAX; ++f)
                    if (f < E) {
#pragma unroll
                        for (int k = 0; k < NPIX; ++k) s[k] += fabs((double)g[e][k] - (double)g[f][k]);
                    }
            }
#pragma unroll
        for (int k = 0; k < NPIX; ++k) {
            const double pw = a.pair_weight * (s[k] / npairs);
            crps[k] += ab[k] / dE - pw;
            mse[k] += q[k] / dE;
            var[k] += v[k] / (dE - 1.0);
        }
    }
    const double dn = (double)a.n_ic;
    double* out = a.maps + (long)r * HW + p;
    const long plane = (long)a.nrows * HW;
#pragma unroll
    for (int k = 0; k < NPIX; ++k)
        if (p + k < HW) {
            const double c = crps[k] / dn, q = mse[k] / dn, v = var[k] / dn;
            const double spread = v / dE;
            out[k] += c;
            out[plane + k] += sqrt(q);
            out[2 * plane + k] += q - spread;
            out[3 * plane + k] += v;
        }
    if (any) a.seen[r] = 1;                              // the same constant from every writer
}

template <int EMAX, int NPIX>
void launch(const EnsArgs& a, int nplanes, hipStream_t s) {
    const long per = (long)NT * NPIX;
    const dim3 grid((unsigned)((a.HW + per - 1) / per), nplanes);
    hipLaunchKernelGGL((ensemble_step_kernel<EMAX, NPIX>), grid, dim3(NT), 0, s, a);
}

}  // namespace

extern "C" int ace_diag_ensemble_step(const float* const* gen, const long* gen_strides, const float* const* target,
                                      const long* target_strides, const int* rows, double* maps, int* seen, int nrows, int slot,
                                      int nslots, double pair_weight, int t, int nplanes, int n_ic, int n_members, int steps, long hw,
                                      void* stream) {
    if (nplanes < 0 || nplanes > 65535) return ace::fail(ACE_ERR_INVALID, "ace_diag_ensemble_step: need 0 <= nplanes <= 65535");
    if (n_members < 2 || n_members > MAX_MEMBERS)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_ensemble_step: need 2 <= n_members <= " + std::to_string(MAX_MEMBERS) +
                                               " (the members of a pixel stay in registers)");
    if (steps < 1 || t < 0 || t >= steps) return ace::fail(ACE_ERR_INVALID, "ace_diag_ensemble_step: need 0 <= t < steps");
    if (nslots < 1 || slot < 0 || slot >= nslots)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_ensemble_step: need 0 <= slot < nslots");
    if (n_ic < 1) return ace::fail(ACE_ERR_INVALID, "ace_diag_ensemble_step: need n_ic >= 1");
    if (hw < 1 || (hw + 2L * NT - 1) / (2L * NT) > 2147483647L || nrows < 1)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_ensemble_step: need 1 <= hw <= 512 * (2^31 - 1), nrows >= 1");
    if (nplanes == 0) return ACE_OK;
    if (!gen || !gen_strides || !target || !target_strides || !rows || !maps || !seen)
        return ace::fail(ACE_ERR_INVALID, "ace_diag_ensemble_step: null argument");
    EnsArgs a;
    a.gen = gen; a.gen_strides = gen_strides; a.target = target; a.target_strides = target_strides; a.rows = rows;
    a.maps = maps + (long)slot * 4 * nrows * hw;
    a.seen = seen + (long)slot * nrows;
    a.pair_weight = pair_weight;
    a.nrows = nrows; a.t = t; a.n_ic = n_ic; a.E = n_members; a.HW = hw;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_members <= 4) launch<4, 4>(a, nplanes, s);
    else if (n_members <= 8) launch<8, 4>(a, nplanes, s);
    else if (n_members <= 16) launch<16, 4>(a, nplanes, s);
    else launch<MAX_MEMBERS, 2>(a, nplanes, s);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}
