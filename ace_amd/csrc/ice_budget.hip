// Sea-ice budget corrector of the stepper as gfx950 kernels: IceBudgetCorrectionConfig (fme/core/corrector/ice.py), applied to
// the denormalised output planes of one step, in place.  The arithmetic per pixel is stated in include/ace_sfno.h ("Sea-ice
// budget corrector") and follows the reference op for op in fp64.
//
// The reference guards each of its up to three stages per variable with `if torch.any(mask)`, and a stage that runs also
// repairs sign violations at pixels outside its mask: a pixel's result depends on tensor-wide flags, each of which depends on
// the results under the earlier ones.  No host readback, so per variable two launches:
//   flags  every pixel evaluates its stage masks under each hypothesis about the earlier flags - F1, F2[a1], F3[a1][a2]: 7
//          bits - which are OR-reduced over the wave, the workgroup (LDS) and the tensor (one atomicOr per workgroup that has a
//          bit to add; an OR is idempotent and order-independent, so no workgroup waits for another)
//   apply  reads the 7 bits, resolves a1 -> a2 = F2[a1] -> a3 = F3[a1][a2] and recomputes its pixel once along that path;
//          variable 0 also leaves one byte per pixel, "the fp64 corrected mass == 0", which later variables' stage 3 reads
// A pass reads 4 planes and writes 4 (apply) of ~0.26 MB at 1 degree: launch-, not bandwidth-bound.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/ace_sfno.h"
#include "errors.h"

// every fp64 operation rounds on its own, as the reference's torch ops do (old + dt * (...) must not become an fma)
#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int NBLK_MAX = 2048;   // workgroups per sample (grid-stride beyond)

struct Terms { double s, k, t; };

__device__ __forceinline__ double new_mass(double o, const Terms& x) { return o + ((x.s + x.k) + x.t); }

// _rebalance of constrain_budgets (ice.py:69-106); `m` is this pixel's stage mask, `mass` is 0 where m is false
__device__ __forceinline__ Terms rebalance(const Terms& x, bool m, double mass, double sign) {
    const bool nz_s = fabs(x.s) > 0.0, nz_k = fabs(x.k) > 0.0, nz_t = fabs(x.t) > 0.0;
    const double n = ((nz_s ? 1.0 : 0.0) + (nz_k ? 1.0 : 0.0)) + (nz_t ? 1.0 : 0.0);
    const double share = (m && n > 0.0) ? mass / (n < 1.0 ? 1.0 : n) : 0.0;
    double r_s = (m && nz_s) ? share : 0.0;
    double r_k = (m && nz_k) ? share : 0.0;
    double r_t = (m && nz_t) ? share : 0.0;
    if (m && n == 0.0) r_t = mass;
    double tmp = x.k + sign * r_k;
    const double ko = tmp > 0.0 ? tmp : 0.0;
    r_k = r_k - ko;
    r_t = r_t + ko;
    tmp = x.s + sign * r_s;
    const double so = tmp < 0.0 ? tmp : 0.0;
    r_s = r_s - sign * so;
    r_t = r_t + sign * so;
    Terms y;
    y.s = x.s + sign * r_s;
    y.k = x.k + sign * r_k;
    y.t = x.t + sign * r_t;
    return y;
}

__device__ __forceinline__ Terms stage1(double o, const Terms& x) {
    const double nm = new_mass(o, x);
    const bool m = nm < 0.0;
    return rebalance(x, m, m ? -nm : 0.0, 1.0);
}
__device__ __forceinline__ Terms stage2(double o, const Terms& x) {
    const double nm = new_mass(o, x);
    const bool m = nm > 1.0;
    return rebalance(x, m, m ? nm - 1.0 : 0.0, -1.0);
}
__device__ __forceinline__ Terms stage3(double o, const Terms& x, bool ice_zero) {
    const double nm = new_mass(o, x);
    const bool m = ice_zero && nm > 0.0;
    return rebalance(x, m, m ? nm : 0.0, -1.0);
}

// flag word of one variable: bit 0 = F1, bit 1 + a1 = F2[a1], bit 3 + 2 * a1 + a2 = F3[a1][a2]
__device__ __forceinline__ unsigned pixel_flags(double o, const Terms& x0, bool area, bool masked, bool ice_zero) {
    unsigned bits = new_mass(o, x0) < 0.0 ? 1u : 0u;
    if (!area && !masked) return bits;
    for (int a1 = 0; a1 < 2; ++a1) {
        const Terms x1 = a1 ? stage1(o, x0) : x0;
        if (area && new_mass(o, x1) > 1.0) bits |= 1u << (1 + a1);
        if (!masked) continue;
        for (int a2 = 0; a2 < (area ? 2 : 1); ++a2) {
            const Terms x2 = a2 ? stage2(o, x1) : x1;
            if (ice_zero && new_mass(o, x2) > 0.0) bits |= 1u << (3 + 2 * a1 + a2);
        }
    }
    return bits;
}

template <int V> struct Vec;
template <> struct Vec<1> { float v[1]; };
template <> struct alignas(16) Vec<4> { float v[4]; };

template <int V> __device__ __forceinline__ Vec<V> ldv(const ace_phys_plane& f, int b, long px) {
    return *reinterpret_cast<const Vec<V>*>(f.p + (long)b * f.stride + px);
}
template <int V> __device__ __forceinline__ void stv(const ace_phys_plane& f, int b, long px, const Vec<V>& x) {
    *reinterpret_cast<Vec<V>*>(f.p + (long)b * f.stride + px) = x;
}

template <int V> struct Bytes;
template <> struct Bytes<1> { unsigned char v[1]; };
template <> struct alignas(4) Bytes<4> { unsigned char v[4]; };

// ---- flags: V consecutive pixels per thread -------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(NT) void ice_flags(ace_ice_var X, double dt, long HW, unsigned* flag, const unsigned char* ice_zero, int nblk) {
    const int b = blockIdx.y;
    const bool area = X.area_mode != 0, masked = X.masked != 0;
    unsigned bits = 0;
    for (long px = ((long)blockIdx.x * NT + threadIdx.x) * V; px < HW; px += (long)nblk * NT * V) {
        const Vec<V> o = ldv<V>(X.old_mass, b, px), s = ldv<V>(X.source, b, px), k = ldv<V>(X.sink, b, px), t = ldv<V>(X.transport, b, px);
        Bytes<V> z = {};
        if (masked) z = *reinterpret_cast<const Bytes<V>*>(ice_zero + (long)b * HW + px);
        for (int i = 0; i < V; ++i) {
            Terms x;
            x.s = (double)s.v[i] * dt;
            x.k = (double)k.v[i] * dt;
            x.t = (double)t.v[i] * dt;
            bits |= pixel_flags((double)o.v[i], x, area, masked, masked && z.v[i] != 0);
        }
    }
    for (int off = 32; off > 0; off >>= 1) bits |= __shfl_xor(bits, off, 64);
    __shared__ unsigned red[NT / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned all = (red[0] | red[1]) | (red[2] | red[3]);
        if (all) atomicOr(flag, all);
    }
}

// ---- apply ----------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(NT) void ice_apply(ace_ice_var X, double dt, long HW, const unsigned* flag, unsigned char* ice_zero, int write_zero,
                                                int nblk) {
    const int b = blockIdx.y;
    const bool area = X.area_mode != 0, masked = X.masked != 0;
    const unsigned F = *flag;
    const int a1 = F & 1u;
    const int a2 = area ? (F >> (1 + a1)) & 1u : 0;
    const int a3 = masked ? (F >> (3 + 2 * a1 + a2)) & 1u : 0;
    for (long px = ((long)blockIdx.x * NT + threadIdx.x) * V; px < HW; px += (long)nblk * NT * V) {
        const Vec<V> o = ldv<V>(X.old_mass, b, px);
        Vec<V> s = ldv<V>(X.source, b, px), k = ldv<V>(X.sink, b, px), t = ldv<V>(X.transport, b, px), mass;
        Bytes<V> z = {};
        if (masked) z = *reinterpret_cast<const Bytes<V>*>(ice_zero + (long)b * HW + px);
        for (int i = 0; i < V; ++i) {
            const double od = (double)o.v[i];
            Terms x;
            x.s = (double)s.v[i] * dt;
            x.k = (double)k.v[i] * dt;
            x.t = (double)t.v[i] * dt;
            if (a1) x = stage1(od, x);
            if (a2) x = stage2(od, x);
            if (a3) x = stage3(od, x, z.v[i] != 0);
            const double bs = x.s / dt, bk = x.k / dt, bt = x.t / dt;
            const double m = od + dt * ((bs + bk) + bt);
            s.v[i] = (float)bs;
            k.v[i] = (float)bk;
            t.v[i] = (float)bt;
            mass.v[i] = (float)m;
            if (write_zero) z.v[i] = m == 0.0 ? 1 : 0;
        }
        stv<V>(X.source, b, px, s);
        stv<V>(X.sink, b, px, k);
        stv<V>(X.transport, b, px, t);
        stv<V>(X.mass, b, px, mass);
        if (write_zero) *reinterpret_cast<Bytes<V>*>(ice_zero + (long)b * HW + px) = z;
    }
}

std::atomic<long> g_flags{0}, g_apply{0}, g_clears{0};

}  // namespace

extern "C" long ace_ice_budget_scratch_bytes(int batch, long hw) {
    if (batch < 1 || hw < 1) return 0;
    return ACE_ICE_FLAG_BYTES + (((long)batch * hw + 15) & ~15L);
}

extern "C" int ace_ice_budget_launches(long* flags, long* apply, long* clears) {
    if (flags) *flags = g_flags.load();
    if (apply) *apply = g_apply.load();
    if (clears) *clears = g_clears.load();
    return ACE_OK;
}

extern "C" int ace_ice_budget_apply(const ace_ice_fields* f, double timestep, int batch, int H, int W, void* scratch, void* stream) {
    if (!f) return ace::fail(ACE_ERR_INVALID, "null fields");
    if (f->nvars < 0 || f->nvars > ACE_ICE_MAX_VARS) return ace::fail(ACE_ERR_INVALID, "nvars outside 0 .. " + std::to_string(ACE_ICE_MAX_VARS));
    if (!(timestep > 0.0) || !std::isfinite(timestep)) return ace::fail(ACE_ERR_INVALID, "the timestep must be a positive finite number");
    if (batch < 1 || batch > 65535) return ace::fail(ACE_ERR_INVALID, "batch outside 1 .. 65535");
    if (H < 1 || W < 1) return ace::fail(ACE_ERR_INVALID, "H and W must be at least 1");
    if (f->nvars == 0) return ACE_OK;
    if (!scratch) return ace::fail(ACE_ERR_INVALID, "null scratch");
    if (reinterpret_cast<uintptr_t>(scratch) % 16) return ace::fail(ACE_ERR_INVALID, "the scratch must be 16-byte aligned");
    const long HW = (long)H * W;
    bool vec = HW % 4 == 0;
    for (int v = 0; v < f->nvars; ++v) {
        const ace_ice_var& X = f->var[v];
        const ace_phys_plane* planes[5] = {&X.old_mass, &X.source, &X.sink, &X.transport, &X.mass};
        for (const ace_phys_plane* p : planes) {
            if (!p->p) return ace::fail(ACE_ERR_INVALID, "variable " + std::to_string(v) + ": a plane is missing");
            if (batch > 1 && p->stride < HW) return ace::fail(ACE_ERR_INVALID, "variable " + std::to_string(v) + ": a per-sample stride is below H * W");
            if (reinterpret_cast<uintptr_t>(p->p) % 4) return ace::fail(ACE_ERR_INVALID, "variable " + std::to_string(v) + ": a plane is not 4-byte aligned");
            vec = vec && reinterpret_cast<uintptr_t>(p->p) % 16 == 0 && (batch == 1 || p->stride % 4 == 0);
        }
        if (v == 0 && X.masked) return ace::fail(ACE_ERR_INVALID, "variable 0 provides the ice mask and cannot be masked");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned* flags = static_cast<unsigned*>(scratch);
    unsigned char* ice_zero = static_cast<unsigned char*>(scratch) + ACE_ICE_FLAG_BYTES;
    if (hipMemsetAsync(flags, 0, ACE_ICE_FLAG_BYTES, s) != hipSuccess) return ace::fail(ACE_ERR_RUNTIME, "clearing the flags failed");
    ++g_clears;
    const int V = vec ? 4 : 1;
    const long work = (HW + V - 1) / V;
    int nblk = (int)((work + NT - 1) / NT);
    if (nblk > NBLK_MAX) nblk = NBLK_MAX;
    dim3 grid((unsigned)nblk, (unsigned)batch), block(NT);
    bool need_zero = false;
    for (int v = 1; v < f->nvars; ++v) need_zero = need_zero || f->var[v].masked;
    for (int v = 0; v < f->nvars; ++v) {
        const ace_ice_var& X = f->var[v];
        const int write_zero = v == 0 && need_zero;
        if (vec) hipLaunchKernelGGL(ice_flags<4>, grid, block, 0, s, X, timestep, HW, flags + v, ice_zero, nblk);
        else hipLaunchKernelGGL(ice_flags<1>, grid, block, 0, s, X, timestep, HW, flags + v, ice_zero, nblk);
        if (hipGetLastError() != hipSuccess) return ace::fail(ACE_ERR_RUNTIME, "ice flags launch failed");
        ++g_flags;
        if (vec) hipLaunchKernelGGL(ice_apply<4>, grid, block, 0, s, X, timestep, HW, flags + v, ice_zero, write_zero, nblk);
        else hipLaunchKernelGGL(ice_apply<1>, grid, block, 0, s, X, timestep, HW, flags + v, ice_zero, write_zero, nblk);
        if (hipGetLastError() != hipSuccess) return ace::fail(ACE_ERR_RUNTIME, "ice apply launch failed");
        ++g_apply;
    }
    return ACE_OK;
}
