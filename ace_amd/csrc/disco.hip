// The DISCO convolution on the sphere (fme/core/disco/_convolution.py; the first layer of AnkurLocalNet, the filter of LocalNet's
// "disco" blocks) as ONE launch in exact fp32: y = act(mix(w, z) + embed) with z[c][k][ho][wo] = sum_e psi[ho][e][k]
// x[c][hi_e][(wi_e + wo) mod W].  The statement is in include/ace_sfno.h ("DISCO convolution"); the plan of a launch - stage
// windows, point offsets, the unit list - in disco_units.h.
//
// A workgroup owns one unit (sample, output row ho, pixels wo0 .. wo0 + npix - 1, groups g0 .. g0 + ng - 1):
//   stage   per pass `cc` of the unit's channels: the band rows hi0 .. hi0 + nrows - 1, columns (wo0 + wlo + j) mod W, j < ncol,
//           into LDS - a wave per (channel, row), lanes along j, the one modulo of the kernel.
//   z       thread (channel c = tid / 16 + 16 i, pixel p = tid % 16) walks the row's points in table order with K accumulators:
//           one LDS read stage[c][off_e + p] per K fmaf, off_e and the K psi values uniform across the wave (scalar loads).  The
//           K sums go to LDS as rows j = c' * K + k of the group's [Jp][16] operand; rows J .. Jp - 1 are +0.
//   mix     wave w takes the (group, tile of 16 outputs) pairs w, w + 4, ...: D[o][p] += A[o][j] B[j][p] on
//           v_mfma_f32_16x16x4_f32, four j per instruction in ascending order - a k-ordered fmaf chain from +0 - with the
//           weight fragment read from the blob (64 consecutive floats per instruction) and B from LDS (64 consecutive floats).
//           Lane (p, q) holds outputs 16 t + 4 q + r, r = 0 .. 3, of pixel p: embedding, activation, one store each.
// z never leaves the chip.  No atomics, no allocation, no host synchronisation in forward.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ace_sfno.h"
#include "disco_units.h"
#include "errors.h"
#include "pixel_act.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 64 * ACE_DISCO_WAVES;
constexpr int RUN = ACE_DISCO_RUN;
static_assert(RUN == 16, "the pixel side of v_mfma_f32_16x16x4_f32");

typedef float f32x4 __attribute__((ext_vector_type(4)));
// the tables of a handle are written before any launch and never after: read through the constant address space, a wave-uniform
// address becomes a scalar load (a plain load after a barrier is a vector load of 64 equal addresses)
typedef const __attribute__((address_space(4))) float* const_f32;
typedef const __attribute__((address_space(4))) int* const_i32;

struct DArgs {
    int H, W, K, in_chans, out_chans, gs, opg, J, Jp, nto, nj4, act, has_embed;
    const int* rows;      // [H][8]: hi0, nrows, wlo, ncol, cs, p0, npts, -
    const int* off;       // [P]
    const float* psi;     // [P][KP], KP = K rounded up to 4: a point's values are 16-byte aligned
    const int* units;     // [nunits][8]: ho, wo0, npix, g0, ng, cc, -, -
    const float* wfrag;   // [groups][nto][nj4][64]
};

struct Disco {
    DArgs a;
    void* blob = nullptr;
    long nunits = 0, cost_max = 0, cost_total = 0, lds_bytes = 0;
};

template <int K>
__global__ __launch_bounds__(NT) void disco_kernel(DArgs a, const float* __restrict__ x, const float* __restrict__ embed,
                                                   float* __restrict__ y, int batch) {
    extern __shared__ __attribute__((aligned(16))) float dc_lds[];
    constexpr int KP = (K + 3) & ~3;
    const int u = blockIdx.x / batch, b = blockIdx.x - u * batch;
    const int* U = a.units + 8 * u;
    const int ho = U[0], wo0 = U[1], npix = U[2], g0 = U[3], ng = U[4], cc = U[5];
    const int* R = a.rows + 8 * ho;
    const int hi0 = R[0], nrows = R[1], wlo = R[2], ncol = R[3], cs = R[4], p0 = R[5], npts = R[6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gs = a.gs, J = a.J, Jp = a.Jp, W = a.W;
    const long HW = (long)a.H * W;
    float* stage = dc_lds;
    float* zl = dc_lds + (long)cc * cs;
    const int nc = ng * gs;
    const float* xb = x + ((long)b * a.in_chans + (long)g0 * gs) * HW;

    if (Jp != J) {                                                       // the padding rows of every group's operand: +0
        const int per = (Jp - J) * RUN;
        for (int i = tid; i < ng * per; i += NT) {
            const int gi = i / per, rem = i - gi * per;
            zl[(gi * Jp + J) * RUN + rem] = 0.0f;
        }
    }
    const int wstart = (wo0 + wlo) % W;
    const int p = tid & 15;
    for (int cbase = 0; cbase < nc; cbase += cc) {
        const int ncc = min(cc, nc - cbase);
        __syncthreads();                                                 // the last pass's reads of the stage are done
        for (int pr = wave; pr < ncc * nrows; pr += ACE_DISCO_WAVES) {
            const int c = pr / nrows, r = pr - c * nrows;
            const float* src = xb + (long)(cbase + c) * HW + (long)(hi0 + r) * W;
            float* dst = stage + (long)c * cs + r * ncol;
            for (int j = lane; j < ncol; j += 64) dst[j] = src[(wstart + j) % W];
        }
        __syncthreads();
        for (int c = tid >> 4; c < ncc; c += NT / 16) {
            float z[K];
#pragma unroll
            for (int k = 0; k < K; ++k) z[k] = 0.0f;
            const float* s = stage + (long)c * cs + p;
            const_i32 oe = (const_i32)(uintptr_t)(a.off + p0);
            const_f32 pe = (const_f32)(uintptr_t)(a.psi + (long)p0 * KP);
#pragma unroll 4
            for (int e = 0; e < npts; ++e) {
                const float xv = s[oe[e]];
#pragma unroll
                for (int k = 0; k < K; ++k) z[k] = __builtin_fmaf(pe[e * KP + k], xv, z[k]);
            }
            const int cl = cbase + c, gi = cl / gs, cp = cl - gi * gs;
            float* zd = zl + ((long)gi * Jp + cp * K) * RUN + p;
#pragma unroll
            for (int k = 0; k < K; ++k) zd[k * RUN] = z[k];
        }
    }
    __syncthreads();
    const int q = lane >> 4, pl = lane & 15, wo = wo0 + pl;
    for (int t = wave; t < ng * a.nto; t += ACE_DISCO_WAVES) {
        const int gi = t / a.nto, to = t - gi * a.nto, g = g0 + gi;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* wf = a.wfrag + ((long)g * a.nto + to) * a.nj4 * 64 + lane;
        const float* zb = zl + (long)gi * Jp * RUN + lane;               // row 4 j4 + q, pixel pl: (4 j4 + q) * 16 + pl = 64 j4 + lane
#pragma unroll 4
        for (int j4 = 0; j4 < a.nj4; ++j4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[j4 * 64], zb[j4 * 64], acc, 0, 0, 0);
        if (pl < npix) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ol = RUN * to + 4 * q + r;
                if (ol >= a.opg) continue;
                const long o = (long)g * a.opg + ol;
                float v = acc[r];
                if (a.has_embed) v = v + embed[(o * a.H + ho) * W + wo];
                y[(((long)b * a.out_chans + o) * a.H + ho) * W + wo] = pixel_act_rt(a.act, v);
            }
        }
    }
}

typedef void (*disco_fn)(DArgs, const float*, const float*, float*, int);
disco_fn kernel_of(int K) {
    switch (K) {
        case 1: return disco_kernel<1>;
        case 4: return disco_kernel<4>;
        case 9: return disco_kernel<9>;
        case 16: return disco_kernel<16>;
        case 25: return disco_kernel<25>;
        default: return nullptr;
    }
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

extern "C" int ace_disco_create(int H, int W, int K, const long* row_off, const int* hi, const int* wi, const float* vals,
                                const float* w_dev, int in_chans, int out_chans, int groups, int act, int has_embed, void* stream,
                                void** handle) {
    if (!handle) return ace::fail(ACE_ERR_INVALID, "ace_disco_create: null handle pointer");
    *handle = nullptr;
    if (!row_off || !hi || !wi || !vals || !w_dev) return ace::fail(ACE_ERR_INVALID, "ace_disco_create: null argument");
    if (!kernel_of(K))
        return ace::fail(ACE_ERR_INVALID, "ace_disco_create: K must be kernel_size^2 with kernel_size in 1 .. 5 (ACE_DISCO_MAX_K = " +
                                           std::to_string(ACE_DISCO_MAX_K) + "), got " + std::to_string(K));
    if (act != ACE_DISCO_ACT_NONE && act != ACE_DISCO_ACT_RELU && act != ACE_DISCO_ACT_GELU && act != ACE_DISCO_ACT_SILU)
        return ace::fail(ACE_ERR_INVALID, "ace_disco_create: act must be one of ACE_DISCO_ACT_*");
    ace_disco::Plan plan;
    const std::string why = ace_disco::make_plan(H, W, K, in_chans, out_chans, groups, row_off, hi, wi, plan);
    if (!why.empty()) return ace::fail(ACE_ERR_INVALID, "ace_disco_create: " + why);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int gs = plan.gs, opg = plan.opg, J = plan.J, nto = (opg + RUN - 1) / RUN, nj4 = plan.Jp / 4;
    const long P = row_off[H];
    const int KP = (K + 3) & ~3;
    // the caller's weight, read back once (the one synchronisation of a handle's life)
    std::vector<float> w((size_t)out_chans * gs * K);
    hipError_t e = hipMemcpyAsync(w.data(), w_dev, w.size() * sizeof(float), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ace::fail(ACE_ERR_RUNTIME, std::string("ace_disco_create: reading the weight: ") + hipGetErrorString(e));
    const size_t o_rows = 0, o_off = align16(o_rows + (size_t)H * 8 * 4), o_units = align16(o_off + (size_t)P * 4),
                 o_psi = align16(o_units + plan.units.size() * 8 * 4), o_w = align16(o_psi + (size_t)P * KP * 4),
                 total = align16(o_w + (size_t)groups * nto * nj4 * 64 * 4);
    std::vector<char> blob(total, 0);
    int* rows = reinterpret_cast<int*>(blob.data() + o_rows);
    for (int ho = 0; ho < H; ++ho) {
        const ace_disco::Row& r = plan.rows[ho];
        const int rec[8] = {r.hi0, r.nrows, r.wlo, r.ncol, r.cs, r.p0, r.npts, 0};
        std::memcpy(rows + 8 * ho, rec, sizeof rec);
    }
    std::memcpy(blob.data() + o_off, plan.off.data(), (size_t)P * 4);
    static_assert(sizeof(ace_disco::Unit) == 32, "a unit is eight ints");
    std::memcpy(blob.data() + o_units, plan.units.data(), plan.units.size() * sizeof(ace_disco::Unit));
    for (long e2 = 0; e2 < P; ++e2) std::memcpy(blob.data() + o_psi + (size_t)e2 * KP * 4, vals + (size_t)e2 * K, (size_t)K * 4);
    float* wf = reinterpret_cast<float*>(blob.data() + o_w);
    for (int g = 0; g < groups; ++g)
        for (int to = 0; to < nto; ++to)
            for (int j4 = 0; j4 < nj4; ++j4)
                for (int lane = 0; lane < 64; ++lane) {
                    const int ol = RUN * to + (lane & 15), j = 4 * j4 + (lane >> 4);
                    float v = 0.0f;
                    if (j >= J) v = -0.0f;                              // meets a +0 row of z: an identity of the chain
                    else if (ol < opg) v = w[((size_t)g * opg + ol) * J + j];
                    wf[(((size_t)g * nto + to) * nj4 + j4) * 64 + lane] = v;
                }
    Disco* h = new Disco();
    e = hipMalloc(&h->blob, total);
    if (e == hipSuccess) e = hipMemcpyAsync(h->blob, blob.data(), total, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                  // `blob` is pageable host memory and dies here
    h->lds_bytes = plan.lds_floats * 4;
    if (e == hipSuccess)                                                // the same bound for every handle: a later one must not lower it
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel_of(K)), hipFuncAttributeMaxDynamicSharedMemorySize,
                                ACE_DISCO_STAGE_BYTES + ACE_DISCO_Z_BYTES);
    if (e != hipSuccess) {
        if (h->blob) (void)hipFree(h->blob);
        delete h;
        return ace::fail(ACE_ERR_RUNTIME, std::string("ace_disco_create: uploading the tables: ") + hipGetErrorString(e));
    }
    const char* d = static_cast<const char*>(h->blob);
    DArgs& a = h->a;
    a.H = H; a.W = W; a.K = K; a.in_chans = in_chans; a.out_chans = out_chans; a.gs = gs; a.opg = opg; a.J = J; a.Jp = plan.Jp;
    a.nto = nto; a.nj4 = nj4; a.act = act; a.has_embed = has_embed ? 1 : 0;
    a.rows = reinterpret_cast<const int*>(d + o_rows);
    a.off = reinterpret_cast<const int*>(d + o_off);
    a.units = reinterpret_cast<const int*>(d + o_units);
    a.psi = reinterpret_cast<const float*>(d + o_psi);
    a.wfrag = reinterpret_cast<const float*>(d + o_w);
    h->nunits = (long)plan.units.size();
    h->cost_max = plan.cost.empty() ? 0 : plan.cost.front();
    for (long c : plan.cost) h->cost_total += c;
    *handle = h;
    return ACE_OK;
}

extern "C" void ace_disco_destroy(void* handle) {
    Disco* h = static_cast<Disco*>(handle);
    if (!h) return;
    if (h->blob) (void)hipFree(h->blob);
    delete h;
}

extern "C" int ace_disco_info(void* handle, long* out4) {
    const Disco* h = static_cast<const Disco*>(handle);
    if (!h || !out4) return ace::fail(ACE_ERR_INVALID, "ace_disco_info: null argument");
    out4[0] = h->nunits; out4[1] = h->cost_max; out4[2] = h->cost_total; out4[3] = h->lds_bytes;
    return ACE_OK;
}

extern "C" int ace_disco_forward(void* handle, const float* x, const float* embed, float* y, int batch, void* stream) {
    const Disco* h = static_cast<const Disco*>(handle);
    if (!h) return ace::fail(ACE_ERR_INVALID, "ace_disco_forward: null handle");
    if (!x || !y) return ace::fail(ACE_ERR_INVALID, "ace_disco_forward: null argument");
    if (batch < 1) return ace::fail(ACE_ERR_INVALID, "ace_disco_forward: need batch >= 1");
    if (h->a.has_embed && !embed)
        return ace::fail(ACE_ERR_INVALID, "ace_disco_forward: the handle was created with an embedding: embed must not be NULL");
    if (h->nunits * batch > 2147483647L)
        return ace::fail(ACE_ERR_INVALID, "ace_disco_forward: batch * units exceeds 2^31 - 1 workgroups");
    if (!h->a.has_embed) embed = nullptr;
    hipLaunchKernelGGL(kernel_of(h->a.K), dim3((unsigned)(h->nunits * batch)), dim3(NT), (size_t)h->lds_bytes,
                       static_cast<hipStream_t>(stream), h->a, x, embed, y, batch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ace::fail(ACE_ERR_RUNTIME, std::string("ace_disco_forward: ") + hipGetErrorString(e));
    return ACE_OK;
}
