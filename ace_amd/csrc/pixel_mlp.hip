// A chain of 1 x 1 convolutions (the LandNet family, fme/ace/models/land/land_net.py: Conv2d(1 x 1) + ReLU per hidden width, an
// optional positional embedding after the first activation, a last Conv2d(1 x 1)) as ONE launch per forward, in exact fp32, with
// the hidden activations never leaving the registers.
//
// v_mfma_f32_16x16x4_f32 computes D[o][p] = C[o][p] + sum_g A[o][g] B[g][p] as the fmaf chain g = 0, 1, 2, 3 (one rounding per
// product).  Lane l = 16 g + p holds A[o = p][g] and B[g][p] in one register each, and D[o = 4 g + r][p] in register r: a lane
// that owns pixel p of a 16-pixel tile holds, of the 16 output channels of a tile t, the channels 16 t + 4 g + r, r = 0 .. 3.
// Register r of such a tile is therefore already the B operand of a following MFMA whose four k slots are the channels
// 16 t + 4 g + r, g = 0 .. 3 - no lane movement, no LDS - provided the weight fragment of that MFMA holds W[o][16 t + 4 g + r] at
// lane (o, g).  create() lays the weights out in that order once; every layer (the first one included: the input is loaded
// straight into the accumulator layout) then sums k in the order "for tile t, for r, for g: k = 16 t + 4 g + r".
//
//   weights   one device blob per handle: per layer the bias padded to whole tiles, then the fragments [to][ti][r][lane].
//             A k beyond the layer's input width holds -0.0f and meets an activation forced to +0.0f: the product is -0 and
//             x + (-0) == x for every x, signed zeros and NaN included, so the padding is an identity of the chain.
//   narrow    every width <= 64: a wave carries 4 pixel tiles (64 pixels; lane (p, g) owns pixels 4 p .. 4 p + 3 of them, one
//             per tile, so that a plane is read and written with one 16-byte access per lane where hw and the three bases allow
//             it - decided once for the whole launch - and with four 4-byte ones otherwise); the blob (28 KB at 30 -> 64 -> 64
//             -> 10) is copied into LDS once per workgroup, which then loops over its pixel units.
//   wide      widths up to 256: 1 pixel tile per wave and up to 16 channel tiles in registers.  Correct, not tuned.
//   streamed  a blob over ACE_PIXEL_MLP_LDS_BYTES (eight layers of width 64 are 133 KB, one 256 x 256 layer 256 KB) is not
//             copied: both kernels then read bias and fragments from global memory at the same offsets, 256 contiguous bytes
//             per fragment and wave, served by L2 after the first workgroup.  Same arithmetic, same bits.
// No atomics, no allocation, no host synchronisation in forward: capturable, and two runs are bitwise identical.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ace_sfno.h"
#include "errors.h"
#include "pixel_act.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 64 * ACE_PIXEL_MLP_WAVES;
constexpr int TILE = ACE_PIXEL_MLP_TILE;
constexpr int LDS_BYTES = ACE_PIXEL_MLP_LDS_BYTES;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct PMArgs {
    int n_layers, embed_layer;
    int embed_first;                           // the embedding is added before the activation of its layer (create2)
    int dims[ACE_PIXEL_MLP_MAX_LAYERS + 1];
    int act[ACE_PIXEL_MLP_MAX_LAYERS];
    int woff[ACE_PIXEL_MLP_MAX_LAYERS];        // floats into the blob: fragments of layer l
    int boff[ACE_PIXEL_MLP_MAX_LAYERS];        // floats into the blob: padded bias of layer l
    int blob_floats;                           // a multiple of 4
};

struct PixelMlp {
    PMArgs a;
    bool soft = false;                         // see pixel_mlp_unit
    float* blob = nullptr;
    int width = 0;                             // the largest of dims
};

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// planes [c][hw] at `base` -> the accumulator layout: v[t][j][r] = plane 16 t + 4 g + r at this lane's pixel of tile j.
// Absent channels and pixels past hw give +0.
template <int MAXT, int NPT, bool VEC>
__device__ __forceinline__ void load_tile(const float* base, long hw, long pix, int nch, int t, int g, f32x4 (&v)[NPT]) {
#pragma unroll
    for (int j = 0; j < NPT; ++j) v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = TILE * t + 4 * g + r;
        if (c >= nch) continue;
        const float* s = base + (long)c * hw + pix;
        if (VEC) {                                                      // NPT == 4: the four tiles' pixels are consecutive
            if (pix < hw) {
                const float4 q = *reinterpret_cast<const float4*>(s);
                v[0][r] = q.x; v[1 % NPT][r] = q.y; v[2 % NPT][r] = q.z; v[3 % NPT][r] = q.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NPT; ++j)
                if (pix + j < hw) v[j][r] = s[j];
        }
    }
}

// SOFT: some layer is GELU / SiLU or adds its embedding before the activation (create2).  The chains that none / ReLU with the
// embedding after the activation describe run the SOFT == false instantiations: the code they ran before those options existed.
template <int MAXT, int NPT, bool VEC, bool SOFT>
__device__ __forceinline__ void pixel_mlp_unit(const PMArgs& a, const float* W, const float* xb, const float* embed, float* yb,
                                               long hw, long pix, int lane) {
    const int g = lane >> 4;
    f32x4 cur[MAXT][NPT];
    {
        const int nt = (a.dims[0] + TILE - 1) / TILE;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            if (t < nt) {
                load_tile<MAXT, NPT, VEC>(xb, hw, pix, a.dims[0], t, g, cur[t]);
            } else {
#pragma unroll
                for (int j = 0; j < NPT; ++j) cur[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    for (int l = 0; l < a.n_layers; ++l) {
        const int din = a.dims[l], dout = a.dims[l + 1];
        const int nti = (din + TILE - 1) / TILE, nto = (dout + TILE - 1) / TILE;
        const float* wl = W + a.woff[l] + lane;
        const float* bl = W + a.boff[l] + 4 * g;
        const int act = a.act[l];
        const bool relu = act != 0, emb = l == a.embed_layer;
        const bool emb_first = SOFT && emb && a.embed_first;
        f32x4 nxt[MAXT][NPT];
#pragma unroll
        for (int to = 0; to < MAXT; ++to) {
            if (to < nto) {
                f32x4 ev[NPT];
                if (emb) load_tile<MAXT, NPT, VEC>(embed, hw, pix, dout, to, g, ev);
                const float4 bq = *reinterpret_cast<const float4*>(bl + TILE * to);
#pragma unroll
                for (int j = 0; j < NPT; ++j) nxt[to][j] = f32x4{bq.x, bq.y, bq.z, bq.w};
                const float* wt = wl + (long)to * nti * 256;
#pragma unroll
                for (int ti = 0; ti < MAXT; ++ti) {
                    if (ti < nti) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float wa = wt[(ti * 4 + r) * 64];
#pragma unroll
                            for (int j = 0; j < NPT; ++j)
                                nxt[to][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa, cur[ti][j][r], nxt[to][j], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < NPT; ++j) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = nxt[to][j][r];
                        if (SOFT) {
                            if (emb_first) v = v + ev[j][r];
                            v = pixel_act_rt(act, v);
                            if (emb && !emb_first) v = v + ev[j][r];
                        } else {
                            if (relu) v = pixel_act<ACE_PIXEL_MLP_ACT_RELU>(v);   // torch.relu: NaN stays NaN, -0 stays -0
                            if (emb) v = v + ev[j][r];
                        }
                        if (TILE * to + 4 * g + r >= dout) v = 0.0f;    // a padded channel is +0, whatever 0 * Inf made of it
                        nxt[to][j][r] = v;
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < NPT; ++j) nxt[to][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
#pragma unroll
            for (int j = 0; j < NPT; ++j) cur[t][j] = nxt[t][j];
        }
    }
    const int dlast = a.dims[a.n_layers];
    const int nt = (dlast + TILE - 1) / TILE;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        if (t >= nt) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = TILE * t + 4 * g + r;
            if (c >= dlast) continue;
            float* d = yb + (long)c * hw + pix;
            if (VEC) {
                if (pix < hw)
                    *reinterpret_cast<float4*>(d) = make_float4(cur[t][0][r], cur[t][1 % NPT][r], cur[t][2 % NPT][r], cur[t][3 % NPT][r]);
            } else {
#pragma unroll
                for (int j = 0; j < NPT; ++j)
                    if (pix + j < hw) d[j] = cur[t][j][r];
            }
        }
    }
}

// unit u = (sample, run of 16 NPT pixels); wave w of workgroup k takes the units 4 k + w, + 4 gridDim.x, ...
template <int MAXT, int NPT, bool LDSW, bool SOFT>
__global__ __launch_bounds__(NT) void pixel_mlp_kernel(PMArgs a, const float* __restrict__ blob, const float* __restrict__ x,
                                                       const float* __restrict__ embed, float* __restrict__ y, long hw,
                                                       long units_per_image, long nunits) {
    extern __shared__ float4 pm_lds[];
    const float* W = blob;
    if (LDSW) {
        const float4* src = reinterpret_cast<const float4*>(blob);
        for (int i = threadIdx.x; i < a.blob_floats / 4; i += NT) pm_lds[i] = src[i];
        __syncthreads();
        W = reinterpret_cast<const float*>(pm_lds);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // one decision for the launch: every (sample, plane) base is then 16-byte aligned and a lane's four pixels are all in or all out
    const bool vec = NPT == 4 && (hw & 3) == 0 && aligned16(x) && aligned16(y) && (embed == nullptr || aligned16(embed));
    const int din = a.dims[0], dlast = a.dims[a.n_layers];
    for (long u = (long)blockIdx.x * ACE_PIXEL_MLP_WAVES + wave; u < nunits; u += (long)gridDim.x * ACE_PIXEL_MLP_WAVES) {
        const long b = u / units_per_image;
        const long pix = (u - b * units_per_image) * (TILE * NPT) + (long)(lane & 15) * NPT;
        const float* xb = x + b * din * hw;
        float* yb = y + b * dlast * hw;
        if (vec)
            pixel_mlp_unit<MAXT, NPT, NPT == 4, SOFT>(a, W, xb, embed, yb, hw, pix, lane);
        else
            pixel_mlp_unit<MAXT, NPT, false, SOFT>(a, W, xb, embed, yb, hw, pix, lane);
    }
}

template <int MAXT, int NPT, bool SOFT>
int launch(const PixelMlp* h, const float* x, const float* embed, float* y, int batch, long hw, hipStream_t st) {
    const long wp = (long)TILE * NPT;
    const long upi = (hw + wp - 1) / wp;
    const long nunits = upi * batch;
    long nwg = (nunits + ACE_PIXEL_MLP_WAVES - 1) / ACE_PIXEL_MLP_WAVES;
    if (nwg > ACE_PIXEL_MLP_MAX_GRID) nwg = ACE_PIXEL_MLP_MAX_GRID;
    const size_t bytes = (size_t)h->a.blob_floats * sizeof(float);
    if (bytes <= (size_t)LDS_BYTES)
        hipLaunchKernelGGL((pixel_mlp_kernel<MAXT, NPT, true, SOFT>), dim3((unsigned)nwg), dim3(NT), bytes, st, h->a, h->blob, x, embed, y,
                           hw, upi, nunits);
    else
        hipLaunchKernelGGL((pixel_mlp_kernel<MAXT, NPT, false, SOFT>), dim3((unsigned)nwg), dim3(NT), 0, st, h->a, h->blob, x, embed, y, hw,
                           upi, nunits);
    ACE_HIP_TRY(hipGetLastError());
    return ACE_OK;
}

}  // namespace

extern "C" int ace_pixel_mlp_create2(int n_layers, const int* dims, const float* const* w_dev, const float* const* bias_dev,
                                     const int* act, int embed_layer, int embed_before_act, void* stream, void** handle) {
    if (!handle) return ace::fail(ACE_ERR_INVALID, "ace_pixel_mlp_create: null handle pointer");
    *handle = nullptr;
    if (n_layers < 1 || n_layers > ACE_PIXEL_MLP_MAX_LAYERS)
        return ace::fail(ACE_ERR_INVALID, "ace_pixel_mlp_create: need 1 <= n_layers <= ACE_PIXEL_MLP_MAX_LAYERS (" +
                                           std::to_string(ACE_PIXEL_MLP_MAX_LAYERS) + ")");
    if (!dims || !w_dev || !act) return ace::fail(ACE_ERR_INVALID, "ace_pixel_mlp_create: null argument");
    for (int l = 0; l <= n_layers; ++l)
        if (dims[l] < 1 || dims[l] > ACE_PIXEL_MLP_MAX_WIDTH)
            return ace::fail(ACE_ERR_INVALID, "ace_pixel_mlp_create: need 1 <= dims[l] <= ACE_PIXEL_MLP_MAX_WIDTH (" +
                                               std::to_string(ACE_PIXEL_MLP_MAX_WIDTH) + ")");
    for (int l = 0; l < n_layers; ++l) {
        if (!w_dev[l]) return ace::fail(ACE_ERR_INVALID, "ace_pixel_mlp_create: null weight");
        if (act[l] != ACE_PIXEL_MLP_ACT_NONE && act[l] != ACE_PIXEL_MLP_ACT_RELU && act[l] != ACE_PIXEL_MLP_ACT_GELU &&
            act[l] != ACE_PIXEL_MLP_ACT_SILU)
            return ace::fail(ACE_ERR_INVALID, "ace_pixel_mlp_create2: act must be one of ACE_PIXEL_MLP_ACT_*");
    }
    if (embed_layer < -1 || embed_layer >= n_layers)
        return ace::fail(ACE_ERR_INVALID, "ace_pixel_mlp_create: need -1 <= embed_layer < n_layers");
    if (embed_before_act != 0 && embed_before_act != 1)
        return ace::fail(ACE_ERR_INVALID, "ace_pixel_mlp_create2: embed_before_act must be 0 or 1");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PixelMlp* h = new PixelMlp();
    PMArgs& a = h->a;
    a = PMArgs{};
    a.n_layers = n_layers;
    a.embed_layer = embed_layer;
    a.embed_first = embed_layer >= 0 ? embed_before_act : 0;
    h->soft = a.embed_first != 0;
    for (int l = 0; l < n_layers; ++l)
        if (act[l] == ACE_PIXEL_MLP_ACT_GELU || act[l] == ACE_PIXEL_MLP_ACT_SILU) h->soft = true;
    long total = 0;
    for (int l = 0; l <= n_layers; ++l) {
        a.dims[l] = dims[l];
        if (dims[l] > h->width) h->width = dims[l];
    }
    for (int l = 0; l < n_layers; ++l) {
        const int nti = (dims[l] + TILE - 1) / TILE, nto = (dims[l + 1] + TILE - 1) / TILE;
        a.act[l] = act[l];
        a.boff[l] = (int)total;
        total += (long)nto * TILE;
        a.woff[l] = (int)total;
        total += (long)nto * nti * 256;
    }
    a.blob_floats = (int)total;
    // the caller's weights, read back once per parameter version (the one synchronisation of a handle's life)
    std::vector<float> blob((size_t)total, 0.0f), w, bias;
    for (int l = 0; l < n_layers; ++l) {
        const int K = dims[l], O = dims[l + 1];
        const int nti = (K + TILE - 1) / TILE, nto = (O + TILE - 1) / TILE;
        w.assign((size_t)O * K, 0.0f);
        bias.assign((size_t)O, 0.0f);
        hipError_t e = hipMemcpyAsync(w.data(), w_dev[l], w.size() * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && bias_dev && bias_dev[l])
            e = hipMemcpyAsync(bias.data(), bias_dev[l], bias.size() * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            delete h;
            return ace::fail(ACE_ERR_RUNTIME, std::string("ace_pixel_mlp_create: reading the weights: ") + hipGetErrorString(e));
        }
        float* bl = blob.data() + a.boff[l];
        for (int o = 0; o < O; ++o) bl[o] = bias[o];
        float* wl = blob.data() + a.woff[l];
        for (int to = 0; to < nto; ++to)
            for (int ti = 0; ti < nti; ++ti)
                for (int r = 0; r < 4; ++r)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int o = TILE * to + (lane & 15), k = TILE * ti + 4 * (lane >> 4) + r;
                        float v = 0.0f;
                        if (k >= K) v = -0.0f;                          // the identity of the chain against a +0 activation
                        else if (o < O) v = w[(size_t)o * K + k];
                        wl[(((size_t)to * nti + ti) * 4 + r) * 64 + lane] = v;
                    }
    }
    hipError_t e = hipMalloc(&h->blob, blob.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(h->blob, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                  // `blob` is pageable host memory and dies here
    if (e != hipSuccess) {
        if (h->blob) (void)hipFree(h->blob);
        delete h;
        return ace::fail(ACE_ERR_RUNTIME, std::string("ace_pixel_mlp_create: uploading the weights: ") + hipGetErrorString(e));
    }
    *handle = h;
    return ACE_OK;
}

extern "C" int ace_pixel_mlp_create(int n_layers, const int* dims, const float* const* w_dev, const float* const* bias_dev,
                                    const int* act, int embed_layer, void* stream, void** handle) {
    // its contract as it stood: the two activations it knew; GELU and SiLU come through create2
    if (handle && act && n_layers >= 1 && n_layers <= ACE_PIXEL_MLP_MAX_LAYERS)
        for (int l = 0; l < n_layers; ++l)
            if (act[l] != ACE_PIXEL_MLP_ACT_NONE && act[l] != ACE_PIXEL_MLP_ACT_RELU) {
                *handle = nullptr;
                return ace::fail(ACE_ERR_INVALID, "ace_pixel_mlp_create: act must be ACE_PIXEL_MLP_ACT_NONE or ACE_PIXEL_MLP_ACT_RELU");
            }
    return ace_pixel_mlp_create2(n_layers, dims, w_dev, bias_dev, act, embed_layer, 0, stream, handle);
}

extern "C" void ace_pixel_mlp_destroy(void* handle) {
    PixelMlp* h = static_cast<PixelMlp*>(handle);
    if (!h) return;
    if (h->blob) (void)hipFree(h->blob);
    delete h;
}

extern "C" int ace_pixel_mlp_forward(void* handle, const float* x, const float* embed, float* y, int batch, long hw, void* stream) {
    const PixelMlp* h = static_cast<const PixelMlp*>(handle);
    if (!h) return ace::fail(ACE_ERR_INVALID, "ace_pixel_mlp_forward: null handle");
    if (!x || !y) return ace::fail(ACE_ERR_INVALID, "ace_pixel_mlp_forward: null argument");
    if (batch < 1 || hw < 1) return ace::fail(ACE_ERR_INVALID, "ace_pixel_mlp_forward: need batch >= 1 and hw >= 1");
    if (h->a.embed_layer >= 0 && !embed)
        return ace::fail(ACE_ERR_INVALID, "ace_pixel_mlp_forward: the handle was created with an embedding layer: embed must not be NULL");
    if (h->a.embed_layer < 0) embed = nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    constexpr int NARROW = ACE_PIXEL_MLP_NARROW_WIDTH / ACE_PIXEL_MLP_TILE, WIDE = ACE_PIXEL_MLP_MAX_WIDTH / ACE_PIXEL_MLP_TILE;
    if (h->width <= ACE_PIXEL_MLP_NARROW_WIDTH)
        return h->soft ? launch<NARROW, ACE_PIXEL_MLP_NARROW_TILES, true>(h, x, embed, y, batch, hw, st)
                       : launch<NARROW, ACE_PIXEL_MLP_NARROW_TILES, false>(h, x, embed, y, batch, hw, st);
    return h->soft ? launch<WIDE, ACE_PIXEL_MLP_WIDE_TILES, true>(h, x, embed, y, batch, hw, st)
                   : launch<WIDE, ACE_PIXEL_MLP_WIDE_TILES, false>(h, x, embed, y, batch, hw, st);
}
