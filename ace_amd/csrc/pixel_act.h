// The activation of the exact-fp32 per-pixel kernels (pixel_mlp.hip, disco.hip), one wording for both.  ACT is one of
// ACE_PIXEL_MLP_ACT_* (include/ace_sfno.h; ACE_DISCO_ACT_* are the same numbers).
//   NONE  v
//   RELU  v < 0 ? +0 : v           torch.relu: NaN stays NaN, -0 stays -0
//   GELU  0.5 v (1 + erf(v / sqrt 2))   nn.GELU(), the erf form with libm's erff - not the fitted erf of the fp16 engines
//   SILU  v / (1 + exp(-v))        nn.SiLU()
// GELU and SiLU are held to torch's own fp32 error, not to bits: erff and expf are this toolchain's.  NaN stays NaN in both.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ace_sfno.h"

template <int ACT>
__device__ __forceinline__ float pixel_act(float v) {
    if (ACT == ACE_PIXEL_MLP_ACT_RELU) return v < 0.0f ? 0.0f : v;
    if (ACT == ACE_PIXEL_MLP_ACT_GELU) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
    if (ACT == ACE_PIXEL_MLP_ACT_SILU) return v / (1.0f + expf(-v));
    return v;
}

__device__ __forceinline__ float pixel_act_rt(int act, float v) {
    switch (act) {
        case ACE_PIXEL_MLP_ACT_RELU: return pixel_act<ACE_PIXEL_MLP_ACT_RELU>(v);
        case ACE_PIXEL_MLP_ACT_GELU: return pixel_act<ACE_PIXEL_MLP_ACT_GELU>(v);
        case ACE_PIXEL_MLP_ACT_SILU: return pixel_act<ACE_PIXEL_MLP_ACT_SILU>(v);
        default: return v;
    }
}
