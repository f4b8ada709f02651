// Host-side numbers every f16x3 operand preparation derives from a weight: its norms and the power-of-two scale its fp16 hi / lo
// split is taken at.  Plain C++ (no HIP), shared by capi.hip, healpix.hip, strip_pack.h and tests/emul/weight_prep_emul.cpp.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>

#include "range_exponent.h"   // the exponent of DYNAMIC operands (planes a kernel rescales from a range slot): one clamp for host and device

namespace ace {

// 2^(top - e) with maxabs = f 2^e, f in [0.5, 1): maxabs * scale lands in [2^(top - 1), 2^top).  1 for zero, infinite or NaN input.
// top = 10 for static operands (hi and lo parts stay in fp16's normal range), 12 for what the kernels rescale per launch.
inline float pow2_scale(float maxabs, int top) {
    int e = 0;
    if (maxabs > 0.f && std::isfinite(maxabs)) { (void)std::frexp(maxabs, &e); e = top - e; }
    return std::ldexp(1.0f, e);
}

// absmax: max |w|.  winf: max row sum of |w|, rounded up (|W x| <= winf max|x| bounds a convolution's output).
struct WeightNorms { float absmax = 0.f, winf = 0.f; };
// host: rows x cols at pitch ld (the padded library copy: ld = pitch; a caller's dense weight: ld = cols)
inline WeightNorms weight_norms(const float* host, int rows, int cols, long ld) {
    WeightNorms nm;
    for (int r = 0; r < rows; ++r) {
        double rs = 0.0;
        for (int c = 0; c < cols; ++c) {
            const float v = host[(size_t)r * ld + c];
            nm.absmax = std::max(nm.absmax, std::fabs(v));
            rs += std::fabs((double)v);
        }
        nm.winf = std::max(nm.winf, (float)(rs * (1.0 + 1e-6)));
    }
    return nm;
}

}  // namespace ace
