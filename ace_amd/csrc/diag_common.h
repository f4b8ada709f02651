// What the diagnostics kernels (diag.hip, hist.hip, regress.hip, calendar.hip, ensemble.hip, timeseg.hip, region.hip, video.hip) share: the pixel partition of a plane, the guarded 4-pixel load,
// the wave reductions, and the library's error report (errors.h).  A new diag kernel starts from here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ace_sfno.h"
#include "errors.h"

// Whether load4 may read 16 bytes at once: a row of HW pixels, or every plane of a field with sample stride sb and step stride st,
// starts 16-byte aligned.  Macros, not inline functions: the function form changed the generated code of all three files.
#define DIAG_VEC4_ROW_OK(row, HW) (((HW) & 3) == 0 && (reinterpret_cast<uintptr_t>(row) & 15u) == 0)
#define DIAG_VEC4_OK(base, HW, sb, st) (DIAG_VEC4_ROW_OK(base, HW) && ((sb) & 3) == 0 && ((st) & 3) == 0)

namespace {

// Workgroup (chunk, plane) owns CHUNK pixels of the plane, thread i the PIX pixels from chunk * CHUNK + i * PIX.  The sizes of the
// partial buffers (ace_diag_*_partial_doubles, ace_diag_hist_scratch_bytes) follow from these.
constexpr int NT = 256;              // four wave64s
constexpr int WAVES = NT / 64;
constexpr int PIX = 4;               // pixels per thread
constexpr int CHUNK = NT * PIX;      // pixels per workgroup

inline long nchunk_for(long hw) { return (hw + CHUNK - 1) / CHUNK; }

__device__ __forceinline__ double wave_sum(double v) {
    // xor butterfly: every lane ends with the same sum (fp add is commutative)
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// pixels p .. p + 3 of a plane of HW pixels; 0 past its end
__device__ __forceinline__ float4 load4(const float* s, long p, long HW, bool vec) {
    if (vec && p + 3 < HW) return *reinterpret_cast<const float4*>(s + p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p < HW) v.x = s[p];
    if (p + 1 < HW) v.y = s[p + 1];
    if (p + 2 < HW) v.z = s[p + 2];
    if (p + 3 < HW) v.w = s[p + 3];
    return v;
}

}  // namespace
