// The exponent of the power-of-two scale a dynamic operand's fp16 hi / lo planes are taken at, from the bound in its range slot.
// ONE function for both sides of a plane: whoever writes planes scales by 2^e, the kernel that reads them undoes 2^e, and both
// get e here - host code included (capi.hip's operator entries; tests/emul/weight_prep_emul.cpp).  Plain C++, host and device.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define ACE_RANGE_HD __host__ __device__
#else
#define ACE_RANGE_HD
#endif

namespace ace {

constexpr int RANGE_EXPONENT_TOP = 12;      // mx 2^e lands in [2^11, 2^12)
constexpr int RANGE_EXPONENT_CLAMP = 100;   // |e| <= 100: 2^e, 2^-e and their products with a static scale stay normal floats

// e = 12 - exponent(mx) clamped to +-100; 0 for a bound that is zero, negative, NaN or >= 3.0e38.  `clamped` (optional): the clamp
// changed e, i.e. mx 2^e is NOT in [2^11, 2^12) - below about 2^-88 the planes lose low bits, above about 2^112 they keep headroom.
ACE_RANGE_HD inline int range_exponent(float mx, bool* clamped = nullptr) {
    int e = 0;
    if (mx > 0.f && mx < 3.0e38f) { (void)frexpf(mx, &e); e = RANGE_EXPONENT_TOP - e; }
    const int c = e > RANGE_EXPONENT_CLAMP ? RANGE_EXPONENT_CLAMP : (e < -RANGE_EXPONENT_CLAMP ? -RANGE_EXPONENT_CLAMP : e);
    if (clamped) *clamped = c != e;
    return c;
}

}  // namespace ace
