// pow2_scale.h — the power-of-two block scale of the split-f16 operands
// (common.h "fp16x3"), on the exponent field.  No HIP dependency: host code and
// tests include this header as it is.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define MJRL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MJRL_HD inline
#endif

namespace mjrl {

constexpr int SPLIT_HR = 15;   // block max -> [2^(SPLIT_HR-1), 2^SPLIT_HR)

MJRL_HD uint32_t f32_bits(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return u;
}
MJRL_HD float bits_f32(uint32_t u) {
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

// Power-of-two scale for a block whose max |value| is M: returns s = 2^(15-E) with
// M * s in [2^14, 2^15) and sets inv = 1 / s = 2^(E-15), E = frexp's exponent of M
// (s = inv = 1 for M <= 0, M >= 3.0e38f, Inf and NaN; blocks below 2^-111,
// subnormal ones included, keep s = 2^126).
//
// Both results are pure exponent fields, so they are built from M's: with e the
// biased exponent (E = e - 126), clamped below at 15 (E >= -111), inv has the field
// e - 14 and s the field 268 - e, both in 1 .. 254 (normal) for every e in 15 .. 254.
// The range test is one unsigned compare on the bits: 0 < bits < bits(3.0e38f)
// holds exactly for the positive finite M < 3.0e38f (a set sign bit, Inf and NaN
// all lie above).  The same bits as the frexpf / ldexpf formulation for every
// float (tests/test_pow2_scale.py walks all 2^32).
MJRL_HD float pow2_scale(float M, float& inv) {
    constexpr uint32_t EXP = 0x7F800000u, LIM = 0x7F61B1E6u;   // LIM = bits(3.0e38f)
    constexpr uint32_t EMIN = 15u << 23, ONE = 141u << 23;     // field 141: inv = s = 1
    const uint32_t u = f32_bits(M);
    uint32_t t = u & EXP;
    t = t < EMIN ? EMIN : t;
    t = u - 1u < LIM - 1u ? t : ONE;
    inv = bits_f32(t - (14u << 23));
    return bits_f32((268u << 23) - t);
}

}  // namespace mjrl
