// denoise_math.h — exp_m, the one exponential of the a-trous denoiser's edge-stopping weight (rt_denoise.hip, include/rt_mi355x.h:
// rt_denoise). Host and device compile the same operations, and tests/test_denoise.py restates them op for op in numpy float32.
//
// The paper's four Gaussian factors exp(-a) exp(-b) exp(-c) exp(-d) are one exp(-(a + b + c + d)): a tap takes one exponential. It is
// built from R1 operations only: no libm, no v_exp_f32, whose result the host could not reproduce.
//   n = rint(x * log2(e))                       the exponent; rint is exact
//   r = (x - n * LN2_HI) - n * LN2_LO           Cody-Waite reduction: LN2_HI has 16 significant bits, so n * LN2_HI is exact for |n| < 256
//   p = Horner(r) of the degree-7 Taylor polynomial, coefficients 1/7! .. 1/2!, 1, 1, one mul and one add per step (no fma)
//   exp_m(x) = p * 2^n                          2^n built from its bits: exact, and normal for every n the cutoff lets through
// Properties (checked by tests/test_denoise.py against float64 exp on a dense sample):
//   within 4 ulp of exp on [-87, 0] (1.2 ulp measured); exp_m(-0) == exp_m(0) == 1 exactly (n = 0, r = -0 or 0, p = 1);
//   exp_m(x) = 0 for x < -87 and for NaN (kCutoff: exp(-87) = 1.6e-38 is still normal, so every result above the cutoff is a normal float).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define RT_HD __host__ __device__ inline
#else
#define RT_HD inline
#endif

namespace rt {

constexpr float kExpCutoff = -87.0f;
constexpr float kLog2E = 1.44269504088896341f;
constexpr float kLn2Hi = 0.693145751953125f;       // 0x3F317200
constexpr float kLn2Lo = 1.42860676533018690e-06f; // ln 2 - kLn2Hi

RT_HD float exp_m(float x) {
    if (!(x >= kExpCutoff)) return 0.0f;
    const float n = __builtin_rintf(x * kLog2E);
    const float r = (x - n * kLn2Hi) - n * kLn2Lo;
    float p = 1.0f / 5040.0f;
    p = p * r + 1.0f / 720.0f;
    p = p * r + 1.0f / 120.0f;
    p = p * r + 1.0f / 24.0f;
    p = p * r + 1.0f / 6.0f;
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    int32_t e = (int32_t)n;
    e = e < -126 ? -126 : (e > 127 ? 127 : e); // (only x > 0, outside the denoiser's use, reaches the upper clamp)
    return p * __builtin_bit_cast(float, (uint32_t)(e + 127) << 23);
}

} // namespace rt
