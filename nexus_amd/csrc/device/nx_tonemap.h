// nx_tonemap.h — Tonemap, LinearToGamma, ToColorUInt (PathTracer.cu:37-62; Utils/Utils.h:51-54): the ONE text every kernel that
// writes an RGBA8 image goes through (accumulate_kernel, compose_kernel, adaptive_accumulate_kernel, the denoiser's kernels in
// nx_aov.hip).  The CPU twin the tests compare with (orc_tonemap_rgba8) holds the same text: the two are changed together and
// agree bit for bit.
//
// The display contract, per colour channel c (tests/image_reference.py, tests/test_gpu_image_chain.py):
//   +0, -0, positive denormals                          level 0
//   finite c >= 0                                       floor(255 clip(N / D, 0, 1)^0.45454545454), x = 0.6 c, N = x (2.51 x + 0.03),
//                                                       D = x (2.43 x + 0.59) + 0.14, as a correct binary32 evaluation rounds it
//   c from the curve's clamp (about 12.07) to FLT_MAX,  level 255
//   and +inf
//   finite c < 0 whose polynomials do not overflow      the curve as it is (N / D > 1 below about -0.02: -1 displays 255)
//   NaN, -inf, c < 0 whose polynomials overflow         level 0
// Alpha is 255 whatever the colour holds; a special value in one channel leaves the other two alone.
//
// One named deviation from the reference: x is saturated at kSaturate before the polynomials.  In binary32 both N and D overflow
// once x is above about 1.2e19 (c about 1.9e19), the quotient is inf / inf = NaN and the channel would be written as 0: everything
// from the clamp to 1.9e19 white, everything brighter (+inf included) black.  A channel at or above the clamp evaluates to exactly 1
// with or without the saturation, so no bit changes below the overflow.  The comparison is false for a NaN, which goes on to the
// clamp below; that clamp is written out (not fminf / fmaxf, whose result for a NaN or a -0 is the compiler's choice) so that a
// NaN, a -0 and a negative quotient all become +0 on the device and in the CPU twin alike.
#pragma once

#include "nx_math.h"

namespace nxd {

NXD uint32_t tonemap_rgba8(f3 c)
{
    constexpr float kSaturate = 1.0e9f;  // far above the clamp (x = 7.24), far below the overflow (x = 1.2e19)
    const float v[3] = {c.x, c.y, c.z};
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float x = v[k] * 0.6f;
        x = x > kSaturate ? kSaturate : x;
        const float q = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
        x = q > 0.0f ? (q < 1.0f ? q : 1.0f) : 0.0f;
        x = (float)nxf_pow((double)x, 0.45454545454);
        x = clampf(x, 0.0f, 1.0f);
        out |= (uint32_t)(uint8_t)(x * 255.0f) << (8 * k);
    }
    return out | (255u << 24);
}

}  // namespace nxd
