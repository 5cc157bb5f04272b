// nx_tonemap.h — Tonemap, LinearToGamma, ToColorUInt (PathTracer.cu:37-62; Utils/Utils.h:51-54): the ONE text every kernel that
// writes an RGBA8 image goes through (accumulate_kernel, compose_kernel, the denoiser's kernels in nx_aov.hip).
#pragma once

#include "nx_math.h"

namespace nxd {

NXD uint32_t tonemap_rgba8(f3 c)
{
    const float v[3] = {c.x, c.y, c.z};
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float x = v[k] * 0.6f;
        x = clampf((x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f), 0.0f, 1.0f);
        x = (float)nxf_pow((double)x, 0.45454545454);
        x = clampf(x, 0.0f, 1.0f);
        out |= (uint32_t)(uint8_t)(x * 255.0f) << (8 * k);
    }
    return out | (255u << 24);
}

}  // namespace nxd
