// nx_lights.h — reading the light table (nx_device.h LightEntry; built by nx_lights.hip): the pick of the light sample and the
// probability lookup of the MIS weight.  Shared by the POWER-mode material kernels (nx_wavefront.hip) and the pick hook.
#pragma once

#include "nx_device.h"
#include "nx_math.h"

namespace nxd {

// one 8-byte load for the cumulative probability and the light
NXD LightEntry light_entry(const NX_G LightEntry* table, const uint32_t i)
{
    const uint2 w = *(const NX_G uint2*)(table + i);
    return LightEntry{__uint_as_float(w.x), w.y};
}

// P(i) = cdf[i] - cdf[i - 1], cdf[-1] = 0: what the sampler and the MIS lookup both use
NXD float light_entry_prob(const NX_G LightEntry* table, const uint32_t i)
{
    const float below = i != 0u ? light_entry(table, i - 1u).cdf : 0.0f;
    return light_entry(table, i).cdf - below;
}

struct LightPick {
    uint32_t entry, light;
    float prob;
};

// The cut-point method: entry guide[floor(u * G)] is the first whose cdf exceeds floor(u * G) / G <= u, so the walk from there reaches
// min(searchsorted(cdf, u, 'right'), entries - 1) in an expected two steps or fewer.  u in [0, 1): u * G is exact (G is a power of two)
// and below G.  cdf[entries - 1] = 1 > u ends the walk; the index test beside it only keeps a table that is being misused in bounds.
NXD LightPick light_pick(const NX_G LightEntry* table, const NX_G uint32_t* guide, const uint32_t guideSize, const uint32_t entries, const float u)
{
    const uint32_t k = (uint32_t)(u * (float)guideSize);
    uint32_t i = guide[k];
    LightEntry e = light_entry(table, i);
    float below = 0.0f;
    bool walked = false;
    while (e.cdf <= u && i + 1u < entries) {
        below = e.cdf;
        walked = true;
        e = light_entry(table, ++i);
    }
    if (!walked && i != 0u) below = light_entry(table, i - 1u).cdf;
    return LightPick{i, e.light, e.cdf - below};
}

}  // namespace nxd
