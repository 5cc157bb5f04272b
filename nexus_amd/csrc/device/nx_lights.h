// nx_lights.h — reading the light table (nx_device.h LightEntry; built by nx_lights.hip): the pick of the light sample and the
// probability lookup of the MIS weight.  Shared by the POWER-mode material kernels (nx_wavefront.h) and the pick hook.
// Below them the same two for the light tree (LightNode; the TREE instances of the material launch and of the medium's scatter kernel).
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

// ---- the light tree (nxhip_set_light_importance, NXHIP_LIGHT_IMPORTANCE_POSITION; the rule's one statement: include/nexus_hip.h) ----------
// Every operation below is one binary32 rounding, in the order the header gives (no fmaf; contraction is off): the pick and the
// probability lookup are pinned bit for bit from a numpy restatement (tests/light_tree_reference.py).

constexpr float kLightTreeUMax = 0.99999994f;  // 1 - 2^-24: a rescaled u stays in [0, 1)

// I = w / max(max(d2, r2), FLT_MIN) of a node with the box (lo, hi) at p; w == 0: 0, whatever the box holds (an empty slot's is +inf / -inf)
NXD float light_tree_importance(const float4 a, const float4 b, const f3 p)  // a = (lo, w), b = (hi, entry)
{
    const float hx = (b.x - a.x) * 0.5f, hy = (b.y - a.y) * 0.5f, hz = (b.z - a.z) * 0.5f;
    const float r2 = (hx * hx + hy * hy) + hz * hz;
    const float dx = p.x - (a.x + b.x) * 0.5f, dy = p.y - (a.y + b.y) * 0.5f, dz = p.z - (a.z + b.z) * 0.5f;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const float I = a.w / fmaxf(fmaxf(d2, r2), 1.17549435e-38f);
    return a.w == 0.0f ? 0.0f : I;
}

// the two children of node k: one aligned 64-byte load
struct LightNodePair {
    float4 l0, l1, r0, r1;
};
NXD LightNodePair light_tree_children(const NX_G LightNode* nodes, const uint32_t k)
{
    const NX_G float4* q = (const NX_G float4*)(nodes + 2u * (size_t)k);
    return LightNodePair{q[0], q[1], q[2], q[3]};
}

// The descent from the root with ONE random number.  false: no light sample (both children of some node have the importance 0 — a tree
// whose weights sum to nothing, or a point so far away that d2 overflows).  entry: the table's entry of the leaf reached; prob: the
// product of the branch probabilities, root to leaf.
NXD bool light_tree_pick(const NX_G LightNode* nodes, const uint32_t leaves, const f3 p, float u, uint32_t& entry, float& prob)
{
    float P = 1.0f;
    uint32_t k = 1u, e = 0u;
    if (leaves == 1u) {  // the root is the leaf
        const NX_G float4* q = (const NX_G float4*)(nodes + 1);
        if (q[0].w == 0.0f) return false;
        e = __float_as_uint(q[1].w);
    }
    while (k < leaves) {
        const LightNodePair c = light_tree_children(nodes, k);
        const float a = light_tree_importance(c.l0, c.l1, p), b = light_tree_importance(c.r0, c.r1, p);
        if (a == 0.0f && b == 0.0f) return false;
        const float s = a + b, qa = a / s, qb = b / s;
        if (b == 0.0f || (a != 0.0f && u < qa)) {
            P *= qa;
            u = fminf(u / qa, kLightTreeUMax);
            k = 2u * k;
            e = __float_as_uint(c.l1.w);
        } else {
            P *= qb;
            u = fmaxf(fminf((u - qa) / qb, kLightTreeUMax), 0.0f);
            k = 2u * k + 1u;
            e = __float_as_uint(c.r1.w);
        }
    }
    entry = e;
    prob = P;
    return true;
}

// The probability the descent from p has of reaching leaf slot `slot`: the ancestors root to leaf, the same a, b, s and the same factor
// as the pick — the pick's P bit for bit.  0: the sampler cannot reach the slot from p.
NXD float light_tree_prob(const NX_G LightNode* nodes, const uint32_t leaves, const f3 p, const uint32_t slot)
{
    float P = 1.0f;
    const uint32_t leaf = leaves + slot;
    if (leaves == 1u) return ((const NX_G float4*)(nodes + 1))[0].w == 0.0f ? 0.0f : 1.0f;
    for (int d = 31 - __clz(leaves) - 1; d >= 0; d--) {
        const uint32_t child = leaf >> d;
        const LightNodePair c = light_tree_children(nodes, child >> 1);
        const float a = light_tree_importance(c.l0, c.l1, p), b = light_tree_importance(c.r0, c.r1, p);
        if (a == 0.0f && b == 0.0f) return 0.0f;
        const float s = a + b;
        P *= (child & 1u) ? b / s : a / s;
    }
    return P;
}

}  // namespace nxd
