// nx_texture.h — software tex2D<float4>: normalised coordinates, wrap, bilinear with 8-bit fractional
// weights, sRGB decode of RGB (256-entry LUT built at context creation) before filtering.
// gfx950 has no image/texture instructions (hipcc rejects tex2D for this target), so the reference's
// cudaTextureObject fetches (/root/reference/Nexus/src/Cuda/PathTracer/PathTracer.cu:78,295,349,401 with the
// descriptor of Assets/Texture.cpp:26-33) become plain loads from linear RGBA8 buffers.
#pragma once

#include "nx_device.h"
#include "nx_math.h"

namespace nxd {

NXD int wrapi(int i, int n)
{
    i %= n;
    return i < 0 ? i + n : i;
}

NXD float4 tex2d(const TextureDev& t, const float* __restrict__ srgbLut, float u, float v)
{
    const int W = (int)t.width, H = (int)t.height;
    const float xb = u * (float)W - 0.5f, yb = v * (float)H - 0.5f;
    const float fx = floorf(xb), fy = floorf(yb);
    const float ax = floorf((xb - fx) * 256.0f + 0.5f) * (1.0f / 256.0f);
    const float ay = floorf((yb - fy) * 256.0f + 0.5f) * (1.0f / 256.0f);
    const int i0 = wrapi((int)fx, W), i1 = wrapi((int)fx + 1, W);
    const int j0 = wrapi((int)fy, H), j1 = wrapi((int)fy + 1, H);
    const uint32_t p00 = t.texels[(size_t)j0 * W + i0], p10 = t.texels[(size_t)j0 * W + i1];
    const uint32_t p01 = t.texels[(size_t)j1 * W + i0], p11 = t.texels[(size_t)j1 * W + i1];
    float out[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint32_t b00 = (p00 >> (8 * c)) & 0xffu, b10 = (p10 >> (8 * c)) & 0xffu;
        const uint32_t b01 = (p01 >> (8 * c)) & 0xffu, b11 = (p11 >> (8 * c)) & 0xffu;
        float t00, t10, t01, t11;
        if (c < 3) { t00 = srgbLut[b00]; t10 = srgbLut[b10]; t01 = srgbLut[b01]; t11 = srgbLut[b11]; }
        else { t00 = (float)b00 / 255.0f; t10 = (float)b10 / 255.0f; t01 = (float)b01 / 255.0f; t11 = (float)b11 / 255.0f; }
        const float top = t00 + ax * (t10 - t00);
        const float bot = t01 + ax * (t11 - t01);
        out[c] = top + ay * (bot - top);
    }
    return make_float4(out[0], out[1], out[2], out[3]);
}

// Channel 3 of tex2d alone, for a reader that wants the alpha only (the any-hit TRANSMIT instance, nx_trace.hip): the same addressing
// and, for that channel, the same expression sequence — so the same bits as tex2d(...).w — without the twelve LUT reads of the others.
NXD float tex2d_alpha(const TextureDev& t, float u, float v)
{
    const int W = (int)t.width, H = (int)t.height;
    const float xb = u * (float)W - 0.5f, yb = v * (float)H - 0.5f;
    const float fx = floorf(xb), fy = floorf(yb);
    const float ax = floorf((xb - fx) * 256.0f + 0.5f) * (1.0f / 256.0f);
    const float ay = floorf((yb - fy) * 256.0f + 0.5f) * (1.0f / 256.0f);
    const int i0 = wrapi((int)fx, W), i1 = wrapi((int)fx + 1, W);
    const int j0 = wrapi((int)fy, H), j1 = wrapi((int)fy + 1, H);
    const uint32_t p00 = t.texels[(size_t)j0 * W + i0], p10 = t.texels[(size_t)j0 * W + i1];
    const uint32_t p01 = t.texels[(size_t)j1 * W + i0], p11 = t.texels[(size_t)j1 * W + i1];
    const float t00 = (float)(p00 >> 24) / 255.0f, t10 = (float)(p10 >> 24) / 255.0f;
    const float t01 = (float)(p01 >> 24) / 255.0f, t11 = (float)(p11 >> 24) / 255.0f;
    const float top = t00 + ax * (t10 - t00);
    const float bot = t01 + ax * (t11 - t01);
    return top + ay * (bot - top);
}

// The detail maps' lookup (normal and roughness maps: nxhip_upload_texture kind 3 / 4): linear data, so no sRGB table — every channel is
// byte / 255.0f, as tex2d's alpha — with tex2d's addressing and its 1/256 bilinear weights.
NXD float4 tex2d_linear(const TextureDev& t, float u, float v)
{
    const int W = (int)t.width, H = (int)t.height;
    const float xb = u * (float)W - 0.5f, yb = v * (float)H - 0.5f;
    const float fx = floorf(xb), fy = floorf(yb);
    const float ax = floorf((xb - fx) * 256.0f + 0.5f) * (1.0f / 256.0f);
    const float ay = floorf((yb - fy) * 256.0f + 0.5f) * (1.0f / 256.0f);
    const int i0 = wrapi((int)fx, W), i1 = wrapi((int)fx + 1, W);
    const int j0 = wrapi((int)fy, H), j1 = wrapi((int)fy + 1, H);
    const uint32_t p00 = t.texels[(size_t)j0 * W + i0], p10 = t.texels[(size_t)j0 * W + i1];
    const uint32_t p01 = t.texels[(size_t)j1 * W + i0], p11 = t.texels[(size_t)j1 * W + i1];
    float out[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float t00 = (float)((p00 >> (8 * c)) & 0xffu) / 255.0f, t10 = (float)((p10 >> (8 * c)) & 0xffu) / 255.0f;
        const float t01 = (float)((p01 >> (8 * c)) & 0xffu) / 255.0f, t11 = (float)((p11 >> (8 * c)) & 0xffu) / 255.0f;
        const float top = t00 + ax * (t10 - t00);
        const float bot = t01 + ax * (t11 - t01);
        out[c] = top + ay * (bot - top);
    }
    return make_float4(out[0], out[1], out[2], out[3]);
}

// The float environment map's lookup (nxhip_upload_env_float): the same addressing — normalised coordinates, texel centres at +0.5,
// wrap on both axes — over one float4 of linear radiance per texel, with the EXACT binary32 fractional weights.  The 1/256 steps
// above imitate a texture unit that only ever filtered 8-bit texels; next to a texel of 6e4, 1/512 of a weight is 117, not a
// rounding error.  Three roundings per lerp (no contraction: -ffp-contract=off), two lerps deep: within 6 x 2^-24 x the largest tap
// of the exact bilinear value.
template <class Texels>  // (const float4*: global in a device-state block, plain as a kernel argument)
NXD float4 tex2d_float(const Texels texels, const int W, const int H, float u, float v)
{
    const float xb = u * (float)W - 0.5f, yb = v * (float)H - 0.5f;
    const float fx = floorf(xb), fy = floorf(yb);
    const float ax = xb - fx, ay = yb - fy;
    const int i0 = wrapi((int)fx, W), i1 = wrapi((int)fx + 1, W);
    const int j0 = wrapi((int)fy, H), j1 = wrapi((int)fy + 1, H);
    const float4 t00 = texels[(size_t)j0 * W + i0], t10 = texels[(size_t)j0 * W + i1];
    const float4 t01 = texels[(size_t)j1 * W + i0], t11 = texels[(size_t)j1 * W + i1];
    const float tx = t00.x + ax * (t10.x - t00.x), bx = t01.x + ax * (t11.x - t01.x);
    const float ty = t00.y + ax * (t10.y - t00.y), by = t01.y + ax * (t11.y - t01.y);
    const float tz = t00.z + ax * (t10.z - t00.z), bz = t01.z + ax * (t11.z - t01.z);
    return make_float4(tx + ay * (bx - tx), ty + ay * (by - ty), tz + ay * (bz - tz), 1.0f);
}

}  // namespace nxd
