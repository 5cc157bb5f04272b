// nx_adaptive.hip — adaptive sampling: per-pixel noise statistics, the per-block stop rule and the device-built active set.
//
// No counterpart in the reference, which renders a caller-chosen number of frames through every pixel.  The context's BASE set (what
// nxhip_set_pixel_map / nxhip_set_pixel_order / the identity define) keeps sizing the image; a pass renders the ACTIVE set, whole blocks
// of 64 consecutive base paths whose pixels are not all settled yet, through DeviceState::pixelMap / localCount / activeIndex.
//   adaptive_accumulate_kernel   accumulate_kernel's running mean with the PIXEL's sample count for the frame number, Welford's mean and
//                                M2 of the luminance and the tonemap — one kernel, a path's radiance is read once.
//   adaptive_aov_fold_kernel     aov_fold_kernel (nx_aov.hip) the same way: features and colour cover the same samples.
//   adaptive_decide_kernel       one wave per block: the relative standard error of every pixel's mean luminance, one ballot for "any
//                                pixel unsettled" (no floating-point reduction: exact and order-free), the block's largest error.
//   adaptive_scan_kernel         block flags -> exclusive prefix in base order, one workgroup (1080p: 32 400 blocks, 32 per thread).
//   adaptive_fill_kernel         one wave per active block: 64 entries of activeIndex and pixelMap, 256-byte coalesced stores.
#define NX_KERNEL_TU 1
#include "nx_device.h"
#include "nx_math.h"
#include "nx_tonemap.h"

namespace nxd {

constexpr int kAdBlock = 256;
constexpr int kAdScanThreads = 1024;

__global__ void __launch_bounds__(kAdBlock) adaptive_accumulate_kernel(const DeviceState* __restrict__ S)
{
    const uint32_t slices = S->framesPerPass, active = S->localCount;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < active; k += gridDim.x * blockDim.x) {
        const uint32_t i = S->activeIndex[k];
        uint32_t n = S->adCount[i];
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float2 st = make_float2(0.0f, 0.0f);  // (meanY, M2)
        if (n != 0u) { a = S->accumulation[i]; st = S->adStats[i]; }
        for (uint32_t sl = 0; sl < slices; sl++) {
            const float4 r = S->radiance[(size_t)sl * active + k];
            const float Y = (0.2126f * r.x + 0.7152f * r.y) + 0.0722f * r.z;
            n++;
            if (n == 1u) {
                a = make_float4(r.x, r.y, r.z, 0.0f);
                st = make_float2(Y, 0.0f);
            } else {
                const float f = (float)n;
                a.x += (r.x - a.x) / f;
                a.y += (r.y - a.y) / f;
                a.z += (r.z - a.z) / f;
                const float d = Y - st.x;
                st.x += d / f;
                st.y += d * (Y - st.x);
            }
        }
        S->adCount[i] = n;
        S->adStats[i] = st;
        S->accumulation[i] = a;
        S->rgba8[i] = tonemap_rgba8(mk3(a.x, a.y, a.z));
    }
}

// fold_mean (nx_aov.hip) with the pixel's count: `before` samples are in acc[i] already
NXD float4 fold_mean_counted(const NX_G float4* acc, const NX_G float4* in, const uint32_t i, const uint32_t k, const uint32_t slices, const uint32_t sliceStride, const uint32_t before)
{
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (before != 0u) a = acc[i];
    for (uint32_t sl = 0; sl < slices; sl++) {
        const float4 r = in[(size_t)sl * sliceStride + k];
        const uint32_t n = before + sl + 1u;
        if (n == 1u) a = r;
        else {
            const float f = (float)n;
            a.x += (r.x - a.x) / f;
            a.y += (r.y - a.y) / f;
            a.z += (r.z - a.z) / f;
            a.w += (r.w - a.w) / f;
        }
    }
    return a;
}

// Launched BEHIND adaptive_accumulate_kernel of the same pass: the counts already include the pass's slices.
__global__ void __launch_bounds__(kAdBlock) adaptive_aov_fold_kernel(const DeviceState* __restrict__ S)
{
    const uint32_t slices = S->framesPerPass, active = S->localCount;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < active; k += gridDim.x * blockDim.x) {
        const uint32_t i = S->activeIndex[k];
        const uint32_t before = S->adCount[i] - slices;
        S->aovAccumAlbedo[i] = fold_mean_counted(S->aovAccumAlbedo, S->aovAlbedo, i, k, slices, active, before);
        S->aovAccumNormalDepth[i] = fold_mean_counted(S->aovAccumNormalDepth, S->aovNormalDepth, i, k, slices, active, before);
    }
}

// One wave per block of 64 consecutive base paths (AdaptiveLaunch: nx_device.h).  A pixel with fewer than two samples has no
// estimate: unsettled, and it adds nothing to the block's maximum.
__global__ void __launch_bounds__(kAdBlock) adaptive_decide_kernel(const AdaptiveLaunch L)
{
    const uint32_t block = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (block >= L.blocks) return;  // (the whole wave)
    const uint32_t i = block * 64u + lane;
    bool unsettled = false;
    uint32_t eBits = 0u;
    if (i < L.baseCount) {
        const uint32_t n = L.count[i];
        unsettled = true;
        if (n >= 2u) {
            const float2 st = L.stats[i];
            const float nf = (float)n;
            const float e = sqrtf(st.y / (nf * (nf - 1.0f))) / fmaxf(st.x, L.lumFloor);
            unsettled = n < L.minSamples || !(e <= L.threshold);
            eBits = e >= 0.0f ? __float_as_uint(e) & 0x7fffffffu : 0x7f800000u;  // non-negative floats order like their bits; NaN counts as +inf
        }
    }
    const bool any = __ballot(unsettled) != 0ull;
    for (int x = 1; x < 64; x <<= 1) eBits = max(eBits, (uint32_t)__shfl_xor((int)eBits, x));
    if (lane == 0u) {
        L.blockMax[block] = __uint_as_float(eBits);
        if (!any) L.blockFlag[block] = 0u;  // (a culled block stays culled: the flag is only ever cleared)
    }
}

// Exclusive prefix of the block flags in base order, and the totals: out[0] = pixels of the flagged blocks (the base set's last block
// may be partial), out[1] = flagged blocks.
__global__ void __launch_bounds__(kAdScanThreads) adaptive_scan_kernel(const AdaptiveLaunch L)
{
    __shared__ uint32_t sums[kAdScanThreads];
    const uint32_t t = threadIdx.x, per = (L.blocks + kAdScanThreads - 1u) / kAdScanThreads;
    const uint32_t b0 = min(L.blocks, t * per), b1 = min(L.blocks, b0 + per);
    uint32_t own = 0u;
    for (uint32_t b = b0; b < b1; b++) own += L.blockFlag[b] != 0u ? 1u : 0u;
    sums[t] = own;
    __syncthreads();
    for (uint32_t off = 1u; off < (uint32_t)kAdScanThreads; off <<= 1) {
        const uint32_t v = t >= off ? sums[t - off] : 0u;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    uint32_t run = sums[t] - own;
    for (uint32_t b = b0; b < b1; b++) {
        L.blockOffset[b] = run;
        run += L.blockFlag[b] != 0u ? 1u : 0u;
    }
    if (t == (uint32_t)kAdScanThreads - 1u) {
        const uint32_t total = sums[t];
        const bool lastActive = L.blocks != 0u && L.blockFlag[L.blocks - 1u] != 0u;
        L.totals[0] = total * 64u - (lastActive ? L.blocks * 64u - L.baseCount : 0u);
        L.totals[1] = total;
    }
}

// One wave per flagged block: its 64 paths' base-local indices and global pixels, at the block's place among the flagged ones.  The
// partial block, if there is one, is the last of the base order and so the last of the active order: no entry lands beyond the total.
__global__ void __launch_bounds__(kAdBlock) adaptive_fill_kernel(const AdaptiveLaunch L)
{
    const uint32_t block = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (block >= L.blocks || L.blockFlag[block] == 0u) return;
    const uint32_t i = block * 64u + lane;
    if (i >= L.baseCount) return;
    const uint32_t dst = L.blockOffset[block] * 64u + lane;
    L.activeIndex[dst] = i;
    L.pixelMap[dst] = L.basePixelMap ? L.basePixelMap[i] : i;
}

const void* adaptive_accumulate_kernel_ptr() { return (const void*)adaptive_accumulate_kernel; }
const void* adaptive_aov_fold_kernel_ptr() { return (const void*)adaptive_aov_fold_kernel; }
const void* adaptive_decide_kernel_ptr() { return (const void*)adaptive_decide_kernel; }
const void* adaptive_scan_kernel_ptr() { return (const void*)adaptive_scan_kernel; }
const void* adaptive_fill_kernel_ptr() { return (const void*)adaptive_fill_kernel; }

uint64_t layout_stamp_adaptive() { return layout_stamp(); }

}  // namespace nxd
