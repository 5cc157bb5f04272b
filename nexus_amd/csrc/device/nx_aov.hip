// nx_aov.hip — feature buffers of the camera ray's hit and the edge-avoiding a-trous filter that uses them.
//
// No counterpart in the reference (its only image is the running mean, PathTracer.cu:480-496).  Three groups of kernels:
//   aov_kernel          per path of a pass: albedo + coverage and shading normal + hit distance of the PRIMARY ray's closest hit.  Reads
//                       what the primary closest-hit launch left at the ray's slot (hit, hitInst, rays[0]) and sits in the pass graph as
//                       one more branch beside the bounce-1 material step, which only reads the same records.  One thread per path in
//                       path order: 16-byte loads at the slot, 16-byte stores at the path; the gathers are the instance's shading
//                       record, the triangle and, where the material has a diffuse map, four texels.
//   aov_fold_kernel     accumulate_kernel's running mean, in its frame order, over the two feature buffers (all four components).
//   denoise_*_kernel    Dammertz et al. 2010: `iterations` passes of a 5 x 5 B3-spline kernel with holes (step 2^i) whose taps are
//                       weighted by colour, normal, albedo and depth differences.  Image space: the first kernel gathers colour and
//                       features through the pixel map into row-major planes, the iterations ping-pong between two colour planes.
#define NX_KERNEL_TU 1
#include "nx_device.h"
#include "nx_math.h"
#include "nx_queue.h"
#include "nx_texture.h"
#include "nx_tonemap.h"

namespace nxd {

constexpr int kAovBlock = 256;

__global__ void __launch_bounds__(kAovBlock) aov_kernel(const DeviceState* __restrict__ S)
{
    const uint32_t n = S->pathCount;
    const uint32_t piece = dense_piece(n, S->queueShards), cap = S->queueShardCap;
    // SCAN pipeline: the closest-hit launch leaves the logic step's code above the instance (nx_device.h kHitCodeShift)
    const uint32_t instMask = S->compactMode == NX_COMPACT_FAST ? kHitInstMask : 0xffffffffu;
    for (uint32_t index = blockIdx.x * blockDim.x + threadIdx.x; index < n; index += gridDim.x * blockDim.x) {
        const uint32_t region = index / piece, slot = region * cap + (index - region * piece);  // (where generate_kernel put the path's ray)
        const float4 hit = S->trace.hit[slot];
        float4 albedo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), normalDepth = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (hit.x != NX_MISS_DISTANCE) {
            const uint32_t instanceIdx = S->trace.hitInst[slot] & instMask;
            const float4 rd = S->trace.rays[0].rayD[slot];
            const f3 rayDirection = mk3(rd.x, rd.y, rd.z);
            const float hu = hit.y, hv = hit.z;
            const NX_G ShadeInst* inst = &S->shadeInst[instanceIdx];
            const NX_G nx_triangle* tri = shade_tri(inst->tris, __float_as_uint(hit.w));
            const NX_G float* IT = inst->invTransform;
            const f3 tp0 = ld3(tri->pos0), tp1 = ld3(tri->pos1), tp2 = ld3(tri->pos2);
            // the normals exactly as shade_path forms them (nx_wavefront.hip)
            f3 normal = bary3(ld3(tri->normal0), ld3(tri->normal1), ld3(tri->normal2), hu, hv);
            normal = normalize3(mat_vec_transposed(IT, normal));
            const f3 gNormal = normalize3(mat_vec_transposed(IT, cross3(tp1 - tp0, tp2 - tp0)));
            if (dot3(gNormal, rayDirection) > 0.0f) normal = -normal;  // towards the camera, whatever the material
            const int32_t diffuseMapId = inst->material.diffuseMapId;
            f3 a = inst->material.type == NX_MAT_CONDUCTOR ? mk3(1.0f) : ld3(inst->material.diffuse.albedo);
            if (diffuseMapId != -1) {  // the map replaces the albedo (shade_path)
                const f2 texUv = bary2(tri->texCoord0, tri->texCoord1, tri->texCoord2, hu, hv);
                const float4 color = tex2d(S->diffuseMaps[diffuseMapId], S->srgbLut, texUv.x, texUv.y);
                a = mk3(color.x, color.y, color.z);
            }
            albedo = make_float4(a.x, a.y, a.z, 1.0f);
            normalDepth = make_float4(normal.x, normal.y, normal.z, hit.x);
        }
        S->aovAlbedo[index] = albedo;
        S->aovNormalDepth[index] = normalDepth;
    }
}

// accumulate_kernel's update (nx_wavefront.hip) on four components
NXD float4 fold_mean(const NX_G float4* acc, const NX_G float4* in, const uint32_t k, const uint32_t slices, const uint32_t sliceStride, const uint32_t firstFrame)
{
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (firstFrame != 1u) a = acc[k];
    for (uint32_t sl = 0; sl < slices; sl++) {
        const float4 r = in[(size_t)sl * sliceStride + k];
        const uint32_t frame = firstFrame + sl;
        if (frame == 1u) a = r;
        else {
            const float f = (float)frame;
            a.x += (r.x - a.x) / f;
            a.y += (r.y - a.y) / f;
            a.z += (r.z - a.z) / f;
            a.w += (r.w - a.w) / f;
        }
    }
    return a;
}

__global__ void __launch_bounds__(kAovBlock) aov_fold_kernel(const DeviceState* __restrict__ S)
{
    const uint32_t slices = S->framesPerPass, count = S->localCount;
    const uint32_t firstFrame = S->frame->frameNumber - (slices - 1u);
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        S->aovAccumAlbedo[k] = fold_mean(S->aovAccumAlbedo, S->aovAlbedo, k, slices, count, firstFrame);
        S->aovAccumNormalDepth[k] = fold_mean(S->aovAccumNormalDepth, S->aovNormalDepth, k, slices, count, firstFrame);
    }
}

// ------------------------------------------------------------------------------------------------------
// The filter.  One thread per pixel, workgroups of 32 x 8 pixels (a wave: two rows of 32, so every load and store of a wave is two
// runs of 512 consecutive bytes).  Per tap 48 bytes: colour, albedo + coverage, normal + depth.
//   LDS = true   (steps 1 and 2): the workgroup's tile plus its halo of 2 x step pixels is staged in LDS once, 16 bytes per lane and
//                access.  Row pitch = tile width, unpadded: the lanes of a 16-byte LDS read conflict only inside one of the four
//                16-lane groups of their 32-lane half, a half reads 32 consecutive 16-byte slots of one row, and any 16 of those
//                fall on distinct banks modulo the 256-byte bank row.
//   LDS = false  (steps 4 and up, where the halo would be most of the tile): the taps straight from the planes — neighbouring lanes
//                still read neighbouring pixels, and the planes stay in L2 / Infinity Cache.

constexpr int kDnTileW = 32, kDnTileH = 8;

// (DenoiseLaunch, the kernels' one argument: nx_device.h)

NXD float sq3(float4 a, float4 b)
{
    const float x = a.x - b.x, y = a.y - b.y, z = a.z - b.z;
    return (x * x + y * y) + z * z;
}

template <bool LDS, int STEP>
__global__ void __launch_bounds__(kDnTileW * kDnTileH) denoise_iteration_kernel(const DenoiseLaunch L)
{
    constexpr int kHalo = LDS ? 2 * STEP : 0;
    constexpr int kLw = LDS ? kDnTileW + 2 * kHalo : 1, kLh = LDS ? kDnTileH + 2 * kHalo : 1;
    __shared__ float4 sC[kLw * kLh], sA[kLw * kLh], sN[kLw * kLh];
    const int step = LDS ? STEP : L.step;
    const int W = L.width, H = L.height;
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    const int x0 = (int)blockIdx.x * kDnTileW, y0 = (int)blockIdx.y * kDnTileH;
    const int x = x0 + tx, y = y0 + ty;
    if (LDS) {
        for (int r = ty; r < kLh; r += kDnTileH) {
            const int gy = y0 - kHalo + r;
            if (gy < 0 || gy >= H) continue;
            for (int q = tx; q < kLw; q += kDnTileW) {
                const int gx = x0 - kHalo + q;
                if (gx < 0 || gx >= W) continue;  // (entries outside the image are never read: the tap loop skips them too)
                const size_t g = (size_t)gy * W + gx;
                sC[r * kLw + q] = L.colour[g];
                sA[r * kLw + q] = L.albedo[g];
                sN[r * kLw + q] = L.normalDepth[g];
            }
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    float4 cp, ap, np;
    if (LDS) { const int l = (ty + kHalo) * kLw + tx + kHalo; cp = sC[l]; ap = sA[l]; np = sN[l]; }
    else { cp = L.colour[p]; ap = L.albedo[p]; np = L.normalDepth[p]; }
    const float sz = L.sigmaDepth * fmaxf(np.w, 1e-6f);
    const float invDepth = fminf(1.0f / (sz * sz), 3.402823466e38f);
    const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float sx = 0.0f, sy = 0.0f, szz = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * step;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * step;
            if (qx < 0 || qx >= W) continue;
            float4 cq, aq, nq;
            if (LDS) { const int l = (ty + kHalo + dy * STEP) * kLw + tx + kHalo + dx * STEP; cq = sC[l]; aq = sA[l]; nq = sN[l]; }
            else { const size_t q = (size_t)qy * W + qx; cq = L.colour[q]; aq = L.albedo[q]; nq = L.normalDepth[q]; }
            const float aw = ap.w - aq.w, dz = np.w - nq.w;
            const float e = ((sq3(cp, cq) * L.invColour + sq3(np, nq) * L.invNormal) + (sq3(ap, aq) + aw * aw) * L.invAlbedo) + (dz * dz) * invDepth;
            const float w = (h[dx + 2] * h[dy + 2]) * nxf_expf(-e);
            sx += w * cq.x;
            sy += w * cq.y;
            szz += w * cq.z;
            sw += w;
        }
    }
    const float4 o = make_float4(sx / sw, sy / sw, szz / sw, 0.0f);
    L.out[p] = o;
    if (L.rgba8) L.rgba8[p] = tonemap_rgba8(mk3(o.x, o.y, o.z));
}

// Path order -> image space: element k of the context's accumulation and accumulated features belongs to pixel pixelMap[k]
// (nullptr: k).  With rgba8 (iterations = 0: the filter is a copy) the tonemapped image as well.
__global__ void __launch_bounds__(kAovBlock) denoise_gather_kernel(const DeviceState* __restrict__ S, float4* __restrict__ colour, float4* __restrict__ albedo,
                                                                    float4* __restrict__ normalDepth, uint32_t* __restrict__ rgba8)
{
    const uint32_t count = S->baseCount;  // (the base set: what `accumulation` is sized by, whatever set the passes render — nx_adaptive.hip)
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const uint32_t g = S->basePixelMap ? S->basePixelMap[k] : k;
        const float4 c = S->accumulation[k];
        colour[g] = make_float4(c.x, c.y, c.z, 0.0f);
        albedo[g] = S->aovAccumAlbedo[k];
        normalDepth[g] = S->aovAccumNormalDepth[k];
        if (rgba8) rgba8[g] = tonemap_rgba8(mk3(c.x, c.y, c.z));
    }
}

const void* aov_kernel_ptr() { return (const void*)aov_kernel; }
const void* aov_fold_kernel_ptr() { return (const void*)aov_fold_kernel; }
const void* denoise_gather_kernel_ptr() { return (const void*)denoise_gather_kernel; }
// step 1 / 2 from LDS, larger steps from the planes; `forceDirect`: the plane variant for every step (the measurement of one against the other)
const void* denoise_iteration_kernel_ptr(int step, bool forceDirect)
{
    if (!forceDirect && step == 1) return (const void*)denoise_iteration_kernel<true, 1>;
    if (!forceDirect && step == 2) return (const void*)denoise_iteration_kernel<true, 2>;
    return (const void*)denoise_iteration_kernel<false, 0>;
}

uint64_t layout_stamp_aov() { return layout_stamp(); }

}  // namespace nxd
