// nx_wavefront.hip — the plain kernels of a pass (begin-frame, generate, count-scan, accumulate, compose; the ray-batch hooks' queue
// sizes) and the BASE instances of the material kernel families: the contexts without detail maps, a fifth material type or alpha modes.
//
// The families' text is nx_wavefront.h, which says how the kernels run; the instances with a newer feature are units of their own
// (nx_wavefront_detail.hip / _metal.hip / _solid.hip), and the array test hooks are nx_hook_kernels.hip.  The four family units are
// the build's longest compiles, about a minute and a half each (profiles/analytic_lights.txt section 3, profiles/kernel_units.txt: the
// build's wall time is theirs), so only what a pass graph launches lives in them.
// What the plain kernels compute is the reference's GenerateKernel and AccumulateKernel
// (Nexus/src/Cuda/PathTracer/PathTracer.cu:85-122, 480-496).
#define NX_KERNEL_TU 1
#include "nx_wavefront.h"
#include "nx_tonemap.h"

namespace nxd {

// ------------------------------------------------------------------------------------------------------
// begin pass: the pass size (frames batched into this pass) and the number of its last frame arrive as kernel arguments and
// are published to the other kernels through the device state, so neither a pass of a different size nor several passes
// in flight (each in its own slot, numbered by the host) need a host-side state upload or a synchronisation.  Also: zero
// every counter, traceSize[0] = localCount * frames (GenerateKernel's thread 0 in the reference, PathTracer.cu:112-113; the
// memset of PathTracer.cpp:263; the frame counter of PathTracer.cpp:250).

__global__ void __launch_bounds__(kWideBlock) begin_frame_kernel(DeviceState* __restrict__ S, const uint32_t frames, const uint32_t frameLast, const uint32_t scanEpoch)
{
    int* c = reinterpret_cast<int*>(S->counters);
    constexpr int n = (int)(sizeof(Counters) / sizeof(int));
    for (int i = threadIdx.x; i < n; i += blockDim.x) c[i] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        S->framesPerPass = frames;
        S->pathCount = S->localCount * frames;
        S->frame->frameNumber = frameLast;
        S->frame->scanEpoch = scanEpoch;
        // a pending pixel query (D_PixelQuery, PathTracer.cuh:54-58) starts the pass as "nothing hit": the bounce-1 material kernel
        // writes the instance a primary ray of that pixel hits (the reference's logic kernel writes -1 on a miss, PathTracer.cu:160;
        // the SCAN pipeline has no kernel that looks at misses when the background is black)
        if (S->frame->pixelQueryPixel >= 0) S->frame->pixelQueryInstance = -1;
    }
    if (threadIdx.x < kQueueShards) {
        // the primary rays: path i goes to region i / piece (generate_kernel)
        const uint32_t n = S->localCount * frames, piece = dense_piece(n, S->queueShards), k = threadIdx.x;
        S->counters->region[k].traceSize[0] = k < S->queueShards ? (int)min(piece, n - min(n, k * piece)) : 0;
    }
}

// The ray-batch hooks (nxhip_trace_batch / nxhip_trace_shadow_batch): `n` rays in the dense numbering of dense_piece — the sizes of
// the regions in use and zeroed fetch heads at bounce slot `slot`.
__global__ void hook_sizes_kernel(DeviceState* __restrict__ S, const uint32_t n, const int anyHit, const int slot)
{
    const uint32_t k = threadIdx.x;
    if (k >= (uint32_t)kQueueShards) return;
    const uint32_t shards = S->queueShards, piece = dense_piece(n, shards);
    const int32_t size = k < shards ? (int32_t)min(piece, n - min(n, k * piece)) : 0;
    NX_G RegionCounters* r = &S->counters->region[k];
    if (anyHit) { r->traceShadowSize[slot] = size; r->shadowHead[slot] = 0; }
    else { r->traceSize[slot] = size; r->traceHead[slot] = 0; }
    if (k == 0) { S->counters->thinCount[0][slot] = 0; S->counters->thinCount[1][slot] = 0; }  // (the hooks may run with the thin hand-over on: nxhip_debug_set_thin)
}

// ------------------------------------------------------------------------------------------------------
// GenerateKernel — PathTracer.cu:85-122

__global__ void __launch_bounds__(kWideBlock) generate_kernel(const DeviceState* __restrict__ S)
{
    const uint32_t n = S->pathCount;
    const uint32_t frameLast = S->frame->frameNumber;
    const uint32_t resX = S->camera.resolution[0], resY = S->camera.resolution[1];
    const f3 camPos = ld3(S->camera.position), camRight = ld3(S->camera.right), camUp = ld3(S->camera.up);
    const f3 llc = ld3(S->camera.lowerLeftCorner), vpX = ld3(S->camera.viewportX), vpY = ld3(S->camera.viewportY);
    const float lensRadius = S->camera.lensRadius;
    const uint32_t piece = dense_piece(n, S->queueShards), cap = S->queueShardCap;
    for (uint32_t index = blockIdx.x * blockDim.x + threadIdx.x; index < n; index += gridDim.x * blockDim.x) {
        const PathId id = path_id(S, index, frameLast);
        const uint32_t g = global_pixel(S, id.pixel);
        const uint32_t j = g / resX;
        const uint32_t i = g - j * resX;
        uint32_t rng = rng_init_pixel(i, j, resX, id.frame);
        const float x = ((float)i + rng_next(rng)) / (float)resX;
        const float y = ((float)j + rng_next(rng)) / (float)resY;
        const f2 disk = unit_disk(rng);
        const float rdx = lensRadius * disk.x, rdy = lensRadius * disk.y;
        const f3 offset = camRight * rdx + camUp * rdy;
        const f3 origin = camPos + offset;
        const f3 direction = normalize3((((llc + vpX * x) + vpY * y) - camPos) - offset);
        // the path's radiance starts at zero here (a coalesced 16-byte store) so that the first hit adds to it only when it
        // emits, like every later one.  (The path's previous vertex is kept by the logic step: keep_previous_vertex.)
        S->radiance[index] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        // throughput / lastPdf start as (1, 1, 1, 1e10): the bounce-1 logic and shade kernels use those constants instead of
        // reading them back, and the logic kernel stores them for every path that survives its first hit
        const uint32_t region = index / piece, slot = region * cap + (index - region * piece);
        // w: kRaySurvives — the bounce-1 logic step draws against a throughput of 1, and rng_next() < 1 always (PathTracer.cu:167-175
        // with the implicit throughput of :149)
        // ... and, with entry points on, the number of the entry state of the path's run of 64 (nx_entry.hip)
        const uint32_t entryBits = S->entry ? ((id.pixel >> 6) + 1u) << kRayEntryShift : 0u;
        S->trace.rays[0].rayO[slot] = make_float4(origin.x, origin.y, origin.z, __uint_as_float(kRaySurvives | entryBits));
        S->trace.rays[0].rayD[slot] = make_float4(direction.x, direction.y, direction.z, __uint_as_float(index));
    }
}

// The reference's queue sizes count the hits of a material type whether or not a kernel shades them (its conductor kernel's body is
// commented out, PathTracer.cu:475-478, but the logic kernel still fills that queue): with NX_CONDUCTOR_REFERENCE the SCAN
// pipeline has no conductor kernel to count its items, so this one does (4 B per ray; in the graph only in that mode).
__global__ void __launch_bounds__(kWideBlock) count_scan_kernel(const DeviceState* __restrict__ S, const int bounce, const int type)
{
    Counters* C = S->counters;
    const QueueView in = queue_view(&C->region[0].traceSize[bounce - 1], S->queueShardCap);
    int n = 0;
    for (int index = (int)(blockIdx.x * blockDim.x + threadIdx.x); index < in.total; index += (int)(gridDim.x * blockDim.x))
        n += (S->trace.hitInst[in.slot(index)] >> kHitCodeShift) == (uint32_t)(type + 1) ? 1 : 0;
    n = wave_sum(n);
    if ((threadIdx.x & (kWave - 1)) == 0 && n) atomicAdd(&C->region[0].materialSize[type][bounce], n);
}

// ------------------------------------------------------------------------------------------------------
// AccumulateKernel, Tonemap, LinearToGamma, ToColorUInt — PathTracer.cu:37-62, 480-496; Utils/Utils.h:51-54

// (tonemap_rgba8: nx_tonemap.h — the denoiser's kernels write their RGBA8 image through the same text)

// Running mean over `slices` consecutive frames per pixel, then tonemap.  src == nullptr: this context's own radiance
// (slices = framesPerPass, the pass's frame numbers); otherwise externally gathered radiance laid out
// [slices][sliceStride] whose element k belongs to full-image pixel dstMap[k] (nullptr: k), first frame = firstFrame.
__global__ void __launch_bounds__(kWideBlock) accumulate_kernel(const DeviceState* __restrict__ S, const float4* __restrict__ src, const uint32_t count,
                                                                 const uint32_t slicesIn, const uint32_t sliceStrideIn, const uint32_t firstFrameIn,
                                                                 const uint32_t* __restrict__ dstMap)
{
    const float4* in = src ? src : S->radiance;
    const uint32_t slices = src ? slicesIn : S->framesPerPass;
    const uint32_t sliceStride = src ? sliceStrideIn : S->localCount;
    const uint32_t firstFrame = src ? firstFrameIn : S->frame->frameNumber - (S->framesPerPass - 1u);
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const uint32_t i = dstMap ? dstMap[k] : k;
        float4 a = firstFrame == 1u ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : S->accumulation[i];
        for (uint32_t sl = 0; sl < slices; sl++) {
            const float4 r = in[(size_t)sl * sliceStride + k];
            const uint32_t frame = firstFrame + sl;
            if (frame == 1u) a = make_float4(r.x, r.y, r.z, 0.0f);
            else {
                const float f = (float)frame;
                a.x += (r.x - a.x) / f;
                a.y += (r.y - a.y) / f;
                a.z += (r.z - a.z) / f;
            }
        }
        S->accumulation[i] = a;
        S->rgba8[i] = tonemap_rgba8(mk3(a.x, a.y, a.z));
    }
}

// Multi-GPU image assembly on the root: element k of a rank's local-order accumulation tile belongs to full-image pixel
// dstMap[k] (nullptr: k).  A copy and a tonemap, no arithmetic on the accumulated values.
__global__ void __launch_bounds__(kWideBlock) compose_kernel(const float4* __restrict__ src, const uint32_t count, const uint32_t* __restrict__ dstMap,
                                                              float4* __restrict__ dstAccum, uint32_t* __restrict__ dstRgba8)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const uint32_t i = dstMap ? dstMap[k] : k;
        const float4 a = src[k];
        dstAccum[i] = a;
        if (dstRgba8) dstRgba8[i] = tonemap_rgba8(mk3(a.x, a.y, a.z));
    }
}

// ------------------------------------------------------------------------------------------------------

// This unit's instances: the contexts without detail maps, a fifth material type or alpha modes.
// (the classic pipeline — logic kernel and per-type material kernels — runs under the ordered compaction only: see frame_levels)
using ShadeSets = Instances<kMfPower | kMfAnalytic, kMfAnalytic, kMfPower, 0u>;
using ShadeScanSets = Instances<kMfPower | kMfNoMaps | kMfAnalytic, kMfNoMaps | kMfAnalytic, kMfTree | kMfPower | kMfAnalytic, kMfPower | kMfAnalytic, kMfAnalytic,
                                kMfPower | kMfNoMaps, kMfNoMaps, kMfTree | kMfPower, kMfPower, 0u>;
using TailSets = Instances<kMfPower | kMfAnalytic, kMfAnalytic, kMfPower, 0u>;
namespace wavefront {
// `items` per thread: kLogicItems (2) unless the caller asks for 1 — what a scene with an environment map gets, whose misses run the
// map lookups (binary64 arc functions) in this kernel: with a second item's state live beside them the 64-register budget spills
// into that path (configs[3]: logic kernel +8 % with two items, -6 % on configs[1])
// (ANALYTIC: only the one-item instance has the form — the count enters the weighted miss, which needs an environment map)
const void* logic(int items, unsigned set)
{
    if (items == 1 || kLogicItems == 1) return Instances<kMfAnalytic, 0u>::find(set, [](auto f) { return (const void*)logic_kernel<kOrdered, 1, decltype(f)::value>; });
    return set == 0u ? (const void*)logic_kernel<kOrdered, kLogicItems> : nullptr;
}
const void* shade(int type, unsigned set) { return shade_instance<ShadeSets, NX_MAT_DIFFUSE, NX_MAT_DIELECTRIC, NX_MAT_PLASTIC, NX_MAT_CONDUCTOR>(type, set); }
const void* shade_scan(unsigned set) { return shade_scan_instance<ShadeScanSets>(set); }
const void* tail(unsigned set) { return tail_instance<TailSets>(set); }
}  // namespace wavefront
const void* count_scan_kernel_ptr() { return (const void*)count_scan_kernel; }
const void* begin_frame_kernel_ptr() { return (const void*)begin_frame_kernel; }
const void* hook_sizes_kernel_ptr() { return (const void*)hook_sizes_kernel; }
const void* generate_kernel_ptr() { return (const void*)generate_kernel; }
const void* accumulate_kernel_ptr() { return (const void*)accumulate_kernel; }
const void* compose_kernel_ptr() { return (const void*)compose_kernel; }

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_wavefront() { return layout_stamp(); }

}  // namespace nxd
