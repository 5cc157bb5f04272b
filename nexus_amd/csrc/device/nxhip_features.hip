// nxhip_features.hip — feature buffers and the denoiser, adaptive sampling, the light table of NXHIP_LIGHTS_POWER.
// (the C-ABI device layer declared in include/nexus_hip.h; helpers shared with the other nxhip_*.hip units: nx_host.h)
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nx_hookbatch.h"

using namespace nxd;

// ---- adaptive sampling (nx_adaptive.hip): the host side of the statistics and of the active set ------------------------------

static AdaptiveLaunch adaptive_launch(const nxhip_ctx* c)
{
    AdaptiveLaunch L{};
    L.count = c->adCount.as<uint32_t>();
    L.stats = c->adStats.as<float2>();
    L.blockFlag = c->adBlockFlag.as<uint32_t>();
    L.blockMax = c->adBlockMax.as<float>();
    L.blockOffset = c->adBlockOffset.as<uint32_t>();
    L.totals = c->adTotals.as<uint32_t>();
    L.basePixelMap = c->pixelMap.as<uint32_t>();
    L.activeIndex = c->adActiveIndex.as<uint32_t>();
    L.pixelMap = c->adPixelMap.as<uint32_t>();
    L.baseCount = c->localCount;
    L.blocks = c->adBlocks;
    L.minSamples = c->adParams.minSamples;
    L.threshold = c->adParams.threshold;
    L.lumFloor = c->adParams.lumFloor;
    return L;
}

// Flags -> prefix -> (with `fill`) the active set's two arrays, on the context's stream; the totals travel to pinned memory behind them.
static int adaptive_compact(nxhip_ctx* c, bool decide, bool fill)
{
    const AdaptiveLaunch L = adaptive_launch(c);
    const dim3 perBlock((unsigned)((size_t)c->adBlocks * 64u + 255u) / 256u);
    if (c->adBlocks != 0u) {
        if (decide) NX_HIP(launch_untimed(kernels::adaptive_decide(), perBlock, 256, c->stream, L));
        NX_HIP(launch_untimed(kernels::adaptive_scan(), 1, 1024, c->stream, L));
        if (fill) NX_HIP(launch_untimed(kernels::adaptive_fill(), perBlock, 256, c->stream, L));
    }
    NX_HIP(hipMemcpyAsync(c->adHostTotals, c->adTotals.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    NX_HIP(hipStreamSynchronize(c->stream));
    return NXHIP_OK;
}

static void adaptive_release(nxhip_ctx* c)
{
    for (DevBuf* b : {&c->adCount, &c->adStats, &c->adActiveIndex, &c->adPixelMap, &c->adBlockFlag, &c->adBlockMax, &c->adBlockOffset, &c->adTotals}) b->release();
    c->adBlocks = 0;
}

// The statistics start over for the context's current base set: all counts 0, every block active, the active set = the base set.
// (Re)allocates the buffers when the base set's size has changed.  Nothing may be in flight that uses them: synchronises first.
int nxd::adaptive_restart(nxhip_ctx* c)
{
    NX_SYNC_ALL(c);
    const uint32_t n = c->localCount, blocks = (n + 63u) / 64u;
    if (!c->adHostTotals) NX_HIP(hipHostMalloc((void**)&c->adHostTotals, 2 * sizeof(uint32_t), hipHostMallocDefault));
    if (!c->adCount.p || c->adCount.bytes != std::max<size_t>((size_t)n * 4, 16) || c->adBlocks != blocks) {
        DevBuf count, stats, index, map, flag, bmax, offset, totals;  // all or nothing
        if (!count.alloc((size_t)n * 4) || !stats.alloc((size_t)n * 8) || !index.alloc((size_t)n * 4) || !map.alloc((size_t)n * 4) ||
            !flag.alloc((size_t)blocks * 4) || !bmax.alloc((size_t)blocks * 4) || !offset.alloc((size_t)blocks * 4) || !totals.alloc(16)) return NXHIP_ERR_HIP;
        c->adCount = std::move(count);
        c->adStats = std::move(stats);
        c->adActiveIndex = std::move(index);
        c->adPixelMap = std::move(map);
        c->adBlockFlag = std::move(flag);
        c->adBlockMax = std::move(bmax);
        c->adBlockOffset = std::move(offset);
        c->adTotals = std::move(totals);
        c->adBlocks = blocks;
    }
    NX_HIP(hipMemsetAsync(c->adCount.p, 0, (size_t)n * 4, c->stream));
    NX_HIP(hipMemsetAsync(c->adStats.p, 0, (size_t)n * 8, c->stream));
    NX_HIP(hipMemsetAsync(c->adBlockMax.p, 0, (size_t)blocks * 4, c->stream));
    NX_HIP(hipMemsetAsync(c->adTotals.p, 0, 16, c->stream));
    if (blocks) NX_HIP(hipMemsetD32Async((hipDeviceptr_t)c->adBlockFlag.p, 1, blocks, c->stream));
    NX_TRY(adaptive_compact(c, false, true));
    c->unsettledPixels = c->adHostTotals[0];
    c->unsettledBlocks = c->adHostTotals[1];
    c->activeCount = n;
    publish_pixel_set(c);
    return NXHIP_OK;
}

// NXHIP_LIGHT_IMPORTANCE_POSITION (in POWER mode): the light tree (nx_lights.hip) over the entries of the table that refresh_light_table has
// just laid out and queued the build of.  The buffers follow G = nxhip_light_tree_leaves_for(entries); with another importance they are
// dropped and the state block names no tree.  The caller has waited for the passes in flight where there is more than one slot.
static int refresh_light_tree(nxhip_ctx* c)
{
    const bool wanted = c->lightImportance == NXHIP_LIGHT_IMPORTANCE_POSITION;
    const uint32_t n = c->lightEntries, leaves = wanted ? nxhip_light_tree_leaves_for(n) : 0u;
    if (wanted && n > kLightTreeLeavesMax) return fail_invalid("NXHIP_LIGHT_IMPORTANCE_POSITION: the mesh lights have more than 2^23 triangles");
    if (leaves != c->lightTreeLeaves || (leaves != 0u && c->lightTreeOrder.bytes != std::max<size_t>((size_t)n * 4, 16))) {
        NX_SYNC_ALL(c);
        if (leaves == 0u) {
            for (DevBuf* b : {&c->lightTreeNodes, &c->lightTreeWeight, &c->lightTreeSlotOf, &c->lightTreeBounds, &c->lightTreeKeys, &c->lightTreeSorted, &c->lightTreeOrder,
                              &c->lightTreeSortTemp})
                b->release();
        } else {
            size_t sortBytes = 0;
            NX_TRY(light_tree_sort_bytes(n, &sortBytes));
            NX_ALLOC(c->lightTreeNodes, 2 * (size_t)leaves * sizeof(LightNode));
            NX_ALLOC(c->lightTreeWeight, 2 * (size_t)leaves * sizeof(double));
            NX_ALLOC(c->lightTreeSlotOf, (size_t)n * 4);
            NX_ALLOC(c->lightTreeOrder, (size_t)n * 4);
            NX_ALLOC(c->lightTreeKeys, (size_t)n * 8);
            NX_ALLOC(c->lightTreeSorted, (size_t)n * 8);
            NX_ALLOC(c->lightTreeBounds, 6 * 4);
            NX_ALLOC(c->lightTreeSortTemp, std::max<size_t>(sortBytes, 16));
            c->lightTreeSortBytes = sortBytes;
        }
        c->lightTreeLeaves = leaves;
        c->h.lightTree = leaves ? c->lightTreeNodes.as<LightNode>() : nullptr;
        c->h.lightSlotOf = leaves ? c->lightTreeSlotOf.as<uint32_t>() : nullptr;
        c->h.lightTreeLeaves = leaves;
        c->stateDirty = true;
        NX_TRY(upload_state(c));
    }
    if (leaves == 0u) return NXHIP_OK;
    LightTreeBuild b{};
    b.shadeInst = c->shadeInst.as<ShadeInst>();
    b.lights = c->lights.as<nx_light>();
    b.lightBase = c->lightBase.as<uint32_t>();
    b.table = c->lightTable.as<LightEntry>();
    b.mapMean64 = c->lightMapMean64.as<double>();
    b.bounds = c->lightTreeBounds.as<uint32_t>();
    b.keys = c->lightTreeKeys.as<uint64_t>();
    b.sorted = c->lightTreeSorted.as<uint64_t>();
    b.order = c->lightTreeOrder.as<uint32_t>();
    b.slotOf = c->lightTreeSlotOf.as<uint32_t>();
    b.nodes = c->lightTreeNodes.as<LightNode>();
    b.nodeWeight = c->lightTreeWeight.as<double>();
    b.header = c->lightHeader.as<LightHeader>();
    b.entries = n;
    b.leaves = leaves;
    return light_tree_build(c->stream, b, c->lightTreeSortTemp.p, c->lightTreeSortBytes);
}

// The context's base pixel set (count or map) has just changed.
// NXHIP_LIGHTS_POWER: the light table (nx_lights.hip) brought up to date, once, before the next pass or hook call that reads it —
// in the manner of refresh_updated_blas.  The shading records and the triangles it reads are current by then (the caller has run
// refresh_shade_inst; transforms and refits are ahead of it in stream order).  The host knows the entry LAYOUT (lights, instances,
// triangle counts) and re-allocates only when that changes; the weights never come back.  Nothing happens in the default mode.
int nxd::refresh_light_table(nxhip_ctx* c)
{
    if (c->lightSampling != NXHIP_LIGHTS_POWER || !c->lightTableDirty) return NXHIP_OK;
    const size_t nLights = c->hostLights.size(), nInst = c->hostInstances.size();
    std::vector<uint32_t> base(nLights + 1, 0u), instLight(std::max<size_t>(1, nInst), kNotALight);
    uint64_t n = 0;
    for (size_t l = 0; l < nLights; l++) {
        base[l] = (uint32_t)n;
        const nx_light& light = c->hostLights[l];
        if (light.type != NX_LIGHT_MESH) continue;  // (no triangles: no entries)
        const nx_bvh_instance& inst = c->hostInstances[light.mesh.meshId];
        if (inst.bvhIdx >= c->blas.size()) return fail_invalid("instance refers to a BLAS id that has not been uploaded");
        n += c->blas[inst.bvhIdx].triCount;
        if (n >= 0xffffffffull) return fail_invalid("NXHIP_LIGHTS_POWER: the mesh lights have 2^32 triangles or more");
        instLight[light.mesh.meshId] = (uint32_t)l;
    }
    base[nLights] = (uint32_t)n;
    uint32_t guide = 1u;
    while (guide < n && guide < kLightGuideMax) guide <<= 1;
    if (slot_count(c) > 1) NX_SYNC_ALL(c);  // passes on the other slots' streams still read the old table
    if (!c->lightHeader.p || base != c->hostLightBase || instLight != c->hostInstLight) {
        NX_SYNC_ALL(c);
        NX_ALLOC(c->lightHeader, sizeof(LightHeader));
        NX_ALLOC(c->lightBase, base.size() * 4);
        NX_ALLOC(c->instLight, instLight.size() * 4);
        NX_HIP(hipMemcpy(c->lightBase.p, base.data(), base.size() * 4, hipMemcpyHostToDevice));
        NX_HIP(hipMemcpy(c->instLight.p, instLight.data(), instLight.size() * 4, hipMemcpyHostToDevice));
        if ((uint32_t)n != c->lightEntries || !c->lightTable.p) {
            size_t scanBytes = 0;
            NX_TRY(light_scan_bytes((size_t)std::max<uint64_t>(n, 1), &scanBytes));
            NX_ALLOC(c->lightTable, (size_t)std::max<uint64_t>(n, 1) * sizeof(LightEntry));
            NX_ALLOC(c->lightWeight, (size_t)std::max<uint64_t>(n, 1) * sizeof(double));
            NX_ALLOC(c->lightPrefix, (size_t)std::max<uint64_t>(n, 1) * sizeof(double));
            NX_ALLOC(c->lightGuide, (size_t)guide * 4);
            NX_ALLOC(c->lightScanTemp, std::max<size_t>(scanBytes, 16));
            c->lightScanBytes = scanBytes;
        }
        c->lightEntries = (uint32_t)n;
        c->lightGuideSize = guide;
        c->hostLightBase.swap(base);
        c->hostInstLight.swap(instLight);
        c->h.lightTable = n ? c->lightTable.as<LightEntry>() : nullptr;
        c->h.lightGuide = n ? c->lightGuide.as<uint32_t>() : nullptr;
        c->h.lightBase = c->lightBase.as<uint32_t>();
        c->h.instLight = c->instLight.as<uint32_t>();
        c->h.lightHeader = c->lightHeader.as<LightHeader>();
        c->h.lightEntries = c->lightEntries;
        c->h.lightGuideSize = c->lightGuideSize;
        c->stateDirty = true;
        NX_TRY(upload_state(c));
    }
    if (c->lightEntries == 0u) {
        NX_HIP(hipMemsetAsync(c->lightHeader.p, 0, sizeof(LightHeader), c->stream));  // valid = 0: no mesh-light samples
    } else {
        // the emissive maps' means, for the maps uploaded since the last build
        const size_t maps = c->emissiveMaps.size();
        if (c->lightMapMeans < maps) {
            if (c->lightMapMeanCapacity < maps) {
                NX_SYNC_ALL(c);
                NX_ALLOC(c->lightMapMean, 2 * maps * 16);
                NX_ALLOC(c->lightMapMean64, 2 * maps * 32);
                c->lightMapMeanCapacity = 2 * maps;
                c->lightMapMeans = 0;
            }
            for (size_t m = c->lightMapMeans; m < maps; m++) {
                const TextureHost& th = c->emissiveMaps[m];
                const TextureDev t{th.texels.as<uint32_t>(), th.width, th.height};
                NX_TRY(light_map_mean(c->stream, t, c->srgbLut.as<float>(), c->lightMapMean.as<float>() + 4 * m, c->lightMapMean64.as<double>() + 4 * m));
            }
            c->lightMapMeans = maps;
        }
        LightBuild b{};
        b.shadeInst = c->shadeInst.as<ShadeInst>();
        b.lights = c->lights.as<nx_light>();
        b.lightBase = c->lightBase.as<uint32_t>();
        b.mapMean = c->lightMapMean.as<float>();
        b.weight = c->lightWeight.as<double>();
        b.prefix = c->lightPrefix.as<double>();
        b.table = c->lightTable.as<LightEntry>();
        b.guide = c->lightGuide.as<uint32_t>();
        b.header = c->lightHeader.as<LightHeader>();
        b.lightCount = (uint32_t)nLights;
        b.entries = c->lightEntries;
        b.guideSize = c->lightGuideSize;
        NX_TRY(light_table_build(c->stream, b, c->lightScanTemp.p, c->lightScanBytes));
    }
    NX_TRY(refresh_light_tree(c));  // (NXHIP_LIGHT_IMPORTANCE_POSITION: the tree over the table just built, behind it in stream order)
    // passes on the other slots' streams must not start on a table half built
    if (slot_count(c) > 1) NX_HIP(hipStreamSynchronize(c->stream));
    c->lightTableDirty = false;
    return NXHIP_OK;
}

extern "C" {

// ---- feature buffers and the denoiser (nx_aov.hip) ---------------------------------------------------

int nxhip_set_aov(nxhip_ctx* c, int on)
{
    NX_CHECK_CTX(c);
    if ((on != 0) == c->aov) return NXHIP_OK;
    if (on && c->frameNumber != 0u) return fail_invalid("nxhip_set_aov: frames have been accumulated without feature buffers - reset the frame number first (colour and features must cover the same frames)");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    if (on) {
        const size_t full = std::max<size_t>((size_t)c->width * c->height, c->localCount);
        DevBuf a, n;  // all or nothing
        if (!a.alloc(full * 16) || !n.alloc(full * 16)) return NXHIP_ERR_HIP;
        NX_HIP(hipMemset(a.p, 0, full * 16));
        NX_HIP(hipMemset(n.p, 0, full * 16));
        c->aovAccumAlbedo = std::move(a);
        c->aovAccumNormalDepth = std::move(n);
    } else {
        c->aovAccumAlbedo.release();
        c->aovAccumNormalDepth.release();
        for (uint32_t k = 0; k < slot_count(c); k++) {
            slot_at(c, k)->aovAlbedo.release();
            slot_at(c, k)->aovNormalDepth.release();
        }
        release_denoise_planes(c);
    }
    c->aov = on != 0;
    c->h.aovAccumAlbedo = c->aovAccumAlbedo.as<float4>();
    c->h.aovAccumNormalDepth = c->aovAccumNormalDepth.as<float4>();
    c->stateDirty = true;  // (the pass graphs follow by their flavor: kFlavorAov)
    return NXHIP_OK;
}

static int aov_required(nxhip_ctx* c, const char* who)
{
    if (!c->aov) return fail_invalid(std::string(who) + ": the feature buffers are off (nxhip_set_aov)");
    return NXHIP_OK;
}

int nxhip_read_aov(nxhip_ctx* c, float* albedo4, float* normalDepth4)
{
    NX_CHECK_CTX(c);
    NX_TRY(aov_required(c, "nxhip_read_aov"));
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    if (albedo4) NX_HIP(hipMemcpy(albedo4, c->aovAccumAlbedo.p, (size_t)c->localCount * 16, hipMemcpyDeviceToHost));
    if (normalDepth4) NX_HIP(hipMemcpy(normalDepth4, c->aovAccumNormalDepth.p, (size_t)c->localCount * 16, hipMemcpyDeviceToHost));
    return NXHIP_OK;
}

int nxhip_read_aov_frame(nxhip_ctx* c, float* albedo4, float* normalDepth4)
{
    NX_CHECK_CTX(c);
    NX_TRY(aov_required(c, "nxhip_read_aov_frame"));
    const PassSlot* q = c->lastRendered ? c->lastRendered : static_cast<PassSlot*>(c);
    const size_t bytes = (size_t)(c->adaptive && c->lastRendered ? q->passPixels * q->frames : c->pathCount) * 16;
    if (!q->aovAlbedo.p || !q->aovNormalDepth.p || q->aovAlbedo.bytes < bytes || q->aovNormalDepth.bytes < bytes)
        return fail_invalid("nxhip_read_aov_frame: no pass has been rendered with the feature buffers on (or its queues were released)");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    if (albedo4) NX_HIP(hipMemcpy(albedo4, q->aovAlbedo.p, bytes, hipMemcpyDeviceToHost));
    if (normalDepth4) NX_HIP(hipMemcpy(normalDepth4, q->aovNormalDepth.p, bytes, hipMemcpyDeviceToHost));
    return NXHIP_OK;
}

int nxhip_write_aov(nxhip_ctx* c, const float* albedo4, const float* normalDepth4)
{
    NX_CHECK_CTX(c);
    NX_TRY(aov_required(c, "nxhip_write_aov"));
    if (c->adaptive) return fail_invalid("nxhip_write_aov: adaptive sampling is on (the sample counts have no checkpoint form)");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    if (albedo4) NX_HIP(hipMemcpy(c->aovAccumAlbedo.p, albedo4, (size_t)c->localCount * 16, hipMemcpyHostToDevice));
    if (normalDepth4) NX_HIP(hipMemcpy(c->aovAccumNormalDepth.p, normalDepth4, (size_t)c->localCount * 16, hipMemcpyHostToDevice));
    return NXHIP_OK;
}

// ---- adaptive sampling (nx_adaptive.hip) ------------------------------------------------------------

int nxhip_adaptive_defaults(nx_adaptive_params* p)
{
    if (!p) return fail_invalid("nxhip_adaptive_defaults: null destination");
    // (starting values, not tuned)
    p->threshold = 0.05f;
    p->lumFloor = 0.01f;
    p->minSamples = 16u;
    p->cull = 1u;
    return NXHIP_OK;
}

static int adaptive_required(nxhip_ctx* c, const char* who)
{
    if (!c->adaptive) return fail_invalid(std::string(who) + ": adaptive sampling is off (nxhip_set_adaptive)");
    return NXHIP_OK;
}

int nxhip_set_adaptive(nxhip_ctx* c, const nx_adaptive_params* p)
{
    NX_CHECK_CTX(c);
    if (!p) {
        if (!c->adaptive) return NXHIP_OK;
        NX_HIP(hipSetDevice(c->device));
        const int rcFold = nxhip_accumulate(c);  // (a pending pass was rendered through the active set: it is folded the way it was rendered)
        if (rcFold != NXHIP_OK) return rcFold;
        NX_SYNC_ALL(c);
        c->adaptive = false;
        adaptive_release(c);
        c->activeCount = c->localCount;
        publish_pixel_set(c);  // the base set again
        return NXHIP_OK;
    }
    if (!(p->threshold >= 0.0f) || !std::isfinite(p->threshold) || !(p->lumFloor > 0.0f) || !std::isfinite(p->lumFloor))
        return fail_invalid("nxhip_set_adaptive: threshold must be a finite number >= 0 and lumFloor a finite number > 0");
    if (c->h.rngMode != NX_RNG_PIXEL_KEYED)
        return fail_invalid("nxhip_set_adaptive: needs NX_RNG_PIXEL_KEYED (a path's radiance must depend on its pixel and frame only, not on a queue slot)");
    if (c->mgpuComm) return fail_invalid("nxhip_set_adaptive: the context is part of a multi-GPU tile split (nxhip_mgpu_*)");
    if (c->adaptive) {  // new parameters for the statistics gathered so far
        c->adParams = *p;
        return NXHIP_OK;
    }
    if (c->frameNumber != 0u) return fail_invalid("nxhip_set_adaptive: frames have been accumulated without sample counts - reset the frame number first");
    NX_HIP(hipSetDevice(c->device));
    c->adaptive = true;
    c->adParams = *p;
    const int rc = adaptive_restart(c);
    if (rc != NXHIP_OK) {
        c->adaptive = false;
        adaptive_release(c);
        publish_pixel_set(c);
    }
    return rc;
}

int nxhip_adaptive_update(nxhip_ctx* c, uint32_t* activePixels, uint32_t* activeBlocks)
{
    NX_CHECK_CTX(c);
    NX_TRY(adaptive_required(c, "nxhip_adaptive_update"));
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(nxhip_accumulate(c));  // (nothing pending: nothing)
    // behind the accumulates, on the context's stream: decide, compact, and — when blocks are culled — the new active set in place
    // (entry k of the new set comes from a base index at or behind the one entry k held, and the kernels read the base arrays only)
    const bool cull = c->adParams.cull != 0u;
    NX_TRY(adaptive_compact(c, true, cull));
    NX_SYNC_ALL(c);
    c->unsettledPixels = c->adHostTotals[0];
    c->unsettledBlocks = c->adHostTotals[1];
    if (cull) {
        c->activeCount = c->unsettledPixels;
        publish_pixel_set(c);  // to every slot's device state before the next pass (upload_state)
    }
    if (activePixels) *activePixels = c->unsettledPixels;
    if (activeBlocks) *activeBlocks = c->unsettledBlocks;
    return NXHIP_OK;
}

int nxhip_render_adaptive(nxhip_ctx* c, uint32_t maxFrames, uint32_t interval, uint32_t* framesRendered, uint32_t* activePixels)
{
    NX_CHECK_CTX(c);
    if (framesRendered) *framesRendered = 0u;
    NX_TRY(adaptive_required(c, "nxhip_render_adaptive"));
    if (interval == 0u) return fail_invalid("nxhip_render_adaptive: interval must be at least 1");
    uint32_t issued = 0u;
    int rc = NXHIP_OK;
    while (rc == NXHIP_OK && c->unsettledBlocks != 0u && issued < maxFrames) {
        const uint32_t n = std::min(interval, maxFrames - issued), pixels = std::max(1u, pass_pixels(c));
        // frames per pass of this interval: what the queues already hold (and a caller's radiance buffer, if one is bound)
        size_t room = c->queueCapacity;
        if (c->radianceBoundCapacity != 0) room = std::min(room, c->radianceBoundCapacity);
        const uint32_t per = (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(n, 1024), room / pixels));
        for (uint32_t done = 0; done < n && rc == NXHIP_OK; done += per) {
            rc = render_pass(c, std::min(per, n - done));
            if (rc == NXHIP_OK) rc = nxhip_accumulate(c);
        }
        if (rc == NXHIP_OK) rc = nxhip_adaptive_update(c, nullptr, nullptr);
        if (rc == NXHIP_OK) issued += n;
    }
    if (framesRendered) *framesRendered = issued;
    if (activePixels) *activePixels = c->unsettledPixels;
    return rc;
}

int nxhip_read_sample_counts(nxhip_ctx* c, uint32_t* counts)
{
    NX_CHECK_CTX(c);
    NX_TRY(adaptive_required(c, "nxhip_read_sample_counts"));
    if (!counts) return fail_invalid("null destination");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    NX_HIP(hipMemcpy(counts, c->adCount.p, (size_t)c->localCount * 4, hipMemcpyDeviceToHost));
    return NXHIP_OK;
}

int nxhip_read_noise_stats(nxhip_ctx* c, float* meanM2)
{
    NX_CHECK_CTX(c);
    NX_TRY(adaptive_required(c, "nxhip_read_noise_stats"));
    if (!meanM2) return fail_invalid("null destination");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    NX_HIP(hipMemcpy(meanM2, c->adStats.p, (size_t)c->localCount * 8, hipMemcpyDeviceToHost));
    return NXHIP_OK;
}

int nxhip_read_block_noise(nxhip_ctx* c, float* blockMax, uint8_t* active, uint32_t capacity, uint32_t* blocks)
try {
    NX_CHECK_CTX(c);
    NX_TRY(adaptive_required(c, "nxhip_read_block_noise"));
    if (blocks) *blocks = c->adBlocks;
    if (!blockMax && !active) return NXHIP_OK;
    if (capacity < c->adBlocks) return fail_invalid("nxhip_read_block_noise: capacity below the number of blocks");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    if (blockMax) NX_HIP(hipMemcpy(blockMax, c->adBlockMax.p, (size_t)c->adBlocks * 4, hipMemcpyDeviceToHost));
    if (active) {
        std::vector<uint32_t> flags(c->adBlocks);
        NX_HIP(hipMemcpy(flags.data(), c->adBlockFlag.p, (size_t)c->adBlocks * 4, hipMemcpyDeviceToHost));
        for (uint32_t b = 0; b < c->adBlocks; b++) active[b] = flags[b] != 0u ? 1 : 0;
    }
    return NXHIP_OK;
} NX_CATCH("nxhip_read_block_noise")

int nxhip_read_active_map(nxhip_ctx* c, uint32_t* baseLocalIndex, uint32_t capacity, uint32_t* count)
{
    NX_CHECK_CTX(c);
    NX_TRY(adaptive_required(c, "nxhip_read_active_map"));
    const uint32_t n = pass_pixels(c);
    if (count) *count = n;
    if (!baseLocalIndex) return NXHIP_OK;
    if (capacity < n) return fail_invalid("nxhip_read_active_map: capacity below the number of active paths");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    if (n) NX_HIP(hipMemcpy(baseLocalIndex, c->adActiveIndex.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return NXHIP_OK;
}

int nxhip_denoise_defaults(nx_denoise_params* p)
{
    if (!p) return fail_invalid("nxhip_denoise_defaults: null destination");
    // (chosen from the sweep of profiles/r09_denoise.txt: Cornell box 256 x 256, 16 frames, error against 4 096 frames)
    p->iterations = 5u;
    p->sigmaColor = 2.5f;
    p->sigmaNormal = 0.3f;
    p->sigmaAlbedo = 0.2f;
    p->sigmaDepth = 0.025f;
    return NXHIP_OK;
}

static float inverse_square(float sigma)
{
    const float s2 = sigma * sigma;
    return std::min(1.0f / s2, 3.402823466e38f);  // (a sigma whose square underflows: 0 x "infinity" must not become a NaN)
}

int nxhip_denoise(nxhip_ctx* c, const nx_denoise_params* params)
{
    NX_CHECK_CTX(c);
    NX_TRY(aov_required(c, "nxhip_denoise"));
    nx_denoise_params p;
    (void)nxhip_denoise_defaults(&p);
    if (params) p = *params;
    if (p.iterations > 6u) return fail_invalid("nxhip_denoise: iterations must be in [0, 6]");
    for (const float sigma : {p.sigmaColor, p.sigmaNormal, p.sigmaAlbedo, p.sigmaDepth})
        if (!(sigma > 0.0f) || !std::isfinite(sigma)) return fail_invalid("nxhip_denoise: every sigma must be a positive finite number");
    const uint32_t full = c->width * c->height;
    if (!c->coversFrame || c->localCount != full)
        return fail_invalid("nxhip_denoise: the filter works in image space and needs a context that renders the full frame (NXHIP_ORDER_ROWS / NXHIP_ORDER_TILES); "
                            "this one renders a tile split (nxhip_set_pixel_map with a partial set, nxhip_mgpu_*)");
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(upload_state(c));
    if (!c->dnRgba8.p) {
        DevBuf planes[5], rgba;  // all or nothing
        for (DevBuf& b : planes)
            if (!b.alloc((size_t)full * 16)) return NXHIP_ERR_HIP;
        if (!rgba.alloc((size_t)full * 4)) return NXHIP_ERR_HIP;
        c->dnColour = std::move(planes[0]);
        c->dnAlbedo = std::move(planes[1]);
        c->dnNormalDepth = std::move(planes[2]);
        c->dnPing = std::move(planes[3]);
        c->dnPong = std::move(planes[4]);
        c->dnRgba8 = std::move(rgba);
    }
    // on the context's stream: behind the accumulates already issued
    NX_TRY(launch_now(c, make_launch(kernels::denoise_gather(), c->wideBlocks, kWideBlock, NXHIP_K_ACCUMULATE, c->dState.as<DeviceState>(), c->dnColour.as<float4>(),
                                   c->dnAlbedo.as<float4>(), c->dnNormalDepth.as<float4>(), p.iterations == 0u ? c->dnRgba8.as<uint32_t>() : nullptr)));
    bool forceDirect = false;  // (sweeps only: the plane variant for steps 1 and 2 too)
    if (const char* on = std::getenv("NX_TUNING_KNOBS"); on && std::atoi(on) == 1)
        if (const char* e = std::getenv("NX_DENOISE_DIRECT")) forceDirect = std::atoi(e) != 0;
    const void* in = c->dnColour.p;
    for (uint32_t i = 0; i < p.iterations; i++) {
        void* out = (i & 1u) ? c->dnPong.p : c->dnPing.p;
        const int step = 1 << i;
        DenoiseLaunch dn{};
        dn.colour = static_cast<const float4*>(in);
        dn.albedo = c->dnAlbedo.as<float4>();
        dn.normalDepth = c->dnNormalDepth.as<float4>();
        dn.out = static_cast<float4*>(out);
        dn.rgba8 = i + 1u == p.iterations ? c->dnRgba8.as<uint32_t>() : nullptr;
        dn.width = (int32_t)c->width;
        dn.height = (int32_t)c->height;
        dn.step = step;
        dn.invColour = inverse_square(p.sigmaColor * std::ldexp(1.0f, -(int)i));
        dn.invNormal = inverse_square(p.sigmaNormal);
        dn.invAlbedo = inverse_square(p.sigmaAlbedo);
        dn.sigmaDepth = p.sigmaDepth;
        NX_TRY(launch_now(c, make_launch(kernels::denoise_iteration(step, forceDirect), dim3((c->width + 31u) / 32u, (c->height + 7u) / 8u), dim3(32, 8), NXHIP_K_ACCUMULATE, dn)));
        in = out;
    }
    c->denoised = in;
    return NXHIP_OK;
}

int nxhip_read_denoised(nxhip_ctx* c, float* rgb)
{
    NX_CHECK_CTX(c);
    if (!c->denoised) return fail_invalid("nxhip_read_denoised: nxhip_denoise has not run since the pixel set last changed");
    return read_float4_as_float3(c, c->denoised, c->width * c->height, rgb);
}

int nxhip_read_denoised_rgba8(nxhip_ctx* c, uint32_t* dst)
{
    NX_CHECK_CTX(c);
    if (!dst) return fail_invalid("null destination");
    if (!c->denoised) return fail_invalid("nxhip_read_denoised_rgba8: nxhip_denoise has not run since the pixel set last changed");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    NX_HIP(hipMemcpy(dst, c->dnRgba8.p, (size_t)c->width * c->height * 4, hipMemcpyDeviceToHost));
    return NXHIP_OK;
}

int nxhip_set_light_sampling(nxhip_ctx* c, int mode)
{
    NX_CHECK_CTX(c);
    if (mode != NXHIP_LIGHTS_UNIFORM && mode != NXHIP_LIGHTS_POWER) return fail_invalid("nxhip_set_light_sampling: unknown mode");
    if (mode == c->lightSampling) return NXHIP_OK;
    // (frames accumulated so far stay: the expectation is the same.  The pass graphs are keyed by the mode: pass_flavor)
    c->lightSampling = mode;
    c->lightTableDirty = true;
    return NXHIP_OK;
}

int nxhip_set_light_importance(nxhip_ctx* c, int importance)
{
    NX_CHECK_CTX(c);
    if (importance != NXHIP_LIGHT_IMPORTANCE_POWER && importance != NXHIP_LIGHT_IMPORTANCE_POSITION) return fail_invalid("nxhip_set_light_importance: unknown importance");
    if (importance == c->lightImportance) return NXHIP_OK;
    // (frames accumulated so far stay: the expectation is the same.  The pass graphs are keyed by it: pass_flavor.  Remembered in
    //  every mode; the tree is built or dropped by the next refresh_light_table in POWER mode)
    c->lightImportance = importance;
    c->lightTableDirty = true;
    return NXHIP_OK;
}

uint32_t nxhip_light_tree_leaves_for(uint32_t entries)
{
    if (entries == 0u || entries > kLightTreeLeavesMax) return 0u;
    uint32_t g = 1u;
    while (g < entries) g <<= 1;
    return g;
}

// What a render does before its pass, for the hooks that read the light table
static int light_table_ready(nxhip_ctx* c, const char* who)
{
    NX_CHECK_CTX(c);
    if (c->lightSampling != NXHIP_LIGHTS_POWER) return fail_invalid(std::string(who) + ": the context is not in NXHIP_LIGHTS_POWER");
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(check_scene_ready(c));
    if (c->shadeInstDirty) NX_TRY(refresh_shade_inst(c));
    NX_TRY(upload_state(c));
    NX_TRY(refresh_updated_blas(c));
    return refresh_light_table(c);
}

int nxhip_read_light_table(nxhip_ctx* c, float* cdf, uint32_t* entryLight, uint32_t capacity, uint32_t* lightBase, uint32_t* entries)
try {
    NX_TRY(light_table_ready(c, "nxhip_read_light_table"));
    const uint32_t n = c->lightEntries;
    if (entries) *entries = n;
    if (lightBase) std::memcpy(lightBase, c->hostLightBase.data(), c->hostLightBase.size() * 4);
    if (!cdf && !entryLight) return NXHIP_OK;
    if (capacity < n) return fail_invalid("nxhip_read_light_table: destination too small");
    std::vector<LightEntry> table(n);
    NX_SYNC_ALL(c);
    if (n) NX_HIP(hipMemcpy(table.data(), c->lightTable.p, (size_t)n * sizeof(LightEntry), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        if (cdf) cdf[i] = table[i].cdf;
        if (entryLight) entryLight[i] = table[i].light;
    }
    return NXHIP_OK;
} NX_CATCH("nxhip_read_light_table")

// ... and for a pick: the table (brought up to date) has an entry, and weights that sum to something
static int light_table_pickable(nxhip_ctx* c)
{
    if (c->lightEntries == 0u) return fail_invalid("nxhip_light_pick_batch: the light table is empty (no mesh light has a triangle)");
    // a table whose weights sum to nothing is never sampled by the renderer (its cdf is a filler of ones): the hook refuses it too
    LightHeader header{};
    NX_SYNC_ALL(c);
    NX_HIP(hipMemcpy(&header, c->lightHeader.p, sizeof header, hipMemcpyDeviceToHost));
    if (header.valid == 0u) return fail_invalid("nxhip_light_pick_batch: the light table is invalid (the lights' weights sum to nothing): nothing can be picked");
    return NXHIP_OK;
}

int nxhip_light_pick_batch(nxhip_ctx* c, const float* u, uint32_t count, uint32_t* entry, float* prob)
try {
    NX_CHECK_CTX(c);
    if ((!u || !entry || !prob) && count) return fail_invalid("nxhip_light_pick_batch: null buffer");
    // before anything is launched: floor(u G) of a u outside [0, 1) — or of a NaN — is no index of the guide table
    if (!all_unit(u, count)) return fail_invalid("nxhip_light_pick_batch: u must be in [0, 1)");
    NX_TRY(light_table_ready(c, "nxhip_light_pick_batch"));
    if (count == 0) return NXHIP_OK;
    NX_TRY(light_table_pickable(c));
    HookBatch b(c, count);
    const float* dU = b.in(u, 1);
    uint32_t* dEntry = b.out(entry, 1);
    float* dProb = b.out(prob, 1);
    return b.run(kernels::light_pick(), c->lightTable.as<LightEntry>(), c->lightGuide.as<uint32_t>(), c->lightGuideSize, c->lightEntries, dU, count, dEntry, dProb);
} NX_CATCH("nxhip_light_pick_batch")

// ---- the light tree's hooks --------------------------------------------------------------------------------

static int light_tree_ready(nxhip_ctx* c, const char* who)
{
    NX_CHECK_CTX(c);
    if (c->lightSampling != NXHIP_LIGHTS_POWER || c->lightImportance != NXHIP_LIGHT_IMPORTANCE_POSITION)
        return fail_invalid(std::string(who) + ": the context is not in NXHIP_LIGHTS_POWER with NXHIP_LIGHT_IMPORTANCE_POSITION");
    return light_table_ready(c, who);
}

// ... and for a pick or a probability: the tree (brought up to date) has a leaf, and weights that sum to something
static int light_tree_pickable(nxhip_ctx* c, const char* who)
{
    if (c->lightEntries == 0u || c->lightTreeLeaves == 0u) return fail_invalid(std::string(who) + ": the light tree is empty (no mesh light has a triangle)");
    LightHeader header{};
    NX_SYNC_ALL(c);
    NX_HIP(hipMemcpy(&header, c->lightHeader.p, sizeof header, hipMemcpyDeviceToHost));
    if (header.valid == 0u) return fail_invalid(std::string(who) + ": the light tree is invalid (the lights' weights sum to nothing): nothing can be picked");
    return NXHIP_OK;
}

int nxhip_read_light_tree(nxhip_ctx* c, float* nodes8, uint32_t* order, uint32_t capacityNodes, uint32_t* leaves, uint32_t* entries)
try {
    NX_DEBUG_HOOK("nxhip_read_light_tree");  // (first: a release library refuses whatever it is handed)
    NX_TRY(light_tree_ready(c, "nxhip_read_light_tree"));
    const uint32_t n = c->lightEntries, g = c->lightTreeLeaves;
    if (leaves) *leaves = g;
    if (entries) *entries = n;
    if (!nodes8 && !order) return NXHIP_OK;
    if (g == 0u) return fail_invalid("nxhip_read_light_tree: the light tree is empty (no mesh light has a triangle)");
    if (capacityNodes < 2u * g) return fail_invalid("nxhip_read_light_tree: destination too small");
    static_assert(sizeof(LightNode) == 8 * sizeof(float), "a node is read back as eight words");
    NX_SYNC_ALL(c);
    if (nodes8) NX_HIP(hipMemcpy(nodes8, c->lightTreeNodes.p, 2 * (size_t)g * sizeof(LightNode), hipMemcpyDeviceToHost));
    if (order) NX_HIP(hipMemcpy(order, c->lightTreeOrder.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return NXHIP_OK;
} NX_CATCH("nxhip_read_light_tree")

int nxhip_light_tree_pick_batch(nxhip_ctx* c, const float* points3, const float* u, uint32_t count, uint32_t* entry, float* prob)
try {
    NX_DEBUG_HOOK("nxhip_light_tree_pick_batch");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    if ((!points3 || !u || !entry || !prob) && count) return fail_invalid("nxhip_light_tree_pick_batch: null buffer");
    if (!all_finite(points3, 3 * (size_t)count)) return fail_invalid("nxhip_light_tree_pick_batch: a point is not finite");
    if (!all_unit(u, count)) return fail_invalid("nxhip_light_tree_pick_batch: u must be in [0, 1)");
    NX_TRY(light_tree_ready(c, "nxhip_light_tree_pick_batch"));
    if (count == 0) return NXHIP_OK;
    NX_TRY(light_tree_pickable(c, "nxhip_light_tree_pick_batch"));
    HookBatch b(c, count);
    const float* dP = b.in(points3, 3);
    const float* dU = b.in(u, 1);
    uint32_t* dEntry = b.out(entry, 1);
    float* dProb = b.out(prob, 1);
    return b.run(kernels::light_tree_pick(), c->lightTreeNodes.as<LightNode>(), c->lightTreeLeaves, dP, dU, count, dEntry, dProb);
} NX_CATCH("nxhip_light_tree_pick_batch")

int nxhip_light_tree_prob_batch(nxhip_ctx* c, const float* points3, const uint32_t* entry, uint32_t count, float* prob)
try {
    NX_DEBUG_HOOK("nxhip_light_tree_prob_batch");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    if ((!points3 || !entry || !prob) && count) return fail_invalid("nxhip_light_tree_prob_batch: null buffer");
    if (!all_finite(points3, 3 * (size_t)count)) return fail_invalid("nxhip_light_tree_prob_batch: a point is not finite");
    NX_TRY(light_tree_ready(c, "nxhip_light_tree_prob_batch"));
    // (before anything is launched: an entry past the table would index slotOf wildly)
    for (uint32_t k = 0; k < count; k++)
        if (entry[k] >= c->lightEntries) return fail_invalid("nxhip_light_tree_prob_batch: no such entry");
    if (count == 0) return NXHIP_OK;
    NX_TRY(light_tree_pickable(c, "nxhip_light_tree_prob_batch"));
    HookBatch b(c, count);
    const float* dP = b.in(points3, 3);
    const uint32_t* dEntry = b.in(entry, 1);
    float* dProb = b.out(prob, 1);
    return b.run(kernels::light_tree_prob(), c->lightTreeNodes.as<LightNode>(), c->lightTreeLeaves, c->lightTreeSlotOf.as<uint32_t>(), dP, dEntry, count, dProb);
} NX_CATCH("nxhip_light_tree_prob_batch")

}  // extern "C"

uint64_t nxd::layout_stamp_features() { return layout_stamp(); }
