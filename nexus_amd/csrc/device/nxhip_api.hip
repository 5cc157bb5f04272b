// nxhip_api.hip — implementation of the C-ABI device layer declared in include/nexus_hip.h.
// Each entry point cites, in the header, the reference interface it replaces; the nxhip_*.hip units are the HIP runtime plumbing
// behind it.  This one: errors, the context's lifecycle, synchronisation, queue and pixel-set allocation, settings.  The others:
// nxhip_scene.hip (uploads, builders, refits), nxhip_render.hip (the per-pass hipGraph, accumulate, read-backs), nxhip_features.hip
// (feature buffers, denoiser, adaptive sampling, light table), nxhip_hooks.hip (kernel-level test hooks, kernel times),
// nxhip_multigpu.hip; what they share is declared in nx_host.h.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <new>
#include <thread>
#include <string>
#include <vector>

#include "nx_host.h"

namespace nxd {

static thread_local std::string g_lastError;

void set_error(const std::string& msg) { g_lastError = msg; }

bool hip_ok(hipError_t e, const char* what, const char* file, int line)
{
    if (e == hipSuccess) return true;
    // the failure is reported through the status + message of this call; it must not stay behind as HIP's "last error"
    // (library code that polls hipGetLastError after its launches — rocPRIM does — would report it as its own)
    (void)hipGetLastError();
    char buf[512];
    std::snprintf(buf, sizeof buf, "HIP error %d (%s) in '%s' at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    set_error(buf);
    return false;
}

bool DevBuf::alloc(size_t n)
{
    release();
    if (n == 0) n = 16;
    void* q = nullptr;
    if (!hip_ok(hipMalloc(&q, n), "hipMalloc", __FILE__, __LINE__)) return false;
    p = q;
    bytes = n;
    return true;
}

}  // namespace nxd

using namespace nxd;

int nxd::fail_invalid(const char* msg)
{
    set_error(msg);
    return NXHIP_ERR_INVALID;
}
int nxd::fail_invalid(const std::string& msg) { return fail_invalid(msg.c_str()); }

// Every translation unit of this library must have been compiled with the same device-side layouts (nx_device.h layout_stamp):
// the host code here fills DeviceState / Counters / InstTrav blocks that the kernels of the other units read.
static int check_layouts()
{
    const struct { const char* unit; uint64_t stamp; } units[] = {
        {"nx_trace.hip", layout_stamp_trace()}, {"nx_wavefront.hip", layout_stamp_wavefront()}, {"nx_wavefront_detail.hip", layout_stamp_wavefront_detail()}, {"nx_wavefront_solid.hip", layout_stamp_wavefront_solid()}, {"nx_wavefront_metal.hip", layout_stamp_wavefront_metal()}, {"nx_hook_kernels.hip", layout_stamp_hook_kernels()}, {"nx_medium.hip", layout_stamp_medium()}, {"nx_refit.hip", layout_stamp_refit()}, {"nx_skin.hip", layout_stamp_skin()},
        {"nx_lbvh.hip", layout_stamp_lbvh()}, {"nxhip_multigpu.hip", layout_stamp_multigpu()}, {"nx_entry.hip", layout_stamp_entry()}, {"nx_aov.hip", layout_stamp_aov()},
        {"nx_adaptive.hip", layout_stamp_adaptive()}, {"nx_lights.hip", layout_stamp_lights()}, {"nx_envmap.hip", layout_stamp_envmap()}, {"nx_sky.hip", layout_stamp_sky()}, {"nxhip_scene.hip", layout_stamp_scene()},
        {"nxhip_render.hip", layout_stamp_render()}, {"nxhip_features.hip", layout_stamp_features()}, {"nxhip_hooks.hip", layout_stamp_hooks()},
    };
    for (const auto& u : units) {
        if (u.stamp != layout_stamp()) {
            char buf[320];
            std::snprintf(buf, sizeof buf, "libnexus_amd.so was linked from objects of different source states: %s was compiled with device layout stamp %016llx, "
                          "nxhip_api.hip with %016llx (DeviceState / Counters / record strides differ) - rebuild the library from one tree (make clean && make)",
                          u.unit, (unsigned long long)u.stamp, (unsigned long long)layout_stamp());
            set_error(buf);
            return NXHIP_ERR_ABI;
        }
    }
    return NXHIP_OK;
}

uint64_t nxhip_abi_stamp(void) { return nxhip_header_abi_stamp(); }

int nxhip_check_library(uint64_t callerStamp)
{
    if (callerStamp != nxhip_abi_stamp()) {
        char buf[320];
        std::snprintf(buf, sizeof buf, "ABI mismatch: the caller was built against a nexus_hip.h / nexus_pod.h with stamp %016llx, this library (API version %d) has %016llx - "
                      "a stale or foreign libnexus_amd.so (NEXUS_AMD_LIB, LD_LIBRARY_PATH), or bindings of another version",
                      (unsigned long long)callerStamp, NXHIP_API_VERSION, (unsigned long long)nxhip_abi_stamp());
        set_error(buf);
        return NXHIP_ERR_ABI;
    }
    return check_layouts();
}

// Wait for everything the context has issued, on every slot's stream (scene edits, re-allocations, read-backs).
int nxd::sync_all(nxhip_ctx* c)
{
    for (uint32_t k = 0; k < slot_count(c); k++) {
        PassSlot* s = slot_at(c, k);
        if (s->stream) NX_HIP(hipStreamSynchronize(s->stream));
    }
    return NXHIP_OK;
}

void nxd::invalidate_graph(nxhip_ctx* c)
{
    // a replay may still be executing (render calls are asynchronous): destroying its exec, graph and timing events
    // under it is not allowed.  Not a hot path: settings / mode / timing changes only.
    for (uint32_t k = 0; k < slot_count(c); k++) {
        PassSlot* s = slot_at(c, k);
        if (!s->graphs.empty() && s->stream) (void)hipStreamSynchronize(s->stream);
        for (auto& g : s->graphs) {
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
            if (g.graph) (void)hipGraphDestroy(g.graph);
        }
        s->graphs.clear();
    }
    for (auto& t : c->graphTimers) {
        if (t.start) (void)hipEventDestroy(t.start);
        if (t.stop) (void)hipEventDestroy(t.stop);
    }
    c->graphTimers.clear();
}

// Slots per queue region for a capacity of n paths (nx_device.h, Counters): an even share, 64-aligned, plus the slack a region
// may run over it; a queue buffer holds kQueueShards regions.
static size_t queue_region_cap(size_t n) { return ((n + kQueueShards * 64 - 1) / (kQueueShards * 64)) * 64 + kQueueShardSlack; }
static size_t queue_buffer_slots(size_t n) { return queue_region_cap(n) * kQueueShards; }
// entries per list of rays handed to the thin kernel (nx_trace.hip): a launch hands over at most DeviceState::thinLanes (16) rays per wave, 81 920 for a
// full grid if every wave handed over as many as it may; a list that runs over only makes the waves it has no room for finish their rays themselves
constexpr uint32_t kThinListEntries = 1u << 15;  // (x 2 lists x (4 B + a 320-byte ThinState) = 21 MB per slot)
static size_t scan_status_tiles(size_t n) { return n / (size_t)std::min(kLogicBlock, kShadeBlock) + 2; }

static TraceQueue trace_queue_of(const PassSlot* s)
{
    TraceQueue t{};
    t.rays[0] = TraceRays{s->trRayO.as<float4>(), s->trRayD.as<float4>(), s->trTp.as<float4>()};
    t.rays[1] = TraceRays{s->trRayO2.as<float4>(), s->trRayD2.as<float4>(), s->trTp2.as<float4>()};
    t.hit = s->trHit.as<float4>();
    t.hitInst = s->trHitInst.as<uint32_t>();
    return t;
}

// The queue pointers of a device-state block from a slot's buffers (a released buffer gives nullptr).
static void queue_pointers(const PassSlot* s, DeviceState& v)
{
    v.radiance = s->radiance.as<float4>();
    v.rayOrigin = s->rayOrigin.as<float4>();
    v.trace = trace_queue_of(s);
    v.shadow = ShadowQueue{s->shRayO.as<float4>(), s->shRayD.as<float4>(), s->shRadiance.as<float4>()};
    for (int m = 0; m < 4; m++) v.material[m] = MaterialQueue{s->mqHit[m].as<float4>(), s->mqDirInst[m].as<float4>(), s->mqTp[m].as<float4>()};
}

// The device-state block of a slot: the scene part of the host mirror plus the slot's own queues, counters and frame words.
static void compose_view(nxhip_ctx* c, PassSlot* s)
{
    DeviceState& v = s->view;
    v = c->h;
    if (s != static_cast<PassSlot*>(c)) queue_pointers(s, v);  // (slot 0's are in c->h already: an external radiance binding lives there)
    v.counters = s->counters.as<Counters>();
    v.frame = s->frame.as<FrameState>();
    v.scanStatus = s->scanStatus.as<unsigned long long>();
    v.materialMetal = MaterialQueue{s->mqMetal[0].as<float4>(), s->mqMetal[1].as<float4>(), s->mqMetal[2].as<float4>()};
    v.thinClosest = s->thinLists.as<uint32_t>();
    v.thinAny = s->thinLists.p ? s->thinLists.as<uint32_t>() + kThinListEntries : nullptr;
    v.thinCapacity = (s->thinLists.p && s->thinStates.p) ? kThinListEntries : 0u;
    v.thinStates = s->thinStates.as<ThinState>();
    v.entry = (c->entryPoints && s->entryTable.p) ? s->entryTable.as<EntryState>() : nullptr;
    // (adaptive sampling: the table keeps the base set's size, the pass walks the runs of the active set — whole blocks in base order)
    v.entryRuns = v.entry ? (c->adaptive ? (c->activeCount + 63u) / 64u : s->entryRuns) : 0u;
    v.aovAlbedo = c->aov ? s->aovAlbedo.as<float4>() : nullptr;  // (per slot, like the entry table; the running means are the context's: c->h)
    v.aovNormalDepth = c->aov ? s->aovNormalDepth.as<float4>() : nullptr;
    // queue regions: eight, or one spanning the buffer when slots are handed out in the reference's serial order
    const bool ordered = c->h.compactMode == NX_COMPACT_ORDERED;
    v.queueShards = ordered ? 1u : (uint32_t)kQueueShards;
    v.queueShardCap = (uint32_t)(ordered ? queue_buffer_slots(c->queueCapacity) : queue_region_cap(c->queueCapacity));
}

int nxd::upload_state(nxhip_ctx* c)
{
    if (!c->stateDirty) return NXHIP_OK;
    NX_SYNC_ALL(c);  // no pass in flight may see half of an edit
    for (uint32_t k = 0; k < slot_count(c); k++) {
        PassSlot* s = slot_at(c, k);
        compose_view(c, s);
        NX_HIP(hipMemcpy(s->dState.p, &s->view, sizeof(DeviceState), hipMemcpyHostToDevice));
    }
    c->stateDirty = false;
    return NXHIP_OK;
}

// A slot's queue buffers, in the order they are allocated: what one element takes and what decides how many there are.  The
// pipeline decides which buffers exist: SCAN has no material queues (192 B per path), CLASSIC no second set of rays (48 B).
enum class QueueKind { PerPath, Queue, Material, SecondSet };  // per path; queue (regions + slack); queue, CLASSIC only; queue, SCAN only
struct QueueBuf {
    DevBuf* buf;
    size_t elem;
    QueueKind kind;
};
static std::vector<QueueBuf> slot_queue_buffers(PassSlot* q)
{
    using K = QueueKind;
    std::vector<QueueBuf> v = {{&q->radiance, 16, K::PerPath}, {&q->rayOrigin, 16, K::PerPath}, {&q->trRayO, 16, K::Queue}, {&q->trRayD, 16, K::Queue}, {&q->trHit, 16, K::Queue},
                               {&q->trHitInst, 4, K::Queue}, {&q->trTp, 16, K::Queue}, {&q->shRayO, 16, K::Queue}, {&q->shRayD, 16, K::Queue}, {&q->shRadiance, 16, K::Queue}};
    for (int m = 0; m < 4; m++)
        for (DevBuf* b : {&q->mqHit[m], &q->mqDirInst[m], &q->mqTp[m]}) v.push_back({b, 16, K::Material});
    for (DevBuf* b : {&q->trRayO2, &q->trRayD2, &q->trTp2}) v.push_back({b, 16, K::SecondSet});
    return v;
}

// Queue / path-state buffers for n paths (contents undefined), and the device-state pointers to them.  All or nothing:
// the new set is allocated beside the old one and swapped in only when every allocation has succeeded, so a failed
// growth (out of device memory half-way through 25 buffers) leaves the context exactly as it was, still able to render
// at its previous capacity.
static int alloc_slot_queues(nxhip_ctx* c, PassSlot* q, size_t n)
{
    const std::vector<QueueBuf> bufs = slot_queue_buffers(q);
    const bool scan = scan_pipeline(c);
    std::vector<DevBuf> fresh(bufs.size());
    for (size_t i = 0; i < bufs.size(); i++) {  // (an unused buffer: size 0, which DevBuf::alloc turns into 16 bytes)
        const bool unused = bufs[i].kind == (scan ? QueueKind::Material : QueueKind::SecondSet);
        const size_t slots = unused ? 0 : bufs[i].kind == QueueKind::PerPath ? n : queue_buffer_slots(n);
        if (!fresh[i].alloc(slots * bufs[i].elem)) return NXHIP_ERR_HIP;  // `fresh` frees what it got; the context is untouched
    }
    // ordered compaction: status words of the tiles of the largest possible launch (a queue never holds more than n items;
    // tiles of the smaller of the two workgroup sizes), zeroed once — tag 0 is never a launch's serial
    DevBuf freshStatus;
    const size_t statusBytes = scan_status_tiles(n) * kScanWords * sizeof(unsigned long long);
    if (!freshStatus.alloc(statusBytes)) return NXHIP_ERR_HIP;
    NX_HIP(hipMemset(freshStatus.p, 0, statusBytes));
    DevBuf freshThin;  // (contents: whatever the trace launches of a level write before the thin kernel of that level reads)
    if (!freshThin.alloc((size_t)2 * kThinListEntries * sizeof(uint32_t))) return NXHIP_ERR_HIP;
    DevBuf freshThinStates;  // (entry k of a list and state k belong together: the wave that writes one writes the other)
    if (!freshThinStates.alloc((size_t)2 * kThinListEntries * sizeof(ThinState))) return NXHIP_ERR_HIP;
    // the per-path pair — radiance, and the paths' previous vertices: a read of an entry nobody has written yet is at least deterministic
    for (size_t i = 0; i < bufs.size(); i++)
        if (bufs[i].kind == QueueKind::PerPath) NX_HIP(hipMemset(fresh[i].p, 0, n * bufs[i].elem));
    NX_SYNC_ALL(c);  // nothing in flight may still use the old buffers
    for (size_t i = 0; i < bufs.size(); i++) *bufs[i].buf = std::move(fresh[i]);
    q->scanStatus = std::move(freshStatus);
    q->thinLists = std::move(freshThin);
    q->thinStates = std::move(freshThinStates);
    q->aovAlbedo.release();  // (sized by the capacity: the slot's next pass with feature buffers allocates them again, ensure_slot_aov)
    q->aovNormalDepth.release();
    q->scanEpoch = 0;
    q->pathCapacity = n;
    q->queuesScan = scan;
    if (q == static_cast<PassSlot*>(c)) {
        c->radianceBoundCapacity = 0;
        queue_pointers(c, c->h);
    }
    c->stateDirty = true;
    return NXHIP_OK;
}

// Give a slot's queue buffers back (nothing of it may be in flight: the caller has synchronised).
void nxd::release_slot_queues(nxhip_ctx* c, PassSlot* q)
{
    for (const QueueBuf& b : slot_queue_buffers(q)) b.buf->release();
    q->scanStatus.release();
    for (DevBuf& b : q->mqMetal) b.release();
    q->thinLists.release();
    q->thinStates.release();
    q->aovAlbedo.release();
    q->aovNormalDepth.release();
    q->pathCapacity = 0;
    if (q == static_cast<PassSlot*>(c)) queue_pointers(c, c->h);  // (all null now)
    c->stateDirty = true;
}

// A new nominal capacity: every slot that holds buffers is re-allocated (slot 0 last, so that a failure in an extra slot leaves
// slot 0 untouched); released slots allocate when they are next used.
int nxd::alloc_queues(nxhip_ctx* c, size_t n)
{
    for (uint32_t k = slot_count(c); k-- > 0;) {
        PassSlot* q = slot_at(c, k);
        if (k != 0 && q->pathCapacity == 0) continue;
        NX_TRY(alloc_slot_queues(c, q, n));
    }
    c->queueCapacity = n;
    return NXHIP_OK;
}

// Before a slot is used: its queues exist at the nominal capacity.
bool nxd::slot_queues_ready(const nxhip_ctx* c, const PassSlot* q) { return q->pathCapacity >= c->queueCapacity && q->pathCapacity > 0 && q->queuesScan == scan_pipeline(c); }

// The fifth material queue: three buffers as large as the other queues', for a slot whose next pass runs the classic pipeline over a table
// with an NX_MAT_METALROUGH.  A context that never does allocates nothing.
int nxd::ensure_metal_queue(nxhip_ctx* c, PassSlot* q)
{
    const size_t bytes = queue_buffer_slots(q->pathCapacity) * 16;
    if (q->mqMetal[0].p && q->mqMetal[0].bytes >= bytes) return NXHIP_OK;
    NX_SYNC_ALL(c);
    for (DevBuf& b : q->mqMetal) NX_ALLOC(b, bytes);
    c->stateDirty = true;
    return NXHIP_OK;
}

int nxd::ensure_slot_queues(nxhip_ctx* c, PassSlot* q)
{
    if (slot_queues_ready(c, q)) return NXHIP_OK;
    float4* const boundPtr = c->h.radiance;
    const size_t boundCap = c->radianceBoundCapacity;
    const int rc = alloc_slot_queues(c, q, std::max<size_t>(c->queueCapacity, 1));
    if (rc == NXHIP_OK && boundCap != 0 && q == static_cast<PassSlot*>(c)) {  // an external radiance binding survives
        c->h.radiance = boundPtr;
        c->radianceBoundCapacity = boundCap;
    }
    return rc;
}

void nxd::release_denoise_planes(nxhip_ctx* c)
{
    for (DevBuf* b : {&c->dnColour, &c->dnAlbedo, &c->dnNormalDepth, &c->dnPing, &c->dnPong, &c->dnRgba8}) b->release();
    c->denoised = nullptr;
}

// The pixel set as the kernels see it (DeviceState): the base set always, and the set the passes render — the same while adaptive
// sampling is off, the active part of it while it is on.  Uploaded to every slot before the next pass.
void nxd::publish_pixel_set(nxhip_ctx* c)
{
    DeviceState& h = c->h;
    h.baseCount = c->localCount;
    h.basePixelMap = c->pixelMap.as<uint32_t>();
    h.localCount = pass_pixels(c);
    h.pixelMap = c->adaptive ? c->adPixelMap.as<uint32_t>() : c->pixelMap.as<uint32_t>();
    h.activeIndex = c->adaptive ? c->adActiveIndex.as<uint32_t>() : nullptr;
    h.adCount = c->adaptive ? c->adCount.as<uint32_t>() : nullptr;
    h.adStats = c->adaptive ? c->adStats.as<float2>() : nullptr;
    h.framesPerPass = c->framesPerPass;
    h.pathCount = h.localCount * c->framesPerPass;
    c->stateDirty = true;
    entry_inputs_changed(c);  // (the runs of 64 the entry states are walked for: count, map — its content too: the adaptive set is refilled in place)
}

// Everything sized by the pixel set of this context: queues for localCount * framesPerPass paths and a zeroed image.
static int alloc_paths(nxhip_ctx* c, uint32_t localCount)
{
    const size_t n = (size_t)std::max<uint32_t>(localCount, 1u) * c->framesPerPass;
    const size_t full = std::max<size_t>((size_t)c->width * c->height, localCount);
    if (n > 0x7fffffffull) return fail_invalid("more than 2^31 paths (pixels x frames per pass): lower nxhip_set_frames_per_pass first");
    DevBuf freshAccum, freshRgba;  // all or nothing, as alloc_queues
    if (!freshAccum.alloc(full * 16) || !freshRgba.alloc(full * 4)) return NXHIP_ERR_HIP;
    DevBuf freshAovA, freshAovN;  // the accumulated feature buffers follow the image (nxhip_set_aov)
    if (c->aov && (!freshAovA.alloc(full * 16) || !freshAovN.alloc(full * 16))) return NXHIP_ERR_HIP;
    NX_TRY(alloc_queues(c, n));
    if (c->aov) {
        c->aovAccumAlbedo = std::move(freshAovA);
        c->aovAccumNormalDepth = std::move(freshAovN);
        NX_HIP(hipMemsetAsync(c->aovAccumAlbedo.p, 0, full * 16, c->stream));
        NX_HIP(hipMemsetAsync(c->aovAccumNormalDepth.p, 0, full * 16, c->stream));
        c->h.aovAccumAlbedo = c->aovAccumAlbedo.as<float4>();
        c->h.aovAccumNormalDepth = c->aovAccumNormalDepth.as<float4>();
    }
    release_denoise_planes(c);  // (sized by the frame, and their content belongs to the previous pixel set)
    c->accumulation = std::move(freshAccum);
    c->rgba8 = std::move(freshRgba);
    NX_HIP(hipMemsetAsync(c->accumulation.p, 0, full * 16, c->stream));
    NX_HIP(hipMemsetAsync(c->rgba8.p, 0, full * 4, c->stream));
    c->localCount = localCount;
    c->pixelSetGeneration++;
    c->pathCount = localCount * c->framesPerPass;
    c->activeCount = localCount;  // (adaptive sampling: the caller starts the statistics over once the set's map is in place, pixel_set_changed)
    DeviceState& h = c->h;
    publish_pixel_set(c);
    h.accumulation = c->accumulation.as<float4>();
    h.rgba8 = c->rgba8.as<uint32_t>();
    c->stateDirty = true;
    invalidate_graph(c);
    return NXHIP_OK;
}

// The frame counter lives on the host; every pass's begin_frame_kernel carries the number of its last frame.  Changing it
// must not overtake passes already issued with the old numbering.
int nxd::set_frame_number_device(nxhip_ctx* c, uint32_t f)
{
    NX_SYNC_ALL(c);
    c->frameNumber = f;
    return NXHIP_OK;
}

static int pixel_set_changed(nxhip_ctx* c)
{
    c->activeCount = c->localCount;
    if (c->adaptive) return adaptive_restart(c);
    publish_pixel_set(c);
    return NXHIP_OK;
}

extern "C" {

const char* nxhip_last_error(void) { return g_lastError.c_str(); }

int nxhip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// bit 0: device code for gfx950; bit 1: built with the Makefile's scheduler flags (SCHEDFLAGS: about 10 % on the material kernels);
// bit 2: the nxhip_debug_* test hooks are compiled in (the default build; `make release` leaves them as stubs that refuse)
int nxhip_build_info(void)
{
    int f = 0;
#ifdef NX_BUILT_FOR_GFX950
    f |= 1;
#endif
#ifdef NX_SCHED_FLAGS
    f |= 2;
#endif
#ifndef NX_NO_DEBUG_HOOKS
    f |= 4;
#endif
    return f;
}

int nxhip_has_gfx950_code(void)
{
#ifdef NX_BUILT_FOR_GFX950
    return 1;
#else
    return 0;
#endif
}

int nxhip_create(int device, uint32_t width, uint32_t height, void* stream, nxhip_ctx** out)
{
    if (!out) return fail_invalid("nxhip_create: out is null");
    *out = nullptr;
    if (width == 0 || height == 0) return fail_invalid("nxhip_create: zero-sized viewport");
    if ((uint64_t)width * height > 0x7fffffffull) return fail_invalid("nxhip_create: more than 2^31 pixels");
    if (const int rcLayouts = check_layouts()) return rcLayouts;  // a library of mixed objects is refused before anything is launched
    if (nxhip_device_count() <= device || device < 0) {
        set_error("nxhip_create: no such HIP device");
        return NXHIP_ERR_NO_DEVICE;
    }
    NX_HIP(hipSetDevice(device));
    nxhip_ctx* c = new (std::nothrow) nxhip_ctx();
    if (!c) return fail_invalid("nxhip_create: out of host memory");
    c->device = device;
    c->width = width;
    c->height = height;
    c->queueBudget = queue_budget_from_environment();
    int rc = NXHIP_OK;
    do {
        if (stream) c->stream = (hipStream_t)stream;
        else {
            if (!hip_ok(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate", __FILE__, __LINE__)) { rc = NXHIP_ERR_HIP; break; }
            c->ownsStream = true;
        }
        hipDeviceProp_t prop;
        if (!hip_ok(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties", __FILE__, __LINE__)) { rc = NXHIP_ERR_HIP; break; }
        c->numCUs = prop.multiProcessorCount;

        if (!c->dState.alloc(sizeof(DeviceState)) || !c->counters.alloc(sizeof(Counters)) || !c->frame.alloc(sizeof(FrameState)) ||
            !c->traceStats.alloc(2 * sizeof(TraceStatsDev)) || !c->srgbLut.alloc(256 * sizeof(float))) { rc = NXHIP_ERR_HIP; break; }
        (void)hipMemsetAsync(c->counters.p, 0, sizeof(Counters), c->stream);
        (void)hipMemsetAsync(c->traceStats.p, 0, 2 * sizeof(TraceStatsDev), c->stream);
        FrameState fs{0u, -1, -1, 0u, 0u, {0u, 0u, 0u}};
        (void)hipMemcpyAsync(c->frame.p, &fs, sizeof fs, hipMemcpyHostToDevice, c->stream);
        float lut[256];
        for (int i = 0; i < 256; i++) {
            const float x = (float)i / 255.0f;
            lut[i] = x <= 0.04045f ? x / 12.92f : std::pow((x + 0.055f) / 1.055f, 2.4f);
        }
        (void)hipMemcpyAsync(c->srgbLut.p, lut, sizeof lut, hipMemcpyHostToDevice, c->stream);
        if (!hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize", __FILE__, __LINE__)) { rc = NXHIP_ERR_HIP; break; }

        DeviceState& h = c->h;
        std::memset(&h, 0, sizeof h);
        h.counters = c->counters.as<Counters>();
        h.frame = c->frame.as<FrameState>();
        h.traceStats = c->traceStats.as<TraceStatsDev>();
        h.srgbLut = c->srgbLut.as<float>();
        h.settings.useMIS = 1;  // Renderer/RenderSettings.h:4-10 defaults
        h.settings.pathLength = 10;
        h.settings.backgroundColor[0] = h.settings.backgroundColor[1] = h.settings.backgroundColor[2] = 1.0f;
        h.settings.backgroundIntensity = 0.0f;
        h.camera.resolution[0] = width;
        h.camera.resolution[1] = height;
        // (round 6: 16 / 16 — at most 16 busy lanes for 16 iterations, and still "four average rays" long: nx_trace.hip kThinFactor.  With the
        //  traversal state carried over: driver command +0.8 % over 4 / 64, a rank of 8's share 3.80 -> 3.70 ms; profiles/r06_handover.txt)
        h.thinLanes = 16u;
        h.thinIters = 16u;
        h.rngMode = NX_RNG_REFERENCE_SLOT;
        h.compactMode = NX_COMPACT_FAST;
        h.conductorMode = NX_CONDUCTOR_REFERENCE;
        rc = alloc_paths(c, width * height);
        if (rc != NXHIP_OK) break;

        // persistent launch geometry from the occupancy the kernels actually get
        int perCU = 0;
        const void* const closest = kernels::trace(0u).fn, * const anyHit = kernels::trace(kTfAnyHit).fn;
        if (!closest || !anyHit) { rc = fail_invalid("nxhip_create: no trace_kernel instance of set 0 or of set kTfAnyHit is compiled"); break; }
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, closest, kTraceBlock, 0) != hipSuccess || perCU < 1) perCU = 4;
        c->traceBlocks = std::max(1, perCU) * c->numCUs;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, anyHit, kTraceBlock, 0) != hipSuccess || perCU < 1) perCU = 4;
        c->shadowBlocks = std::max(1, perCU) * c->numCUs;
        c->wideBlocks = 8 * c->numCUs;
        static_assert(sizeof c->tailBlocks / sizeof c->tailBlocks[0] == kMfAll + 1u, "one entry per set of material features");
        for (unsigned set = 0; set <= kMfAll; set++) {  // (every tail instance some unit compiled: a set without one keeps 0)
            const void* const tail = kernels::tail(set).fn;
            if (!tail) continue;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, tail, kTraceBlock, 0) != hipSuccess || perCU < 1) perCU = 2;
            c->tailBlocks[set] = std::max(1, perCU) * c->numCUs;
        }
        // Launch-geometry knobs of the measurement sweeps.  They are read only when NX_TUNING_KNOBS=1 says
        // that a sweep is running: a stray variable in a user's environment does not reconfigure the product.
        if (const char* on = std::getenv("NX_TUNING_KNOBS"); on && std::atoi(on) == 1) {
            if (const char* e = std::getenv("NX_TAIL_BOUNCE")) {  // tuning experiments only: 0 = off
                const int n = std::atoi(e);
                if (n == 0 || n == -1 || (n >= 2 && n <= NX_PATH_MAX_LENGTH)) c->tailBounce = n;
            }
            if (const char* e = std::getenv("NX_TRACE_BLOCKS_PER_CU")) {  // tuning experiments only
                const int n = std::atoi(e);
                if (n >= 1 && n <= 16) { c->traceBlocks = c->shadowBlocks = n * c->numCUs; c->traceGridForced = true; }
            }
            if (const char* e = std::getenv("NX_SHADOW_BLOCKS_PER_CU")) {  // tuning experiments only: the any-hit launches' grid alone
                const int n = std::atoi(e);
                if (n >= 1 && n <= 16) { c->shadowBlocks = n * c->numCUs; c->traceGridForced = true; }
            }
            if (const char* e = std::getenv("NX_CLOSEST_BLOCKS_PER_CU")) {  // tuning experiments only: the closest-hit launches' grid alone
                const int n = std::atoi(e);
                if (n >= 1 && n <= 16) { c->traceBlocks = n * c->numCUs; c->traceGridForced = true; }
            }
            if (const char* e = std::getenv("NX_SHADE_BLOCKS_PER_CU")) {  // tuning experiments only
                const int n = std::atoi(e);
                if (n >= 1 && n <= 64) c->shadeBlocksPerCU = n;
            }
            if (const char* e = std::getenv("NX_LOGIC_BLOCKS_PER_CU")) {  // tuning experiments only
                const int n = std::atoi(e);
                if (n >= 1 && n <= 64) c->logicBlocksPerCU = n;
            }
            if (const char* e = std::getenv("NX_THIN_LANES")) { const int n = std::atoi(e); if (n >= 1 && n <= 64) c->h.thinLanes = (uint32_t)n; }   // sweeps of the hand-over rule
            if (const char* e = std::getenv("NX_THIN_ITERS")) { const int n = std::atoi(e); if (n >= 1 && n <= 4096) c->h.thinIters = (uint32_t)n; }
            if (const char* e = std::getenv("NX_GRAPH_SHAPE")) { const int n = std::atoi(e); if (n == 0 || n == 1) c->shapeForced = n; }  // sweeps of the pass-graph shape (graph_shape)
            if (const char* e = std::getenv("NX_RESIDENT_SLOTS")) { const int n = std::atoi(e); if (n >= 1 && n <= 8) c->residentForced = n; }  // sweeps of the resident-slot rule (resident_slots)
            if (const char* e = std::getenv("NX_TRACE_BLOCKS_TOTAL")) {  // tuning experiments only
                const int n = std::atoi(e);
                if (n >= 1 && n <= 65536) { c->traceBlocks = c->shadowBlocks = n; c->traceGridForced = true; }
            }
        }
    } while (false);
    if (rc != NXHIP_OK) {
        nxhip_destroy(c);
        return rc;
    }
    *out = c;
    return NXHIP_OK;
}

void nxhip_destroy(nxhip_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->dead) {
        // nxhip_sync_timeout gave up on this context.  If the device has finished after all, everything below is safe; if it still has
        // not, waiting for it (stream synchronisation, hipFree) would hang the caller: the context's device memory stays where it is
        // until the process ends — which is what the caller of a timed-out context is about to do.
        bool busy = false;
        for (uint32_t k = 0; k < slot_count(c); k++)
            if (slot_at(c, k)->stream && hipStreamQuery(slot_at(c, k)->stream) != hipSuccess) busy = true;
        if (busy) return;
        c->dead = false;
    }
    (void)sync_all(c);
    (void)nxhip_mgpu_shutdown(c);
    invalidate_graph(c);
    for (uint32_t k = 0; k < slot_count(c); k++) {
        PassSlot* q = slot_at(c, k);
        if (q->done) (void)hipEventDestroy(q->done);
        if (q->accumulated) (void)hipEventDestroy(q->accumulated);
        if (q->hostError) (void)hipHostFree(q->hostError);
        if (k > 0 && q->ownsStream && q->stream) (void)hipStreamDestroy(q->stream);
    }
    c->extra.clear();
    for (auto& t : c->timerPool) {
        if (t.start) (void)hipEventDestroy(t.start);
        if (t.stop) (void)hipEventDestroy(t.stop);
    }
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->ownsStream && c->stream) (void)hipStreamDestroy(c->stream);
    if (c->hostStaging) (void)hipHostFree(c->hostStaging);
    if (c->adHostTotals) (void)hipHostFree(c->adHostTotals);
    for (hipEvent_t e : c->stagingDone)
        if (e) (void)hipEventDestroy(e);
    delete c;
}

// After a synchronisation: did a trace kernel abandon rays (FrameState::errorWord, nx_device.h kStallLimit)?  Read and cleared,
// slot by slot; 4 bytes each.
static int check_device_errors(nxhip_ctx* c)
{
    uint32_t any = 0u;
    for (uint32_t k = 0; k < slot_count(c); k++) {
        PassSlot* const q = slot_at(c, k);
        if (!q->frame.p) continue;  // (a slot that never rendered)
        uint32_t* word = &q->frame.as<FrameState>()->errorWord;
        uint32_t w = 0u;
        // (the caller has synchronised: a pass's own copy of the word is there; anything launched since — the ray-batch hooks — is read here)
        if (q->errorFresh && q->hostError) w = *q->hostError;
        else NX_HIP(hipMemcpy(&w, word, 4, hipMemcpyDeviceToHost));
        q->errorFresh = false;
        if (w) {
            const uint32_t zero = 0u;
            NX_HIP(hipMemcpy(word, &zero, 4, hipMemcpyHostToDevice));
            if (q->hostError) *q->hostError = 0u;
        }
        any |= w;
    }
    if (any & kErrScanStalled) {
        set_error("a workgroup of the ordered compaction gave up waiting for the tile before it (internal error)");
        return NXHIP_ERR_HIP;
    }
    if (any & kErrRaysRetaken) {
        set_error("a trace wave was handed more rays than its launch's queue holds: rays re-enter the queue they were taken from (internal error)");
        return NXHIP_ERR_TRAVERSAL;
    }
    if (any & kErrTraversalStalled) {
        set_error("a trace kernel abandoned rays that made no progress for millions of iterations: the uploaded or device-built BVH is not a tree");
        return NXHIP_ERR_TRAVERSAL;
    }
    return NXHIP_OK;
}

int nxhip_sync(nxhip_ctx* c)
{
    NX_CHECK_CTX(c);
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    return check_device_errors(c);
}

int nxhip_sync_timeout(nxhip_ctx* c, uint32_t timeoutMs)
{
    NX_CHECK_CTX(c);
    NX_HIP(hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        bool busy = false;
        for (uint32_t k = 0; k < slot_count(c); k++) {
            PassSlot* s = slot_at(c, k);
            if (!s->stream) continue;
            const hipError_t e = hipStreamQuery(s->stream);
            if (e == hipErrorNotReady) busy = true;
            else if (e != hipSuccess) NX_HIP(e);
        }
        if (!busy) return check_device_errors(c);
        if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() >= (double)timeoutMs) {
            c->dead = true;
            set_error("nxhip_sync_timeout: the device did not finish within " + std::to_string(timeoutMs) + " ms; the context is dead (exit, or continue in a fresh process)");
            return NXHIP_ERR_TIMEOUT;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

int nxhip_resize(nxhip_ctx* c, uint32_t width, uint32_t height)
{
    NX_CHECK_CTX(c);
    if (width == 0 || height == 0) return fail_invalid("nxhip_resize: zero-sized viewport");
    if ((uint64_t)width * height * c->framesPerPass > 0x7fffffffull)
        return fail_invalid("nxhip_resize: more than 2^31 paths (pixels x frames per pass): lower nxhip_set_frames_per_pass first");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    // the new size is committed only when its buffers exist: a failed allocation leaves viewport, pixel map and image as they were
    const uint32_t oldW = c->width, oldH = c->height;
    c->width = width;  // (alloc_paths sizes the image from these)
    c->height = height;
    const int rc = alloc_paths(c, width * height);
    if (rc != NXHIP_OK) {
        c->width = oldW;
        c->height = oldH;
        return rc;
    }
    c->h.camera.resolution[0] = width;
    c->h.camera.resolution[1] = height;
    c->pixelMap.release();
    c->coversFrame = true;
    NX_TRY(pixel_set_changed(c));
    NX_TRY(set_frame_number_device(c, 0));
    // (the ORDER of the full frame survives a resize; a caller's own pixel map does not: it was made for the old size)
    if (c->pixelOrder != NXHIP_ORDER_ROWS) return nxhip_set_pixel_order(c, c->pixelOrder);
    return NXHIP_OK;
}

// ---- settings ------------------------------------------------------------------------------------------

int nxhip_set_camera(nxhip_ctx* c, const nx_camera* camera)
{
    NX_CHECK_CTX(c);
    if (!camera) return fail_invalid("nxhip_set_camera: null camera");
    if (camera->resolution[0] != c->width || camera->resolution[1] != c->height)
        return fail_invalid("nxhip_set_camera: camera resolution differs from the context viewport (call nxhip_resize first)");
    // (the reference's Render loop hands the camera and the settings over every frame: an unchanged one must not cost the
    //  state upload, which waits for every pass in flight)
    if (std::memcmp(&c->h.camera, camera, sizeof *camera) == 0) return NXHIP_OK;
    c->h.camera = *camera;
    c->stateDirty = true;
    entry_inputs_changed(c);
    return NXHIP_OK;
}

int nxhip_set_render_settings(nxhip_ctx* c, const nx_render_settings* s)
{
    NX_CHECK_CTX(c);
    if (!s) return fail_invalid("nxhip_set_render_settings: null settings");
    if (s->pathLength < 1 || s->pathLength > NX_PATH_MAX_LENGTH - 2) return fail_invalid("nxhip_set_render_settings: pathLength must be in [1, 98]");
    if (std::memcmp(&c->h.settings, s, sizeof *s) == 0) return NXHIP_OK;
    if (s->pathLength != c->h.settings.pathLength) invalidate_graph(c);
    c->h.settings = *s;
    c->stateDirty = true;
    return NXHIP_OK;
}

int nxhip_set_modes(nxhip_ctx* c, int rngMode, int compactMode, int conductorMode)
{
    NX_CHECK_CTX(c);
    if (rngMode < 0 || rngMode > 1 || compactMode < 0 || compactMode > 1 || conductorMode < 0 || conductorMode > 1)
        return fail_invalid("nxhip_set_modes: unknown mode");
    if (c->adaptive && rngMode != NX_RNG_PIXEL_KEYED)
        return fail_invalid("nxhip_set_modes: adaptive sampling is on and needs NX_RNG_PIXEL_KEYED (nxhip_set_adaptive(ctx, NULL) first)");
    if (rngMode == c->h.rngMode && compactMode == c->h.compactMode && conductorMode == c->h.conductorMode) return NXHIP_OK;
    if (compactMode != c->h.compactMode || conductorMode != c->h.conductorMode) invalidate_graph(c);
    c->h.rngMode = rngMode;
    c->h.compactMode = compactMode;
    c->h.conductorMode = conductorMode;
    c->stateDirty = true;
    return NXHIP_OK;
}

int nxhip_set_pixel_map(nxhip_ctx* c, const uint32_t* pixelMap, uint32_t localCount)
{
    NX_CHECK_CTX(c);
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    const uint32_t full = c->width * c->height;
    c->pixelOrder = NXHIP_ORDER_ROWS;  // (a caller's own map, or none: nxhip_set_pixel_order sets it again behind its own call)
    // the queues are re-allocated first (all or nothing): a failure leaves the previous pixel set, map and queues in place
    if (!pixelMap) {
        NX_TRY(alloc_paths(c, full));
        c->pixelMap.release();
        c->coversFrame = true;
        NX_TRY(pixel_set_changed(c));
        return set_frame_number_device(c, 0);
    }
    if (localCount == 0 || localCount > full) return fail_invalid("nxhip_set_pixel_map: localCount out of range");
    for (uint32_t i = 0; i < localCount; i++)
        if (pixelMap[i] >= full) return fail_invalid("nxhip_set_pixel_map: pixel index out of range");
    DevBuf freshMap;
    NX_ALLOC(freshMap, (size_t)localCount * 4);
    NX_HIP(hipMemcpy(freshMap.p, pixelMap, (size_t)localCount * 4, hipMemcpyHostToDevice));
    NX_TRY(alloc_paths(c, localCount));
    c->pixelMap = std::move(freshMap);
    // every pixel of the frame exactly once?  (what nxhip_denoise needs: it filters in image space)
    c->coversFrame = localCount == full;
    if (c->coversFrame) {
        std::vector<bool> seen(full, false);
        for (uint32_t i = 0; i < localCount && c->coversFrame; i++) {
            if (seen[pixelMap[i]]) c->coversFrame = false;
            seen[pixelMap[i]] = true;
        }
    }
    NX_TRY(pixel_set_changed(c));
    return set_frame_number_device(c, 0);
}

int nxhip_set_pixel_order(nxhip_ctx* c, int order)
try {
    NX_CHECK_CTX(c);
    if (order != NXHIP_ORDER_ROWS && order != NXHIP_ORDER_TILES) return fail_invalid("nxhip_set_pixel_order: order must be NXHIP_ORDER_ROWS or NXHIP_ORDER_TILES");
    if (order == NXHIP_ORDER_ROWS) {
        const int rc = nxhip_set_pixel_map(c, nullptr, 0);
        if (rc == NXHIP_OK) c->pixelOrder = order;
        return rc;
    }
    std::vector<uint32_t> map((size_t)c->width * c->height);
    uint32_t n = 0;
    NX_TRY(nxhip_tile_pixel_map(c->width, c->height, 1, 0, 1, 1, map.data(), &n));
    const int rc = nxhip_set_pixel_map(c, map.data(), n);
    if (rc == NXHIP_OK) c->pixelOrder = order;
    return rc;
} NX_CATCH("nxhip_set_pixel_order")

}  // extern "C"
