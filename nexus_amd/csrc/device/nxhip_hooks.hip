// nxhip_hooks.hip — kernel-level test hooks (ray batches, BSDF, texture, binary64 functions), trace statistics, kernel times.
// (the C-ABI device layer declared in include/nexus_hip.h; helpers shared with the other nxhip_*.hip units: nx_host.h)
// A columnar hook (`count` items as flat arrays in and out, one wide kernel) checks its arguments, then states its columns on a
// HookBatch (nx_hookbatch.h) and calls run with the kernel of kernels:: — no allocation, copy or byte count of its own.  The
// ray-batch hooks copy into queue regions instead (HookLayout).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "nx_hookbatch.h"

using namespace nxd;

extern "C" {

// ---- kernel-level hooks -----------------------------------------------------------------------------

// The ray-batch hooks number their n rays densely and cut them into one contiguous piece per queue region in use (as
// generate_kernel does for the primary rays): ray i lives in slot (i / piece) * cap + i % piece.
struct HookLayout {
    uint32_t shards, cap, piece;
    int32_t sizes[kQueueShards];
};
static HookLayout hook_layout(const nxhip_ctx* c, uint32_t n)
{
    HookLayout l{};
    l.shards = c->view.queueShards;
    l.cap = c->view.queueShardCap;
    l.piece = ((n + l.shards * 64u - 1u) / (l.shards * 64u)) * 64u;
    for (uint32_t k = 0; k < (uint32_t)kQueueShards; k++) l.sizes[k] = k < l.shards ? (int32_t)std::min(l.piece, n - std::min(n, k * l.piece)) : 0;
    return l;
}
// host array (n elements of `elem` bytes, dense numbering) <-> a queue buffer's regions
static int hook_copy(nxhip_ctx* c, const HookLayout& l, void* dev, void* host, size_t elem, bool toDevice)
{
    for (uint32_t k = 0; k < l.shards; k++) {
        if (l.sizes[k] <= 0) continue;
        char* d = static_cast<char*>(dev) + (size_t)k * l.cap * elem;
        char* h = static_cast<char*>(host) + (size_t)k * l.piece * elem;
        if (toDevice) NX_HIP(hipMemcpyAsync(d, h, (size_t)l.sizes[k] * elem, hipMemcpyHostToDevice, c->stream));
        else NX_HIP(hipMemcpyAsync(h, d, (size_t)l.sizes[k] * elem, hipMemcpyDeviceToHost, c->stream));
    }
    return NXHIP_OK;
}

static int run_trace_chunk(nxhip_ctx* c, bool anyHit, uint32_t n, bool transmit = false)
{
    // region sizes + zeroed fetch heads for the reserved bounce slot, computed on the device from n (hook_layout's rule): no copy
    // from a stack-local of this function is left in flight when it returns
    NX_HIP(launch_untimed(kernels::hook_sizes(), 1, 64, c->stream, c->dState.as<DeviceState>(), n, anyHit ? 1 : 0, kHookBounceSlot));
    c->errorFresh = false;  // (this launch may set the error word after the last pass's copy of it)
    // (a table with a MASK material: the ALPHA_TEST instances, whatever the hook — nxhip_set_material_alpha)
    const bool alphaTest = c->materialsAlphaMask;
    const bool thin = c->thinInHooks && !c->statsEnabled && !transmit && !alphaTest;  // (the TRANSMIT and ALPHA_TEST instances never hand over)
    const unsigned set = hook_trace_features(c, anyHit, transmit);
    const kernels::BounceKernel trace = kernels::trace(set);
    if (!trace.fn) return fail_invalid("ray batch: trace_kernel has no instance of feature set " + std::to_string(set));
    Launch l = make_launch(trace, anyHit ? c->shadowBlocks : c->traceBlocks, kTraceBlock,
                           anyHit ? NXHIP_K_SHADOW : NXHIP_K_TRACE, c->dState.as<DeviceState>(), kHookBounceSlot | (thin ? kTraceThinFlag : 0));
    int rc = launch_now(c, l);
    if (rc == NXHIP_OK && thin) {  // (nxhip_debug_set_thin: what the dry waves handed over, a wave each)
        Launch t = make_launch(kernels::thin(), 3 * c->numCUs, kTraceBlock, NXHIP_K_THIN, c->dState.as<DeviceState>(), kHookBounceSlot);
        rc = launch_now(c, t);
    }
    return rc;
}

// What the ray-batch hooks bring up to date before they launch.  readsScene: the trace instance reads the shading records, the maps and
// the triangles, so what a render does before its pass is done here too.
static int ray_batch_ready(nxhip_ctx* c, bool readsScene)
{
    if (!c->h.tlasNodes) return fail_invalid("no TLAS has been set");
    if (readsScene) {
        NX_TRY(check_scene_ready(c));
        if (c->shadeInstDirty) NX_TRY(refresh_shade_inst(c));
    }
    NX_TRY(ensure_slot_queues(c, c));
    NX_TRY(upload_state(c));
    return refresh_updated_blas(c);
}

int nxhip_trace_batch(nxhip_ctx* c, const nx_ray* rays, uint32_t count, nx_hit* hits)
try {
    NX_CHECK_CTX(c);
    if (count == 0) return NXHIP_OK;
    if (!rays || !hits) return fail_invalid("nxhip_trace_batch: null buffer");
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(ray_batch_ready(c, c->materialsAlphaMask));  // (the ALPHA_TEST instance reads the scene)
    const uint32_t cap = c->pathCount;
    std::vector<float4> o(std::min(cap, count)), d(std::min(cap, count)), h(std::min(cap, count));
    std::vector<uint32_t> hi(std::min(cap, count));
    for (uint32_t first = 0; first < count; first += cap) {
        const uint32_t n = std::min(cap, count - first);
        for (uint32_t i = 0; i < n; i++) {
            const nx_ray& r = rays[first + i];
            float idx;
            std::memcpy(&idx, &i, 4);
            o[i] = make_float4(r.origin[0], r.origin[1], r.origin[2], 0.0f);
            d[i] = make_float4(r.direction[0], r.direction[1], r.direction[2], idx);
        }
        const HookLayout l = hook_layout(c, n);
        NX_TRY(hook_copy(c, l, c->trRayO.p, o.data(), 16, true));
        NX_TRY(hook_copy(c, l, c->trRayD.p, d.data(), 16, true));
        NX_TRY(run_trace_chunk(c, false, n));
        NX_TRY(hook_copy(c, l, c->trHit.p, h.data(), 16, false));
        NX_TRY(hook_copy(c, l, c->trHitInst.p, hi.data(), 4, false));
        NX_SYNC_ALL(c);
        for (uint32_t i = 0; i < n; i++) {
            nx_hit& out = hits[first + i];
            out.hitDistance = h[i].x;
            out.u = h[i].y;
            out.v = h[i].z;
            std::memcpy(&out.triIdx, &h[i].w, 4);
            out.instanceIdx = hi[i];
        }
    }
    return NXHIP_OK;
} NX_CATCH("nxhip_trace_batch")

// transmittance != nullptr: nxhip_trace_transmittance_batch — the TRANSMIT instance, and T itself instead of "occluded"
static int shadow_batch(nxhip_ctx* c, const char* who, const nx_ray* rays, const float* tmax, uint32_t count, uint8_t* occluded, float* transmittance)
{
    NX_CHECK_CTX(c);
    if (count == 0) return NXHIP_OK;
    if (!rays || !tmax || (!occluded && !transmittance)) return fail_invalid(std::string(who) + ": null buffer");
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(ray_batch_ready(c, transmittance || c->materialsAlphaMask));  // (the TRANSMIT and ALPHA_TEST instances read the scene)
    const uint32_t cap = c->pathCount;
    const uint32_t m = std::min(cap, count);
    std::vector<float4> o(m), d(m), rad(m, make_float4(1.0f, 0.0f, 0.0f, 0.0f)), res(m);
    for (uint32_t first = 0; first < count; first += cap) {
        const uint32_t n = std::min(cap, count - first);
        for (uint32_t i = 0; i < n; i++) {
            const nx_ray& r = rays[first + i];
            float idx;
            std::memcpy(&idx, &i, 4);
            o[i] = make_float4(r.origin[0], r.origin[1], r.origin[2], tmax[first + i]);
            d[i] = make_float4(r.direction[0], r.direction[1], r.direction[2], idx);
        }
        // the kernel's tail adds the request's radiance to the path's pixel when unoccluded: radiance 1 into a zeroed buffer
        const HookLayout l = hook_layout(c, n);
        NX_TRY(hook_copy(c, l, c->shRayO.p, o.data(), 16, true));
        NX_TRY(hook_copy(c, l, c->shRayD.p, d.data(), 16, true));
        NX_TRY(hook_copy(c, l, c->shRadiance.p, rad.data(), 16, true));
        NX_HIP(hipMemsetAsync(c->h.radiance, 0, (size_t)n * 16, c->stream));  // the buffer the kernel adds into (own or bound)
        NX_TRY(run_trace_chunk(c, true, n, transmittance != nullptr));
        NX_HIP(hipMemcpyAsync(res.data(), c->h.radiance, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
        NX_SYNC_ALL(c);
        for (uint32_t i = 0; i < n; i++) {
            if (transmittance) transmittance[first + i] = res[i].x;  // (radiance 1 into a zeroed buffer: .x is T)
            else occluded[first + i] = res[i].x == 1.0f ? 0 : 1;
        }
    }
    return NXHIP_OK;
}

int nxhip_trace_shadow_batch(nxhip_ctx* c, const nx_ray* rays, const float* tmax, uint32_t count, uint8_t* occluded)
try {
    return shadow_batch(c, "nxhip_trace_shadow_batch", rays, tmax, count, occluded, nullptr);
} NX_CATCH("nxhip_trace_shadow_batch")

int nxhip_trace_transmittance_batch(nxhip_ctx* c, const nx_ray* rays, const float* tmax, uint32_t count, float* transmittance)
try {
    return shadow_batch(c, "nxhip_trace_transmittance_batch", rays, tmax, count, nullptr, transmittance);
} NX_CATCH("nxhip_trace_transmittance_batch")

int nxhip_enable_trace_stats(nxhip_ctx* c, int enable)
{
    NX_CHECK_CTX(c);
    if ((enable != 0) != c->statsEnabled) invalidate_graph(c);
    c->statsEnabled = enable != 0;
    return NXHIP_OK;
}

int nxhip_read_trace_stats(nxhip_ctx* c, nxhip_trace_stats* closest, nxhip_trace_stats* shadow, int reset)
{
    NX_CHECK_CTX(c);
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    TraceStatsDev h[2];
    NX_HIP(hipMemcpy(h, c->traceStats.p, sizeof h, hipMemcpyDeviceToHost));
    static_assert(sizeof(nxhip_trace_stats) == sizeof(TraceStatsDev), "stats layouts must match");
    if (closest) std::memcpy(closest, &h[0], sizeof h[0]);
    if (shadow) std::memcpy(shadow, &h[1], sizeof h[1]);
    if (reset) NX_HIP(hipMemset(c->traceStats.p, 0, sizeof h));
    return NXHIP_OK;
}

static int bsdf_hook(nxhip_ctx* c, const nx_material* material, const nx_bsdf_query* queries, uint32_t count, nx_bsdf_result* results, int sample)
{
    NX_CHECK_CTX(c);
    if (!material || (!queries && count) || (!results && count)) return fail_invalid("nxhip_bsdf_*_batch: null buffer");
    if (material->type < NX_MAT_DIFFUSE || material->type > NX_MAT_METALROUGH) return fail_invalid("nxhip_bsdf_*_batch: unknown material type");
    if (count == 0) return NXHIP_OK;
    NX_HIP(hipSetDevice(c->device));
    HookBatch one(c, 1), b(c, count);  // (the material: a column of one item)
    const nx_material* dMat = one.in(material, 1);
    NX_TRY(one.rc);
    const nx_bsdf_query* dQ = b.in(queries, 1);
    nx_bsdf_result* dR = b.out(results, 1);
    // (NX_MAT_METALROUGH has a kernel of its own: bsdf_hook_metal_kernel, nx_hook_kernels.hip — the four reference types keep theirs)
    return b.run(material->type == NX_MAT_METALROUGH ? kernels::bsdf_hook_metal() : kernels::bsdf_hook(), dMat, dQ, count, sample, dR);
}

int nxhip_bsdf_sample_batch(nxhip_ctx* c, const nx_material* material, const nx_bsdf_query* queries, uint32_t count, nx_bsdf_result* results)
{
    return bsdf_hook(c, material, queries, count, results, 1);
}

int nxhip_bsdf_eval_batch(nxhip_ctx* c, const nx_material* material, const nx_bsdf_query* queries, uint32_t count, nx_bsdf_result* results)
{
    return bsdf_hook(c, material, queries, count, results, 0);
}

int nxhip_tex2d_batch(nxhip_ctx* c, int kind, int textureId, const float* uv, uint32_t count, float* rgba)
{
    NX_CHECK_CTX(c);
    if ((!uv || !rgba) && count) return fail_invalid("nxhip_tex2d_batch: null buffer");
    if (kind < 0 || kind > 4) return fail_invalid("nxhip_tex2d_batch: kind must be 0 .. 4");
    // kind -> the table textureId indexes and what its maps are called (2: the environment map, which has no table)
    const std::vector<TextureHost>* const tables[5] = {&c->diffuseMaps, &c->emissiveMaps, nullptr, &c->normalMaps, &c->roughnessMaps};
    static const char* const names[5] = {"diffuse", "emissive", "environment", "normal", "roughness"};
    if (kind != 2 && (textureId < 0 || (size_t)textureId >= tables[kind]->size())) return fail_invalid(std::string("nxhip_tex2d_batch: no such ") + names[kind] + " map");
    if (kind == 2 && !c->hdrMap.texels.p) return fail_invalid("nxhip_tex2d_batch: no environment map has been uploaded");
    if (count == 0) return NXHIP_OK;
    NX_HIP(hipSetDevice(c->device));
    const TextureHost& th = kind == 2 ? c->hdrMap : (*tables[kind])[textureId];
    HookBatch b(c, count);
    const float* dUv = b.in(uv, 2);
    float4* dOut = b.out(reinterpret_cast<float4*>(rgba), 1);
    const TextureDev t{th.texels.as<uint32_t>(), th.width, th.height};
    // a detail map: linear data, its own lookup (nx_texture.h tex2d_linear)
    if (kind >= 3) return b.run(kernels::tex2d_linear_hook(), t, dUv, count, dOut);
    // a float environment map: its own lookup (nx_texture.h tex2d_float), alpha 1
    if (kind == 2 && c->hdrFloat) return b.run(kernels::tex2d_float_hook(), th.texels.as<float4>(), (int)th.width, (int)th.height, dUv, count, dOut);
    return b.run(kernels::tex2d_hook(), t, c->srgbLut.as<float>(), dUv, count, dOut);
}

// ---- the environment sampler's hooks (env_hook_kernel) ----------------------------------------------

// what the three hooks share: a map must be there, and for everything but the colours the sampler must be on
static int env_hook_ready(nxhip_ctx* c, const char* who, bool needSampling)
{
    if (!c->hdrMap.texels.p) return fail_invalid(std::string(who) + ": no environment map has been uploaded");
    if (needSampling && !c->h.envSampling) return fail_invalid(std::string(who) + ": environment sampling is off (nxhip_set_env_sampling)");
    return NXHIP_OK;
}

int nxhip_read_env_tables(nxhip_ctx* c, float* marginalCdf, float* rowCdf, float* density, uint32_t capacityTexels, uint32_t* width, uint32_t* height)
try {
    NX_CHECK_CTX(c);
    NX_TRY(env_hook_ready(c, "nxhip_read_env_tables", true));
    const uint32_t W = c->hdrMap.width, H = c->hdrMap.height;
    if (width) *width = W;
    if (height) *height = H;
    if (!marginalCdf && !rowCdf && !density) return NXHIP_OK;
    // (the marginal cdf has one entry per row; the two per-texel tables decide the capacity only when one of them is asked for)
    if ((size_t)capacityTexels < ((rowCdf || density) ? (size_t)W * H : (size_t)H)) return fail_invalid("nxhip_read_env_tables: destination too small");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    if (marginalCdf) NX_HIP(hipMemcpy(marginalCdf, c->envMarginalCdf.p, (size_t)H * 4, hipMemcpyDeviceToHost));
    if (rowCdf) NX_HIP(hipMemcpy(rowCdf, c->envRowCdf.p, (size_t)W * H * 4, hipMemcpyDeviceToHost));
    if (density) NX_HIP(hipMemcpy(density, c->envDensity.p, (size_t)W * H * 4, hipMemcpyDeviceToHost));
    return NXHIP_OK;
} NX_CATCH("nxhip_read_env_tables")

int nxhip_read_env_guides(nxhip_ctx* c, uint32_t* marginalGuide, uint32_t* rowGuide, uint32_t capacityRows)
try {
    NX_CHECK_CTX(c);
    NX_TRY(env_hook_ready(c, "nxhip_read_env_guides", true));
    const uint32_t H = c->hdrMap.height;
    if (rowGuide && capacityRows < H) return fail_invalid("nxhip_read_env_guides: destination too small");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    if (marginalGuide) NX_HIP(hipMemcpy(marginalGuide, c->envMarginalGuide.p, (size_t)(kEnvGuide + 1) * 4, hipMemcpyDeviceToHost));
    if (rowGuide) NX_HIP(hipMemcpy(rowGuide, c->envRowGuide.p, (size_t)H * (kEnvGuide + 1) * 4, hipMemcpyDeviceToHost));
    return NXHIP_OK;
} NX_CATCH("nxhip_read_env_guides")

int nxhip_read_env_float(nxhip_ctx* c, float* rgb, uint32_t capacityTexels, uint32_t* width, uint32_t* height)
try {
    NX_CHECK_CTX(c);
    if (!c->hdrMap.texels.p || !c->hdrFloat) return fail_invalid("nxhip_read_env_float: no float environment map has been uploaded");
    const uint32_t W = c->hdrMap.width, H = c->hdrMap.height;
    if (width) *width = W;
    if (height) *height = H;
    if (!rgb) return NXHIP_OK;
    const size_t texels = (size_t)W * H;
    if ((size_t)capacityTexels < texels) return fail_invalid("nxhip_read_env_float: destination too small");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    std::vector<float4> staged(texels);
    NX_HIP(hipMemcpy(staged.data(), c->hdrMap.texels.p, texels * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < texels; i++) { rgb[3 * i] = staged[i].x; rgb[3 * i + 1] = staged[i].y; rgb[3 * i + 2] = staged[i].z; }
    return NXHIP_OK;
} NX_CATCH("nxhip_read_env_float")

// in: count x inWidth floats; vec: count x 3; pdf / texel: count each, or null
static int env_hook(nxhip_ctx* c, int sample, const float* in, uint32_t inWidth, uint32_t count, float* vec, float* pdf, uint32_t* texel)
{
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(upload_state(c));
    HookBatch b(c, count);
    const float* dIn = b.in(in, inWidth);
    float* dVec = b.out(vec, 3);
    float* dPdf = b.out(pdf, 1);
    uint32_t* dTexel = b.out(texel, 1);
    return b.run(kernels::env_hook(), c->dState.as<DeviceState>(), sample, dIn, count, dVec, dPdf, dTexel);
}

int nxhip_env_sample_batch(nxhip_ctx* c, const float* r, uint32_t count, float* direction, float* pdf, uint32_t* texel)
try {
    NX_CHECK_CTX(c);
    if ((!r || !direction || !pdf || !texel) && count) return fail_invalid("nxhip_env_sample_batch: null buffer");
    // before anything is launched: floor(r G) of an r outside [0, 1) — or of a NaN — is no bucket of the guide tables
    if (!all_unit(r, (size_t)count * 2)) return fail_invalid("nxhip_env_sample_batch: r must be in [0, 1)");
    NX_TRY(env_hook_ready(c, "nxhip_env_sample_batch", true));
    if (count == 0) return NXHIP_OK;
    return env_hook(c, 1, r, 2, count, direction, pdf, texel);
} NX_CATCH("nxhip_env_sample_batch")

int nxhip_env_eval_batch(nxhip_ctx* c, const float* direction, uint32_t count, float* rgb, float* pdf, uint32_t* texel)
try {
    NX_CHECK_CTX(c);
    if ((!direction || !rgb) && count) return fail_invalid("nxhip_env_eval_batch: null buffer");
    if (!all_finite(direction, (size_t)count * 3)) return fail_invalid("nxhip_env_eval_batch: directions must be finite");
    NX_TRY(env_hook_ready(c, "nxhip_env_eval_batch", pdf || texel));  // (the colours alone need no sampler)
    if (count == 0) return NXHIP_OK;
    return env_hook(c, 0, direction, 3, count, rgb, pdf, texel);
} NX_CATCH("nxhip_env_eval_batch")

// ---- the analytic lights' hook (alight_hook_kernel) -------------------------------------------------

int nxhip_analytic_light_sample_batch(nxhip_ctx* c, uint32_t lightIndex, const float* origins3, const float* r2, uint32_t count, float* direction3, float* tmax,
                                      float* factor3, uint32_t* ok)
try {
    NX_DEBUG_HOOK("nxhip_analytic_light_sample_batch");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    if (lightIndex >= c->h.alightCount) return fail_invalid("nxhip_analytic_light_sample_batch: no such analytic light (nxhip_set_analytic_lights)");
    if ((!origins3 || !r2 || !direction3 || !tmax || !factor3 || !ok) && count) return fail_invalid("nxhip_analytic_light_sample_batch: null buffer");
    if (!all_finite(origins3, (size_t)count * 3)) return fail_invalid("nxhip_analytic_light_sample_batch: origins must be finite");
    if (!all_unit(r2, (size_t)count * 2)) return fail_invalid("nxhip_analytic_light_sample_batch: r must be in [0, 1)");
    if (count == 0) return NXHIP_OK;
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(upload_state(c));
    HookBatch b(c, count);
    const float *dO = b.in(origins3, 3), *dR = b.in(r2, 2);
    float *dDir = b.out(direction3, 3), *dT = b.out(tmax, 1), *dF = b.out(factor3, 3);
    uint32_t* dOk = b.out(ok, 1);
    return b.run(kernels::alight_hook(), c->dState.as<DeviceState>(), lightIndex, dO, dR, count, dDir, dT, dF, dOk);
} NX_CATCH("nxhip_analytic_light_sample_batch")

// ---- the sky's hook (sky_hook_kernel: the map kernel's own sky_radiance) ------------------------------

int nxhip_sky_radiance_batch(nxhip_ctx* c, const nx_sky* sky, const float* dir3, uint32_t count, float* rgb)
try {
    NX_DEBUG_HOOK("nxhip_sky_radiance_batch");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    SkyPlan plan;
    NX_TRY(sky_plan(sky, "nxhip_sky_radiance_batch", &plan));
    if ((!dir3 || !rgb) && count) return fail_invalid("nxhip_sky_radiance_batch: null buffer");
    if (!all_finite(dir3, (size_t)count * 3)) return fail_invalid("nxhip_sky_radiance_batch: directions must be finite");
    if (count == 0) return NXHIP_OK;
    NX_HIP(hipSetDevice(c->device));
    HookBatch b(c, count);
    const float* dDir = b.in(dir3, 3);
    float* dRgb = b.out(rgb, 3);
    return b.run(kernels::sky_hook(), plan.launch, dDir, count, dRgb);
} NX_CATCH("nxhip_sky_radiance_batch")

// ---- the medium's hooks (medium_segment_hook_kernel, medium_phase_hook_kernel) ----------------------

int nxhip_medium_segment_batch(nxhip_ctx* c, const float* origin, const float* dir, const float* tEnd, const float* xi, uint32_t count, float* t0, float* length,
                               float* transmittance, float* scatterT)
try {
    NX_DEBUG_HOOK("nxhip_medium_segment_batch");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    if (!c->h.mediumOn) return fail_invalid("nxhip_medium_segment_batch: no medium with sigmaT > 0 is set (nxhip_set_medium)");
    if ((!origin || !dir || !tEnd || !xi || !t0 || !length || !transmittance || !scatterT) && count) return fail_invalid("nxhip_medium_segment_batch: null buffer");
    if (!all_finite(origin, (size_t)count * 3) || !all_finite(dir, (size_t)count * 3)) return fail_invalid("nxhip_medium_segment_batch: origins and directions must be finite");
    for (size_t k = 0; k < (size_t)count; k++) {  // (item by item: the first bad item decides the message)
        if (!(tEnd[k] > 0.0f)) return fail_invalid("nxhip_medium_segment_batch: tEnd must be positive (+inf allowed)");
        if (!all_unit(xi + k, 1)) return fail_invalid("nxhip_medium_segment_batch: xi must be in [0, 1)");
    }
    if (count == 0) return NXHIP_OK;
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(upload_state(c));
    HookBatch b(c, count);
    const float *dO = b.in(origin, 3), *dD = b.in(dir, 3), *dT = b.in(tEnd, 1), *dXi = b.in(xi, 1);
    float *dT0 = b.out(t0, 1), *dL = b.out(length, 1), *dTr = b.out(transmittance, 1), *dS = b.out(scatterT, 1);
    return b.run(kernels::medium_segment_hook(), c->dState.as<DeviceState>(), dO, dD, dT, dXi, count, dT0, dL, dTr, dS);
} NX_CATCH("nxhip_medium_segment_batch")

int nxhip_medium_phase_batch(nxhip_ctx* c, const float* dirIn, const float* xi1, const float* xi2, uint32_t count, float* dirOut, float* pdf)
try {
    NX_DEBUG_HOOK("nxhip_medium_phase_batch");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    if (!c->h.mediumOn) return fail_invalid("nxhip_medium_phase_batch: no medium with sigmaT > 0 is set (nxhip_set_medium)");
    if ((!dirIn || !xi1 || !xi2 || !dirOut || !pdf) && count) return fail_invalid("nxhip_medium_phase_batch: null buffer");
    if (!all_finite(dirIn, (size_t)count * 3)) return fail_invalid("nxhip_medium_phase_batch: directions must be finite");
    if (!all_unit(xi1, count) || !all_unit(xi2, count)) return fail_invalid("nxhip_medium_phase_batch: xi1 and xi2 must be in [0, 1)");
    if (count == 0) return NXHIP_OK;
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(upload_state(c));
    HookBatch b(c, count);
    const float *dD = b.in(dirIn, 3), *dX1 = b.in(xi1, 1), *dX2 = b.in(xi2, 1);
    float *dOut = b.out(dirOut, 3), *dPdf = b.out(pdf, 1);
    return b.run(kernels::medium_phase_hook(), c->dState.as<DeviceState>(), dD, dX1, dX2, count, dOut, dPdf);
} NX_CATCH("nxhip_medium_phase_batch")

// ---- the density grid's hooks (medium_density_hook_kernel, medium_track_hook_kernel; the bricks as they are) -------------

static bool medium_grid_on(const nxhip_ctx* c) { return c->h.mediumOn && c->h.mediumRho; }

int nxhip_read_medium_majorants(nxhip_ctx* c, float* majorant, uint32_t capacity, uint32_t bricks[3])
try {
    NX_DEBUG_HOOK("nxhip_read_medium_majorants");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    if (!c->mediumBricks.p) return fail_invalid("nxhip_read_medium_majorants: no density grid is set (nxhip_set_medium_density)");
    const uint32_t nb[3] = {(c->mediumGridN[0] + 7u) / 8u, (c->mediumGridN[1] + 7u) / 8u, (c->mediumGridN[2] + 7u) / 8u};
    if (bricks)
        for (int k = 0; k < 3; k++) bricks[k] = nb[k];
    if (!majorant) return NXHIP_OK;  // (the brick counts alone)
    const uint32_t total = nb[0] * nb[1] * nb[2];
    if (capacity < total) return fail_invalid("nxhip_read_medium_majorants: capacity is below the number of bricks");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    NX_HIP(hipMemcpy(majorant, c->mediumBricks.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    return NXHIP_OK;
} NX_CATCH("nxhip_read_medium_majorants")

int nxhip_medium_density_batch(nxhip_ctx* c, const float* points3, uint32_t count, float* rho, float* majorant)
try {
    NX_DEBUG_HOOK("nxhip_medium_density_batch");
    NX_CHECK_CTX(c);
    if (!medium_grid_on(c)) return fail_invalid("nxhip_medium_density_batch: it needs a medium with sigmaT > 0 (nxhip_set_medium) and a density grid (nxhip_set_medium_density)");
    if ((!points3 || !rho || !majorant) && count) return fail_invalid("nxhip_medium_density_batch: null buffer");
    if (!all_finite(points3, (size_t)count * 3)) return fail_invalid("nxhip_medium_density_batch: points must be finite");
    if (count == 0) return NXHIP_OK;
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(upload_state(c));
    HookBatch b(c, count);
    const float* dP = b.in(points3, 3);
    float *dRho = b.out(rho, 1), *dM = b.out(majorant, 1);
    return b.run(kernels::medium_density_hook(), c->dState.as<DeviceState>(), dP, count, dRho, dM);
} NX_CATCH("nxhip_medium_density_batch")

int nxhip_medium_track_batch(nxhip_ctx* c, const float* origin, const float* dir, const float* tEnd, const uint32_t* seed, uint32_t count, float* scatterT, float* transmittance,
                             uint32_t* steps2)
try {
    NX_DEBUG_HOOK("nxhip_medium_track_batch");
    NX_CHECK_CTX(c);
    if (!medium_grid_on(c)) return fail_invalid("nxhip_medium_track_batch: it needs a medium with sigmaT > 0 (nxhip_set_medium) and a density grid (nxhip_set_medium_density)");
    NX_TRY(check_medium_grid(c, "nxhip_medium_track_batch"));
    if ((!origin || !dir || !tEnd || !seed || !scatterT || !transmittance || !steps2) && count) return fail_invalid("nxhip_medium_track_batch: null buffer");
    if (!all_finite(origin, (size_t)count * 3) || !all_finite(dir, (size_t)count * 3)) return fail_invalid("nxhip_medium_track_batch: origins and directions must be finite");
    for (size_t k = 0; k < (size_t)count; k++) {
        if (!(tEnd[k] > 0.0f)) return fail_invalid("nxhip_medium_track_batch: tEnd must be positive (+inf allowed)");
        if (seed[k] == 0u) return fail_invalid("nxhip_medium_track_batch: a seed may not be 0 (xorshift32 stays there)");
    }
    if (count == 0) return NXHIP_OK;
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(upload_state(c));
    HookBatch b(c, count);
    const float *dO = b.in(origin, 3), *dD = b.in(dir, 3), *dT = b.in(tEnd, 1);
    const uint32_t* dSeed = b.in(seed, 1);
    float *dS = b.out(scatterT, 1), *dTr = b.out(transmittance, 1);
    uint32_t* dSteps = b.out(steps2, 2);
    return b.run(kernels::medium_track_hook(), c->dState.as<DeviceState>(), dO, dD, dT, dSeed, count, dS, dTr, dSteps);
} NX_CATCH("nxhip_medium_track_batch")

// ---- the detail maps' hook (shading_frame_hook_kernel) ----------------------------------------------

// The instance and the triangle indices of the two hooks that shade given hits (after check_scene_ready).  The triangle index is followed
// without a bounds test on the device, as a hit record's is: checked here.  metalRough: the instance's material must be of that type.
static int check_hit_columns(const nxhip_ctx* c, const char* name, uint32_t instanceIdx, const uint32_t* triIdx, uint32_t count, bool metalRough)
{
    const std::string who(name);
    if (instanceIdx >= c->hostInstances.size()) return fail_invalid(who + ": no such instance");
    const nx_bvh_instance& inst = c->hostInstances[instanceIdx];
    if (inst.bvhIdx >= c->blas.size()) return fail_invalid(who + ": the instance refers to a BLAS id that has not been uploaded");
    if (metalRough && c->hostMaterials[(size_t)inst.materialId].type != NX_MAT_METALROUGH) return fail_invalid(who + ": the instance's material is not an NX_MAT_METALROUGH");
    const uint32_t triCount = c->blas[inst.bvhIdx].triCount;
    for (uint32_t k = 0; k < count; k++)
        if (triIdx[k] >= triCount) return fail_invalid(who + ": triangle index out of range");
    return NXHIP_OK;
}

int nxhip_shading_frame_batch(nxhip_ctx* c, uint32_t instanceIdx, const uint32_t* triIdx, const float* hitUv, const float* rayDir, uint32_t count, float* normalOut,
                              float* roughnessOut, uint32_t* fellBack)
try {
    NX_DEBUG_HOOK("nxhip_shading_frame_batch");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    if ((!triIdx || !hitUv || !rayDir || !normalOut || !roughnessOut || !fellBack) && count) return fail_invalid("nxhip_shading_frame_batch: null buffer");
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(check_scene_ready(c));
    NX_TRY(check_hit_columns(c, "nxhip_shading_frame_batch", instanceIdx, triIdx, count, false));
    if (count == 0) return NXHIP_OK;
    NX_TRY(refresh_updated_blas(c));
    if (c->shadeInstDirty) NX_TRY(refresh_shade_inst(c));
    NX_TRY(upload_state(c));
    HookBatch b(c, count);
    const uint32_t* dTri = b.in(triIdx, 1);
    const float *dUv = b.in(hitUv, 2), *dDir = b.in(rayDir, 3);
    float *dN = b.out(normalOut, 3), *dR = b.out(roughnessOut, 1);
    uint32_t* dF = b.out(fellBack, 1);
    return b.run(kernels::shading_frame_hook(), c->dState.as<DeviceState>(), instanceIdx, dTri, dUv, dDir, count, dN, dR, dF);
} NX_CATCH("nxhip_shading_frame_batch")

int nxhip_material_inputs_batch(nxhip_ctx* c, uint32_t instanceIdx, const uint32_t* triIdx, const float* hitUv, uint32_t count, float* out)
try {
    NX_DEBUG_HOOK("nxhip_material_inputs_batch");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    if ((!triIdx || !hitUv || !out) && count) return fail_invalid("nxhip_material_inputs_batch: null buffer");
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(check_scene_ready(c));
    NX_TRY(check_hit_columns(c, "nxhip_material_inputs_batch", instanceIdx, triIdx, count, true));
    if (count == 0) return NXHIP_OK;
    NX_TRY(refresh_updated_blas(c));
    if (c->shadeInstDirty) NX_TRY(refresh_shade_inst(c));
    NX_TRY(upload_state(c));
    HookBatch b(c, count);
    const uint32_t* dTri = b.in(triIdx, 1);
    const float* dUv = b.in(hitUv, 2);
    float* dOut = b.out(out, 5);  // (c, r, m)
    return b.run(kernels::material_inputs_hook(), c->dState.as<DeviceState>(), instanceIdx, dTri, dUv, count, dOut);
} NX_CATCH("nxhip_material_inputs_batch")

int nxhip_fmath_batch(nxhip_ctx* c, int op, const double* a, const double* b, uint32_t count, double* out)
{
    NX_CHECK_CTX(c);
    if (op < 0 || op >= NXF_OP_COUNT) return fail_invalid("nxhip_fmath_batch: op must be one of NXF_OP_*");
    if ((!a || !out) && count) return fail_invalid("nxhip_fmath_batch: null buffer");
    if (count == 0) return NXHIP_OK;
    NX_HIP(hipSetDevice(c->device));
    HookBatch hb(c, count);
    const double *dA = hb.in(a, 1), *dB = hb.in(b, 1);  // (b == nullptr: a one-operand op, and the kernel is handed a null pointer)
    double* dOut = hb.out(out, 1);
    return hb.run(kernels::fmath_hook(), op, dA, dB, count, dOut);
}

int nxhip_enable_kernel_timing(nxhip_ctx* c, int enable)
{
    NX_CHECK_CTX(c);
    if (enable < 0 || enable > 3) return fail_invalid("nxhip_enable_kernel_timing: mode must be 0, 1, 2 or 3");
    if (enable != c->timingMode) invalidate_graph(c);
    c->timingMode = enable;
    c->graphTimersPending = false;
    c->timingEnabled = enable != 0;
    return NXHIP_OK;
}

int nxhip_read_graph_timeline(nxhip_ctx* c, int32_t* klass, float* startMs, float* durationMs, uint32_t capacity, uint32_t* count)
{
    NX_CHECK_CTX(c);
    if (!count) return fail_invalid("nxhip_read_graph_timeline: null count");
    if (capacity && (!klass || !startMs || !durationMs)) return fail_invalid("nxhip_read_graph_timeline: null destination");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    *count = (uint32_t)c->graphTimers.size();
    if (c->graphTimers.empty() || !c->lastRendered) return NXHIP_OK;
    for (size_t i = 0; i < c->graphTimers.size() && i < capacity; i++) {
        float s = 0.0f, d = 0.0f;
        NX_HIP(hipEventElapsedTime(&s, c->graphTimers[0].start, c->graphTimers[i].start));
        NX_HIP(hipEventElapsedTime(&d, c->graphTimers[i].start, c->graphTimers[i].stop));
        klass[i] = c->graphTimers[i].klass;
        startMs[i] = s;
        durationMs[i] = d;
    }
    return NXHIP_OK;
}

int nxhip_read_kernel_times(nxhip_ctx* c, nxhip_kernel_times* out, int reset)
{
    NX_CHECK_CTX(c);
    if (!out) return fail_invalid("null destination");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    for (size_t i = 0; i < c->timerPool.size(); i++) {
        float ms = 0.0f;
        NX_HIP(hipEventElapsedTime(&ms, c->timerPool[i].start, c->timerPool[i].stop));
        c->times.ms[c->timerPool[i].klass] += ms;
        (void)hipEventDestroy(c->timerPool[i].start);
        (void)hipEventDestroy(c->timerPool[i].stop);
    }
    c->timerPool.clear();
    if (c->graphTimersPending) {  // mode 3: the events hold the last replay of a back-to-back series
        for (size_t i = 0; i < c->graphTimers.size(); i++) {
            float ms = 0.0f;
            NX_HIP(hipEventElapsedTime(&ms, c->graphTimers[i].start, c->graphTimers[i].stop));
            c->times.ms[c->graphTimers[i].klass] += ms;
            c->times.launches[c->graphTimers[i].klass]++;
        }
        c->graphTimersPending = false;
    }
    *out = c->times;
    if (reset) std::memset(&c->times, 0, sizeof c->times);
    return NXHIP_OK;
}

int nxhip_debug_entry_walks(nxhip_ctx* c, uint64_t* count)
{
    NX_DEBUG_HOOK("nxhip_debug_entry_walks");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    if (!count) return fail_invalid("nxhip_debug_entry_walks: null count");
    *count = c->entryWalks;  // (host bookkeeping: nothing to wait for)
    return NXHIP_OK;
}

// The primary rays of the last pass as generate_kernel left them in trace.rays[0]: nothing is launched, the queue regions are copied
// out into dense path order (hook_layout's numbering IS generate_kernel's: region index / piece, slot index % piece).
int nxhip_debug_read_primary_rays(nxhip_ctx* c, float* origin3, float* direction3, uint32_t* pathIndex, uint32_t capacity, uint32_t* count)
try {
    NX_DEBUG_HOOK("nxhip_debug_read_primary_rays");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    if (!count) return fail_invalid("nxhip_debug_read_primary_rays: null count");
    if (!c->lastRendered) return fail_invalid("nxhip_debug_read_primary_rays: no pass has been rendered");
    if (c->h.settings.pathLength != 1)
        return fail_invalid("nxhip_debug_read_primary_rays: needs settings.pathLength == 1 (the later bounces of a pass write their rays over the primary ones)");
    if (c->passesInFlight > 1 || c->lastRendered != static_cast<PassSlot*>(c))
        return fail_invalid("nxhip_debug_read_primary_rays: needs one pass in flight (nxhip_set_passes_in_flight(1))");
    const PassSlot* q = c->lastRendered;
    const uint64_t n64 = (uint64_t)q->passPixels * q->frames;
    const uint32_t n = (uint32_t)n64;
    *count = n;
    if (n == 0) return NXHIP_OK;
    if (capacity < n || !origin3 || !direction3 || !pathIndex) return fail_invalid("nxhip_debug_read_primary_rays: capacity too small (*count holds the pass's paths)");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    const HookLayout l = hook_layout(c, n);
    // (the pass's queues may have been released or re-allocated since: nxhip_release_queues, nxhip_resize, a pixel map)
    if (n64 > q->pathCapacity || l.shards == 0 || l.piece > l.cap || q->trRayO.bytes < (size_t)l.shards * l.cap * 16 || q->trRayD.bytes < (size_t)l.shards * l.cap * 16)
        return fail_invalid("nxhip_debug_read_primary_rays: the queues of the last pass are gone (released or re-allocated since it was rendered)");
    std::vector<float4> o((size_t)l.shards * l.piece), d((size_t)l.shards * l.piece);
    NX_TRY(hook_copy(c, l, q->trRayO.p, o.data(), 16, false));
    NX_TRY(hook_copy(c, l, q->trRayD.p, d.data(), 16, false));
    NX_SYNC_ALL(c);
    for (uint32_t k = 0; k < n; k++) {
        origin3[3 * (size_t)k + 0] = o[k].x;
        origin3[3 * (size_t)k + 1] = o[k].y;
        origin3[3 * (size_t)k + 2] = o[k].z;
        direction3[3 * (size_t)k + 0] = d[k].x;
        direction3[3 * (size_t)k + 1] = d[k].y;
        direction3[3 * (size_t)k + 2] = d[k].z;
        std::memcpy(&pathIndex[k], &d[k].w, 4);
    }
    return NXHIP_OK;
} NX_CATCH("nxhip_debug_read_primary_rays")

}  // extern "C"

uint64_t nxd::layout_stamp_hooks() { return layout_stamp(); }
