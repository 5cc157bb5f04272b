// nx_host.h — what the host units of the device layer (nxhip_*.hip) share, and what the kernel units export to them: the kernel
// getters with their argument lists, typed launches, the builders' entry points (internal to the device layer).
#pragma once

#include <cstring>
#include <type_traits>
#include <vector>

#include "nx_context.h"
#include "nx_variants.h"

namespace nxd {

// ---- what the kernel units export ---------------------------------------------------------------------
// nx_lbvh.hip, nx_lights.hip and nxhip_multigpu.hip include this header, so the compiler checks their declarations against the
// definitions.  The getters of the other kernel units are declared here as they are defined there (nx_trace.hip, nx_entry.hip,
// nx_hook_kernels.hip and the nx_wavefront*.hip units do not include it).
// The kernel families with compile-time instances: one lookup per family and unit, keyed by the feature set (nx_variants.h: kTf* for
// the trace kernel, kMf* for the rest) and the material type where there is one; nullptr for a set the unit does not hold.
const void* trace_kernel_of(unsigned set);  // nx_trace.hip
namespace wavefront { const void* logic(int items, unsigned set); const void* shade(int type, unsigned set); const void* shade_scan(unsigned set); const void* tail(unsigned set); }  // nx_wavefront.hip
namespace wavefront_detail { const void* shade(int type, unsigned set); const void* shade_scan(unsigned set); const void* tail(unsigned set); }  // the DETAIL instances (kFlavorDetail)
namespace wavefront_metal { const void* shade(int type, unsigned set); const void* shade_scan(unsigned set); const void* tail(unsigned set); }  // the METAL instances (kFlavorMetal); shade: the fifth type's
namespace wavefront_solid { const void* shade(int type, unsigned set); const void* shade_scan(unsigned set); }  // the SOLID instances (kFlavorSolid): METAL and DETAIL ones too; no tail kernel
const void* medium_scatter_kernel_of(bool grid, unsigned set);  // nx_medium.hip: the medium's kernels (kFlavorMedium; grid: kFlavorMediumGrid) and its hooks'
const void* thin_kernel_ptr();  // nx_trace.hip
const void* entry_state_kernel_ptr();  // nx_entry.hip
const void* count_scan_kernel_ptr();  // nx_wavefront.hip
const void* begin_frame_kernel_ptr();
const void* hook_sizes_kernel_ptr();
const void* generate_kernel_ptr();
const void* accumulate_kernel_ptr();
const void* compose_kernel_ptr();
const void* logic_metal_kernel_ptr();  // nx_wavefront_metal.hip (the classic pipeline's fifth queue)
const void* bsdf_hook_kernel_ptr();  // nx_hook_kernels.hip: the array test hooks
const void* bsdf_hook_metal_kernel_ptr();
const void* fmath_hook_kernel_ptr();
const void* tex2d_hook_kernel_ptr();
const void* tex2d_float_hook_kernel_ptr();
const void* tex2d_linear_hook_kernel_ptr();
const void* env_hook_kernel_ptr();
const void* alight_hook_kernel_ptr();
const void* shading_frame_hook_kernel_ptr();
const void* material_inputs_hook_kernel_ptr();
const void* medium_shadow_kernel_ptr();  // nx_medium.hip
const void* medium_segment_hook_kernel_ptr();
const void* medium_phase_hook_kernel_ptr();
const void* medium_shadow_grid_kernel_ptr();  // ... the density grid's (kFlavorMediumGrid), its build and its hooks'
const void* medium_brick_kernel_ptr();
const void* medium_density_hook_kernel_ptr();
const void* medium_track_hook_kernel_ptr();
const void* aov_kernel_ptr();  // nx_aov.hip
const void* aov_fold_kernel_ptr();
const void* denoise_gather_kernel_ptr();
const void* denoise_iteration_kernel_ptr(int step, bool forceDirect);
const void* adaptive_accumulate_kernel_ptr();  // nx_adaptive.hip
const void* adaptive_aov_fold_kernel_ptr();
const void* adaptive_decide_kernel_ptr();
const void* adaptive_scan_kernel_ptr();
const void* adaptive_fill_kernel_ptr();
const void* light_pick_kernel_ptr();  // nx_lights.hip
const void* light_tree_pick_kernel_ptr();
const void* light_tree_prob_kernel_ptr();
const void* inst_code_kernel_ptr();  // nx_refit.hip
const void* inst_code_metal_kernel_ptr();  // (... of a material table with an NX_MAT_METALROUGH)
const void* instance_transform_kernel_ptr();
const void* tlas_refit_kernel_ptr();
const void* blas_refit_kernel_ptr();
const void* pose_kernel_ptr(bool lds);  // nx_skin.hip: the palette from the LDS, or from global memory
const void* pose_morph_kernel_ptr(bool skin, bool lds);  // ... with the morph stage in front; skin off: morph only
uint64_t layout_stamp_trace();
uint64_t layout_stamp_wavefront();
uint64_t layout_stamp_wavefront_detail();
uint64_t layout_stamp_wavefront_solid();
uint64_t layout_stamp_wavefront_metal();
uint64_t layout_stamp_hook_kernels();
uint64_t layout_stamp_medium();
uint64_t layout_stamp_refit();
uint64_t layout_stamp_skin();
uint64_t layout_stamp_lbvh();
uint64_t layout_stamp_multigpu();
uint64_t layout_stamp_entry();
uint64_t layout_stamp_aov();
uint64_t layout_stamp_adaptive();
uint64_t layout_stamp_lights();
uint64_t layout_stamp_envmap();
uint64_t layout_stamp_sky();
uint64_t layout_stamp_scene();  // the host units nxhip_*.hip that fill DeviceState, each its own
uint64_t layout_stamp_render();
uint64_t layout_stamp_features();
uint64_t layout_stamp_hooks();
int light_scan_bytes(size_t entries, size_t* bytes);
int light_map_mean(hipStream_t st, const TextureDev& t, const float* srgbLut, float* mean4, double* mean64);
int light_table_build(hipStream_t st, const LightBuild& b, void* scanTemp, size_t scanBytes);
int light_tree_sort_bytes(size_t entries, size_t* bytes);
int light_tree_build(hipStream_t st, const LightTreeBuild& b, void* sortTemp, size_t sortBytes);
// nx_envmap.hip: the float environment map's sampler tables, built on the device in stream order (temp: 2 x height doubles)
int env_float_tables_build(hipStream_t st, const float4* texels, uint32_t width, uint32_t height, double* temp, float* marginalCdf, float* rowCdf, float* density,
                           uint32_t* marginalGuide, uint32_t* rowGuide);
// nx_sky.hip: the sun-and-sky environment (nxhip_set_sky).  SkyLaunch: what the kernels take, kilometres, binary32.  SkyPlan: a validated
// nx_sky in binary64 (sky_plan refuses what nxhip_set_sky refuses, naming `who`).  SkyDisc: the baked sun disc of one map — its bounding
// box (wrapping in x), the cap and Lsun x k.
struct SkyLaunch {
    float r0, q0;  // the observer's |p| and |p|^2 - Rg^2
    float sun[3];
    float betaR[3], betaMs, betaMe;
    float g;
    float irradiance[3], albedo[3];
    uint32_t nv, nl;
};
struct SkyDisc {
    uint32_t x0, y0, w, h;
    float add[3];  // Lsun x k per channel
    double sun[3], chord2;  // |d - s|^2 <= chord2 = 4 sin^2(alpha / 2)
};
struct SkyPlan {
    double sun[3], alpha, q0, r0, betaR[3], betaMs, betaMe;
    SkyLaunch launch;
};
int sky_plan(const nx_sky* sky, const char* who, SkyPlan* out);
void sky_sun_transmittance(const SkyPlan& p, uint32_t segments, double T[3]);  // T_sun(observer) by the light-ray rule
int sky_disc_plan(const nx_sky* sky, const SkyPlan& p, const char* who, SkyDisc* out);
int sky_generate(hipStream_t st, const SkyPlan& p, const SkyDisc* disc, float4* texels, uint32_t width, uint32_t height);
const void* sky_hook_kernel_ptr();
int lbvh_build(nxhip_ctx* c, const nx_triangle* dTris, uint32_t n, int plocRadius, DevBuf& nodes, DevBuf& primIdx, DevBuf& isect, uint32_t* nodeCount);
int lbvh_build_batch(nxhip_ctx* c, const nx_triangle* dTris, const std::vector<uint32_t>& counts, DevBuf& nodes, DevBuf& primIdx, DevBuf& isect, std::vector<uint32_t>& nodeFirst,
                     std::vector<uint32_t>& nodeCounts);
int lbvh_write_isect(nxhip_ctx* c, const nx_triangle* dTris, const uint32_t* dPrimIdx, uint32_t n, float4* dIsect);
int lbvh_build_tlas(nxhip_ctx* c, const nx_bvh_instance* dInstances, uint32_t n, int plocRadius, DevBuf& nodes, DevBuf& primIdx, DevBuf& box, bool* boxesAreTight, uint32_t* nodeCount);

// (threads per workgroup of the kernels the host sizes grids for: kTraceBlock / kShadeBlock / kLogicBlock / kWideBlock, nx_device.h)
constexpr int kHookBounceSlot = NX_PATH_MAX_LENGTH - 1;  // queue-size slot used by the batch test hooks

// ---- typed launches ------------------------------------------------------------------------------------
// A kernel with its parameter list: the one place that says what a launch of it must pass.  make_launch / launch_untimed take
// exactly these types (converting at the call site), so a call that does not fit the list does not compile.
template <class... A> struct Kernel { const void* fn; };

// The parameter lists, each read against the kernel's __global__ definition.  (Pointers to structures private to nx_refit.hip —
// InstBox, Box, NodeBox32 — are stated as void*: the same 8 bytes.)
namespace kernels {
using State = const DeviceState*;
using U32 = uint32_t;
using StateKernel = Kernel<State>;            // (S)
using BounceKernel = Kernel<State, int>;      // (S, bounce | flags)
using TypeKernel = Kernel<State, int, int>;   // (S, bounce | flags, type or type mask)
// The families with compile-time instances, one getter each: the owning unit is asked for the set's instance.  The caller has made the
// set canonical (nxhip_render.hip material_features / trace_features): nothing is dropped here, and a set nobody compiled gives
// fn == nullptr, which no launch is made of (frame_levels and the ray-batch hooks refuse: NXHIP_ERR_INVALID).
inline BounceKernel trace(unsigned set) { return {trace_kernel_of(set)}; }
inline BounceKernel thin() { return {thin_kernel_ptr()}; }
inline StateKernel entry_state() { return {entry_state_kernel_ptr()}; }
inline BounceKernel logic(int items, unsigned set) { return {wavefront::logic(items, set)}; }
inline BounceKernel logic_metal() { return {logic_metal_kernel_ptr()}; }
// (the units split the material kernels' instances by their newest feature: nx_wavefront_detail.hip says why the split exists)
inline BounceKernel tail(unsigned set) { return {(set & kMfMetal) ? wavefront_metal::tail(set) : (set & kMfDetail) ? wavefront_detail::tail(set) : wavefront::tail(set)}; }
inline TypeKernel shade_scan(unsigned set)
{
    return {(set & kMfSolid) ? wavefront_solid::shade_scan(set) : (set & kMfMetal) ? wavefront_metal::shade_scan(set) : (set & kMfDetail) ? wavefront_detail::shade_scan(set) : wavefront::shade_scan(set)};
}
inline BounceKernel shade(int type, unsigned set)  // (classic pipeline: the set names no METAL, the type does)
{
    return {(set & kMfSolid) ? wavefront_solid::shade(type, set) : type == NX_MAT_METALROUGH ? wavefront_metal::shade(type, set) : (set & kMfDetail) ? wavefront_detail::shade(type, set) : wavefront::shade(type, set)};
}
inline TypeKernel count_scan() { return {count_scan_kernel_ptr()}; }
inline Kernel<DeviceState*, U32, U32, U32> begin_frame() { return {begin_frame_kernel_ptr()}; }  // (S, frames, frameLast, scanEpoch)
inline Kernel<DeviceState*, U32, int, int> hook_sizes() { return {hook_sizes_kernel_ptr()}; }    // (S, n, anyHit, slot)
inline StateKernel generate() { return {generate_kernel_ptr()}; }
// (S, src, count, slices, sliceStride, firstFrame, dstMap)
inline Kernel<State, const float4*, U32, U32, U32, U32, const U32*> accumulate() { return {accumulate_kernel_ptr()}; }
inline Kernel<const float4*, U32, const U32*, float4*, U32*> compose() { return {compose_kernel_ptr()}; }  // (src, count, dstMap, dstAccum, dstRgba8)
inline Kernel<const nx_material*, const nx_bsdf_query*, U32, int, nx_bsdf_result*> bsdf_hook() { return {bsdf_hook_kernel_ptr()}; }  // (material, q, count, sample, out)
inline Kernel<const nx_material*, const nx_bsdf_query*, U32, int, nx_bsdf_result*> bsdf_hook_metal() { return {bsdf_hook_metal_kernel_ptr()}; }  // (the same list; NX_MAT_METALROUGH)
inline Kernel<State, U32, const U32*, const float*, U32, float*> material_inputs_hook() { return {material_inputs_hook_kernel_ptr()}; }  // (S, instance, triIdx, hitUv, count, out)
inline Kernel<int, const double*, const double*, U32, double*> fmath_hook() { return {fmath_hook_kernel_ptr()}; }                   // (op, a, b, count, out)
inline Kernel<TextureDev, const float*, const float*, U32, float4*> tex2d_hook() { return {tex2d_hook_kernel_ptr()}; }              // (t, srgbLut, uv, count, out)
inline Kernel<const float4*, int, int, const float*, U32, float4*> tex2d_float_hook() { return {tex2d_float_hook_kernel_ptr()}; }       // (texels, W, H, uv, count, out)
inline Kernel<State, int, const float*, U32, float*, float*, U32*> env_hook() { return {env_hook_kernel_ptr()}; }                    // (S, sample, in, count, vec, pdf, texel)
inline Kernel<SkyLaunch, const float*, U32, float*> sky_hook() { return {sky_hook_kernel_ptr()}; }                                    // (P, dir, count, rgb)
inline Kernel<TextureDev, const float*, U32, float4*> tex2d_linear_hook() { return {tex2d_linear_hook_kernel_ptr()}; }                  // (t, uv, count, out)
// (S, instance, triIdx, hitUv, rayDir, count, normal, roughness, fellBack)
inline Kernel<State, U32, const U32*, const float*, const float*, U32, float*, float*, U32*> shading_frame_hook() { return {shading_frame_hook_kernel_ptr()}; }
// (S, light, origin, r, count, direction, tmax, factor, ok)
inline Kernel<State, U32, const float*, const float*, U32, float*, float*, float*, U32*> alight_hook() { return {alight_hook_kernel_ptr()}; }
inline BounceKernel medium_scatter(bool grid, unsigned set) { return {medium_scatter_kernel_of(grid, set)}; }  // (S, bounce | kShadeDropEnded)
inline BounceKernel medium_shadow() { return {medium_shadow_kernel_ptr()}; }
// (S, origin, dir, tEnd, xi, count, t0, length, transmittance, scatterT)
inline Kernel<State, const float*, const float*, const float*, const float*, U32, float*, float*, float*, float*> medium_segment_hook() { return {medium_segment_hook_kernel_ptr()}; }
// (S, dirIn, xi1, xi2, count, dirOut, pdf)
inline Kernel<State, const float*, const float*, const float*, U32, float*, float*> medium_phase_hook() { return {medium_phase_hook_kernel_ptr()}; }
inline BounceKernel medium_shadow_grid() { return {medium_shadow_grid_kernel_ptr()}; }
// (rho, nx, ny, nz, nbx, nby, nbz, bricks)
inline Kernel<const float*, U32, U32, U32, U32, U32, U32, float*> medium_brick() { return {medium_brick_kernel_ptr()}; }
// (S, points, count, rho, majorant)
inline Kernel<State, const float*, U32, float*, float*> medium_density_hook() { return {medium_density_hook_kernel_ptr()}; }
// (S, origin, dir, tEnd, seed, count, scatterT, transmittance, steps2)
inline Kernel<State, const float*, const float*, const float*, const U32*, U32, float*, float*, U32*> medium_track_hook() { return {medium_track_hook_kernel_ptr()}; }
inline StateKernel aov() { return {aov_kernel_ptr()}; }
inline StateKernel aov_fold() { return {aov_fold_kernel_ptr()}; }
inline Kernel<State, float4*, float4*, float4*, U32*> denoise_gather() { return {denoise_gather_kernel_ptr()}; }  // (S, colour, albedo, normalDepth, rgba8)
inline Kernel<DenoiseLaunch> denoise_iteration(int step, bool forceDirect) { return {denoise_iteration_kernel_ptr(step, forceDirect)}; }
inline StateKernel adaptive_accumulate() { return {adaptive_accumulate_kernel_ptr()}; }
inline StateKernel adaptive_aov_fold() { return {adaptive_aov_fold_kernel_ptr()}; }
inline Kernel<AdaptiveLaunch> adaptive_decide() { return {adaptive_decide_kernel_ptr()}; }
inline Kernel<AdaptiveLaunch> adaptive_scan() { return {adaptive_scan_kernel_ptr()}; }
inline Kernel<AdaptiveLaunch> adaptive_fill() { return {adaptive_fill_kernel_ptr()}; }
// (table, guide, guideSize, entries, u, count, entry, prob)
inline Kernel<const LightEntry*, const U32*, U32, U32, const float*, U32, U32*, float*> light_pick() { return {light_pick_kernel_ptr()}; }
// (nodes, leaves, points, u, count, entry, prob)
inline Kernel<const LightNode*, U32, const float*, const float*, U32, U32*, float*> light_tree_pick() { return {light_tree_pick_kernel_ptr()}; }
// (nodes, leaves, slotOf, points, entry, count, prob)
inline Kernel<const LightNode*, U32, const U32*, const float*, const U32*, U32, float*> light_tree_prob() { return {light_tree_prob_kernel_ptr()}; }
inline Kernel<State, InstTrav*, const ShadeInst*, U32> inst_code(bool metal = false) { return {metal ? inst_code_metal_kernel_ptr() : inst_code_kernel_ptr()}; }  // (S, trav, shadeInst, count)
// (S, instances, trav, leafOfInstance, ids, transforms, count, tightBoxes, shadeInst, blasRefresh)
inline Kernel<State, nx_bvh_instance*, InstTrav*, const U32*, const U32*, const float*, U32, void*, ShadeInst*, U32> instance_transform() { return {instance_transform_kernel_ptr()}; }
// (nodes, primIdx, instances, order, levelStart, levels, nodeBox, tightBoxes)
inline Kernel<nx_bvh8_node*, const U32*, const nx_bvh_instance*, const U32*, const U32*, U32, void*, const void*> tlas_refit() { return {tlas_refit_kernel_ptr()}; }
// (nodes, triIdx, tris, order, levelStart, firstLevel, levelCount, nodeBox)
inline Kernel<uint4*, const U32*, const nx_triangle*, const U32*, const U32*, U32, U32, void*> blas_refit() { return {blas_refit_kernel_ptr()}; }
// (bind, skin, palette, jointCount, primIdx, n, tris, shadeTris, isect); lds: launched with 48 B of dynamic LDS per joint
inline Kernel<const uint4*, const uint4*, const float4*, U32, const U32*, U32, uint4*, uint4*, float4*> pose(bool lds) { return {pose_kernel_ptr(lds)}; }
// (the list of pose, then: morph, active, activeCount); skin off: skin and palette are not read
inline Kernel<const uint4*, const uint4*, const float4*, U32, const U32*, U32, uint4*, uint4*, float4*, const uint4*, const uint2*, U32> pose_morph(bool skin, bool lds)
{
    return {pose_morph_kernel_ptr(skin, lds)};
}
}  // namespace kernels

constexpr size_t arg_end(size_t at, size_t size, size_t align) { return (at + align - 1) / align * align + size; }
template <class... A> constexpr size_t args_bytes()
{
    size_t at = 0;
    ((at = arg_end(at, sizeof(A), alignof(A))), ...);
    return at;
}

// One kernel launch of a pass, kept until it is issued (launch_now) or becomes a graph node (pass_graph).  The argument VALUES live
// in `bytes`, each at its `offset`: a Launch is copied into vectors between construction and use, so it holds no pointer into
// itself — params() makes the void* array at the moment of the HIP call, which copies the values out during the call.
struct Launch {
    static constexpr size_t kMaxArgs = 8, kArgBytes = sizeof(DenoiseLaunch);  // the largest block any kernel of a pass takes
    const void* fn = nullptr;
    dim3 grid, block;
    int klass = 0;   // NXHIP_K_*
    int after = -1;  // -1: depends on the previous level; k: on launch k of ITS OWN level only (a chain inside the level)
    uint8_t argCount = 0, offset[kMaxArgs] = {};
    alignas(8) unsigned char bytes[kArgBytes] = {};
    void params(void** out) const
    {
        for (int i = 0; i < argCount; i++) out[i] = const_cast<unsigned char*>(bytes) + offset[i];
    }
};

template <class... A> Launch make_launch(Kernel<A...> k, dim3 grid, dim3 block, int klass, std::common_type_t<A>... args)
{
    static_assert(sizeof...(A) <= Launch::kMaxArgs && args_bytes<A...>() <= Launch::kArgBytes, "the arguments do not fit a Launch");
    static_assert((std::is_trivially_copyable<A>::value && ...) && ((alignof(A) <= 8) && ...), "kernel arguments are plain values");
    Launch l;
    l.fn = k.fn;
    l.grid = grid;
    l.block = block;
    l.klass = klass;
    size_t at = 0;
    ((at = arg_end(at, 0, alignof(A)), l.offset[l.argCount++] = (uint8_t)at, std::memcpy(l.bytes + at, &args, sizeof(A)), at += sizeof(A)), ...);
    return l;
}

// A launch outside the passes (scene edits, test hooks): not timed, and the slot's error word is none of its business.
template <class... A> hipError_t launch_untimed(Kernel<A...> k, dim3 grid, dim3 block, hipStream_t stream, std::common_type_t<A>... args)
{
    void* params[] = {(void*)&args...};
    return hipLaunchKernel(k.fn, grid, block, params, 0, stream);
}
// ... of a kernel that sizes an `extern __shared__` array by the launch (ldsBytes <= 64 KiB: no attribute needed)
template <class... A> hipError_t launch_untimed_lds(Kernel<A...> k, dim3 grid, dim3 block, size_t ldsBytes, hipStream_t stream, std::common_type_t<A>... args)
{
    void* params[] = {(void*)&args...};
    return hipLaunchKernel(k.fn, grid, block, params, ldsBytes, stream);
}

// ---- what the host units share ---------------------------------------------------------------------------
int fail_invalid(const char* msg);  // sets the error string; returns NXHIP_ERR_INVALID
int fail_invalid(const std::string& msg);

#define NX_CHECK_CTX(ctx)                      \
    do {                                       \
        if (!(ctx)) {                          \
            ::nxd::set_error("null context");  \
            return NXHIP_ERR_INVALID;          \
        }                                      \
        if ((ctx)->dead) {                     \
            ::nxd::set_error("the context is dead: nxhip_sync_timeout gave up waiting for the device (see include/nexus_hip.h)"); \
            return NXHIP_ERR_TIMEOUT;          \
        }                                      \
    } while (0)

// `} NX_CATCH("nxhip_name")` closes the function-try-block of an entry point: nothing may unwind through the C boundary
#define NX_CATCH(name)                                          \
    catch (const std::exception& e) {                           \
        ::nxd::set_error(std::string(name ": ") + e.what());    \
        return NXHIP_ERR_INVALID;                               \
    }

// a step of an entry point that returns a status: on anything but NXHIP_OK the entry point returns it
#define NX_TRY(call)                                    \
    do {                                                \
        const int rcTry_ = (call);                      \
        if (rcTry_ != NXHIP_OK) return rcTry_;          \
    } while (0)

#define NX_ALLOC(buf, n)                                  \
    do {                                                  \
        if (!(buf).alloc(n)) return NXHIP_ERR_HIP;        \
    } while (0)

// slot k of the context: 0 is the context itself, k >= 1 the extra in-flight passes
inline PassSlot* slot_at(nxhip_ctx* c, uint32_t k) { return k == 0 ? static_cast<PassSlot*>(c) : c->extra[k - 1].get(); }
inline uint32_t slot_count(const nxhip_ctx* c) { return 1u + (uint32_t)c->extra.size(); }

// Wait for everything the context has issued, on every slot's stream (scene edits, re-allocations, read-backs).
int sync_all(nxhip_ctx* c);
#define NX_SYNC_ALL(c)                                  \
    do {                                                \
        const int rcSync_ = ::nxd::sync_all(c);         \
        if (rcSync_ != NXHIP_OK) return rcSync_;        \
    } while (0)

// The nxhip_debug_* entry points exist for the tests (one of them plants a cycle in an uploaded BVH).  A `make release` library
// (NX_NO_DEBUG_HOOKS) keeps the symbols — the header and the ABI stamp are the same — and refuses the calls.
#ifdef NX_NO_DEBUG_HOOKS
#define NX_DEBUG_HOOK(name) return ::nxd::fail_invalid(name ": this library was built without the test hooks (make release)")
#else
#define NX_DEBUG_HOOK(name) do { } while (0)
#endif

// Which pipeline a pass runs (nx_wavefront.h): SCAN — the logic step's decision rides in the hit records and the material kernels
// pick their items out of the trace queue — whenever slots are handed out by racing atomics; the CLASSIC logic kernel + material
// queues for the ordered compaction, whose serial slot order IS the reference's copy order (PathTracer.cu:183-206).
inline bool scan_pipeline(const nxhip_ctx* c) { return c->h.compactMode == NX_COMPACT_FAST; }

// Pixels per frame slice of the next pass: the context's pixel set, or the active part of it (adaptive sampling).  c->localCount stays
// the size of the image and of every read-back.
inline uint32_t pass_pixels(const nxhip_ctx* c) { return c->adaptive ? c->activeCount : c->localCount; }

// Something the entry-state walk reads has changed (the list: nxhip_ctx::entryGeneration): every slot's table is stale from here on.
inline void entry_inputs_changed(nxhip_ctx* c) { c->entryGeneration++; }

// nxhip_api.hip: the context's state block, queues and pixel set
void invalidate_graph(nxhip_ctx* c);
int upload_state(nxhip_ctx* c);
void refresh_medium_grid(nxhip_ctx* c);                      // nxhip_scene.hip: the density grid's words of the state block
int check_medium_grid(const nxhip_ctx* c, const char* who);  // ... and the thickness a render or a walking hook refuses
int alloc_queues(nxhip_ctx* c, size_t n);
bool slot_queues_ready(const nxhip_ctx* c, const PassSlot* q);
int ensure_slot_queues(nxhip_ctx* c, PassSlot* q);
int ensure_metal_queue(nxhip_ctx* c, PassSlot* q);  // the classic pipeline's fifth material queue, while a material is an NX_MAT_METALROUGH
void release_slot_queues(nxhip_ctx* c, PassSlot* q);
void release_denoise_planes(nxhip_ctx* c);
void publish_pixel_set(nxhip_ctx* c);
int set_frame_number_device(nxhip_ctx* c, uint32_t f);
// nxhip_scene.hip: what a pass or a hook brings up to date before it reads the scene
int refresh_shade_inst(nxhip_ctx* c);
bool material_see_through(const nxhip_ctx* c, const nx_material& m);  // a shadow ray of NXHIP_SHADOWS_TRANSMIT may pass it
void refresh_alpha_modes(nxhip_ctx* c);  // nxhip_ctx::materialsAlphaMask / materialsAlphaSolid, after the alpha table has changed
int check_alpha_table(const nxhip_ctx* c);  // the table's count and the MASK-on-a-mesh-light refusal (check_scene_ready and the ray-batch hooks)
void refresh_detail_maps(nxhip_ctx* c);  // nxhip_ctx::materialsNameDetail, after the detail table has changed
void refresh_see_through(nxhip_ctx* c);  // nxhip_ctx::materialsSeeThrough, and the shading records' copy of the fact
int refresh_updated_blas(nxhip_ctx* c);
// nxhip_render.hip
int check_scene_ready(nxhip_ctx* c);
int launch_now(nxhip_ctx* c, const Launch& l, hipStream_t stream = nullptr);  // (stream: the context's own unless given)
int render_pass(nxhip_ctx* c, uint32_t framesArg);
unsigned hook_trace_features(const nxhip_ctx* c, bool anyHit, bool transmit);  // the ray-batch hooks' trace launch, by the passes' own rule (trace_features)
uint32_t queue_budget_from_text(const char* text);  // what a value of GPU_MAX_HW_QUEUES means: a whole number in [1, 32], else 4
uint32_t queue_budget_from_environment();           // ... of the variable as it is now (nxhip_create, nxhip_set_queue_budget)
uint32_t resident_slots_for(uint32_t passes, uint32_t budget);  // of `passes` in flight, the slots whose launches a budget keeps on the chip at once
int read_float4_as_float3(nxhip_ctx* c, const void* dev, uint32_t count, float* dst);
// nxhip_features.hip
int adaptive_restart(nxhip_ctx* c);
int refresh_light_table(nxhip_ctx* c);

}  // namespace nxd
