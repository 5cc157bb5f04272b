// nexus/PathTracer.h — host driver of the hot path with the reference's interface
// (/root/reference/Nexus/src/Renderer/PathTracer.h:9-70, PathTracer.cpp:5-317).  Every method maps onto the C-ABI device
// layer (include/nexus_hip.h) instead of CUDA symbols, kernels and a CUDA graph.
#pragma once

#include <cstdint>
#include <vector>

#include "../nexus_hip.h"
#include "Scene.h"

namespace nexus {

class PathTracer {
public:
    PathTracer(uint32_t width, uint32_t height, int device = 0);
    ~PathTracer();
    PathTracer(const PathTracer&) = delete;
    PathTracer& operator=(const PathTracer&) = delete;

    void Reset();
    // the queue / path-state buffers go back to the device allocator (the reference frees them in Reset and on resize,
    // PathTracer.cpp:31, :300); the next Render() brings them back
    void FreeDeviceBuffers();
    void ResetFrameNumber();
    void Render(const Scene& scene);  // one frame: generate, trace, pathLength x (logic, shade, trace, shadow), accumulate
    void OnResize(uint32_t width, uint32_t height);
    void UpdateDeviceScene(const Scene& scene);
    // Extension, off by default: meshes added to `scene` from now on get their BVH8 from the device builder (nxhip_build_blas:
    // the reference's binned-SAH rule and SAH-DP collapse run in HBM, a tenth of the host builder's time) instead of
    // AssetManager::CreateBVH's host build; the nodes come back once, so BVH8::nodes / triangleIdx hold the tree as they do for
    // a host-built one.  The scene must not outlive this PathTracer while the switch is on.
    void SetDeviceBlasBuild(Scene& scene, bool enable);
    // Extension (skinned meshes): pose the mesh whose BVH is `bvhId` with a joint palette (Scene::JointPalette: joints x 12 floats).  An
    // immediate call, made BEFORE Scene::Update: the mesh's skin goes to the device on first use (nxhip_set_blas_skin), the device blends
    // the vertices and refits the BLAS (nxhip_pose_blas), and the box its root then encodes comes back (nxhip_read_blas_bounds: one small
    // read per posed mesh) for AssetManager::SetPosedBounds — from there Scene::Update and UpdateDeviceScene proceed as for a deformed
    // mesh, in all three TLAS modes.  The host's copy of the triangles stays the bind pose.  Throws for a mesh without a skin.
    void PoseMesh(Scene& scene, int32_t bvhId, const std::vector<float>& palette);
    // Extension (morph targets): the same for a mesh with morph targets — one weight per target (Scene::MorphWeights) and, where the mesh is
    // skinned too, its palette; an empty palette for an unskinned mesh.  Morph and skin go to the device on first use
    // (nxhip_set_blas_morph, nxhip_set_blas_skin), the device adds the active targets' deltas, blends the joints and refits the BLAS in one
    // pass (nxhip_pose_blas_morph).  Weights do not persist: the next pose names them again.  Throws for a mesh without a morph.
    void PoseMesh(Scene& scene, int32_t bvhId, const std::vector<float>& weights, const std::vector<float>& palette);
    void SetPixelQuery(uint32_t x, uint32_t y);
    int32_t GetSelectedInstance();
    uint32_t GetFrameNumber() const { return m_FrameNumber; }
    // The reference hands out a GL pixel buffer; headless here: the RGBA8 image, read back on demand.
    const std::vector<uint32_t>& GetPixelBuffer();
    // Extensions (see nexus_pod.h)
    void SetModes(int rngMode, int compactMode, int conductorMode);
    // Render() renders `frames` consecutive frames per call (bit-identical to as many single calls), lets `passes`
    // consecutive calls overlap on the GPU, and finishes the late bounces of small passes in one launch: the three
    // small-pass measures of the device layer (include/nexus_hip.h), none of which changes the image.
    void SetFramesPerPass(uint32_t frames);
    void SetPassesInFlight(uint32_t passes);
    // Hardware queues the device layer may count on when it shapes the passes in flight (nxhip_set_queue_budget): 0 = as
    // GPU_MAX_HW_QUEUES says (else 4), 1 .. 32 = this many.  Does not change the image.
    void SetQueueBudget(int queues);
    void SetTailBounce(uint32_t bounce);
    // Primary rays start from the traversal state the first node steps of their run of 64 paths provably share instead of the TLAS
    // root (nxhip_set_entry_points: hit records unchanged, pinhole cameras only).  Off by default.
    void SetEntryPoints(bool on);
    // How the light sample chooses among the mesh lights' triangles (nxhip_set_light_sampling): NXHIP_LIGHTS_UNIFORM (0, the reference's
    // rule and the default) or NXHIP_LIGHTS_POWER (1: in proportion to area x emitted luminance, from a table built on the device).
    // Same expectation either way: may be switched between frames.
    void SetLightSampling(int mode);
    // What an entry's probability depends on in NXHIP_LIGHTS_POWER (nxhip_set_light_importance): NXHIP_LIGHT_IMPORTANCE_POWER (0, the
    // default) or NXHIP_LIGHT_IMPORTANCE_POSITION (1: the shading point's position too, from a light tree built on the device).
    // Remembered in every mode; same expectation either way.
    void SetLightImportance(int importance);
    // Transparent shadows (nxhip_set_shadow_transmittance): NXHIP_SHADOWS_OPAQUE (0, the reference's rule and the default: a shadow ray ends
    // at the first triangle) or NXHIP_SHADOWS_TRANSMIT (1: every crossing multiplies the ray's transmittance by 1 - opacity x alpha(uv)).
    void SetShadowTransmittance(int mode);
    // The order of the frame's paths: NXHIP_ORDER_ROWS (the reference's, default) or NXHIP_ORDER_TILES (8 x 8 pixel tiles: the rays a
    // wave fetches together are a compact block of the image; kept across OnResize).  nxhip_set_pixel_order.
    void SetPixelOrder(int order);
    // Feature buffers of the camera ray's hit (nxhip_set_aov: albedo + coverage, shading normal + depth, accumulated like the colour;
    // what Renderer::SetDenoise and any external denoiser or compositor need).  Off by default; switching them on starts the
    // accumulation over (colour and features must cover the same frames).
    void SetFeatureBuffers(bool on);
    // The accumulated feature buffers as full-frame, row-major images (4 floats per pixel each), whatever the pixel order.  Not on a
    // tile split (each rank holds its own tiles only).
    void ReadFeatureBuffers(std::vector<float>& albedo4, std::vector<float>& normalDepth4);
    // Adaptive sampling (nxhip_set_adaptive: per-pixel noise statistics, a per-block stop rule and — params->cull — passes that render the
    // unsettled blocks only).  nullptr: off.  Switching it on starts the accumulation over.  Not on a tile split.  The image of an adaptive
    // run is not an unbiased estimate (include/nexus_hip.h).
    void SetAdaptive(const nx_adaptive_params* params);
    // {render `interval` frames, accumulate, decide} until no block is active or maxFrames frames were issued (nxhip_render_adaptive);
    // returns the frames issued.  activePixels: pixels still active afterwards.
    uint32_t RenderAdaptive(const Scene& scene, uint32_t maxFrames, uint32_t interval, uint32_t* activePixels = nullptr);
    // Samples folded into every pixel, as a full-frame, row-major image, whatever the pixel order.  Needs SetAdaptive.
    void ReadSampleCounts(std::vector<uint32_t>& counts);
    // Multi-GPU extension (no counterpart in the reference): one PathTracer per GPU, each renders and
    // accumulates the interleaved row tiles of its rank; Render() then ends with ONE RCCL gather of the accumulated tiles to
    // rank 0, whose GetPixelBuffer() returns the full frame.  `id128`: the 128 bytes rank 0 obtained from
    // CreateTileSplitId() and handed to every rank.  Call after construction / OnResize, before the first Render.
    static void CreateTileSplitId(void* id128);
    void EnableTileSplit(int worldSize, int rank, const void* id128, uint32_t tileRows = 5);
    void DisableTileSplit();
    bool IsTileSplitRoot() const { return m_TileSplit && m_Rank == 0; }
    nxhip_ctx* GetDeviceContext() const { return m_Ctx; }
    uint32_t GetWidth() const { return m_ViewportWidth; }
    uint32_t GetHeight() const { return m_ViewportHeight; }

private:
    void UploadPendingBlas(AssetManager& assets);
    nxhip_ctx* m_Ctx = nullptr;
    uint32_t m_FrameNumber = 0;
    uint32_t m_FramesPerPass = 1;
    uint32_t m_ViewportWidth = 0, m_ViewportHeight = 0;
    std::vector<uint32_t> m_Pixels;
    bool m_PixelQueryPending = false;
    bool m_TileSplit = false;
    int m_PixelOrder = 0;  // NXHIP_ORDER_* (SetPixelOrder)
    int m_Rank = 0;
};

}  // namespace nexus
