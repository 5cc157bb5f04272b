/*
 * nexus_hip.h — C-ABI of the MI355X (gfx950) device layer: the wavefront path-tracing hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI layer: its host classes reach the device
 * through CUDA symbols and bare kernel pointers (17 GetDevice*Address() getters,
 * /root/reference/Nexus/src/Cuda/PathTracer/PathTracer.cuh:86-103, and (void*)XxxKernel pointers,
 * Renderer/PathTracer.cpp:99-107).  Each entry point below names the reference interface it replaces.
 * Plain C: opaque context, plain pointers and sizes, int status (0 = ok, message via
 * nxhip_last_error()); no HIP, torch or C++ types in any signature.  Host arrays passed in are copied
 * before the call returns.  A context belongs to one host thread at a time; one context per GPU.
 */
#ifndef NEXUS_HIP_H
#define NEXUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "nexus_fmath.h"
#include "nexus_pod.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nxhip_ctx nxhip_ctx;

enum {
    NXHIP_OK = 0,
    NXHIP_ERR_INVALID = 1, /* bad argument / state */
    NXHIP_ERR_HIP = 2,     /* a HIP runtime call failed */
    NXHIP_ERR_NO_DEVICE = 3,
    NXHIP_ERR_TRAVERSAL = 4, /* a trace kernel gave up on rays that made no progress (malformed BVH): reported by nxhip_sync and the read-backs */
    NXHIP_ERR_ABI = 5,       /* caller and library (or the library's own translation units) disagree about a struct layout / the API version */
    NXHIP_ERR_TIMEOUT = 6    /* nxhip_sync_timeout gave up waiting: the context is DEAD from then on (every later call returns this) */
};

/* Bumped whenever an entry point changes its signature or meaning, or a struct of this header / nexus_pod.h its layout.  (Entry points
 * and structs that are only ADDED — adaptive sampling, nx_adaptive_params — leave it alone: the struct's words join the ABI stamp below,
 * so a library without them is still refused.) */
#define NXHIP_API_VERSION 8

/* Thread-local message of the last failing call (replaces CheckCudaErrors -> exit(99), Utils/Utils.cpp:3-12). */
const char *nxhip_last_error(void);

/* Number of visible HIP devices (0 if none / runtime unavailable). */
int nxhip_device_count(void);

/* PathTracer::PathTracer(width, height) + Reset() — Renderer/PathTracer.cpp:5-28, 92-241: allocates every
 * queue for `localPixels` paths.  `stream` is a hipStream_t passed as void* (NULL: the context creates its own). */
int nxhip_create(int device, uint32_t width, uint32_t height, void *stream, nxhip_ctx **out);
/* PathTracer::~PathTracer / FreeDeviceBuffers — PathTracer.cpp:30-90 */
void nxhip_destroy(nxhip_ctx *ctx);
/* PathTracer::OnResize — PathTracer.cpp:290-303 (frees and re-allocates queues, resets the frame number) */
int nxhip_resize(nxhip_ctx *ctx, uint32_t width, uint32_t height);
int nxhip_sync(nxhip_ctx *ctx);
/* nxhip_sync with a wall-clock limit (milliseconds).  The reference waits for the device without one and a kernel that never ends hangs
 * the viewer (CheckCudaErrors only sees launches that RETURN: Utils/Utils.cpp:3-12, Renderer/PathTracer.cpp:280-284).  Polls the
 * context's streams; work done in time: as nxhip_sync.  Otherwise NXHIP_ERR_TIMEOUT and the context is marked DEAD: nothing can be
 * said about the device's state, every later call on it returns NXHIP_ERR_TIMEOUT without touching the device (nxhip_destroy frees
 * the host side only); the caller reports and exits, or starts a fresh process — there is no in-process recovery from a hung GPU. */
int nxhip_sync_timeout(nxhip_ctx *ctx, uint32_t timeoutMs);

/* ---- scene upload -------------------------------------------------------------------------------- */

/* BVH8::InitDeviceData + AssetManager::InitDeviceData — Geometry/BVH/BVH8.cpp:28-33, Assets/AssetManager.cpp:45-49
 * (symbol `bvhs`).  Returns the BLAS id == index instances refer to as bvhIdx.  ids are dense from 0.
 * Any node array that is a tree is taken, whatever its shape; the traversal keeps 32 stack entries per ray, TLAS and BLAS together, as
 * the reference does (BVH8Traversal.cuh:17), and a ray that needs more loses the subtrees whose entries did not fit (they are dropped,
 * nothing else is disturbed).  Builder-made trees stay far below that: the test scenes measure 1 ... 5 entries (3 000-triangle soup 3,
 * 20 instances 5, Cornell box 1, 65 k-triangle torus 5), 120 instances scaled in geometric progression 18. */
int nxhip_upload_blas(nxhip_ctx *ctx, const nx_bvh8_node *nodes, uint32_t nodeCount, const nx_triangle *tris,
                      uint32_t triCount, const uint32_t *triIdx, int32_t *blasId);
/* BLAS built ON THE DEVICE from triangles alone.  Replaces BVH2::Build + BVH8Builder::Init /
 * Build + BVH8::InitDeviceData (Geometry/BVH/BVH.cpp:13-210, BVH8Builder.cpp:10-393, BVH8.cpp:28-33) with the same two
 * steps in HBM: a binary tree by the reference's rule — top-down, binned surface-area heuristic over the centroid bounds,
 * one primitive per leaf, "split in half" when nothing separates (level-synchronous: atomics into 16 bins per axis and node,
 * a scan partition per level, nodes of up to 8 primitives finished by an exact sweep) — and the reference's SAH dynamic
 * programme for the collapse into 80-byte 8-wide nodes (cost table bottom-up, decisions followed top-down, the reference's
 * octant slot assignment and quantisation).  29 ms per million triangles (host builder of this repo: 0.4 s on 16 threads; the
 * reference: ~10 s on one) and fewer node visits per ray than the host build on every mesh of
 * profiles/r03_builder_quality.txt.  A valid, conservative CWBVH whose node bytes differ from the host builder's (another
 * tree); hit records are the same up to equidistant ties.  Returns the BLAS id like nxhip_upload_blas. */
int nxhip_build_blas(nxhip_ctx *ctx, const nx_triangle *tris, uint32_t triCount, int32_t *blasId);
/* The BLASes of `meshCount` meshes in ONE device build.  The reference creates one BVH8 per aiMesh of a file
 * (Assets/OBJLoader.cpp:213-239 -> AssetManager::AddMesh -> CreateBVH, Assets/AssetManager.cpp:23-37: a glTF scene is hundreds
 * or thousands of small meshes); built one by one on the device each of them pays the build's ~25 level synchronisations and
 * its allocations.  Here the meshes are a forest over the concatenated triangles — per-mesh Morton order, one root segment per
 * mesh, then the level loops of nxhip_build_blas (binning, split, partition; cost table; collapse) over all meshes at once — and
 * the BLASes share four pooled allocations.  Each tree is the tree nxhip_build_blas(tris[m], triCounts[m]) builds (same
 * decisions from the same counts, boxes and orders; node numbering differs as between two single builds).  blasIds[m] (may be
 * NULL) = the id of mesh m; ids are consecutive.  With another builder selected (nxhip_set_device_builder) the meshes are built
 * one by one.  1 000 meshes of 1 000 triangles: see profiles/r04_blas_batch.txt. */
int nxhip_build_blas_batch(nxhip_ctx *ctx, const nx_triangle *const *tris, const uint32_t *triCounts, uint32_t meshCount, int32_t *blasIds);
/* nxhip_read_blas for `count` consecutive BLAS ids: nodes and primitive indices concatenated in id order (either may be NULL),
 * nodeCounts[k] = nodes of BLAS firstBlasId + k.  One transfer each when the range comes from one nxhip_build_blas_batch call. */
int nxhip_read_blas_batch(nxhip_ctx *ctx, int32_t firstBlasId, uint32_t count, nx_bvh8_node *nodes, uint32_t nodeCapacity, uint32_t *nodeCounts,
                          uint32_t *primIdx, uint32_t primCapacity);
/* Which binary tree the device builders (nxhip_build_blas, nxhip_rebuild_tlas) collapse into 8-wide nodes.
 * NXHIP_BUILDER_SAH (default): the top-down binned SAH build described above.  0: the binary radix tree of the 63-bit
 * Morton codes (LBVH: sort + one launch; 15 ms per million triangles).  clusteringRadius > 0: parallel locally-ordered
 * clustering — the Morton-sorted primitives are merged bottom-up, every cluster pairing with the neighbour within `radius`
 * places whose union has the smallest surface area; a few dozen rounds.  All three go through the same SAH collapse.
 * Measured (profiles/r03_builder_quality.txt, node visits per ray against the host SAH build): top-down SAH -1 ... -14 %,
 * radix tree +1 ... +25 %, clustering +2 ... +15 %.  Either way the result is a valid conservative CWBVH. */
#define NXHIP_BUILDER_SAH (-1)
int nxhip_set_device_builder(nxhip_ctx *ctx, int clusteringRadius);
/* Read a BLAS's nodes / primitive index list back (either may be NULL; *nodeCount = nodes it has). */
int nxhip_read_blas(nxhip_ctx *ctx, int32_t blasId, nx_bvh8_node *nodes, uint32_t nodeCapacity, uint32_t *primIdx, uint32_t primCapacity,
                    uint32_t *nodeCount);
int nxhip_clear_blas(nxhip_ctx *ctx);
/* TLAS::UpdateDeviceData — Geometry/BVH/TLAS.cpp:93-100 (symbols `tlas`, `blas`).  The 32 stack entries of nxhip_upload_blas's note are
 * shared with the TLAS: the entries a ray holds when it enters an instance stay below those of the BLAS. */
int nxhip_set_tlas(nxhip_ctx *ctx, const nx_bvh8_node *nodes, uint32_t nodeCount, const uint32_t *instanceIdx,
                   const nx_bvh_instance *instances, uint32_t instanceCount);
/* TLAS built ON THE DEVICE from the instances alone ("refit / rebuild on device"): the builder
 * of nxhip_build_blas (whichever nxhip_set_device_builder selected; default: top-down binned SAH) run over the instances'
 * world-space boxes, collapsed into 80-byte nodes with up to three instances per leaf slot, then
 * installed exactly as nxhip_set_tlas installs a host-built tree (instances[i].boundsMin / boundsMax must be filled in, as
 * BVHInstance::SetTransform does).  Replaces TLAS::Build + TLAS::Convert — the reference's O(n^2) agglomerative clustering
 * on the CPU and BVH8 conversion, re-run on every edit (Geometry/BVH/TLAS.cpp:13-91, Scene/Scene.cpp:29-55) — when instances are
 * added or removed: 16 000 instances take the host clustering 0.8 s and this build about a millisecond.  A different tree
 * than the host's (hits identical up to equidistant ties).  Afterwards nxhip_set_instance_transforms refits it in place. */
int nxhip_rebuild_tlas(nxhip_ctx *ctx, const nx_bvh_instance *instances, uint32_t instanceCount);
/* The installed TLAS's instance index list (leaf order; instanceCount entries; NULL: only the node count). */
int nxhip_read_tlas_index(nxhip_ctx *ctx, uint32_t *instanceIdx, uint32_t capacity, uint32_t *nodeCount);
/* Dynamic transforms without a host round trip of the scene.  Replaces, for instances that
 * already exist, MeshInstance::SetTransform -> BVHInstance::SetTransform -> TLAS::Build -> TLAS::UpdateDeviceData
 * (Geometry/BVH/BVHInstance.cpp:4-29, Scene/Scene.cpp:29-55, Geometry/BVH/TLAS.cpp:13-100: an O(n^2) agglomerative rebuild
 * on the CPU per edit).  transforms16: count row-major object-to-world matrices.  On the device: inverse matrix and world
 * bounds of every listed instance (bit-identical to nexus::BVHInstance::SetTransform), its traversal record, then a
 * bottom-up refit of the TLAS BVH8 with unchanged topology (bit-identical to nexus::collapse::Refit / nxh_tlas_refit).
 * Runs on the context's stream after the frames already issued. */
int nxhip_set_instance_transforms(nxhip_ctx *ctx, const uint32_t *instanceIds, const float *transforms16, uint32_t count);
/* Deforming meshes: new vertices for an existing BLAS, refitted on the device.  The reference has
 * nothing of the kind — a changed mesh there is a new BVH8Builder run (Assets/AssetManager.cpp:23-37), as nxhip_build_blas is
 * here, with a new id, new instances and a new TLAS.  triCount must equal the BLAS's; triangle i replaces triangle i (the index
 * hit records report).  Topology, node count, ids and every device pointer stay, so pass graphs and entry-state tables need no
 * rebuild.  Works on any BLAS id: uploaded, device-built or one of a batch.  On the context's stream, with no read-back of the tree
 * and no allocation after the first update of that BLAS: the triangles are copied, the intersection stream is rewritten, and the
 * nodes are refitted bottom-up level by level (bit-identical to nexus::collapse::Refit over the triangles' vertex boxes,
 * nxh_bvh8_refit).  Ordered behind every pass already issued on any pass slot and before every later one; frame number and
 * accumulation are left alone.  What embeds the BLAS's root — its instances' world bounds, their traversal records, the TLAS — is
 * brought up to date once, for all BLASes updated since, by the next render, ray-batch hook or nxhip_read_tlas.
 * The _device form takes the 96-byte records from device memory (a caller's own skinning kernel), copied device to device in
 * stream order; it does not wait for the device.  A bad id, NULL or another count: NXHIP_ERR_INVALID, nothing changed. */
int nxhip_update_blas(nxhip_ctx *ctx, int32_t blasId, const nx_triangle *tris, uint32_t triCount);
int nxhip_update_blas_device(nxhip_ctx *ctx, int32_t blasId, const void *trisDevice, uint32_t triCount);
/* Extension — skinned meshes: the step in front of the refit above.  A BLAS is given a skin once (four joints and weights per triangle
 * corner, glTF's JOINTS_0 / WEIGHTS_0 de-indexed like the positions); after that a pose is `jointCount` matrices, and ONE kernel turns
 * the bind-pose triangles and the joint palette into the BLAS's 96-byte triangles, its shading copy and its intersection stream (the
 * stream bit-identical to what nxhip_update_blas makes of those triangles); the level-by-level node refit of nxhip_update_blas runs
 * behind it.  The reference has nothing of the kind (its loader drops skins: Assets/OBJLoader.cpp).
 *
 * nxhip_set_blas_skin: cornerCount must be 3 x the BLAS's triangle count; corner 3 i + v belongs to vertex v of triangle i.  The call
 * copies the BLAS's CURRENT triangles device to device into a bind copy and stores the corners; every later pose starts from that bind
 * copy — poses never accumulate.  Weights are re-normalised on the host in binary64 to sum 1 and rounded once; a joint whose weight is 0
 * is rewritten to index 0.  Refused with NXHIP_ERR_INVALID before anything is allocated, the previous state left in place: a bad id,
 * another count, jointCount 0 or above 65536, a joint index >= jointCount on a corner whose weight for it is not 0, a weight that is
 * negative or not finite, a corner whose weights sum to 0.  corners == NULL removes the skin and frees both buffers: the BLAS is then
 * exactly what it was (triangles and nodes stay as last posed; nothing a pass is built from changes).  Works on any BLAS id: uploaded,
 * device-built or one of a batch.  nxhip_update_blas(_device) on a skinned BLAS still works and does not touch the bind copy.
 *
 * nxhip_pose_blas: jointMatrices = jointCount x 12 floats, the row-major 3 x 4 object-space matrices (rotation-scale | translation) —
 * for glTF, inverse(meshNodeWorld) x jointWorld[j] x inverseBind[j].  Copied to the BLAS's device palette in stream order, then the pose
 * kernel and the refit; ordering and side effects are exactly nxhip_update_blas's (behind every pass already issued on any slot, before
 * every later one; instances, traversal records and the TLAS follow at the next render, ray-batch hook or nxhip_read_tlas), and the call
 * waits for the device only as nxhip_update_blas's host form does, for the pageable array.  A BLAS without a skin, another joint count,
 * NULL or a matrix entry that is not finite: NXHIP_ERR_INVALID, nothing changed.
 *
 * THE BLENDING RULE, all of it in binary32; per corner, with its joints j_k and weights w_k, k = 0..3:
 *   M  = sum_k w_k J[j_k]                     a 3 x 4 matrix
 *   p' = M (p, 1)
 *   N  = cof(M3), the cofactor matrix of M's upper 3 x 3 (= det(M3) M3^-T: correct under non-uniform scale)
 *   n' = N n, negated when det(M3) < 0 (a mirroring pose), then normalised
 * A bind normal of exactly (0, 0, 0) stays (0, 0, 0) (the loaders write one for meshes without NORMAL); a result whose length is 0 or
 * not finite becomes (0, 0, 0) too.  Texture coordinates are copied.  Evaluation order and fma contraction are the compiler's: the tests
 * bound the result (positions: gamma_8 x sum_k w_k sum_c |J_k[r][c]| |(p, 1)_c|), not its bits.  The palette is read from the LDS up to
 * 1024 joints (48 KiB) and from global memory above.
 * Not covered: more than four influences (JOINTS_1) — the loaders warn and ignore them —; CUBICSPLINE samplers — the
 * loaders warn, read the value component of each key and interpolate it linearly —; dual-quaternion blending; motion blur (one pose holds
 * for a frame; nothing in traversal or shading changes); a restatement in the CPU oracle (the tests compare with float64 arithmetic and
 * with nxhip_update_blas of the read-back triangles). */
int nxhip_set_blas_skin(nxhip_ctx *ctx, int32_t blasId, const nx_skin_corner *corners, uint32_t cornerCount, uint32_t jointCount);
int nxhip_pose_blas(nxhip_ctx *ctx, int32_t blasId, const float *jointMatrices, uint32_t jointCount);
/* Extension — morph targets (glTF blend shapes): the stage in front of the joint blend, in the same single pass.  A BLAS is given its
 * targets once — per target and triangle corner a position and a normal delta, glTF's target POSITION / NORMAL de-indexed like the
 * positions —; after that a pose is `targetCount` weights, plus the joint palette where the BLAS is skinned.  The deltas live in device
 * memory (80 bytes per target and triangle); a pose costs what its ACTIVE targets cost — those whose weight is not 0 —, not what the BLAS
 * has.  The reference has nothing of the kind.
 *
 * nxhip_set_blas_morph: `deltas` is target-major: record t x cornerCount + 3 i + v belongs to vertex v of triangle i under target t (the
 * corner numbering of nxhip_set_blas_skin).  Refused with NXHIP_ERR_INVALID before anything is allocated, the previous state left in
 * place: a bad id, a cornerCount that is not 3 x the BLAS's triangle count, targetCount 0 or above 1024, a delta component that is not
 * finite.  deltas == NULL removes the morph (the device is waited for first, as for the skin); triangles and nodes stay as last posed.
 * Works on any BLAS id: uploaded, device-built or one of a batch.
 *
 * THE BIND COPY is one, shared by the skin and the morph of a BLAS:
 *   - whichever of nxhip_set_blas_skin and nxhip_set_blas_morph finds the BLAS with NEITHER takes the copy from the BLAS's current triangles;
 *   - the one that finds the OTHER already present keeps that copy: deltas and skin then describe the same shape, in either order of setting;
 *   - a skin set again on a BLAS that has only a skin re-takes the copy, and so does a morph set again on a BLAS that has only a morph;
 *   - removing one of the two leaves the copy to the other; removing the last frees it;
 *   - nxhip_update_blas(_device) never touches it.
 *
 * nxhip_pose_blas_morph: the BLAS must have a morph and targetCount must equal its own; weights must be finite — negative weights and
 * weights above 1 are allowed, as glTF allows them.  On a skinned BLAS jointMatrices / jointCount are required and validated as by
 * nxhip_pose_blas; on an unskinned BLAS they must be NULL and 0.  Anything else: NXHIP_ERR_INVALID, nothing changed.  The host compacts
 * the weights into the list of active targets — (index, weight) pairs, ascending index — and uploads it in stream order; the kernel loops
 * over that list only.  Ordering, side effects and the final wait are exactly nxhip_pose_blas's.  Weights do not persist and poses do not
 * accumulate: every pose starts from the bind copy, and nxhip_pose_blas on a BLAS that also has a morph does what it always did — it is
 * the pose with all weights 0.
 *
 * THE RULE, all of it in binary32; per corner, A = the active targets in ascending order:
 *   p' = p + sum_{t in A} w_t dPosition_t          n' = n + sum_{t in A} w_t dNormal_t, then normalised
 * summed left to right starting from the bind value.  A bind normal of exactly (0, 0, 0) stays (0, 0, 0) and its deltas are not applied;
 * an n' whose length is 0 or not finite becomes (0, 0, 0).  On a skinned BLAS the rule of nxhip_pose_blas is then applied to (p', n'),
 * unchanged: glTF's order, morph first, then skin.  Texture coordinates are copied.  With NO active target the stage is absent, not a sum
 * of zeros: an unskinned BLAS gets its bind copy back bit for bit (normals not renormalised), a skinned one nxhip_pose_blas's triangles.
 * Contraction is the compiler's, so the tests bound the result, not its bits:
 *   positions  |err_c| <= gamma_{A+1} (|p_c| + sum_t |w_t| |dP_t,c|)        (A products and A additions; gamma_k = k u / (1 - k u), u = 2^-24)
 *   normals    with v the exact unnormalised sum and t_c = |n_c| + sum_t |w_t| |dN_t,c|: the computed sum is v + e, |e_c| <= gamma_{A+1} t_c;
 *              normalising v + e instead of v moves the unit vector by at most 2 ||e|| / ||v||, and the squares, their sum, the root and
 *              the division stay within 4 u per component:  ||n' - v / ||v|| ||_inf <= 2 gamma_{A+1} ||t|| / ||v|| + 4 u
 *              (as nxhip_pose_blas's normal bound is derived, with the sum's gamma in place of the cofactor product's).
 *   skinned    the bound of nxhip_pose_blas evaluated at |p'|, plus the position bound above carried through sum_c |M[r][c]|.
 * Not covered: TANGENT deltas (the 96-byte triangle has no tangents), more than 1024 targets per BLAS, motion blur, and a restatement in
 * the CPU oracle (the tests compare with float64 arithmetic and with nxhip_update_blas of the read-back triangles). */
int nxhip_set_blas_morph(nxhip_ctx *ctx, int32_t blasId, const nx_morph_corner *deltas, uint32_t cornerCount, uint32_t targetCount);
int nxhip_pose_blas_morph(nxhip_ctx *ctx, int32_t blasId, const float *weights, uint32_t targetCount, const float *jointMatrices, uint32_t jointCount);
/* The BLAS's current 96-byte triangles (as uploaded, last updated or last posed); capacity >= its triangle count. */
int nxhip_read_blas_triangles(nxhip_ctx *ctx, int32_t blasId, nx_triangle *out, uint32_t capacity);
/* The box the BLAS's root node encodes after the last build, refit or pose: its quantisation frame [p, p + 255 x 2^(e - 127)], decoded as
 * BVHInstance::SetTransform decodes it.  One 80-byte read behind the context's stream. */
int nxhip_read_blas_bounds(nxhip_ctx *ctx, int32_t blasId, float lo[3], float hi[3]);
/* Read the device's TLAS nodes / instance table back (tests; either destination may be NULL). */
int nxhip_read_tlas(nxhip_ctx *ctx, nx_bvh8_node *nodes, uint32_t nodeCapacity, nx_bvh_instance *instances, uint32_t instanceCapacity);
/* AssetManager device materials — Assets/AssetManager.cpp:57-62,106-116
 *
 * Extension — NX_MAT_METALROUGH (type 4): glTF's metallic-roughness material as ONE BSDF.  The wavefront sorts hits by material type
 * before any texture lookup, so per-texel metalness needs a single type whose BSDF blends inside.  View `metalrough` of the union:
 * albedo[3], roughness, ior (plastic's fields) and metallic at byte 20.
 *
 * THE SHADING RULE.  Inputs at the hit, in this order:
 *   c   albedo, or the diffuse map's texel if the material names one (the existing rule, the stochastic alpha pass-through in front of it);
 *   r   roughness x the G channel of the detail table's roughnessMapId lookup (the existing rule: nxhip_set_material_detail);
 *   m   metallic x the B channel of THAT lookup (this type only: one lookup for both channels); then m = clamp(m, 0, 1), NaN -> 0;
 *   a   = clamp(r^2, 1e-3, 1) — glTF's mapping, not the reference's rough_alpha, which stays with the four reference types.
 * Local frame, z the shading normal: ci = |wi.z|, co = |wo.z|, h = normalize(wi + wo) (on wi's side), u = wi.h.
 *   f0d   = ((ior - 1) / (ior + 1))^2                     F0 = f0d + (c - f0d) m  (= lerp(f0d, c, m), per channel)
 *   F     = F0 + (1 - F0)(1 - u)^5                        Fd(x) = f0d + (1 - f0d)(1 - x)^5
 *   D     = a^2 / (pi (a^2 h.z^2 + h.x^2 + h.y^2)^2)      (this denominator, not h.z^2 (a^2 - 1) + 1, which cancels in binary32 near the clamp)
 *   L(x)  = sqrt(a^2 + (1 - a^2) x^2)                     G1(x) = 2x / (x + L(x))
 *   G2    = 2 ci co / (co L(ci) + ci L(co))               (height-correlated: the form glTF's Appendix B names)
 *   f cos = [ F D G2 / (4 ci co) + (1 - m) c / pi (1 - Fd(ci)) (1 - Fd(co)) ] co            — what eval returns as the throughput
 * The diffuse weight is the PRODUCT (1 - Fd(ci))(1 - Fd(co)), a departure from the appendix's 1 - Fd(u): the appendix (non-normative)
 * reflects up to 1.39 of the incoming energy at grazing incidence (binary64 quadrature, white base colour), the product stays <= 1.000
 * over r in {0.05 .. 1}, m in {0, 0.5, 1}, ci in [0.05, 0.95], and is reciprocal.
 *   lobe  ws = mean(F0 + (1 - F0)(1 - ci)^5),  wd = mean((1 - m) c) (1 - Fd(ci)),  ps = ws / (ws + wd);  ws + wd == 0: invalid sample
 *   pdf   = ps G1(ci) D / (4 ci) + (1 - ps) co / pi
 * Validity: wi.z wo.z > 0, then the project's pdf_valid(pdf) (finite and > 1e-4).
 * sample draws exactly THREE numbers on both branches: u0 — the specular lobe when u0 < ps — then (u1, u2):
 *   specular  visible normals of GGX (Heitz 2018), V = wi on the upper side:  Vh = normalize(a V.x, a V.y, V.z);
 *             T1 = (-Vh.y, Vh.x, 0) / |.| ((1, 0, 0) when Vh.x^2 + Vh.y^2 == 0), T2 = Vh x T1;  rr = sqrt(u1), phi = 2 pi u2,
 *             t1 = rr cos phi, t2 = rr sin phi;  s = (1 + Vh.z) / 2,  t2 := (1 - s) sqrt(1 - t1^2) + s t2;
 *             Nh = t1 T1 + t2 T2 + sqrt(max(0, 1 - t1^2 - t2^2)) Vh;  h = normalize(a Nh.x, a Nh.y, max(0, Nh.z)), on wi's side;
 *             wo = reflect(-wi, h), rejected when wo.z wi.z <= 0;
 *   diffuse   the existing cosine_hemisphere (u1, u2), on wi's side.
 * It returns the mixture estimator: pdf is the full mixture pdf above and the throughput is f cos / pdf with the full f, so
 * sample.throughput x sample.pdf == eval.throughput at the sampled direction (the weight stays below about 1.7).  Unlike the
 * reference's plastic, eval and sample are the same model.
 * The back-face flip applies as for every type but the DIELECTRIC; light sampling, MIS, transparent shadows, analytic lights, the power
 * light table, fog and normal maps work through eval / sample as for the other types; the AOV albedo of the type is c.
 * Out of scope: multiple-scattering energy compensation (a white metal at r = 1 reflects 0.33 at ci = 0.9); clearcoat, sheen and specular
 * extensions; transmission inside this type; a CPU-oracle restatement.
 * Both pipelines shade the type.  SCAN: one more case of the material launch.  CLASSIC (NX_COMPACT_ORDERED): the reference's logic kernel
 * and its four queues stay as they are; a kernel behind it queues the surviving hits of the type into a fifth queue (the same roulette
 * number, so the same decision), and the type's material kernel runs after the reference's four.  Under pixel-keyed numbers both give
 * the same frames bit for bit.  A SCAN pass with the type hands no closest-hit ray to the thin kernel (its replay names the reference
 * types' codes only); its any-hit rays are handed over as ever.
 * The kernels that know the type are compile-time instances launched only while some material has it (bit 15 of
 * nxhip_debug_pass_flavor's word); they are DETAIL instances too and imply the general material launch.  A context without such a
 * material launches what it always did and has the same flavor word. */
int nxhip_set_materials(nxhip_ctx *ctx, const nx_material *materials, uint32_t count);
/* Scene::m_DeviceLights — Scene/Scene.cpp:142-176.  Only NX_LIGHT_MESH entries are sampled: an NX_LIGHT_POINT or NX_LIGHT_AREA entry yields
 * no light sample (the 12-byte record has no position).  Lights that are not geometry go through nxhip_set_analytic_lights below. */
int nxhip_set_lights(nxhip_ctx *ctx, const nx_light *lights, uint32_t count);
/* Extension — analytic lights: point, sphere, spot, and sun (delta or disc), nx_analytic_light of nexus_pod.h, world space.  Radiometric RGB
 * throughout (no 683 lm/W); glTF `range` is ignored.  The call replaces the table; count 0 removes it, and the context is then exactly
 * what it was before the first call (the default kernel instances, the same frames bit for bit).  nxhip_set_lights is untouched by it.
 *
 * Validation, on the host before anything is allocated — NXHIP_ERR_INVALID and the previous table stays in place: lights NULL with
 * count > 0; any field not finite; radius, intensity, a colour component or angularRadius below 0; angularRadius >= pi/2; a direction of
 * length 0, whatever the kind (any other length is normalised on the host, in binary64); SPOT cone angles outside
 * 0 <= inner < outer <= pi/2; an unknown type; lightCount + count + 1 > 2^23 (the resolution of the random number that picks — while the
 * table is not empty nxhip_set_lights refuses a count that would pass the same bound).
 * The device table is derived on the host in binary64 and rounded once: the unit axis, colour x intensity, radius^2,
 * angleScale = 1 / max(1e-3, cos inner - cos outer), angleOffset = -cos outer x angleScale, q = 1 - cos(angularRadius) =
 * 2 sin^2(angularRadius / 2).
 *
 * THE SAMPLING RULE.  A = the number of analytic lights.  The light sample picks uniformly among
 *   nLights = lightCount + A + [environment sampled],
 * in the order mesh lights, analytic lights, environment — in NXHIP_LIGHTS_UNIFORM and in NXHIP_LIGHTS_POWER alike (there the table still
 * decides which mesh triangle; analytic lights are uniform among themselves).  For a pick of analytic light l at shading point x:
 *   origin     o = x offset along the geometric normal to the light's side (the side of the light's centre; of -direction for a
 *              DIRECTIONAL light), as the environment branch offsets its origin.
 *   axis       a = (P - o) / d, d = |P - o| (POINT, SPOT);  a = -direction, d := 1 (DIRECTIONAL).
 *   cone       s^2 = radius^2 / d^2; no sample when d <= radius.  q = 1 - cos thetaMax = s^2 / (1 + sqrt(1 - s^2)) (POINT, SPOT); q from
 *              the table (DIRECTIONAL).  Never 1 - sqrt(1 - s^2): in binary32 that is 7 % off at radius / d = 1e-3 and 32 % off at
 *              3e-4; the stated form is good to 1e-7.
 *   direction  cos theta = 1 - r1 q;  sin^2 theta = r1 q (2 - r1 q) (no 1 - cos^2);  phi = 2 pi r2 about a.  Two random numbers are
 *              drawn whatever the kind, so a path's stream does not depend on the kind.  direction = t0 cos phi sin theta +
 *              t1 sin phi sin theta + a cos theta in the branch-free frame of Duff et al. 2017: s = copysign(1, a.z), k = -1 / (s + a.z),
 *              b = a.x a.y k, t0 = (1 + s a.x^2 k, s b, -s a.x), t1 = (b, s + a.y^2 k, -a.y).
 *   shadow ray tmax = d cos theta - sqrt(max(0, radius^2 - d^2 sin^2 theta)), the near intersection with the sphere (POINT, SPOT);
 *              1e30 (DIRECTIONAL).
 *   radiance   throughput x fcos x colour x intensity x att x 2 / (d^2 (1 + cos thetaMax)) x nLights, fcos = the BSDF evaluation's
 *              throughput (Bsdf::eval, whose own validity rule stays in force as for mesh lights).  The factor is radiance / pdf of the
 *              uniform cone — L = I / (pi r^2) for the sphere, E / (pi sin^2 alpha) for the disc — and tends to I / d^2 and E as the
 *              radius goes to 0.
 *   att        SPOT only, else 1: clamp(cd x angleScale + angleOffset, 0, 1)^2, cd = the cosine between the spot's axis and the
 *              direction from the light's centre to o — KHR_lights_punctual's formula, taken at the centre, not per sampled point.
 *   weight     none.  Analytic lights are not geometry: camera and bounce rays do not see them, no BSDF-sampled ray can reach one, the
 *              MIS weight is 1.  No validity test on the cone's density either (it is never below 1 / 4 pi).
 * useMIS == 0: without analytic lights no light sample is taken at all; with A > 0 one is taken among the analytic lights alone
 * (nLights := A), because nothing else can find them.  The MIS weight of an emissive hit and of a weighted miss uses the same nLights,
 * A included.
 * The kernels that know these lights are compile-time instances launched only while A > 0 (bit 10 of nxhip_debug_pass_flavor's word). */
int nxhip_set_analytic_lights(nxhip_ctx *ctx, const nx_analytic_light *lights, uint32_t count);
/* Texture::ToDevice — Assets/Texture.cpp:10-39 (RGBA8, sRGB, wrap, bilinear).  kind: 0 diffuse, 1 emissive, 2 hdr map, and — an
 * extension, see nxhip_set_material_detail — 3 normal map, 4 roughness map (RGBA8 holding LINEAR data: no sRGB decode).
 * Diffuse, emissive, normal and roughness maps get ids in upload order, counted per kind; the hdr map replaces the previous one.
 * nxhip_clear_textures removes the maps of every kind. */
int nxhip_upload_texture(nxhip_ctx *ctx, int kind, const uint8_t *rgba8, uint32_t width, uint32_t height, int32_t *texId);
int nxhip_clear_textures(nxhip_ctx *ctx);
/* Extension — detail maps: a tangent-space normal map and a roughness map per material (glTF normalTexture and the G channel of
 * pbrMetallicRoughness.metallicRoughnessTexture).  `details` is index-parallel to the material table (nx_material_detail of nexus_pod.h:
 * normalMapId, roughnessMapId — ids of nxhip_upload_texture kind 3 / 4, -1 = none — and normalScale); the call replaces the table; count 0
 * removes it, and the context is then exactly what it was before the first call (the same flavor word, the same frames bit for bit).  So
 * is a context whose table names no map at all.
 *
 * Validation — NXHIP_ERR_INVALID and the previous table stays in place: details NULL with count > 0; an id below -1; a normalScale that is
 * not finite.  A render (and every hook that reads the shading records) refuses, next to the checks of the diffuse and emissive ids: a
 * table whose count differs from the material count; an id with no uploaded texture.
 *
 * THE SHADING RULE.
 *   lookup     tex2d_linear: the addressing (normalised coordinates, wrap, texel centres at +0.5) and the 1/256 bilinear weights of the
 *              diffuse maps' lookup; every channel is byte / 255.0f, there is no sRGB table.  Texture coordinate set 0, at the hit.
 *   roughness  only if the material names a roughness map: roughness := roughness x g, g = the lookup's G channel (glTF's assignment),
 *              before the BSDF sees it.  No effect on NX_MAT_DIFFUSE.
 *   normal     only if the material names a normal map, and only where a path is continued (bounce != pathLength): there ns takes the
 *              place of the interpolated normal in the shading frame, in the light sample and in the signs of the ray offsets (the
 *              offsets themselves stay along the geometric normal).  The MIS weight of an emissive hit keeps the interpolated normal,
 *              and so does the light sample OF an emitter.
 *              N = the interpolated world normal before the back-face flip; c = the lookup; s = normalScale;
 *                m = ((2 c.r - 1) s, (2 c.g - 1) s, 2 c.b - 1).
 *              Object space, per triangle: e1 = p1 - p0, e2 = p2 - p0, (du1, dv1) = uv1 - uv0, (du2, dv2) = uv2 - uv0,
 *                det = du1 dv2 - du2 dv1,  Tu = (e1 dv2 - e2 dv1) sgn(det),  Tv = (e2 du1 - e1 du2) sgn(det).
 *              World space: Tu_w, Tv_w = the instance's forward 3 x 3 applied to Tu, Tv as vectors.
 *              Frame: t = normalize(Tu_w - N (N . Tu_w));  b = +-cross(N, t) with the sign that makes b . (-Tv_w) >= 0 — glTF's v runs down
 *              the image and green points up; mirrored UVs and mirroring transforms need no case of their own.
 *              ns = normalize(t m.x + b m.y + N m.z); then the existing flip (dot(gNormal, rayDirection) > 0 and the material is not a
 *              DIELECTRIC) negates ns as it negates N and gNormal.
 *   fallback   ns := N when: !(|det| > 0); the projected tangent is not finite or has length 0; ns is not finite or has length 0; or, with
 *              v = -rayDirection, (ns . v)(N . v) <= 0 — the view is below the mapped horizon.  One rule for all four material types.
 * Tangents are per triangle, from positions and UVs: the 96-byte triangle has no room for glTF's TANGENT attribute.
 * Out of scope: vertex TANGENT attributes; per-texel metalness for the four reference types (the material type picks the queue before any
 * lookup; NX_MAT_METALROUGH reads metallic and the B channel: nxhip_set_materials); the AOV normal and the denoiser's normal term keep the interpolated normal; .mtl bump maps; mip-mapping;
 * texCoord sets other than 0 and KHR_texture_transform (the loaders warn).  The closest-hit and any-hit kernels and the feature buffers do
 * not change.
 * The kernels that know these maps are compile-time instances launched only while some material names one (bit 12 of
 * nxhip_debug_pass_flavor's word); they imply the general material launch. */
int nxhip_set_material_detail(nxhip_ctx *ctx, const nx_material_detail *details, uint32_t count);
/* Extension: a FLOAT environment map — linear radiance, nothing clamped to 1 (the RGBA8 map above runs through the sRGB table: no
 * texel brighter than 1, a sun 10^5 times the sky arrives as a dot 50 times the sky).  rgb = width x height x 3 floats, row 0 the
 * top row (d.y = +1); orientation and the (u, v) of a direction are the RGBA8 map's.  The array is copied before the call returns.
 * It replaces the environment map of either kind; nxhip_upload_texture(kind 2) replaces a float one, nxhip_clear_textures removes it.
 *   lookup:  bilinear, wrap on both axes, texel centres at +0.5: xb = u width - 1/2, x0 = floor(xb), a = xb - x0 (likewise in v),
 *            value = lerp(lerp(t00, t10, a), lerp(t01, t11, a), b) in binary32 with the EXACT fractional weights — not the 1/256
 *            steps of the RGBA8 lookup, which imitate a texture unit that only ever filtered 8-bit texels: next to a texel of 6e4,
 *            1/512 of a weight is not a rounding error.
 *   sampler: under nxhip_set_env_sampling the texel weight is the integral of the FILTERED luminance over the texel's footprint,
 *              Lf(x, y) = sum over dy, dx in {-1, 0, 1} of k[dy] k[dx] lum(x + dx, y + dy),  k = (1/8, 3/4, 1/8)  (sums to 1 exactly),
 *              weight(x, y) = Lf(x, y) x sin(pi (y + 1/2) / height) + 1e-6,  lum = 0.2126 R + 0.7152 G + 0.0722 B (linear),
 *            neighbours wrapping on both axes as the lookup's do; the floor is absolute, as for the RGBA8 maps.  The RGBA8 rule — the
 *            texel's own luminance — is wrong here: the bilinear lookup bleeds a bright texel half a texel into its neighbours, whose
 *            pdf would know nothing of it, so value / pdf is bounded by sun / sky (10^6) instead of about 255 and the estimator has a
 *            tail no frame count meets (a 32 x 16 map with a one-texel sun of 6e4: 400 000 draws 43 % low).  The RGBA8 map keeps
 *            its own rule bit for bit.
 *   tables:  built on the device (binary64 weights and scans, cdfs and density rounded once to binary32, each cdf ending in exactly
 *            1), with no read-back and no host copy of the texels: by this call when the sampler is on (a new map under an enabled
 *            sampler gets new tables), by nxhip_set_env_sampling(1) on a float map otherwise.
 * NXHIP_ERR_INVALID, the previous map and tables left in place: rgb NULL or a zero size; width or height above 32768 or more than
 * 2^27 texels; any component negative or not finite (checked on the host before anything is allocated). */
int nxhip_upload_env_float(nxhip_ctx *ctx, const float *rgb, uint32_t width, uint32_t height);
/* Extension: sun and sky — a float environment map GENERATED on the device from a physically based single-scattering atmosphere
 * (Nishita et al. 1993: Rayleigh and Mie terms only), for outdoor scenes without a .hdr file.  nx_sky: nexus_pod.h.
 * Geometry.  Up is +y.  The map's orientation is env_uv's: texel (x, y) has u = (x + 1/2) / W, v = (y + 1/2) / H, latitude
 *   phi = pi/2 - pi v, longitude theta = 2 pi u - pi, direction d = (cos phi cos theta, sin phi, cos phi sin theta).
 * Constants.  Planet radius Rg = 6 360 000 m, atmosphere top Rt = 6 420 000 m, the observer at (0, Rg + altitude, 0).
 *   Rayleigh: betaR = (5.802e-6, 13.558e-6, 33.1e-6) m^-1 x rayleighScale, scale height 8000 m, phase PR = 3/(16 pi) (1 + mu^2).
 *   Mie:      scattering betaM = 3.996e-6 m^-1 x mieScale (grey), extinction betaM / 0.9, scale height 1200 m, Cornette-Shanks phase
 *             PM = 3/(8 pi) (1 - g^2)(1 + mu^2) / ((2 + g^2)(1 + g^2 - 2 g mu)^1.5), g = mieG; mu = d . s, s the unit sun direction.
 *   rho(h) = exp(-h / scale height) with h the height above Rg.  Radiometric RGB throughout (no 683 lm/W, as for the analytic lights);
 *   sunIrradiance is the sun's irradiance at the top of the atmosphere.
 * View ray.  From the observer along d; tEnd = the first hit with the Rg sphere if the ray hits the planet, else the exit from the Rt
 *   sphere.  viewSteps = Nv segments with edges t_i = tEnd (i / Nv)^2 — quadratic, because the density is near the observer — and the
 *   midpoint rule: one sample in the middle of each segment (in t), the optical depths to it = the full earlier segments + half of its own.
 * Light ray.  From each sample towards the sun: if it hits the Rg sphere ahead of it the sample contributes nothing; otherwise
 *   lightSteps = Nl segments to the Rt exit, the same quadratic edges and midpoint rule, summed in full.
 * Radiance.  L = sunIrradiance x sum_i [betaR rhoR_i PR + betaM rhoM_i PM] ds_i
 *                x exp(-(betaR (tauR_view + tauR_light) + betaM_ext (tauM_view + tauM_light))), per channel.
 * Ground.  A view ray that ended on the planet adds T_view x groundAlbedo / pi x sunIrradiance x T_sun(ground point) x max(0, n . s):
 *   n the outward normal there, T_view the transmittance of the whole view ray, T_sun the light-ray rule from the ground point (Nl
 *   segments), 0 when the sun is below that point's horizon.
 * Quadrature.  The defaults Nv = 64, Nl = 16 are within 0.5 % of 1024 x 128 steps at altitude 1 m over the zenith, the horizon towards
 *   the sun and oblique views, for sun elevations from 60 degrees to -4 degrees (tests/test_sky.py measures it; uniform spacing with
 *   32 x 8 steps is 5 % off).
 * Sun disc (sunDisc = 1).  Lsun x c x k is added to the texels: Lsun = sunIrradiance x T_sun(observer) / (pi sin^2 alpha) — the
 *   analytic lights' disc rule, T_sun by the light-ray rule with Nl segments, 0 when the sun is below the observer's geometric horizon;
 *   c = the share of the texel's 8 x 8 regular sub-positions ((i + 1/2) / 8, (j + 1/2) / 8) of its (u, v) cell whose direction lies within
 *   alpha of s; k = 2 pi (1 - cos alpha) / sum(c Omega), one factor per map, computed on the host in binary64 over the disc's bounding
 *   rows and columns, Omega = (2 pi / W)(sin phi_top - sin phi_bottom) the texel's exact solid angle — so the disc carries its full
 *   energy at any resolution.  sum = 0 (the disc fell between sub-positions): NXHIP_ERR_INVALID — use a larger map or a larger
 *   sunAngularRadius.  No limb darkening.
 * Device.  The texels are computed one lane each, straight into the float4 buffer the passes read (binary32, heights in a
 *   cancellation-free form, hardware exponentials; the disc's coverage in binary64); no host copy of the texels, no read-back.  The map
 *   is installed exactly as nxhip_upload_env_float installs its own: it replaces a map of either kind, nxhip_upload_texture(kind 2) or
 *   nxhip_upload_env_float replaces it, nxhip_clear_textures removes it; lookup, sampler weight and tables are the float map's, built
 *   by this call when the sampler is on.  A context that never calls it is unchanged.
 * NXHIP_ERR_INVALID, the previous map and tables left in place, checked on the host before anything is allocated: sky NULL; any field
 *   not finite; a zero sunDirection; a negative irradiance, albedo or scale; an albedo above 1; |mieG| >= 1; altitude outside [1, 50000];
 *   sunAngularRadius outside [0, pi/2); sizes outside nxhip_upload_env_float's limits; steps outside [1, 1024]; sunDisc above 1;
 *   sunDisc = 1 with sunAngularRadius = 0.
 * Out of scope: multiple scattering; ozone; limb darkening; a moon or stars; aerial perspective on scene geometry (the fog volume is the
 *   medium, the sky is at infinity); photometric units.
 * nxhip_sky_defaults: sun at 45 degrees elevation along +x, angular radius 0.004675, irradiance (1, 1, 1), altitude 1, scales 1, g 0.8,
 *   albedo 0.3, map 2048 x 1024, steps 64 / 16, no disc.  NXHIP_ERR_INVALID for NULL.
 * nxhip_sky_sun_light: the sky's sun as an NX_ALIGHT_DIRECTIONAL record for the caller to append to its nxhip_set_analytic_lights
 *   table — direction = -sunDirection (unit), angularRadius = alpha, colour = sunIrradiance x T_sun(observer), intensity = 1; T_sun by the
 *   light-ray rule with a fixed 256 segments, the colour 0 when the sun is below the observer's geometric horizon.  Needs no context;
 *   host, binary64; validates as nxhip_set_sky does.  The baked disc and this record are ALTERNATIVES: both together make two suns.  As
 *   for every analytic light, camera rays and BSDF-sampled rays do not see the record: mirrors show the sun only with sunDisc = 1. */
int nxhip_sky_defaults(nx_sky *sky);
int nxhip_set_sky(nxhip_ctx *ctx, const nx_sky *sky);
int nxhip_sky_sun_light(const nx_sky *sky, nx_analytic_light *out);
/* Extension (BASELINE.json configs[3] asks for "HDR envmap NEE/MIS"; the reference only adds the environment when a ray
 * misses, PathTracer.cu:152-164, and its NEE knows mesh lights only, :227): with enable != 0 the next-event estimation
 * treats the environment map as one more light — picked with probability 1 / (lightCount + 1), direction drawn from the
 * map's luminance x sin(theta) distribution, shadow ray to infinity — and a BSDF-sampled ray that misses is weighted
 * against that sampler with the power heuristic.  Unbiased either way; the expectation of a frame is unchanged.  Needs an
 * uploaded environment map (kind 2, or nxhip_upload_env_float — whose texel weight is its own, see there); off by default. */
int nxhip_set_env_sampling(nxhip_ctx *ctx, int enable);
/* Extension: how the next-event estimation chooses its mesh-light sample.
 *   NXHIP_LIGHTS_UNIFORM (default)  the reference's rule, bit for bit: one light uniformly, then one of its triangles uniformly
 *                                   (PathTracer.cu:227-240) — a candle as often as a ceiling panel, the slivers of a tessellated
 *                                   emitter as often as its large triangles.
 *   NXHIP_LIGHTS_POWER              every emissive triangle of every mesh light in proportion to w = world-space area x Y, with
 *                                   Y = intensity x (0.2126 r + 0.7152 g + 0.0722 b) of the light's material; (r, g, b) is the emissive
 *                                   factor or, with an emissive map, the mean of the map's sRGB-decoded texels (alpha ignored).  A weight
 *                                   that is negative or not finite counts as 0.
 * The table (entries ordered by light — the order of nxhip_set_lights — then by triangle index; N = the mesh lights' triangles) is built
 * on the device with no read-back: binary64 prefix sums of w, cdf[i] = binary32(prefix[i] / total) with the last entry exactly 1, and a
 * guide table of G = the power of two >= N (at most 2^23) cut points, so that a pick costs one random number and an expected two loads:
 * k = floor(u G), i = guide[k], while (cdf[i] <= u) i++  —  by definition min(searchsorted(cdf, u, 'right'), N - 1).  P(i) = cdf[i] -
 * cdf[i - 1] is the probability both the sampler and the MIS weight of an emissive hit use, read from the table, never recomputed.
 * The light sample draws as many random numbers as in the default mode (the one u replaces the uniform triangle index); the uniform
 * pick among lightCount (+ 1 with nxhip_set_env_sampling) still decides between "a mesh light" and the environment.  An emissive hit
 * whose instance is no light, or whose entry has P = 0, gets the MIS weight 1: the sampler cannot reach it.  A total weight of 0: no
 * mesh-light samples at all.  Unbiased either way; the expectation of a frame does not change, so the mode may be switched at any
 * time, also between accumulated frames.
 * Granularity: u has 23 bits (rng_next), the limit the reference's uniform index has too; an entry whose share is below about 2^-25
 * can round to P = 0 and is then never sampled (and weighted 1 when hit).
 * The table is rebuilt, once, by the next render or hook call after anything it depends on has changed: nxhip_set_lights,
 * nxhip_set_materials, nxhip_set_tlas / nxhip_rebuild_tlas, an emissive texture upload or clear, nxhip_set_instance_transforms (a scale
 * changes areas), nxhip_update_blas(_device), the mode itself.  In the default mode nothing is allocated, built or launched.
 * With more than one pass in flight (nxhip_set_passes_in_flight) a rebuild waits for every pass issued and the next pass waits for the
 * rebuild — the passes read ONE table — so a light that deforms every frame serialises the passes in flight; one pass at a time the
 * rebuild is just ahead of the pass in stream order.
 * In POWER mode a light list that names one instance twice is refused by the render (NXHIP_ERR_INVALID).  Another mode: NXHIP_ERR_INVALID. */
enum { NXHIP_LIGHTS_UNIFORM = 0, NXHIP_LIGHTS_POWER = 1 };
int nxhip_set_light_sampling(nxhip_ctx *ctx, int mode);
/* Extension, a refinement of NXHIP_LIGHTS_POWER: what the probability of a table entry depends on.
 *   NXHIP_LIGHT_IMPORTANCE_POWER (default)  the table's P(i), the same at every shading point.
 *   NXHIP_LIGHT_IMPORTANCE_POSITION         ... and the shading point's position p: a bounding hierarchy over the table's entries (the
 *                                           light BVH of Conty & Kulla 2018 and of pbrt-v4), descended per light sample with a
 *                                           probability proportional to a bound on each subtree's contribution at p.  The emitters
 *                                           here are two-sided, so the method's orientation half is not needed: the importance
 *                                           depends on p alone, which serves surfaces and the medium's scatter points alike.
 * The setting is remembered in every light-sampling mode and has an effect only while the mode is NXHIP_LIGHTS_POWER: in
 * NXHIP_LIGHTS_UNIFORM nothing is allocated, built or launched and frames are what they were, bit for bit.  Unbiased either way; the
 * expectation of a frame does not change, so the setting may be switched at any time, also between accumulated frames.
 *
 * The tree.  Its entries are the light table's, in the table's order; N entries.  An entry's weight w is the table's formula — world-space
 * area x Y — evaluated in binary64 throughout: the binary32 corners, matrix, emissive factor (or the map's mean before its rounding) and
 * intensity as given, every operation in binary64, the same clamp (negative or not finite: 0).  The table's own w takes the binary32
 * area of the light sample's density; the tree does not need to agree with it to the last bit — sampler and MIS weight both read the
 * tree — and binary32 loses up to 1e-5 of the area of a small triangle far from the origin.  G =
 * nxhip_light_tree_leaves_for(N) is the power of two >= N (N above 2^23: the render refuses, NXHIP_ERR_INVALID).  The tree is implicit
 * and complete, a 1-based heap: node 1 is the root, the children of node k are 2k and 2k + 1, the leaves are nodes G .. 2G - 1; no child
 * pointers.  Leaf slot j < N holds entry order[j]; `order` lists the entries sorted by (m, entry index), m = the 30-bit Morton code
 * (x the most significant of each bit triple, then y, then z) of the triangle's world-space centroid ((a + b) + c) * (1 / 3) in
 * cells of extent / 1024 from the minimum of all centroids, `extent` the largest of the three extents of all centroids (ONE scale: a flat
 * arrangement stays flat in the code), each cell index clamped to 0 .. 1023.  The sort key is m << 23 | entry — no two alike — sorted by
 * rocPRIM's radix sort: two contexts with the same scene hold the same tree bit for bit.  Slots j >= N are empty: weight 0, box +inf / -inf.
 * A node is 32 bytes, { float lo[3]; float w; float hi[3]; uint32_t entry; }, so the two children of a node are one aligned 64-byte load.
 * A leaf's box is the min / max of its triangle's three corners transformed in binary64 (((m0 x + m1 y) + m2 z) + m3 per row), rounded to
 * binary32 once — the mat_point values the light sample itself computes differ from them by binary32's rounding of that sum, which the
 * importance, continuous in the box, does not tell apart —, an inner node's the min / max of its children's; the binary64 weight W of an inner node is left + right; the stored w is
 * binary32(W_node / W_root).  `entry` is the table entry in a leaf (0xffffffff in an empty slot) and 0 in an inner node.  slotOf[entry] is
 * the inverse of `order`.  A root weight that is 0 or not finite clears the table header's `valid` and sets every w to 0: no mesh-light
 * samples, the table's rule.  Built on the device with no read-back — min / max and the fixed shape make every value independent of the
 * order threads run in — by the event that rebuilds the table (above) and with its ordering against passes in flight; a change of this
 * setting is such an event.
 *
 * The importance I of a node at p.  Every operation is one binary32 rounding, in this order; no fused multiply-add:
 *   w == 0: I = 0, and the box is not looked at.  Otherwise
 *   c = (lo + hi) * 0.5f;  h = (hi - lo) * 0.5f;  r2 = (h.x*h.x + h.y*h.y) + h.z*h.z;
 *   d = p - c;  d2 = (d.x*d.x + d.y*d.y) + d.z*d.z;  I = w / max(max(d2, r2), FLT_MIN).
 * I is continuous in p, and positive for every node of positive weight unless d2 overflows.
 *
 * The pick uses ONE random number u, the one that replaces the uniform triangle index, so a path draws as many numbers as in both other
 * modes.  P = 1.0f, k = 1; while k < G:  a = I(2k), b = I(2k + 1); both 0: no light sample, and no further number is drawn;
 * s = a + b, qa = a / s, qb = b / s;  if b == 0 or (a != 0 and u < qa):  P *= qa, u = min(u / qa, 1 - 2^-24), k = 2k;  otherwise
 * P *= qb, u = max(min((u - qa) / qb, 1 - 2^-24), 0), k = 2k + 1.  The entry is leaf k's.  N = 1: G = 1, the root is the leaf, P = 1.
 * The probability of a given entry at p — the MIS weight of an emissive hit — walks the ancestors of slotOf[entry] root to leaf with the
 * same a, b, s and the same factor: the pick's P bit for bit.  P = 0: the sampler cannot reach the entry from p and the MIS weight is 1,
 * POWER mode's rule, which also covers an instance that is no light.
 * The density is POWER mode's with this P in place of the table's: (P * (lightCount / nLights)) / area * dSquared / cosThetaO.
 *
 * Where p comes from: the light sample passes the hit point (the medium: the scatter point); the emissive hit passes the previous
 * ray's origin, which the ray offset has moved off the surface by a few ulp of the position.  The two points differ by that offset, so the
 * two MIS weights of one light path sum to one only up to (offset / distance to the nearest box) — I is continuous.  The path state
 * carries no field to remove this.
 *
 * First-version restrictions: while the setting is in effect nxhip_set_tail_bounce is ignored (the tail kernel has no such instance);
 * under the classic pipeline (NX_COMPACT_ORDERED) the setting is ignored and frames are POWER mode's bit for bit; there is no map-free
 * instance.  Another value: NXHIP_ERR_INVALID. */
enum { NXHIP_LIGHT_IMPORTANCE_POWER = 0, NXHIP_LIGHT_IMPORTANCE_POSITION = 1 };
int nxhip_set_light_importance(nxhip_ctx *ctx, int importance);
/* G of a light tree over `entries` entries: the power of two >= entries; 0 for 0 entries or for more than 2^23.  Pure host code. */
uint32_t nxhip_light_tree_leaves_for(uint32_t entries);
/* Extension: transparent shadows.  A material's `opacity` and the alpha of its diffuse map let a PATH pass a surface with probability
 * 1 - opacity x alpha(uv) (the material kernels, the reference's rule); the reference's shadow rays end at the first triangle whatever its
 * material, so a delta light behind a see-through surface contributes 0 and, with useMIS, the light-sample share of every emitter
 * behind one is lost (the image converges to the BSDF-sampled share alone: "MIS == naive" fails for such scenes).
 *   NXHIP_SHADOWS_OPAQUE (default)  the reference's rule, bit for bit.
 *   NXHIP_SHADOWS_TRANSMIT          a shadow ray carries a transmittance T, binary32, 1.0f at the start.  Every triangle the any-hit
 *                                   traversal accepts (its test of today: 0 < t < tmax, u, v inside) is a crossing and multiplies
 *                                   T by 1.0f - s, in the traversal's own visiting order, with s = o * a:
 *                                     o = the instance material's opacity clamped to [0, 1]; `!(opacity < 1)` is opaque, a NaN included
 *                                         (rng_next > NaN never passes in the material kernel);
 *                                     a = 1 without a diffuse map, else the .w of the bilinear lookup of diffuseMaps[diffuseMapId] at the
 *                                         texture coordinates of the ORIGINAL triangle interpolated with the u, v of this very test —
 *                                         the arithmetic of the material kernel, so the alpha it would fetch at that hit.
 *                                   T == 0.0f ends the ray (occluded); there is no other threshold.  At retirement T x the request's
 *                                   radiance is added to the path: exactly the default's addition when nothing was crossed (T is 1.0f),
 *                                   exactly nothing when only opaque surfaces were.
 * In expectation this is the stochastic pass-through of the material kernels (pass probability 1 - o a, up to the 2^-23 granularity of
 * rng_next).  Deterministic: no random number is drawn, no random stream moves.  Limits: dielectrics block shadow rays as before (only
 * opacity and alpha count); a pass-through on the path side spends a bounce, a crossing of a shadow ray does not, so at the pathLength
 * cut-off the two strategies see one segment more or less; glTF alphaMode MASK / alphaCutoff: nxhip_set_material_alpha, below.
 * The mode changes a pass only while some material of the table is see-through (opacity < 1, or a diffuse map with a texel of alpha <
 * 255): otherwise the default kernels run.  While it does, the any-hit launches do not hand rays to the thin kernel and the tail kernel
 * is off (nxhip_set_tail_bounce is ignored): restrictions of a first version.  Results do not depend on nxhip_enable_trace_stats.
 * May be switched at any time, also between accumulated frames.  Another mode: NXHIP_ERR_INVALID. */
enum { NXHIP_SHADOWS_OPAQUE = 0, NXHIP_SHADOWS_TRANSMIT = 1 };
int nxhip_set_shadow_transmittance(nxhip_ctx *ctx, int mode);
/* Extension: alpha-tested geometry (glTF alphaMode MASK).  Without a table every material is read as a stochastic blend (above): the
 * traversal accepts every carrier triangle, and the material step decides.  `alphas` runs index-parallel to the material table
 * (nx_material_alpha of nexus_pod.h: mode, cutoff), like nx_material_detail; count 0 / NULL clears it.  Entries default to NX_ALPHA_BLEND,
 * which is the behaviour without a table, bit for bit: an all-BLEND table and a cleared one launch the default kernels.
 *   NX_ALPHA_MASK   every traversal test — closest hit and any hit — that accepts a triangle of an instance with such a material (the test
 *                   of today: 0 < t < tmax, u, v inside) computes s = o x a, the o and a of NXHIP_SHADOWS_TRANSMIT exactly:
 *                     o = the material's opacity clamped to [0, 1]; `!(opacity < 1)` counts as 1, a NaN included;
 *                     a = 1 without a diffuse map, else the .w of the bilinear lookup of diffuseMaps[diffuseMapId] at the texture
 *                         coordinates of the ORIGINAL triangle interpolated with the u, v of this very test.
 *                   s < cutoff: the triangle is rejected as if the ray had missed it — the closest-hit search goes on with its hit
 *                   distance unchanged, an any-hit ray is not occluded.  s >= cutoff: the triangle is accepted as solid.  Under
 *                   NXHIP_SHADOWS_TRANSMIT a surviving crossing of a MASK material ends the shadow ray (T = 0), a rejected one leaves T
 *                   untouched.  The first-hit feature buffers (nxhip_set_aov) and the pixel query (nxhip_get_selected_instance) follow
 *                   the closest hit, so they see through the holes; a hole costs a path no bounce and no material launch.
 *   NX_ALPHA_OPAQUE (glTF's default: alpha is ignored) traversal is unchanged: every crossing counts, no fetch.  Under
 *                   NXHIP_SHADOWS_TRANSMIT a crossing ends the shadow ray.
 * The material step under MASK and OPAQUE: the path never passes through.  The random numbers of the pass-through test (shade_path:
 * rng_next > opacity || (map && rng_next > alpha)) are still drawn, exactly those of a BLEND material and in the same order; only their
 * outcome is ignored, so every later draw of the path is the one it was.  Colour still comes from the map's rgb.  The rule has one
 * device text (shade_path's SOLID form) which both pipelines' material launches reach; the medium's scatter step shades no surface.
 * Validation, on the host — NXHIP_ERR_INVALID and the previous table stays in place: alphas NULL with count > 0; a mode outside the
 * enum; a MASK cutoff that is not finite or lies outside [0, 1].  At render time (and in the ray-batch hooks, which follow the table
 * too): a count that differs from the material count; a MASK material on an instance that is a mesh light (NX_LIGHT_MESH) — the light
 * sampler would pick points inside the holes.  Out of scope: holes in emitters, an order for BLEND (it stays stochastic), doubleSided,
 * mip-mapping.
 * Restrictions of a first version.  While some material of the table is MASK or OPAQUE (host-known, as the see-through fact of
 * NXHIP_SHADOWS_TRANSMIT is): the material launches are their SOLID instances — general ones, no map-free form — and the tail kernel is
 * off (nxhip_set_tail_bounce is ignored).  Said outright: ONE such entry — and OPAQUE is glTF's default, so any .glb read with its alpha
 * modes has one — moves EVERY material launch of the context onto those instances, which are also the ones that read detail records and
 * know all five material types.  They compute the same shading rule, but they are other kernels: frames of such a context are not
 * promised to be bit-identical to frames of the same scene without the table, on any surface, and its passes are somewhat slower (no
 * map-free launch, no tail kernel).  Equal bits hold within the family: both pipelines, every pass shape.  While some material is MASK (the pass flavor's alpha-test bit):
 *   - the trace launches are the ALPHA_TEST instances (nx_trace.hip): no hand-over to the thin kernel, no IDENTITY instance, no ENTRY
 *     instance;
 *   - nxhip_set_entry_points is ignored by the pass: an entry state "walks past the first triangles" of a run of rays on the assumption
 *     that those tests are final, which they are not when one of them may be rejected.
 * nxhip_trace_batch, nxhip_trace_shadow_batch and nxhip_trace_transmittance_batch use the ALPHA_TEST instances whenever the table has a
 * MASK material.  Results do not depend on nxhip_enable_trace_stats.  May be set at any time, also between accumulated frames. */
int nxhip_set_material_alpha(nxhip_ctx *ctx, const nx_material_alpha *alphas, uint32_t count);
/* Extension — fog: ONE homogeneous participating medium per context, confined to a world-space axis-aligned box (nx_medium of nexus_pod.h:
 * boxMin, boxMax, grey extinction sigmaT per world unit, Henyey-Greenstein asymmetry g, single-scattering albedo per channel).  Off by
 * default.  The call replaces the medium; NULL removes it.  After NULL, or a medium with sigmaT == 0, the context is exactly what it was
 * before the first call: the same flavor word, the same graphs, the same frames bit for bit.
 *
 * Validation, on the host — NXHIP_ERR_INVALID and the previous medium stays: a field that is not finite; sigmaT < 0; an albedo component
 * outside [0, 1]; |g| > 0.99; boxMin[i] >= boxMax[i].
 * Pipeline restriction of this first version: the medium needs the SCAN pipeline (NX_COMPACT_FAST) and pixel-keyed random numbers
 * (NX_RNG_PIXEL_KEYED); while a medium with sigmaT > 0 is set, a render in any other mode is refused (NXHIP_ERR_INVALID, with a message
 * that says so) — the classic pipeline and the slot-keyed stream have no stage of their own to draw from.
 *
 * THE RULE.  All arithmetic is binary32 without contraction; logf / expf / cosf / sinf are include/nexus_fmath.h's nxf_logf, nxf_expf,
 * nxf_cosf, nxf_sinf.  It applies to every ray (o, d) of the closest-hit queue of bounce b >= 1 whose record says "shade this hit" (codes
 * 1..4) or "miss" (code 7); tEnd = the record's t, or +inf for a miss.
 *   segment    per axis i with d_i != 0: a_i = (boxMin_i - o_i) / d_i, b_i = (boxMax_i - o_i) / d_i; an axis with d_i == 0 contributes
 *              (-inf, +inf) if boxMin_i <= o_i <= boxMax_i, otherwise the segment is empty.
 *              t0 = max(0, max_i min(a_i, b_i)),  t1 = min(tEnd, min_i max(a_i, b_i)),  L = t1 - t0.
 *              L <= 0 (or empty): the record is not touched and no random number is drawn.
 *   flight     xi = the first number of the stream keyed by (global pixel, bounce b, frame, STAGE 256); stages 0 and 1 are the roulette's and
 *              the material step's, and the key mixes bounce * 2 + stage + 1, so stage 2 of bounce b would be stage 0 of bounce b + 1: 256
 *              lies past every value those two can form.  s = -logf(1.0f - xi) / sigmaT  (1 - xi is exact and lies in (0, 1]);  scatter iff s < L.
 *              xi has 23 bits, so no flight exceeds -ln(2^-23) = 15.95 mean free paths: a box more than 15.95 / sigmaT deep is opaque
 *              to the camera, where the true transmittance would be at most 1.2e-7.
 *              No scatter: the record is not touched; the material launch shades the hit, or adds the miss, exactly as without a medium
 *              (arriving has probability T = exp(-sigmaT L), so the throughput needs no factor).
 *   scatter    at x = o + d * (t0 + s).  The record's code becomes 5 (kHitCodeMedium: no material type and no miss type looks at the
 *              record again); t, u, v, the triangle and the instance bits stay (the feature buffers read them).
 *              If the ray's roulette bit (kRaySurvives) is clear the path ends here.  Otherwise beta = tp.rgb / maxcomp(tp.rgb) as at a
 *              surface ((1, 1, 1) at bounce 1), then beta *= albedo.  If b == pathLength the path ends.
 *   light      taken when the surfaces' is (useMIS on, or analytic lights present), by the surfaces' own function: the same pick among
 *   sample     nLights, the same count of random numbers per branch, in NXHIP_LIGHTS_UNIFORM and POWER, over mesh lights, analytic lights
 *              and the sampled environment, continuing the medium's stream.  The origin is x with no offset (the offset vector is 0).  In
 *              place of BSDF x cosine stands p(c), c = dot(d, omega) for the sampled direction omega:
 *                p(c) = (1 - g*g) * (1 / (4 pi)) / (t * sqrtf(t)),  t = (1 + g*g) - (2 g) c;
 *              p(c) is also the "BSDF pdf" of the power heuristic for mesh lights and the environment; analytic lights carry no weight.
 *              (The function is handed the shading normal (0, 0, 1), whose frame rotation is the identity, and a zero geometric normal.)
 *   continue   xi1, xi2 = the next numbers of the same stream, after the light sample's.  |g| < 1e-3: c = 1 - 2 xi1; otherwise
 *              q = (1 - g*g) / ((1 - g) + (2 g) xi1),  c = ((1 + g*g) - q*q) / (2 g), clamped to [-1, 1].  sinT = sqrtf(max(0, 1 - c*c)),
 *              phi = 6.28318531f * xi2; with (t0, t1) the branch-free orthonormal frame about d of Duff et al. 2017 (as for the analytic
 *              lights), omega = normalize((t0 * (cosf(phi) sinT) + t1 * (sinf(phi) sinT)) + d * c).
 *              The new ray starts at x (no offset) with throughput beta (phase / pdf is 1) and last pdf p(c); it is an ordinary sampled ray,
 *              so x becomes the path's previous vertex.  Its roulette draw for bounce b + 1 is made as the material launch makes it.
 *   shadow     every shadow request of a bounce — the material launch's and the medium vertex's alike — is attenuated before the any-hit
 *   rays       launch reads it: Ls = the segment rule on (origin, direction, tEnd = tmax); if Ls > 0 the request's radiance is multiplied by
 *              expf(-sigmaT * Ls); Ls <= 0: no multiplication at all, the bits of a request that does not cross the box are the default's.
 *              Deterministic, and it composes with NXHIP_SHADOWS_TRANSMIT: the product is in the request before the crossings multiply.
 * A medium whose box no camera ray, bounce ray or shadow ray crosses gives the frames of a context without one, bit for bit: its random
 * numbers come from a stage nobody else reads.
 * Out of scope: coloured extinction; more than one medium, or media bound to meshes; emission; heterogeneous density; an unbounded
 * medium (a box larger than the scene serves: a sun's or an environment's shadow ray then has a finite Ls); the classic pipeline and the
 * slot-keyed stream; a tail-kernel form (the tail kernel is off while a medium is set, as under NXHIP_SHADOWS_TRANSMIT); fog in the
 * feature buffers (they keep the camera ray's surface hit).
 * The two kernels of the medium (nx_medium.hip) are in the pass graphs only while a medium with sigmaT > 0 is set (bit 13 of
 * nxhip_debug_pass_flavor's word); without it the graphs are launch for launch what they were. */
int nxhip_set_medium(nxhip_ctx *ctx, const nx_medium *medium);
/* Extension — fog density grid: a heterogeneous medium.  rho holds nz x ny x nx floats, x fastest, over the medium's box; the extinction at a
 * point p of the box becomes sigmaT x rho(p).  The grid is copied before the call returns, belongs to the context and is independent of
 * nxhip_set_medium, which leaves it alone: it modulates whichever medium is set, and takes effect only while a medium with sigmaT > 0 is
 * set.  NULL removes it and releases its memory; the context is then exactly what it was before the first call: the same flavor word,
 * graphs and frames.
 *
 * Validation, on the host and before anything is allocated — NXHIP_ERR_INVALID and the previous grid stays: a dimension of 0; a dimension
 * above 512; more than 2^27 voxels; a value that is negative or not finite; a grid whose maximum is 0.
 * A render — and the hook that walks — also refuses sigmaT x max(rho) x |boxMax - boxMin| > 512 (NXHIP_ERR_INVALID, with a message that
 * says what to do): the walk below is bounded by 4096 iterations, and this keeps the bound out of reach.
 *
 * THE RULE.  All arithmetic is binary32 without contraction; logf is nxf_logf.  The segment t0, L, t1 = t0 + L of a ray (o, d) is the
 * medium's segment rule above, unchanged; with L <= 0 nothing below happens.
 *   lookup     n = (nx, ny, nz); vscale_i = n_i / (boxMax_i - boxMin_i), formed on the host in binary64 and rounded once.
 *              g_i = (p_i - boxMin_i) * vscale_i - 0.5f,  i0 = floor(g_i),  f_i = g_i - floor(g_i); i0 and i0 + 1 are both clamped to
 *              [0, n_i - 1] (clamp to edge).  rho(p) = three nested lerps a + f * (b - a): along x, then y, then z.  A constant grid
 *              returns its constant exactly.
 *   bricks     8 x 8 x 8 voxels each, nb_i = ceil(n_i / 8), the last one possibly partial.  M[b] = the maximum of rho over the voxels
 *              [8 b_i - 1, 8 b_i + 8] per axis, clamped to the grid: the one-voxel apron is what the trilinear footprint of a point of the
 *              brick can reach.  Built on the device in the call; the host keeps no copy of the voxels.
 *              Brick space: u_i(t) = ((o_i + d_i t) - boxMin_i) * bscale_i,  bscale_i = n_i / (8 (boxMax_i - boxMin_i)), formed like vscale.
 *   walk       start brick b_i = clamp(floor(u_i(t0)), 0, nb_i - 1).  The next boundary of an axis with d_i != 0:
 *              tNext_i = (((b_i + [d_i > 0]) / bscale_i + boxMin_i) - o_i) / d_i — recomputed from the integer index after every step,
 *              never accumulated; d_i == 0: tNext_i = +inf.  t = t0; tau = -logf(1.0f - xi), xi the next number of the stream (the first
 *              tau is the stream's first number).  Per iteration:
 *                ax = the axis of the smallest tNext (ties: the lowest axis); tExit = min(tNext_ax, t1); mu = sigmaT * M[b];
 *                depth = mu * (tExit - t).
 *                tau < depth: a TENTATIVE COLLISION — t += tau / mu, p = o + d * t, r = rho(p); the mode below decides; if the walk goes
 *                  on it draws a new tau and stays in the brick.
 *                otherwise: tau -= max(depth, 0); the walk ends if !(tNext_ax < t1); else t = tExit, b_ax moves by one (the walk ends if it
 *                  leaves [0, nb_ax)) and tNext_ax is recomputed.
 *              A brick with M == 0 costs one iteration and no random number.  Bound: 4096 iterations, brick steps and collisions together;
 *              at the bound a free flight ends the path (absorbed, no continuation) and a shadow request gets T = 0.
 *   free       the stream of the homogeneous flight, keyed (pixel, bounce, frame, stage 256).  At a tentative collision zeta = the next
 *   flight     number; the collision is REAL iff zeta * M[b] < r, and the path then scatters at t: everything after it is the medium's
 *              rule above, unchanged, continuing the same stream (code 5, beta, light sample, continuation, roulette).  A walk that ends
 *              without a real collision does not touch the record.
 *   shadow     ratio tracking, from a stream keyed (pixel, bounce, frame, STAGE 257), formed as the free flight forms its own (a path has
 *   rays       at most one shadow request per bounce).  T = 1.0f; at every tentative collision T *= max(0.0f, 1.0f - r / M[b]) (a binary32
 *              lerp may overshoot its corner maximum by an ulp); T == 0.0f ends the walk.  The request's radiance is multiplied by T only if
 *              at least one tentative collision happened: a request that crosses no brick with M > 0 keeps the default's bits and draws
 *              nothing.  It composes with NXHIP_SHADOWS_TRANSMIT as the homogeneous product does.
 * The GRID instances of the medium's two kernels are in the pass graphs while a medium with sigmaT > 0 AND a grid are set (bit 14 of
 * nxhip_debug_pass_flavor's word, beside bit 13); the homogeneous instances keep their code.
 * Out of scope: coloured or per-channel density; emission; more than one grid; grids bound to meshes; animated grids beyond calling the
 * setter again; residual or decomposition tracking; a tail-kernel form; fog in the feature buffers; file formats other than .npy. */
int nxhip_set_medium_density(nxhip_ctx *ctx, const float *rho, uint32_t nx, uint32_t ny, uint32_t nz);
/* PathTracer::UpdateDeviceScene / Scene::ToDevice — Renderer/PathTracer.cpp:305-308, Scene/Scene.cpp:115-140 */
int nxhip_set_camera(nxhip_ctx *ctx, const nx_camera *camera);
int nxhip_set_render_settings(nxhip_ctx *ctx, const nx_render_settings *settings);
/* Extensions that do not exist in the reference (see nexus_pod.h): RNG keying, compaction order, conductor. */
int nxhip_set_modes(nxhip_ctx *ctx, int rngMode, int compactMode, int conductorMode);
/* Multi-GPU tile split: this context renders `localCount` pixels; pixelMap[i] = global pixel index of local
 * pixel i (NULL: identity over width*height).  Re-allocates the queues for localCount paths. */
int nxhip_set_pixel_map(nxhip_ctx *ctx, const uint32_t *pixelMap, uint32_t localCount);
/* The order of the context's paths over the FULL frame (no tile split): NXHIP_ORDER_ROWS = image rows, the reference's (thread k of
 * GenerateKernel is pixel k: PathTracer.cu:85-100) and the default; NXHIP_ORDER_TILES = 8 x 8 pixel tiles, row-major inside a
 * tile, tiles left to right in bands of eight rows — the 64 primary rays a wave fetches together are then a compact block of the
 * image instead of a 64 x 1 strip (coherent node fetches, and what entry points need: nxhip_set_entry_points).  With the
 * pixel-keyed RNG the image does not depend on it.  Equivalent to nxhip_set_pixel_map with the map nxhip_tile_pixel_map(width,
 * height, 1, 0, 1, order, ...) returns; unlike a caller's map the ORDER is kept across nxhip_resize.  A later nxhip_set_pixel_map /
 * nxhip_mgpu_init replaces it. */
enum { NXHIP_ORDER_ROWS = 0, NXHIP_ORDER_TILES = 1 };
int nxhip_set_pixel_order(nxhip_ctx *ctx, int order);

/* Batch `frames` consecutive frames into one pass of the wavefront (default 1 = the reference's one frame per
 * Render()).  Every queue then holds localCount * frames paths, so each kernel launch carries `frames` times the work:
 * the latency tail of a trace launch (its slowest ray) and the per-launch overheads are amortised, at the price of
 * HBM capacity (about 0.3 KB per path).  Each frame keeps its own frame number / RNG streams; the accumulate step
 * applies the frames' running-mean updates in order.  The queues grow when needed and are kept when `frames` shrinks
 * (a shorter last pass of a frame budget costs no allocation); the frame number and the accumulation are untouched. */
int nxhip_set_frames_per_pass(nxhip_ctx *ctx, uint32_t frames);

/* Passes in flight (default 1 = the reference's behaviour: a pass starts when the previous one has finished).  With
 * R > 1 consecutive nxhip_render_frame calls go round robin to R slots, each with its own queues (R times the queue memory),
 * stream and graph instance, so that the drain phase of a pass — a few long rays, most of the GPU idle, at one frame per
 * pass more than half of the pass — overlaps with the bulk of the next passes.  nxhip_accumulate folds every finished pass
 * into the one accumulation, oldest first: the image is bit-identical to R = 1.  Worth it for small passes (one frame per
 * pass: 2.2x at R = 6; 20 frames per pass: +20 % at R = 4; the persistent trace launches of the slots are sized to share the
 * CUs).  Fastest with enough hardware queues: export GPU_MAX_HW_QUEUES=24 before the process touches HIP; with the runtime's
 * default of 4 the pass graphs take the shape that fits them (nxhip_set_queue_budget), and the trace launches the size that fits
 * the slots the queues keep resident (nxhip_resident_slots_for): R is the number of passes that may await nxhip_accumulate, how many
 * of them are on the chip at once is the library's choice.  Kernel timing, the counting variant and
 * a bound radiance buffer fall back to one pass at a time. */
int nxhip_set_passes_in_flight(nxhip_ctx *ctx, uint32_t passes);

/* Queue budget: the hardware queues the library may count on when it shapes the work of R passes in flight.  Resolved at
 * nxhip_create: GPU_MAX_HW_QUEUES if the environment sets it to a whole number in [1, 32], else 4 (the runtime's own default).  The
 * library only READS the variable and never changes the runtime's queues.  R passes in flight need 2 R + 1 lanes (two parallel graph
 * branches per slot — closest-hit beside any-hit — and the context's stream for the accumulates).  Where that exceeds the budget, a
 * slot's pass graph is built as a single chain (every launch of a level behind the one in front of it), so that a slot is one lane
 * and no branch of its graph queues behind another slot's launches (four passes in flight on four queues: +13 %).  Same kernels,
 * arguments and grids either way: the image is bit-identical.  The accumulates stay on the context's stream.  One pass at a time and
 * every run whose lanes fit the budget keep the parallel graphs.
 * nxhip_set_queue_budget: queues = 0 reads the environment again, 1 .. 32 is an explicit budget, anything else NXHIP_ERR_INVALID; waits
 * for everything issued, like nxhip_set_passes_in_flight; the next pass picks or builds the graph instance of the matching shape.
 * nxhip_get_queue_budget (each destination may be NULL): the resolved budget; 1 if a pass issued now would replay the chain shape, else 0;
 * the largest number of pass-graph instances any slot holds. */
int nxhip_set_queue_budget(nxhip_ctx *ctx, int queues);
int nxhip_get_queue_budget(nxhip_ctx *ctx, uint32_t *queues, uint32_t *chained, uint32_t *graphInstances);
/* The budget a value of GPU_MAX_HW_QUEUES resolves to (NULL: the variable is not set): a whole number in [1, 32] is itself, anything
 * else 4.  Needs no context and no device. */
uint32_t nxhip_queue_budget_from_text(const char *text);
/* Of `passes` in flight, the slots the library keeps resident under a budget: all of them where 2 passes + 1 lanes fit, else as many
 * as the budget's queues serve side by side (budget - 1: one queue carries the context's stream), at least 1 and at most `passes`.  The persistent trace launches are sized to share the chip among that many slots (four passes in
 * flight on four queues: the shares of three, +6 %); nothing else follows it: nxhip_render_frame still goes round robin over all `passes`
 * slots, and `passes` remains the number of passes that may await nxhip_accumulate.  Same kernels and arguments, other grids: the
 * image is bit-identical.  Needs no context and no device. */
uint32_t nxhip_resident_slots_for(uint32_t passes, uint32_t budget);
/* Test hook: the resident slots of a pass issued now, the workgroups of its closest-hit launches, and which of the slots
 * (0 .. passes - 1) the last pass rendered in.  Each destination may be NULL. */
int nxhip_debug_resident_slots(nxhip_ctx *ctx, uint32_t *resident, uint32_t *traceBlocks, uint32_t *slotOfLastPass);
/* Test hook: the pass graph the last pass replayed, counted from the runtime's graph object when the instance was built — kernel nodes,
 * dependency edges, and the largest number of nodes that depend on one and the same node (1: a chain; 2: closest-hit beside any-hit).
 * Each destination may be NULL. */
int nxhip_debug_last_graph(nxhip_ctx *ctx, uint32_t *nodes, uint32_t *edges, uint32_t *fanOut);

/* Tail kernel (no counterpart in the reference, whose graph has one node per kernel and bounce, PathTracer.cpp:114-124).
 * From bounce `bounce` on — 2 .. pathLength, 0 = off — the rest of every path is run by ONE launch after the trace of
 * bounce - 1: each wave takes 64 paths and loops logic -> shade -> shadow ray -> continuation ray per lane.  Late bounces
 * carry a few per cent of a pass's rays but each costs a trace level as long as its slowest ray plus five more launches.
 * Default NXHIP_TAIL_AUTO: for passes of up to four 1080p frames' worth of paths, bounce 5 (bounce 3 for up to 2.5 frames with
 * at most three passes in flight) — one frame per pass +21 %, with six passes in flight +16 % — off for larger ones (where it
 * loses).  Same functions and the same order of additions per pixel:
 * the image is bit-identical.  Only with NX_RNG_PIXEL_KEYED and NX_COMPACT_FAST, and not while kernel timing or the counting
 * variant is enabled (those passes use the level-by-level graph). */
#define NXHIP_TAIL_AUTO 0xffffffffu
int nxhip_set_tail_bounce(nxhip_ctx *ctx, uint32_t bounce);
/* Entry points of the primary rays (off by default).  on != 0: every pass first walks, once per run of 64 consecutive paths, the
 * node steps whose outcome is provably the same for every primary ray the run can contain (conservative bundle-against-box tests:
 * nx_entry.hip), and the closest-hit launch of the primary rays starts each ray from that state instead of the TLAS root — the
 * reference starts every ray at the root (Cuda/BVH/BVH8Traversal.cuh:165-192).  Hit records are unchanged bit for bit; the node
 * visit counts of nxhip_read_trace_stats drop by the steps saved.  Takes effect for a pinhole camera (lens radius 0). */
int nxhip_set_entry_points(nxhip_ctx *ctx, int on);
/* The entry states of the last rendered pass, 160 bytes each (nx_device.h EntryState: six stack entries, node group, leaf group,
 * int32 sp, instSp, leafSlot, steps, the instance's BLAS pointers, then the consumed triangle's record and bookkeeping) — a test
 * hook: how many node steps the walk saved per run, which triangles it consumed or skipped.  *count = number of runs. */
int nxhip_read_entry_states(nxhip_ctx *ctx, void *out, uint32_t capacityRuns, uint32_t *count);
/* Test hook: how many times the context has launched the entry-state walk since it was created.  A slot's table outlives the pass:
 * it is walked again, in front of the slot's next pass, only after a call that changed something the walk reads (camera, pixel set,
 * TLAS, instances, BLASes, materials' types, entry points switched on) — one launch per slot that renders afterwards. */
int nxhip_debug_entry_walks(nxhip_ctx *ctx, uint64_t *count);
/* Test hook: the primary rays of the pass rendered last, as GenerateKernel left them in the trace queue (PathTracer.cu:85-122).  Nothing
 * is launched: the call waits for the pass and copies the queue regions out into dense path order, path k = slice x localCount + local
 * pixel (slice s of a pass of F frames is frame frameLast - F + 1 + s; local pixel p is global pixel pixelMap[p], or p).  The ray of
 * global pixel g = i + j x width goes through the point lowerLeftCorner + viewportX (i + r1) / width + viewportY (j + r2) / height of the
 * focal plane: image row 0 is the BOTTOM row of the viewport (Renderer.h: screenshots are written last row first).
 * origin3[3k..], direction3[3k..] = x, y, z of the ray (the w words are not part of them: origin.w carries the entry bits, direction.w
 * the path number); pathIndex[k] = the bit pattern of direction.w, which must be k.  *count = the pass's paths, also when the call
 * refuses for capacity.  NXHIP_ERR_INVALID with a message: no pass has been rendered; settings.pathLength != 1 (the later bounces of a
 * pass write their rays over the primary ones); more than one pass in flight; capacity < *count or a NULL array; the queues of that pass
 * released or re-allocated since. */
int nxhip_debug_read_primary_rays(nxhip_ctx *ctx, float *origin3, float *direction3, uint32_t *pathIndex, uint32_t capacity, uint32_t *count);
/* Test hook for the kernel instances a pass graph picks by scene (pass_flavor, nxhip_render.hip).  *flavor (may be NULL): the flavor
 * bits of the graph the last pass replayed; 256 = trace instances without the transform path, 512 = map-free material launch.
 * forceGeneral: those of the two bits whose specialised instances later passes must not use (0xffffffff: unchanged). */
int nxhip_debug_pass_flavor(nxhip_ctx *ctx, uint32_t forceGeneral, uint32_t *flavor);
/* Test hook: the compile-time instance sets (nx_variants.h: kMf* material features, kTf* trace features) the launches of the last pass
 * were looked up by, as recorded when the graph the pass replayed was built — beside its flavor word, not recomputed from the context
 * at the call.  sets[0] the SCAN pipeline's material launch; sets[1] the tail kernel and sets[2] the bounce it takes over from;
 * sets[3] the medium's scatter kernel, bit 16 set for the GRID form; sets[4] the classic pipeline's logic kernel; sets[5], sets[6],
 * sets[7] the primary, the closest-hit and the any-hit trace launches.  A family the pass does not launch reads 0xffffffff (so do
 * sets[1] and sets[2] without a tail kernel).  NXHIP_ERR_INVALID with a message: no pass has been rendered, or a NULL array. */
int nxhip_debug_pass_instances(nxhip_ctx *ctx, uint32_t sets[8]);
/* Test hook for the thin kernel (nx_trace.hip): the hand-over rule — at most `lanes` busy lanes of a dry wave for at least `iters`
 * iterations (product: 16 / 16; 64 / 0 makes every wave hand over the first rays it takes, after one iteration) — and whether the ray-batch
 * hooks (nxhip_trace_batch, nxhip_trace_shadow_batch) use the hand-over + thin launch too, so that a test can put arbitrary rays
 * through the cooperative search and compare the records with the oracle's (inHooks bit 0).  inHooks bit 1: hand over after `iters`
 * iterations of EVERY stretch between two refill points, dry queue or not — the rays then reach the thin kernel with the traversal
 * state of exactly that many steps (round 6: the hand-over carries the state).  nxhip_debug_thin_counts: the rays the last hook call
 * handed over (closest-hit, any-hit). */
int nxhip_debug_set_thin(nxhip_ctx *ctx, uint32_t lanes, uint32_t iters, int inHooks);
/* ... and how many items a thin wave's pool may hold (0 = the product's 960 of 1 024): a round whose children do not fit puts items back and
 * goes on with fewer per round — a test lowers the limit so that ordinary scenes drive that path; results must not change. */
int nxhip_debug_set_thin_pool(nxhip_ctx *ctx, uint32_t slots);
int nxhip_debug_thin_counts(nxhip_ctx *ctx, int32_t counts[2]);
/* ... and of level `bounce` (0 = the primary rays) of the pass rendered last: what its trace launches handed over (closest-hit, any-hit). */
int nxhip_debug_thin_counts_of_pass(nxhip_ctx *ctx, uint32_t bounce, int32_t counts[2]);
/* Test hook: the continuation rays the material launch of `bounce` of the pass rendered last did not queue because their Russian-
 * roulette draw was lost when they were made (SCAN pipeline, pixel-keyed random numbers, no environment map and a black
 * background: nothing could read what they hit).  nxhip_read_queue_sizes counts them in traceSize[bounce] as the reference does;
 * this is the part of that size no trace launch saw.  0 for every other kind of pass. */
int nxhip_debug_ended_rays_of_pass(nxhip_ctx *ctx, uint32_t bounce, int32_t *count);

/* ---- rendering ----------------------------------------------------------------------------------- */

/* PathTracer::ResetFrameNumber — PathTracer.cpp:243-246 */
int nxhip_reset_frame_number(nxhip_ctx *ctx);
int nxhip_set_frame_number(nxhip_ctx *ctx, uint32_t frameNumber); /* next render uses frameNumber + 1 */
uint32_t nxhip_frame_number(nxhip_ctx *ctx);
/* PathTracer::Render minus AccumulateKernel — PathTracer.cpp:248-276: frameNumber++, Generate, Trace, then
 * pathLength x (Logic, 4 x Shade, Trace || TraceShadow), replayed as one hipGraph.  Asynchronous.  Renders one pass
 * = frames-per-pass frames (1 unless nxhip_set_frames_per_pass was called). */
int nxhip_render_frame(nxhip_ctx *ctx);
/* AccumulateKernel — Cuda/PathTracer/PathTracer.cu:480-496, PathTracer.cpp:278.  Asynchronous. */
int nxhip_accumulate(nxhip_ctx *ctx);
/* `frames` frames: passes of frames-per-pass frames (render + accumulate), the last one shorter if `frames` is not a
 * multiple. */
int nxhip_render(nxhip_ctx *ctx, uint32_t frames);

/* Read-back (synchronises).  radiance: localCount * framesPerPass x 3 floats (frame slices one after the other);
 * accumulation: localCount x 3 floats; rgba8: localCount uint32
 * (the reference's GL pixel buffer, OpenGL/PixelBuffer.cpp:4-41). */
int nxhip_read_radiance(nxhip_ctx *ctx, float *dst);
int nxhip_read_accumulation(nxhip_ctx *ctx, float *dst);
int nxhip_read_rgba8(nxhip_ctx *ctx, uint32_t *dst);
/* Resume: load a previously read accumulation (localCount x 3 floats) and continue as if `frameNumber` frames had been
 * rendered; the next frame is frameNumber + 1 and the running mean continues bit for bit.  (The reference keeps the
 * accumulation on the device only and restarts on every change, PathTracer.cpp:243-246.) */
int nxhip_write_accumulation(nxhip_ctx *ctx, const float *src, uint32_t frameNumber);
/* Device pointers for zero-copy consumers on the same GPU (e.g. an RCCL gather of radiance tiles):
 * float4 per local pixel (xyz = radiance, w unused).  Valid until the next resize / set_pixel_map. */
/* PathTracer::FreeDeviceBuffers (Renderer/PathTracer.cpp:35-92): give the path-state and queue buffers of every pass slot back
 * (about 0.28 KB per path and slot: 36 GB at 1080p x 64 frames per pass).  The accumulated image, the scene and the
 * configuration stay; the next nxhip_render_frame (or ray-batch hook) allocates what it needs again. */
int nxhip_release_queues(nxhip_ctx *ctx);
void *nxhip_radiance_device_ptr(nxhip_ctx *ctx);
void *nxhip_accumulation_device_ptr(nxhip_ctx *ctx);
/* Make the context write its per-frame radiance into caller-owned device memory (float4[capacity], capacity >=
 * localCount * framesPerPass) — e.g. a torch tensor that is then handed to an RCCL gather without a copy.  NULL: back to the
 * context's own buffer.  The binding is dropped by nxhip_resize / nxhip_set_pixel_map. */
int nxhip_bind_radiance(nxhip_ctx *ctx, void *radianceDevice, uint32_t capacity);
/* Root-side accumulate + tonemap of externally gathered radiance: src = device float4 laid out [slices][sliceStride];
 * element k (< count) of slice s is the radiance of frame firstFrame + s at full-image pixel srcPixelMapDevice[k]
 * (device uint32[count]; NULL: k).  Writes the context's accumulation / RGBA8 buffers, which always cover
 * width*height pixels. */
int nxhip_accumulate_external(nxhip_ctx *ctx, const void *srcRadianceDevice, uint32_t count, uint32_t slices, uint32_t sliceStride,
                              uint32_t firstFrame, const void *srcPixelMapDevice);
/* Root-side image assembly when every rank accumulates its own tiles (nxhip_accumulate with a pixel map) and only the
 * accumulated tiles travel: element k (< count) of srcAccumulationDevice (device float4[count], a rank's local-order
 * accumulation) is copied to dstAccumulationDevice[srcPixelMapDevice[k]] (device float4[width*height], caller-owned) and,
 * if dstRgba8Device is not NULL, tonemapped into dstRgba8Device[...] (device uint32[width*height]).  No arithmetic is
 * applied to the accumulated values, so the assembled image is bit-identical to a single-GPU accumulation. */
int nxhip_compose_tiles(nxhip_ctx *ctx, const void *srcAccumulationDevice, uint32_t count, const void *srcPixelMapDevice,
                        void *dstAccumulationDevice, void *dstRgba8Device);
/* Read-back of the full width*height accumulation / RGBA8 image (after nxhip_accumulate_external). */
int nxhip_read_full_accumulation(nxhip_ctx *ctx, float *dst);
int nxhip_read_full_rgba8(nxhip_ctx *ctx, uint32_t *dst);

/* ---- multi-GPU: interleaved row tiles + one RCCL gather per pass ---------------------------------------
 * No counterpart in the reference (single GPU; SURVEY.md section 8e defines the layer).  One context per GPU — one process
 * or one host thread each.  RCCL (librccl.so.1, or $NX_RCCL_LIB) is loaded on first use.  Call sequence per rank:
 *   rank 0: nxhip_mgpu_unique_id(id) -> hand the 128 bytes to every rank (MPI, a file, a socket: the caller's choice)
 *   all   : nxhip_mgpu_init(ctx, world, rank, id, tileRows)   [ncclCommInitRank; installs the rank's pixel map]
 *   loop  : nxhip_render_frame, nxhip_accumulate, nxhip_mgpu_gather   [asynchronous, one stream]
 *   rank 0: nxhip_mgpu_read_rgba8 / nxhip_mgpu_read_accumulation      [full width x height image]
 * With the pixel-keyed RNG (nxhip_set_modes) the assembled image equals the single-GPU image bit for bit. */
/* Row r belongs to rank (r / tileRows) % worldSize; height must be a multiple of tileRows * worldSize.  Writes the global
 * pixel index of every local pixel in the context's path order (tiledOrder != 0: 8x8 pixel tiles; 0: rows);
 * out == NULL: only *localCount. */
int nxhip_tile_pixel_map(uint32_t width, uint32_t height, int worldSize, int rank, uint32_t tileRows, int tiledOrder, uint32_t *out,
                         uint32_t *localCount);
int nxhip_mgpu_unique_id(void *id128);
int nxhip_mgpu_init(nxhip_ctx *ctx, int worldSize, int rank, const void *id128, uint32_t tileRows);
/* The same with a communicator the caller already owns (an ncclComm_t passed as void*; it is not destroyed). */
int nxhip_mgpu_attach(nxhip_ctx *ctx, void *ncclComm, int worldSize, int rank, uint32_t tileRows);
/* ncclGather of every rank's accumulated tile (16 B per local pixel) to rank 0 on the context's stream; rank 0 then
 * scatters the tiles into the full image and tonemaps (a copy: no arithmetic on the accumulated values). */
int nxhip_mgpu_gather(nxhip_ctx *ctx);
int nxhip_mgpu_read_rgba8(nxhip_ctx *ctx, uint32_t *dst);        /* rank 0: width*height uint32 */
int nxhip_mgpu_read_accumulation(nxhip_ctx *ctx, float *dst);    /* rank 0: width*height x 3 floats */
int nxhip_mgpu_shutdown(nxhip_ctx *ctx);

/* ---- feature buffers and the denoiser ------------------------------------------------------------------
 * No counterpart in the reference, whose only image is the running mean (AccumulateKernel, PathTracer.cu:480-496): a viewer built
 * on it shows noise for hundreds of frames.  Two steps, the second needs the first.
 *
 * Feature buffers (AOVs), off by default.  on != 0: every pass also records, per path, two float4 of the CAMERA ray's closest
 * hit, whatever the material does next (opacity / alpha pass-through included):
 *   albedo       xyz: the diffuse map's colour at the hit if the material has a map (it replaces the albedo, as in the shading
 *                     code), else the albedo of a diffuse / plastic / dielectric material, else (conductor) (1, 1, 1); w: coverage,
 *                     1 on a hit.  A miss: all 0.
 *   normalDepth  xyz: the world-space shading normal, turned towards the camera; w: the hit distance.  A miss: all 0.
 * nxhip_accumulate folds them into two context-wide running means with the update and frame order of the colour, so the
 * accumulated values do not depend on frames per pass, passes in flight, pipeline, pixel order, tail bounce or entry points.
 * With the switch off nothing is allocated or launched for them.  Turning it on after frames were accumulated is
 * NXHIP_ERR_INVALID (colour and features must cover the same frames): nxhip_reset_frame_number first. */
int nxhip_set_aov(nxhip_ctx *ctx, int on);
/* The accumulated feature buffers, localCount x 4 floats each, in the order of nxhip_read_accumulation (either may be NULL). */
int nxhip_read_aov(nxhip_ctx *ctx, float *albedo4, float *normalDepth4);
/* The per-path values of the pass rendered last: localCount * framesPerPass x 4 floats each, frame slices one after the other
 * (for consumers that accumulate themselves). */
int nxhip_read_aov_frame(nxhip_ctx *ctx, float *albedo4, float *normalDepth4);
/* The twin of nxhip_write_accumulation: load accumulated feature buffers (a checkpoint resumes colour AND features; the frame
 * number comes with nxhip_write_accumulation).  Either may be NULL (left as it is). */
int nxhip_write_aov(nxhip_ctx *ctx, const float *albedo4, const float *normalDepth4);
/* Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over the accumulated colour C_0, guided by the accumulated feature
 * buffers A (albedo + coverage, 4 components), N (normal) and Z (depth).  p = centre pixel, q = tap:
 *   iteration i = 0 .. iterations - 1, step s = 2^i, taps q = p + s (dx, dy), dx, dy in {-2 .. 2}, taps outside the image skipped
 *   h = (1/16, 1/4, 3/8, 1/4, 1/16)
 *   w(p, q) = h[dx] h[dy] exp(-(|C_i(p) - C_i(q)|^2 / (sigmaColor 2^-i)^2 + |N(p) - N(q)|^2 / sigmaNormal^2
 *                               + |A(p) - A(q)|^2 / sigmaAlbedo^2 + (Z(p) - Z(q))^2 / (sigmaDepth max(Z(p), 1e-6))^2))
 *   C_{i+1}(p) = sum_q w(p, q) C_i(q) / sum_q w(p, q)        sums in the order dy-major, dx-minor; exp = nxf_expf
 * The result is a SEPARATE full-frame image (row-major) and its RGBA8 (the tonemap of nxhip_read_rgba8): the accumulation and
 * its RGBA8 are not touched, rendering goes on afterwards.  params == NULL: nxhip_denoise_defaults.  iterations == 0 copies.
 * iterations > 6 or a sigma that is not a positive finite number: NXHIP_ERR_INVALID.  Needs the feature buffers, and a context
 * that renders the full frame (identity map, NXHIP_ORDER_ROWS / NXHIP_ORDER_TILES): on a tile split (nxhip_set_pixel_map with a
 * partial set, nxhip_mgpu_*) NXHIP_ERR_INVALID.  Asynchronous, on the context's stream behind the accumulates. */
int nxhip_denoise(nxhip_ctx *ctx, const nx_denoise_params *params);
int nxhip_denoise_defaults(nx_denoise_params *params);
/* Read-back of the last nxhip_denoise (synchronises): width * height x 3 floats / width * height uint32, row-major. */
int nxhip_read_denoised(nxhip_ctx *ctx, float *rgb);
int nxhip_read_denoised_rgba8(nxhip_ctx *ctx, uint32_t *dst);

/* ---- adaptive sampling ------------------------------------------------------------------------------------
 * No counterpart in the reference, which sends a path through every pixel for as many frames as the caller guesses.  Off by
 * default; with it off nothing is allocated and nothing extra is launched.
 *
 * The context's BASE set is what nxhip_set_pixel_map / nxhip_set_pixel_order / the identity define.  It keeps sizing the
 * accumulation, the RGBA8 image, the accumulated feature buffers and every read-back.  Per pixel of it there are three more words:
 * count (uint32), meanY and M2 (float).  While the mode is on, nxhip_accumulate folds a pass with ONE kernel; for a pixel that the
 * pass rendered, per frame slice in frame order (binary32, no fused operation):
 *   n = ++count
 *   colour  a += (r - a) / n                                   (n == 1: a = r)  — the running mean with the PIXEL's count
 *   Y = (0.2126 r.x + 0.7152 r.y) + 0.0722 r.z
 *   d = Y - meanY;  meanY += d / n;  M2 += d * (Y - meanY)     (n == 1: meanY = Y, M2 = 0)   — Welford
 * and the accumulated feature buffers (nxhip_set_aov) the same way, so features and colour cover the same samples.  While no
 * pixel has been culled count == frame number, and accumulation, RGBA8 and radiance are what the plain path gives, bit for bit.
 *
 * A BLOCK is 64 consecutive paths of the base order (NXHIP_ORDER_TILES: an 8 x 8 pixel tile); the base set's last block may be
 * partial.  nxhip_adaptive_update decides per pixel with count >= 2
 *   e = sqrt(M2 / (n (n - 1))) / max(meanY, lumFloor)          relative standard error of the mean luminance
 * unsettled = count < minSamples or not (e <= threshold) — a non-finite e keeps its block alive — and a pixel with count < 2 is
 * unsettled.  A block stays active iff any of its pixels is unsettled; a block that has been deactivated stays so.  The
 * block's largest e (NaN counts as +inf, pixels with count < 2 as 0) is kept for diagnostics.  With cull != 0 the passes that
 * follow render the pixels of the active blocks only, in base order; with cull == 0 (estimate only) they keep rendering the whole
 * base set and the block flags are the stop rule alone.
 *
 * BIAS.  A stop rule that reads the same samples it stops on biases the estimate (Kirk & Arvo 1991): pixels whose first samples
 * happen to agree stop early and keep their too-dark (or too-bright) mean.  Deciding per block and the minSamples floor reduce
 * that; they do not remove it.  The image of an adaptive run is NOT an unbiased estimate.
 *
 * Rules:
 *   - needs NX_RNG_PIXEL_KEYED (a path's radiance must depend on (pixel, frame) only): nxhip_set_adaptive with slot-keyed numbers
 *     is NXHIP_ERR_INVALID, and so is nxhip_set_modes back to slot-keyed while it is on;
 *   - turning it on after frames were accumulated is NXHIP_ERR_INVALID (nxhip_reset_frame_number first), as nxhip_set_aov;
 *   - on a context with nxhip_mgpu_* it is NXHIP_ERR_INVALID, and so is nxhip_mgpu_init / nxhip_mgpu_attach while it is on;
 *   - nxhip_write_accumulation / nxhip_write_aov while it is on are NXHIP_ERR_INVALID (the counts have no checkpoint form);
 *   - nxhip_resize, nxhip_set_pixel_map, nxhip_set_pixel_order and nxhip_reset_frame_number start the statistics over: all counts
 *     0, every block active;
 *   - cull != 0 and no active block: nxhip_render_frame / nxhip_render return NXHIP_OK, launch nothing and leave the frame number;
 *   - nxhip_accumulate with nothing pending does nothing (folding the same radiance again would count samples twice);
 *   - nxhip_read_radiance / nxhip_read_aov_frame return the paths of the last pass: its active count x its frames, active order;
 *   - every other read-back stays in base order and base size.
 * params: threshold >= 0, lumFloor > 0 (both finite), else NXHIP_ERR_INVALID.  NULL: off, buffers released, base set restored. */
int nxhip_adaptive_defaults(nx_adaptive_params *p);   /* threshold 0.05, lumFloor 0.01, minSamples 16, cull 1: starting values, not tuned */
int nxhip_set_adaptive(nxhip_ctx *ctx, const nx_adaptive_params *p);
/* Folds the pending passes, decides, rebuilds the active set and synchronises.  activePixels / activeBlocks (either may be NULL):
 * the pixels / blocks still active. */
int nxhip_adaptive_update(nxhip_ctx *ctx, uint32_t *activePixels, uint32_t *activeBlocks);
/* Repeats { render `interval` frames, accumulate, update } until no block is active or maxFrames frames have been issued by this
 * call.  As the active set shrinks, more frames go into one pass: min(interval, paths the queues already hold / active pixels),
 * at least 1; nothing is allocated.  Decisions happen at interval boundaries only, so the packing changes no result.
 * framesRendered: frames issued by this call; activePixels: as of the last update (either may be NULL). */
int nxhip_render_adaptive(nxhip_ctx *ctx, uint32_t maxFrames, uint32_t interval, uint32_t *framesRendered, uint32_t *activePixels);
int nxhip_read_sample_counts(nxhip_ctx *ctx, uint32_t *counts);   /* base localCount */
int nxhip_read_noise_stats(nxhip_ctx *ctx, float *meanM2);        /* base localCount x 2: (meanY, M2) */
/* As of the last update (before the first: every block active, maxima 0).  blockMax / active may be NULL; capacity in blocks. */
int nxhip_read_block_noise(nxhip_ctx *ctx, float *blockMax, uint8_t *active, uint32_t capacity, uint32_t *blocks);
/* The set the next pass renders: base-local index of every path of a frame slice, in order. */
int nxhip_read_active_map(nxhip_ctx *ctx, uint32_t *baseLocalIndex, uint32_t capacity, uint32_t *count);

/* D_QueueSize after the last rendered frame — Cuda/PathTracer/PathTracer.cuh:61-73.  Each array NX_PATH_MAX_LENGTH ints. */
typedef struct nxhip_queue_sizes {
    int32_t traceSize[NX_PATH_MAX_LENGTH];
    int32_t traceShadowSize[NX_PATH_MAX_LENGTH];
    int32_t diffuseSize[NX_PATH_MAX_LENGTH];
    int32_t plasticSize[NX_PATH_MAX_LENGTH];
    int32_t dielectricSize[NX_PATH_MAX_LENGTH];
    int32_t conductorSize[NX_PATH_MAX_LENGTH];
} nxhip_queue_sizes;
int nxhip_read_queue_sizes(nxhip_ctx *ctx, nxhip_queue_sizes *out);
/* One material type's row of the same table, for ANY type (NX_MAT_METALROUGH has no field above: the struct keeps the reference's
 * layout): out[b] = items the material step shaded as `type` at bounce slot b, NX_PATH_MAX_LENGTH ints. */
int nxhip_read_material_queue_sizes(nxhip_ctx *ctx, int type, int32_t *out);

/* PathTracer::SetPixelQuery / GetSelectedInstance — PathTracer.cpp:310-317, PathTracer.h:25 */
int nxhip_set_pixel_query(nxhip_ctx *ctx, uint32_t x, uint32_t y);
int nxhip_get_selected_instance(nxhip_ctx *ctx, int32_t *instanceIdx);

/* ---- kernel-level hooks (tests, bench) ----------------------------------------------------------- */

/* TraceKernel on a caller-supplied ray batch — Cuda/BVH/BVH8Traversal.cuh:148-322.  Host buffers. */
int nxhip_trace_batch(nxhip_ctx *ctx, const nx_ray *rays, uint32_t count, nx_hit *hits);
/* TraceShadowKernel's any-hit test — BVH8Traversal.cuh:326-518.  occluded[i] = 1 if blocked within tmax[i]. */
int nxhip_trace_shadow_batch(nxhip_ctx *ctx, const nx_ray *rays, const float *tmax, uint32_t count, uint8_t *occluded);
/* The same batch through the any-hit TRANSMIT instance (nxhip_set_shadow_transmittance), whatever the context's mode: transmittance[i] =
 * the ray's T (0 = occluded).  Needs what a render needs (TLAS, materials, every diffuse map a material names): the kernel follows
 * instance -> material -> texture -> triangle without bounds tests, so the tables are checked and brought up to date first.
 * nxhip_trace_shadow_batch itself launches the plain instance in every mode. */
int nxhip_trace_transmittance_batch(nxhip_ctx *ctx, const nx_ray *rays, const float *tmax, uint32_t count, float *transmittance);

/* Test hook: overwrite ONE node of an uploaded BLAS in device memory WITHOUT the checks of nxhip_upload_blas.  Exists so that
 * the trace kernels' behaviour on a BVH that is not a tree (a child that points back at its parent) can be tested: they must
 * abandon such rays and nxhip_sync must report NXHIP_ERR_TRAVERSAL (nx_device.h kStallLimit) instead of never returning.
 * The node's child / leaf ranges must still lie inside the BLAS (that part is checked: a wild index is a wild device read). */
int nxhip_debug_write_blas_node(nxhip_ctx *ctx, int32_t blasId, uint32_t nodeIdx, const nx_bvh8_node *node);
/* Test hook: the number of passes every slot has begun since its ordered-compaction status words were last cleared.  The words
 * are tagged with that number instead of being cleared per launch (NX_COMPACT_ORDERED); it wraps after 2^20 - 1 passes — a
 * viewer at a thousand one-frame passes per second gets there in 17 minutes — where the words are cleared in stream order and
 * the count starts over.  The test sets it just below the limit and renders across the wrap. */
int nxhip_debug_set_scan_epoch(nxhip_ctx *ctx, uint32_t epoch);
/* Test hook: the trace kernels hand the same rays out again and again (a ray that re-queues itself — what an in-kernel restart did in
 * round 5 until the host's watchdog ended the process).  The per-launch progress check must end every such launch with
 * NXHIP_ERR_TRAVERSAL from nxhip_sync within milliseconds. */
int nxhip_debug_set_requeue(nxhip_ctx *ctx, int on);
/* Test hook: the BINARY tree a device build collapses, which the build otherwise frees.  While `on`, every single build — nxhip_build_blas,
 * nxhip_rebuild_tlas; not nxhip_build_blas_batch — copies its tree and the collapse's cost table to the host before it returns; the last
 * one stays with the context (switching the hook off drops it).  Off, the default, costs a build one branch.
 * nxhip_debug_read_binary_tree copies it out.  With n primitives: internal nodes 0 .. n-2 (the root is 0), leaf k = node n-1+k =
 * primitive leafOrder[k].  left / right / count: n-1 entries; parent: 2n-1 (the root's is -1); box6: 2n-1 x {lo[3], hi[3]};
 * leafOrder: n; eval: 7 (n-1) entries of 8 bytes {float cost; int8_t decision (0 leaf slot, 1 wide node, 2 distribute), leftCount,
 * rightCount, pad}, entry i of node x at 7 x + i.  *primCost: the collapse's price of a primitive (0.75 for triangles, 4 for
 * instances); *builder: the nxhip_set_device_builder value the build ran with.  A build of at most 8 primitives is a single node
 * without a binary tree: *n == 0 and no array is written.  `capacity`: the primitives the arrays have room for.  *n, *primCost and
 * *builder are filled whenever a tree is stashed; NXHIP_ERR_INVALID when none is, when capacity < *n, or when an array is null
 * although *n > 0. */
int nxhip_debug_keep_binary_tree(nxhip_ctx *ctx, int on);
int nxhip_debug_read_binary_tree(nxhip_ctx *ctx, uint32_t capacity, uint32_t *n, float *primCost, int32_t *builder, int32_t *left, int32_t *right,
                                 int32_t *parent, int32_t *count, float *box6, uint32_t *leafOrder, uint64_t *eval);

/* Kernel-level test hooks for the shading functions (same role as nxhip_trace_batch for the traversal): run the device
 * BSDF sample / eval (the headers of Cuda/BSDF/ as restated in nx_bsdf.h) and the software texture fetch on host arrays.
 * sample: uses wi and rng (the xorshift state before the call); eval: uses wi and wo.  Directions are in the local
 * shading frame (z = normal).  `material` is one nx_material; its type selects the BSDF (a CONDUCTOR runs the extended
 * conductor BSDF whatever the context's conductor mode).  nx_bsdf_query / nx_bsdf_result: nexus_pod.h. */
int nxhip_bsdf_sample_batch(nxhip_ctx *ctx, const nx_material *material, const nx_bsdf_query *queries, uint32_t count, nx_bsdf_result *results);
int nxhip_bsdf_eval_batch(nxhip_ctx *ctx, const nx_material *material, const nx_bsdf_query *queries, uint32_t count, nx_bsdf_result *results);
/* kind as in nxhip_upload_texture (0 diffuse, 1 emissive, 2 hdr; textureId ignored for hdr); uv = 2*count floats,
 * rgba = 4*count floats (sRGB-decoded, bilinear, wrap addressing: what the shade kernels see).  kind 2 on a float environment map
 * (nxhip_upload_env_float): that map's own lookup, linear, alpha 1. */
int nxhip_tex2d_batch(nxhip_ctx *ctx, int kind, int textureId, const float *uv, uint32_t count, float *rgba);
/* (kind 3 / 4: a normal / roughness map through tex2d_linear — linear, every channel byte / 255) */
/* The detail maps' rule on arrays — a test hook over the device function the material kernels call (a `make release` library refuses
 * it): for every k < count, the hit on triangle triIdx[k] of instance `instanceIdx` at barycentrics hitUv[2k..] (the hit record's u, v),
 * reached along rayDir[3k..]: normalOut[3k..] = the world-space shading normal after fallback and flip (the interpolated normal, flipped,
 * when the material names no normal map), roughnessOut[k] = the roughness handed to the BSDF, fellBack[k] = 1 when a normal map was named
 * and a fallback condition took ns back to N.  NXHIP_ERR_INVALID: a NULL array, no such instance, a triangle index out of range, a scene
 * a render would refuse. */
int nxhip_shading_frame_batch(nxhip_ctx *ctx, uint32_t instanceIdx, const uint32_t *triIdx, const float *hitUv, const float *rayDir, uint32_t count,
                              float *normalOut, float *roughnessOut, uint32_t *fellBack);

/* The inputs of an NX_MAT_METALROUGH material at a hit — a test hook (a `make release` library refuses it).  An exception to the hooks'
 * habit of calling ONE device function the kernels call: shade_path has no such function to call without changing the text of the kernels
 * every context launches, so the hook's kernel restates its sequence — bary2, the diffuse map's tex2d, detail_shading_frame (the G and B
 * channels of one lookup), the clamp of m that the BSDF applies (metal_clamp01) — from the same device functions, in the same order: for every k < count, the hit on triangle triIdx[k] of instance `instanceIdx` at barycentrics
 * hitUv[2k..]: out[5k..] = c.r, c.g, c.b, r, m as the rule of nxhip_set_materials states them (m after the clamp).  NXHIP_ERR_INVALID: a
 * NULL array, no such instance, an instance whose material is of another type, a triangle index out of range, a scene a render would
 * refuse. */
int nxhip_material_inputs_batch(nxhip_ctx *ctx, uint32_t instanceIdx, const uint32_t *triIdx, const float *hitUv, uint32_t count, float *out);

/* Test hooks of the light table (NXHIP_LIGHTS_POWER only, else NXHIP_ERR_INVALID; both bring the table up to date first).
 * read: cdf / entryLight (either may be NULL) hold `capacity` entries, lightBase (may be NULL) lightCount + 1 words; *entries = N.
 * pick: entry[k], prob[k] = the device's pick for u[k] and its P.  A u outside [0, 1) — NaN included, which would index the guide
 * table wildly — is refused on the host before anything is launched; so is an empty table, and a table whose weights sum to
 * nothing (`valid` = 0: the renderer never samples it; the hook reads the flag back). */
int nxhip_read_light_table(nxhip_ctx *ctx, float *cdf, uint32_t *entryLight, uint32_t capacity, uint32_t *lightBase, uint32_t *entries);
int nxhip_light_pick_batch(nxhip_ctx *ctx, const float *u, uint32_t count, uint32_t *entry, float *prob);
/* Test hooks of the light tree (a `make release` library refuses them; NXHIP_LIGHTS_POWER with NXHIP_LIGHT_IMPORTANCE_POSITION only, else
 * NXHIP_ERR_INVALID; all three bring the tree up to date first).
 * read: nodes8 (may be NULL) receives 2G nodes of eight words each — lo xyz, w, hi xyz, entry; node 0 is unused — and holds
 *       `capacityNodes` nodes; order (may be NULL) receives N words; *leaves = G, *entries = N (either may be NULL).
 * pick: entry[k], prob[k] = the device's descent from points3[3k..] with u[k]; entry 0xffffffff and prob 0: no light sample.
 * prob: prob[k] = the probability the descent from points3[3k..] has of entry[k].
 * Refused on the host before anything is launched: a point that is not finite, a u outside [0, 1), an entry >= N, an empty tree, a tree
 * whose weights sum to nothing. */
int nxhip_read_light_tree(nxhip_ctx *ctx, float *nodes8, uint32_t *order, uint32_t capacityNodes, uint32_t *leaves, uint32_t *entries);
int nxhip_light_tree_pick_batch(nxhip_ctx *ctx, const float *points3, const float *u, uint32_t count, uint32_t *entry, float *prob);
int nxhip_light_tree_prob_batch(nxhip_ctx *ctx, const float *points3, const uint32_t *entry, uint32_t count, float *prob);

/* Test hooks of the environment lookup and of its importance sampler (nxhip_set_env_sampling).  All three refuse with
 * NXHIP_ERR_INVALID while no environment map is uploaded; read and sample — and eval when it is asked for a pdf or a texel —
 * also while environment sampling is off.  count == 0 returns NXHIP_OK after those checks; a null array with count > 0 is refused.
 * read:   the three float tables as uploaded (any of them may be NULL; all NULL: only *width / *height are written, which may be
 *         NULL too).  marginalCdf receives `height` entries, rowCdf and density width x height each; `capacityTexels` is the number
 *         of entries every destination given can hold: >= width x height when rowCdf or density is asked for, >= height for the
 *         marginal cdf alone, else NXHIP_ERR_INVALID.  marginalCdf[y] and rowCdf[y * width + x]:
 *         non-decreasing, each cdf ends in exactly 1; density[y * width + x] = P(texel) x width x height / (2 pi^2), i.e. the pdf per
 *         solid angle x cos(latitude).  P(texel) is proportional to luminance(sRGB-decoded texel) x sin(pi (y + 1/2) / height) + 1e-6,
 *         luminance = 0.2126 R + 0.7152 G + 0.0722 B; the additive floor keeps a black map samplable.
 * sample: r = count x 2 numbers, each in [0, 1) (anything else — NaN included — is refused on the host before anything is launched);
 *         direction[3k..] = the unit direction the NEE draws for (r[2k], r[2k + 1]): row from the first, column from the second;
 *         pdf[k] its pdf per solid angle (light-selection probability excluded), formed as the NEE forms it, from the direction;
 *         texel[k] = y * width + x that the cdf inversion PICKED (the first index whose cdf exceeds r, on both axes).
 * eval:   direction = count x 3 finite numbers (unit length is the caller's business; a non-finite component is refused);
 *         rgb[3k..] = the background a ray leaving in that direction sees (SampleBackground, PathTracer.cu:65-83); pdf[k] (may be
 *         NULL) = the sampler's pdf per solid angle there, density[texel] / max(cos(latitude), 1e-6); texel[k] (may be NULL) = the
 *         texel the direction's map coordinates fall in.  With sampling off it returns the colours only: pdf and texel must be NULL. */
int nxhip_read_env_tables(nxhip_ctx *ctx, float *marginalCdf, float *rowCdf, float *density, uint32_t capacityTexels, uint32_t *width, uint32_t *height);
int nxhip_env_sample_batch(nxhip_ctx *ctx, const float *r, uint32_t count, float *direction, float *pdf, uint32_t *texel);
int nxhip_env_eval_batch(nxhip_ctx *ctx, const float *direction, uint32_t count, float *rgb, float *pdf, uint32_t *texel);
/* The analytic lights' draw on arrays — a test hook over the product's own sampling function (a `make release` library refuses it):
 * for light `lightIndex` of the table and every k < count, origins3[3k..] = o as the rule above uses it (already offset), r2[2k..] = (r1, r2)
 * in [0, 1): direction3[3k..], tmax[k], factor3[3k..] = colour x intensity x att x 2 / (d^2 (1 + cos thetaMax)), ok[k] = 0 when d <= radius
 * (the other outputs of that k are then meaningless).  NXHIP_ERR_INVALID: no such light, a NULL array, an origin that is not finite, an
 * r outside [0, 1). */
int nxhip_analytic_light_sample_batch(nxhip_ctx *ctx, uint32_t lightIndex, const float *origins3, const float *r2, uint32_t count,
                                      float *direction3, float *tmax, float *factor3, uint32_t *ok);
/* The medium's rule on arrays — two test hooks over the device functions the medium's kernels call (a `make release` library refuses them).
 * Both need a medium with sigmaT > 0 (NXHIP_ERR_INVALID otherwise, as for a NULL array or an input that is not finite or out of range).
 * segment: for every k < count, origin[3k..], dir[3k..] (d as given: unit length is the caller's business), tEnd[k] > 0 (+inf allowed),
 *          xi[k] in [0, 1): t0[k] and length[k] = the segment rule's t0 and L, both 0 where L <= 0 or the segment is empty;
 *          transmittance[k] = expf(-sigmaT L), exactly 1 where L <= 0; scatterT[k] = t0 + s where the flight scatters (s < L), else -1.
 * phase:   dirIn[3k..] = d (unit), xi1[k], xi2[k] in [0, 1): dirOut[3k..] = the continuation's omega, pdf[k] = p(dot(d, omega)) as the scatter
 *          kernel stores it. */
int nxhip_medium_segment_batch(nxhip_ctx *ctx, const float *origin, const float *dir, const float *tEnd, const float *xi, uint32_t count,
                               float *t0, float *length, float *transmittance, float *scatterT);
int nxhip_medium_phase_batch(nxhip_ctx *ctx, const float *dirIn, const float *xi1, const float *xi2, uint32_t count, float *dirOut, float *pdf);
/* The density grid's rule on arrays — three test hooks (a `make release` library refuses them).
 * majorants: bricks[0..2] = nb; majorant (NULL: the counts alone) receives the nb[2] x nb[1] x nb[0] brick majorants as the device built
 *          them, x fastest; capacity counts floats.  Needs a grid.
 * density: rho[k] = the lookup at points3[3k..] (any finite point: clamp to edge), majorant[k] = M of the brick the walk's start rule gives
 *          that point.  Needs a medium with sigmaT > 0 and a grid, as the next.
 * track:   the walk in both modes for the ray origin[3k..], dir[3k..] that ends at tEnd[k] > 0 (+inf allowed); each mode starts from its own
 *          copy of the xorshift32 state seed[k] != 0.  scatterT[k] = the parameter of the real collision, -1 where there is none;
 *          transmittance[k] = the ratio tracking's T, exactly 1 where no tentative collision happened; steps2[2k] (free flight) and
 *          steps2[2k + 1] (ratio tracking) = iterations | tentative collisions << 16, both 0 where the ray does not cross the box. */
int nxhip_read_medium_majorants(nxhip_ctx *ctx, float *majorant, uint32_t capacity, uint32_t bricks[3]);
int nxhip_medium_density_batch(nxhip_ctx *ctx, const float *points3, uint32_t count, float *rho, float *majorant);
int nxhip_medium_track_batch(nxhip_ctx *ctx, const float *origin, const float *dir, const float *tEnd, const uint32_t *seed,
                             uint32_t count, float *scatterT, float *transmittance, uint32_t *steps2);
/* The three above work on an environment map of either kind (a float map's P(texel) follows nxhip_upload_env_float's weight).
 * read_env_float: the float map as it is stored, rgb = width x height x 3 floats, bit for bit what was uploaded (rgb NULL: only
 * *width / *height are written, which may be NULL too); NXHIP_ERR_INVALID while the environment map is not a float one or
 * capacityTexels < width x height. */
int nxhip_read_env_float(nxhip_ctx *ctx, float *rgb, uint32_t capacityTexels, uint32_t *width, uint32_t *height);
/* The cut points the cdf inversion starts from (either kind of map, sampler on): 65 entries per cdf, entry b = the first index whose
 * cdf exceeds b / 64, clamped to the cdf's last index.  marginalGuide receives 65 words, rowGuide height x 65 (either may be NULL);
 * capacityRows >= height when rowGuide is given, else NXHIP_ERR_INVALID. */
int nxhip_read_env_guides(nxhip_ctx *ctx, uint32_t *marginalGuide, uint32_t *rowGuide, uint32_t capacityRows);
/* The sky's radiance on arrays — a test hook over the device function the map kernel of nxhip_set_sky calls (a `make release` library
 * refuses it): rgb[3k..] = the sky term alone (ground included, no disc) along the unit direction dir3[3k..], for the parameters of
 * `sky` (validated as nxhip_set_sky validates them; width, height and sunDisc are not used).  The context's map is not touched.
 * NXHIP_ERR_INVALID: a NULL array with count > 0, a direction that is not finite, a sky nxhip_set_sky would refuse. */
int nxhip_sky_radiance_batch(nxhip_ctx *ctx, const nx_sky *sky, const float *dir3, uint32_t count, float *rgb);

/* The transcendental functions of the shading path (include/nexus_fmath.h: the ONE text the kernels and the CPU oracle both
 * compile — sin / cos / exp / log / pow / atan2 / asin replacing the libm calls of Random.cuh:119-121, Microfacet.cuh:18,75,
 * PathTracer.cu:65-83, Utils.h:51-54) on host arrays: out[i] = nxf_apply(op, a[i], b[i]), op = NXF_OP_*; b may be NULL for the
 * one-argument functions.  tests/test_fmath.py compares the device's results with the oracle's bit for bit. */
int nxhip_fmath_batch(nxhip_ctx *ctx, int op, const double *a, const double *b, uint32_t count, double *out);

/* Visit counters of the two trace kernels (algorithmic bytes for the roofline).  When enabled
 * the trace kernels run their counting variant; off by default. */
typedef struct nxhip_trace_stats {
    uint64_t rays, nodes, tris, instances;
    /* SIMD-efficiency diagnostics: traversal-loop iterations summed over waves, and the number of lanes that were
     * busy / took a node step / took a primitive step in them (ideal: 64 per iteration). */
    uint64_t waveIters, lanesActive, lanesNode, lanesPrim;
    /* shader-clock cycles per loop section summed over waves: 0 refill, 1 pop/retire, 2 node select+fetch, 3 node
     * decode, 4 instance entry, 5 triangle fetch+test, 6-7 unused */
    uint64_t cycles[8];
} nxhip_trace_stats;
int nxhip_enable_trace_stats(nxhip_ctx *ctx, int enable);
int nxhip_read_trace_stats(nxhip_ctx *ctx, nxhip_trace_stats *closest, nxhip_trace_stats *shadow, int reset);

/* Per-kernel-class device time.  enable = 1: frames are launched kernel by kernel on the context's stream with a
 * hipEvent pair around every launch (no graph, no overlap between the trace and shadow-trace kernels).  enable = 2: the
 * frame graph is rebuilt with an event-record node before and after every kernel node, so each kernel is timed under the
 * conditions of the production replay (closest-hit and shadow traces of a bounce run concurrently); the events are read
 * after every replay.  enable = 3: the same graph, but replays are NOT separated by a sync: nxhip_read_kernel_times then
 * returns the kernels of the LAST replay only, timed under the sustained clocks of a back-to-back series.  0: off.  Classes: 0 generate, 1 trace, 2 shadow, 3 logic, 4 shade, 5 accumulate,
 * 6 thin (the launch behind the two trace launches of a level that finishes the last long rays of their dry waves: nx_trace.hip thin_kernel). */
enum { NXHIP_K_GENERATE = 0, NXHIP_K_TRACE = 1, NXHIP_K_SHADOW = 2, NXHIP_K_LOGIC = 3, NXHIP_K_SHADE = 4, NXHIP_K_ACCUMULATE = 5, NXHIP_K_THIN = 6, NXHIP_K_COUNT = 7 };
typedef struct nxhip_kernel_times {
    double ms[NXHIP_K_COUNT];
    uint64_t launches[NXHIP_K_COUNT];
} nxhip_kernel_times;
int nxhip_enable_kernel_timing(nxhip_ctx *ctx, int enable);
int nxhip_read_kernel_times(nxhip_ctx *ctx, nxhip_kernel_times *out, int reset);
/* With enable = 2 or 3: the kernels of the LAST timed replay one by one, in graph order — class (NXHIP_K_*), start relative to
 * the replay's first kernel and duration, both in ms — so that a caller can set the launches of one pass beside that pass's wall
 * time (bench.py: the nine closest-hit launches of the repetition its roofline is computed from).  Up to `capacity` entries are
 * written, *count receives the number of kernels in the graph.  Call it before nxhip_read_kernel_times(reset). */
int nxhip_read_graph_timeline(nxhip_ctx *ctx, int32_t *klass, float *startMs, float *durationMs, uint32_t capacity, uint32_t *count);

/* Build-time facts for tests: 1 if the library was compiled with device code for gfx950. */
int nxhip_has_gfx950_code(void);
/* Build facts as bits: 1 = device code for gfx950, 2 = built with the Makefile's scheduler flags, 4 = nxhip_debug_* hooks compiled in
 * (the default; a `make release` library keeps the symbols and refuses the calls). */
int nxhip_build_info(void);

/* ---- ABI stamp ---------------------------------------------------------------------------------------
 * A library that does not match its caller — a stale build picked up through NEXUS_AMD_LIB / LD_LIBRARY_PATH, a header of
 * another version — used to show as a GPU memory fault in the first launch (round 3: gpurun_out/r3_07).
 * Now it is an error status before anything is launched.
 *   nxhip_header_abi_stamp()  what THIS header says, compiled into the caller: API version + size and key offsets of every
 *                             struct that crosses the boundary, FNV-1a hashed;
 *   nxhip_abi_stamp()         the same function as compiled into the library;
 *   nxhip_check_library(s)    NXHIP_OK if s equals the library's stamp AND every translation unit of the library was compiled
 *                             with the same device-side layouts (DeviceState, Counters, InstTrav, record strides ...: a library
 *                             linked from objects of different source states is refused), else NXHIP_ERR_ABI + message.
 * nxhip_create performs the library-internal half by itself.  C / C++ callers: nxhip_check_library(nxhip_header_abi_stamp())
 * once after loading; the Python binding does the equivalent with the sizes of its own ctypes / numpy mirrors. */
uint64_t nxhip_abi_stamp(void);
int nxhip_check_library(uint64_t callerStamp);

static inline uint64_t nxhip_abi_mix(uint64_t h, uint64_t v)
{
    int i;
    for (i = 0; i < 8; i++) { h = (h ^ (v & 0xffu)) * 0x100000001b3ull; v >>= 8; }
    return h;
}
static inline uint64_t nxhip_header_abi_stamp(void)
{
    /* (the list the Python binding mirrors: nexus_amd/capi.py abi_words) */
    const uint64_t w[] = {
        NXHIP_API_VERSION, NX_PATH_MAX_LENGTH,
        sizeof(nx_bvh8_node), offsetof(nx_bvh8_node, meta), sizeof(nx_triangle), offsetof(nx_triangle, texCoord0),
        sizeof(nx_bvh_instance), offsetof(nx_bvh_instance, transform), offsetof(nx_bvh_instance, materialId),
        sizeof(nx_material), offsetof(nx_material, emissive), offsetof(nx_material, type), sizeof(nx_light), offsetof(nx_light, type),
        sizeof(nx_analytic_light), offsetof(nx_analytic_light, direction), offsetof(nx_analytic_light, colour), offsetof(nx_analytic_light, innerConeAngle), offsetof(nx_analytic_light, type),
        sizeof(nx_material_detail), offsetof(nx_material_detail, normalScale), sizeof(nx_medium), sizeof(nx_material_alpha), offsetof(nx_material_alpha, cutoff),
        sizeof(nx_skin_corner), offsetof(nx_skin_corner, weight), sizeof(nx_morph_corner), offsetof(nx_morph_corner, dNormal),
        sizeof(nx_camera), offsetof(nx_camera, resolution), sizeof(nx_render_settings), offsetof(nx_render_settings, backgroundColor),
        sizeof(nx_ray), sizeof(nx_hit), sizeof(nx_bsdf_query), sizeof(nx_bsdf_result), offsetof(nx_bsdf_result, rngOut),
        sizeof(nxhip_queue_sizes), sizeof(nxhip_trace_stats), offsetof(nxhip_trace_stats, cycles), sizeof(nxhip_kernel_times), NXHIP_K_COUNT,
        sizeof(nx_sky), offsetof(nx_sky, altitude), offsetof(nx_sky, groundAlbedo), offsetof(nx_sky, width), offsetof(nx_sky, sunDisc),
        sizeof(nx_adaptive_params), offsetof(nx_adaptive_params, minSamples), offsetof(nx_adaptive_params, cull),
        sizeof(nx_denoise_params), offsetof(nx_denoise_params, sigmaColor), offsetof(nx_denoise_params, sigmaDepth),
    };
    uint64_t h = 0xcbf29ce484222325ull;
    size_t i;
    for (i = 0; i < sizeof w / sizeof w[0]; i++) h = nxhip_abi_mix(h, w[i]);
    return h;
}

#ifdef __cplusplus
}
#endif
#endif /* NEXUS_HIP_H */
