/*
 * nexus_host.h — flat C view of the host-side data producers (BVH2 / BVH8 / TLAS builders, instance and
 * camera set-up) for callers that cannot use the C++ classes in include/nexus/ (the Python tests and bench).
 * The C++ classes mirror the reference's host API; these functions only wrap them.
 *   nxh_bvh8_build      BVH8Builder(tris).Init(); Build()     /root/reference/Nexus/src/Assets/AssetManager.cpp:23-37
 *   nxh_bvh2_build      BVH2(tris).Build()                     Geometry/BVH/BVH.cpp:13-26
 *   nxh_instance_init   BVHInstance::SetTransform + ToDevice   Geometry/BVH/BVHInstance.cpp:4-45
 *   nxh_tlas_build      TLAS::Build(); TLAS::Convert()         Geometry/BVH/TLAS.cpp:13-68
 *   nxh_camera_init     Camera::ToDevice                       Scene/Camera.cpp:142-168
 * All functions return 0 on success.
 */
#ifndef NEXUS_HOST_H
#define NEXUS_HOST_H

#include <stdint.h>

#include "nexus_pod.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nxh_bvh8 nxh_bvh8; /* owns nodes + primitive indices */

/* threads = 0: all hardware threads.  The result does not depend on the thread count. */
int nxh_bvh8_build(const nx_triangle *tris, uint32_t triCount, uint32_t threads, nxh_bvh8 **out);
int nxh_tlas_build(const nx_bvh_instance *instances, uint32_t instanceCount, nxh_bvh8 **out);
/* TLAS refit after instance transforms changed (same instances, same topology): recomputes, in place, every node's
 * frame and its children's quantised boxes bottom-up from instances[].boundsMin/Max with the builder's formulas; imask,
 * meta and indices stay.  O(n), against the O(n^2) agglomerative rebuild (Geometry/BVH/TLAS.cpp:13-91, 2.8 s for 16 000
 * instances).  The refitted tree bounds the same instances, so closest hits are those of a rebuilt tree; only the order
 * of visits (and which of two equidistant hits wins) may differ.  Returns 0, or 1 on malformed input. */
int nxh_tlas_refit(nx_bvh8_node *nodes, uint32_t nodeCount, const uint32_t *instanceIdx, const nx_bvh_instance *instances, uint32_t instanceCount);
/* BLAS refit after a mesh's vertices moved (same triangles in the same order, same topology; BVH8::Refit): recomputes, in
 * place, every node's frame and its children's quantised boxes bottom-up from the triangles' vertex boxes — pos0, pos1, pos2
 * grown from the empty box — with the builder's formulas; imask, meta and indices stay.  With unchanged triangles it gives the
 * builder's bytes.  The byte reference of nxhip_update_blas.  The reference rebuilds instead (Assets/AssetManager.cpp:23-37).
 * Children need not follow their parent in the array (the device builders' trees).  Returns 0, or 1 on malformed input. */
int nxh_bvh8_refit(nx_bvh8_node *nodes, uint32_t nodeCount, const uint32_t *triIdx, const nx_triangle *tris, uint32_t triCount);
uint32_t nxh_bvh8_node_count(const nxh_bvh8 *b);
uint32_t nxh_bvh8_prim_count(const nxh_bvh8 *b);
const nx_bvh8_node *nxh_bvh8_nodes(const nxh_bvh8 *b);
const uint32_t *nxh_bvh8_prim_indices(const nxh_bvh8 *b);
void nxh_bvh8_free(nxh_bvh8 *b);

/* BVH2 only (tests): nodes32 receives 2*triCount-1 32-byte nodes, triIdx triCount indices. */
int nxh_bvh2_build(const nx_triangle *tris, uint32_t triCount, uint32_t threads, void *nodes32, uint32_t *triIdx);

void nxh_mat4_from_trs(const float pos[3], const float rotDeg[3], const float scale[3], float out16[16]);
void nxh_mat4_invert(const float in16[16], float out16[16]);
int nxh_instance_init(nx_bvh_instance *out, uint32_t bvhIdx, int32_t materialId, const float transform16[16],
                      const nx_bvh8_node *blasRoot);
int nxh_camera_init(nx_camera *out, const float position[3], const float forward[3], float horizontalFovDeg,
                    uint32_t width, uint32_t height, float focusDist, float defocusAngleDeg);

/* ---- flat view of nexus::Scene / nexus::AssetManager / nexus::PathTracer (include/nexus/Scene.h, PathTracer.h) ------
 * The call sequence is the reference's: load meshes -> AssetManager::CreateBVH + AddMesh, Scene::CreateMeshInstance,
 * Scene::Update (TLAS build), PathTracer::UpdateDeviceScene, PathTracer::Render (Renderer/Renderer.cpp:41-77). */
/* ---- scene files (nexus::OBJLoader, include/nexus/OBJLoader.h): binary glTF 2.0 (.glb) and Wavefront .obj without Assimp.
 * Replaces what Assets/OBJLoader.cpp:8-239 obtains through Assimp: one mesh per glTF primitive, one instance per
 * (node, primitive) with the node transform decomposed to position / Euler degrees / scale, the reference's material
 * heuristics.  Returns 0 on success; the message of a failure is in nxs_last_error(). */
typedef struct nxh_loaded_scene nxh_loaded_scene;
typedef struct nx_loaded_instance {
    int32_t mesh, material;
    float position[3], rotation[3] /* Euler XYZ, degrees */, scale[3];
} nx_loaded_instance;
int nxh_load_scene_file(const char *file, nxh_loaded_scene **out);
/* ... with options (flags 0: exactly nxh_load_scene_file).  NXH_LOAD_METAL_ROUGH: a .glb material without transmission is read as glTF's own
 * metallic-roughness model — an NX_MAT_METALROUGH with albedo = baseColorFactor.rgb, roughness = roughnessFactor, metallic =
 * metallicFactor (defaults 1, 1), ior from KHR_materials_ior (default 1.5) — instead of the reference's PLASTIC; everything else stays. */
#define NXH_LOAD_METAL_ROUGH 1u
/* NXH_LOAD_ALPHA_MODES: a .glb material's alphaMode (glTF's default: OPAQUE) and alphaCutoff (default 0.5) are read as well and come back
 * from nxh_loaded_material_alpha; without the flag that call reports no table (every material blends, as it always has). */
#define NXH_LOAD_ALPHA_MODES 2u
/* NXH_LOAD_SKINS: a .glb's skins (JOINTS_0 / WEIGHTS_0 de-indexed like the positions), joint animations and node tree are read as well;
 * nxh_loaded_skin reports a mesh's.  JOINTS_1 is ignored with a warning, and so are morph targets unless NXH_LOAD_MORPHS is given too; a
 * CUBICSPLINE sampler is read as its keys' values and interpolated linearly, with a warning.  Without the flag every mesh is unskinned,
 * as it always has been. */
#define NXH_LOAD_SKINS 4u
/* NXH_LOAD_MORPHS: a .glb's morph targets (POSITION and NORMAL, float VEC3, sparse accessors included, de-indexed like the positions) are
 * read as well, with the node tree and the animations — their `weights` channels kept —; nxh_loaded_morph reports a mesh's.  All primitives
 * of a mesh must have the same number of targets.  Without the flag no mesh has targets, as it always has been. */
#define NXH_LOAD_MORPHS 8u
int nxh_load_scene_file_ex(const char *file, uint32_t flags, nxh_loaded_scene **out);
void nxh_loaded_scene_free(nxh_loaded_scene *s);
uint32_t nxh_loaded_mesh_count(const nxh_loaded_scene *s);
uint32_t nxh_loaded_mesh_triangle_count(const nxh_loaded_scene *s, uint32_t mesh);
int nxh_loaded_mesh_triangles(const nxh_loaded_scene *s, uint32_t mesh, nx_triangle *dst);
uint32_t nxh_loaded_material_count(const nxh_loaded_scene *s);
int nxh_loaded_materials(const nxh_loaded_scene *s, nx_material *dst);
uint32_t nxh_loaded_instance_count(const nxh_loaded_scene *s);
int nxh_loaded_instances(const nxh_loaded_scene *s, nx_loaded_instance *dst);
/* Images the file's materials refer to (glTF baseColorTexture -> kind 0 diffuse, emissiveTexture -> kind 1 emissive; what
 * OBJLoader.cpp:115-160 creates through Assimp + stb_image), decoded to RGBA8 with row 0 = top row.  Per material the index
 * of its diffuse / emissive texture in this list, -1 for none.  An image that cannot be decoded (PNG only) is dropped with
 * a warning, as the reference prints and carries on (IMGLoader.cpp:24-25). */
uint32_t nxh_loaded_texture_count(const nxh_loaded_scene *s);
int nxh_loaded_texture_info(const nxh_loaded_scene *s, uint32_t index, uint32_t *width, uint32_t *height, int32_t *kind);
int nxh_loaded_texture_pixels(const nxh_loaded_scene *s, uint32_t index, uint8_t *dstRgba8);
int nxh_loaded_material_textures(const nxh_loaded_scene *s, int32_t *diffuseTexture, int32_t *emissiveTexture);
/* glTF KHR_lights_punctual: one record per node that carries a light — position = the node's world translation, direction = its -Z axis,
 * colour x intensity as written (radiometric, no 683 lm/W), spot cone angles defaulting to 0 and pi/4, radius and angular radius 0;
 * `range` is ignored.  dst receives nxh_loaded_analytic_light_count records. */
uint32_t nxh_loaded_analytic_light_count(const nxh_loaded_scene *s);
int nxh_loaded_analytic_lights(const nxh_loaded_scene *s, nx_analytic_light *dst);
/* Detail maps (glTF normalTexture -> kind 3, pbrMetallicRoughness.metallicRoughnessTexture -> kind 4: linear data, the kinds of
 * nxhip_upload_texture), a list of their own beside the one above.  Per material the index of its normal / roughness texture in THIS
 * list (-1: none) and normalTexture.scale (1 without one).  texCoord sets other than 0 and KHR_texture_transform produce a warning. */
uint32_t nxh_loaded_detail_texture_count(const nxh_loaded_scene *s);
int nxh_loaded_detail_texture_info(const nxh_loaded_scene *s, uint32_t index, uint32_t *width, uint32_t *height, int32_t *kind);
int nxh_loaded_detail_texture_pixels(const nxh_loaded_scene *s, uint32_t index, uint8_t *dstRgba8);
int nxh_loaded_material_detail(const nxh_loaded_scene *s, int32_t *normalTexture, int32_t *roughnessTexture, float *normalScale);
/* The materials' alpha modes (nx_material_alpha, nexus_pod.h): *count = the material count when the file was read with NXH_LOAD_ALPHA_MODES,
 * else 0; dst (may be NULL) receives up to `capacity` records. */
int nxh_loaded_material_alpha(const nxh_loaded_scene *s, nx_material_alpha *dst, uint32_t capacity, uint32_t *count);
/* The skin of loaded mesh `mesh` (NXH_LOAD_SKINS): *cornerCount = 3 x its triangles — 0 for a mesh without one — and *jointCount; dst (may
 * be NULL) receives up to `capacity` nx_skin_corner records (nexus_pod.h), corner 3 i + v = vertex v of triangle i. */
int nxh_loaded_skin(const nxh_loaded_scene *s, uint32_t mesh, nx_skin_corner *dst, uint32_t capacity, uint32_t *cornerCount, uint32_t *jointCount);
/* The morph targets of loaded mesh `mesh` (NXH_LOAD_MORPHS): *targetCount — 0 for a mesh without any — and *cornerCount = 3 x its triangles;
 * dst (may be NULL) receives up to `capacity` nx_morph_corner records (nexus_pod.h), target-major: record t x cornerCount + 3 i + v = vertex v
 * of triangle i under target t; defaultWeights (may be NULL) receives *targetCount floats: the placing node's weights, else the mesh's, else 0. */
int nxh_loaded_morph(const nxh_loaded_scene *s, uint32_t mesh, nx_morph_corner *dst, uint32_t capacity, uint32_t *cornerCount, uint32_t *targetCount, float *defaultWeights);
uint32_t nxh_loaded_animation_count(const nxh_loaded_scene *s);
uint32_t nxh_loaded_warning_count(const nxh_loaded_scene *s);
const char *nxh_loaded_warning(const nxh_loaded_scene *s, uint32_t index);
/* IMGLoader::LoadIMG (Assets/IMGLoader.cpp:17-41: stbi_load with 4 channels) for PNG data: RGBA8, row 0 first.
 * dstRgba8 may be NULL to query the size first; *channels = channels of the file (1-4). */
int nxh_decode_png(const uint8_t *data, size_t size, uint32_t *width, uint32_t *height, uint32_t *channels, uint8_t *dstRgba8, size_t dstCapacity);

typedef struct nxs_scene nxs_scene;
typedef struct nxs_pathtracer nxs_pathtracer;
struct nxhip_ctx;

const char *nxs_last_error(void);
int nxs_scene_create(uint32_t width, uint32_t height, nxs_scene **out);
void nxs_scene_destroy(nxs_scene *s);
int nxs_scene_add_material(nxs_scene *s, const nx_material *m, int32_t *materialId);
int nxs_scene_add_texture(nxs_scene *s, int kind /*0 diffuse, 1 emissive, 3 normal, 4 roughness*/, const uint8_t *rgba8, uint32_t w, uint32_t h, int32_t *texId);
int nxs_scene_set_hdr_map(nxs_scene *s, const uint8_t *rgba8, uint32_t w, uint32_t h);
/* Extension — Scene::AddHDRMapFloat(width, height, rgb): the environment as w x h x 3 floats of linear radiance, row 0 the top row
 * (nxhip_upload_env_float at the next device update).  Either kind of map replaces the other. */
int nxs_scene_set_hdr_map_float(nxs_scene *s, const float *rgb, uint32_t w, uint32_t h);
/* Extension — Scene::SetSky(sky): the environment generated on the device from the sun-and-sky model (nxhip_set_sky at the next device
 * update, which validates it; the model is stated in include/nexus_hip.h).  It replaces a map of either kind and is replaced by one.
 * nxs_scene_clear_sky — Scene::ClearSky(): no environment. */
int nxs_scene_set_sky(nxs_scene *s, const nx_sky *sky);
int nxs_scene_clear_sky(nxs_scene *s);
int nxs_scene_add_mesh(nxs_scene *s, const nx_triangle *tris, uint32_t triCount, int32_t materialId, int32_t *meshId);
int nxs_scene_create_instance(nxs_scene *s, uint32_t meshId, int32_t materialId, const float pos[3], const float rotDeg[3],
                              const float scale[3], int32_t *instanceId);
/* Extension (deforming meshes; the reference builds a new BVH instead, Assets/AssetManager.cpp:23-37):
 * AssetManager::UpdateMeshTriangles — the same triangles of mesh `meshId`, in the same order, at new positions; as many as the mesh
 * has.  The host tree is refitted; the next nxs_scene_update re-derives the bounds of the mesh's instances and brings the TLAS up
 * to date by the mode in force, the next nxs_pathtracer_update_device_scene sends the mesh through nxhip_update_blas.  The scene
 * counts as changed (nxs_renderer_render restarts the accumulation). */
int nxs_scene_update_mesh(nxs_scene *s, uint32_t meshId, const nx_triangle *tris, uint32_t triCount);
/* MeshInstance::AssignMaterial + Scene::InvalidateMeshInstance (the viewer's material picker): applied by the next nxs_scene_update. */
int nxs_scene_assign_material(nxs_scene *s, uint32_t instanceId, int32_t materialId);
/* MeshInstance::SetTransform + Scene::InvalidateMeshInstance: move an existing instance; applied by the next nxs_scene_update. */
int nxs_scene_set_instance_transform(nxs_scene *s, uint32_t instanceId, const float pos[3], const float rotDeg[3], const float scale[3]);
/* Extension (off by default): refit the TLAS in nxs_scene_update when only existing instances changed, instead of the
 * reference's full rebuild. */
int nxs_scene_set_tlas_refit(nxs_scene *s, int enable);
/* Extension (off by default): the TLAS is built and refitted on the device (Scene::SetDeviceTlasBuild -> nxhip_rebuild_tlas /
 * nxhip_set_instance_transforms); nxs_scene_update then runs no TLAS builder on the host. */
int nxs_scene_set_device_tlas(nxs_scene *s, int enable);
/* Scene::CreateMeshInstanceFromFile — Scene.cpp:83-91: adds the file's materials, meshes (one BVH8 each) and instances. */
int nxs_scene_load_file(nxs_scene *s, const char *path, const char *fileName);
/* Extension, off by default: files loaded from here on read their materials as NXH_LOAD_METAL_ROUGH does (Scene::SetMetalRoughMaterials). */
int nxs_scene_set_metal_rough(nxs_scene *s, int on);
/* Extension, off by default: files loaded from here on carry their materials' alpha modes as NXH_LOAD_ALPHA_MODES reads them
 * (Scene::SetMaterialAlphaModes); the next device update sends the table (nxhip_set_material_alpha).  nxs_scene_material_alphas: the
 * AssetManager's table — *count records, 0 while no material has a mode; dst (may be NULL) receives up to `capacity` of them. */
int nxs_scene_set_material_alpha_modes(nxs_scene *s, int on);
int nxs_scene_material_alphas(const nxs_scene *s, nx_material_alpha *dst, uint32_t capacity, uint32_t *count);
/* Extension (skinned meshes), off by default: files loaded from here on keep their skins, joint animations and node tree as
 * NXH_LOAD_SKINS reads them (Scene::SetSkins).  nxs_scene_mesh_joint_count: joints of mesh `meshId`'s skin, 0 for a mesh without one.
 * nxs_scene_joint_palette — Scene::JointPalette: the pose of animation `animationIdx` (-1: the rest pose) at time t, evaluated on the host
 * in binary64 and rounded once: *jointCount x 12 floats into dst (capacity in joints), row j the row-major 3 x 4 matrix
 * inverse(meshNodeWorld) x jointWorld[j] x inverseBind[j] — what nxhip_pose_blas and nxs_pathtracer_pose_mesh take. */
int nxs_scene_set_skins(nxs_scene *s, int on);
uint32_t nxs_scene_mesh_count(const nxs_scene *s);
uint32_t nxs_scene_animation_count(const nxs_scene *s);
uint32_t nxs_scene_mesh_joint_count(const nxs_scene *s, uint32_t meshId);
int nxs_scene_joint_palette(const nxs_scene *s, uint32_t meshId, int32_t animationIdx, double t, float *dst, uint32_t capacity, uint32_t *jointCount);
/* Extension (morph targets), off by default: files loaded from here on keep their morph targets, node tree and animations as
 * NXH_LOAD_MORPHS reads them (Scene::SetMorphs).  nxs_scene_mesh_target_count: targets of mesh `meshId`, 0 for a mesh without any.
 * nxs_scene_morph_weights — Scene::MorphWeights: the file's default weights, or the weights channel of animation `animationIdx` (-1: the
 * defaults) on the mesh's node at time t, evaluated in binary64 and rounded once: *targetCount floats into dst (capacity in floats) — what
 * nxhip_pose_blas_morph and nxs_pathtracer_pose_mesh_morph take. */
int nxs_scene_set_morphs(nxs_scene *s, int on);
uint32_t nxs_scene_mesh_target_count(const nxs_scene *s, uint32_t meshId);
int nxs_scene_morph_weights(const nxs_scene *s, uint32_t meshId, int32_t animationIdx, double t, float *dst, uint32_t capacity, uint32_t *targetCount);
int nxs_scene_set_camera(nxs_scene *s, const float pos[3], const float forward[3], float horizontalFovDeg, float focusDist,
                         float defocusAngleDeg);
int nxs_scene_set_render_settings(nxs_scene *s, const nx_render_settings *settings);
int nxs_scene_update(nxs_scene *s);
uint32_t nxs_scene_light_count(const nxs_scene *s);
/* Extension: Scene::AddAnalyticLight / GetAnalyticLights — point, sphere, spot and sun lights (nx_analytic_light, nexus_pod.h), uploaded by
 * the next device update (nxhip_set_analytic_lights, which validates them).  nxs_scene_load_file adds a .glb's KHR_lights_punctual lights.
 * *index (may be NULL) = the light's place in the list; nxs_scene_analytic_lights copies up to `capacity` records out. */
int nxs_scene_add_analytic_light(nxs_scene *s, const nx_analytic_light *light, uint32_t *index);
/* AssetManager::SetMaterialDetail / ClearMaterialDetails / GetMaterialDetails: the detail maps of a material (ids of nxs_scene_add_texture
 * kind 3 / 4); the list is empty while no material has any, else one record per material. */
int nxs_scene_set_material_detail(nxs_scene *s, int32_t materialId, const nx_material_detail *detail);
int nxs_scene_clear_material_details(nxs_scene *s);
uint32_t nxs_scene_material_detail_count(const nxs_scene *s);
int nxs_scene_material_details(const nxs_scene *s, nx_material_detail *dst, uint32_t capacity);
int nxs_scene_remove_analytic_light(nxs_scene *s, uint32_t index);
uint32_t nxs_scene_analytic_light_count(const nxs_scene *s);
int nxs_scene_analytic_lights(const nxs_scene *s, nx_analytic_light *dst, uint32_t capacity);
/* Extension: Scene::SetMedium / ClearMedium / GetMedium — fog, one homogeneous medium in a world-space box (nx_medium, nexus_pod.h), uploaded by
 * the next device update (nxhip_set_medium, which validates it).  nxs_scene_medium: *has = 1 and *dst = the medium, or *has = 0 (dst may be NULL). */
int nxs_scene_set_medium(nxs_scene *s, const nx_medium *medium);
int nxs_scene_clear_medium(nxs_scene *s);
int nxs_scene_medium(const nxs_scene *s, nx_medium *dst, int *has);
/* Extension: Scene::SetMediumDensity / ClearMediumDensity / GetMediumDensity — the fog's density grid, nz x ny x nx floats over the medium's
 * box with x fastest, copied; uploaded by the next device update under its own dirty flag (nxhip_set_medium_density, which validates the
 * values).  nxs_scene_medium_density: dims = (nx, ny, nz), all 0 while there is none; dst may be NULL (sizes only; dstCapacity in floats). */
int nxs_scene_set_medium_density(nxs_scene *s, const float *rho, uint32_t nx, uint32_t ny, uint32_t nz);
int nxs_scene_clear_medium_density(nxs_scene *s);
int nxs_scene_medium_density(const nxs_scene *s, uint32_t dims[3], float *dst, size_t dstCapacity);
/* IMGLoader::LoadNPYGrid on a file in memory: a NumPy .npy file, format 1.x or 2.x, '<f4', C order, 3-D shape (nz, ny, nx) — anything else is
 * refused with a message (nxs_last_error).  dims = (nx, ny, nz); dst may be NULL (sizes only; dstCapacity in floats). */
int nxh_decode_npy_grid(const uint8_t *data, size_t size, uint32_t dims[3], float *dst, size_t dstCapacity);
uint32_t nxs_scene_instance_count(const nxs_scene *s);

int nxs_pathtracer_create(uint32_t width, uint32_t height, int device, nxs_pathtracer **out);
void nxs_pathtracer_destroy(nxs_pathtracer *p);
int nxs_pathtracer_set_modes(nxs_pathtracer *p, int rngMode, int compactMode, int conductorMode);
/* PathTracer::SetFramesPerPass / SetPassesInFlight (extensions, include/nexus/PathTracer.h): frames per Render() call,
 * Render() calls in flight */
int nxs_pathtracer_set_frames_per_pass(nxs_pathtracer *p, uint32_t frames);
int nxs_pathtracer_set_passes_in_flight(nxs_pathtracer *p, uint32_t passes);
/* PathTracer::SetPixelOrder / SetEntryPoints (extensions): NXHIP_ORDER_* of the frame's paths; primary rays from their run's entry state */
int nxs_pathtracer_set_pixel_order(nxs_pathtracer *p, int order);
int nxs_pathtracer_set_entry_points(nxs_pathtracer *p, int on);
/* PathTracer::SetLightSampling (extension): NXHIP_LIGHTS_* — how the light sample chooses among the mesh lights' triangles */
int nxs_pathtracer_set_light_sampling(nxs_pathtracer *p, int mode);
/* PathTracer::SetLightImportance (extension): NXHIP_LIGHT_IMPORTANCE_* — in NXHIP_LIGHTS_POWER, whether the pick depends on the shading point */
int nxs_pathtracer_set_light_importance(nxs_pathtracer *p, int importance);
/* PathTracer::SetShadowTransmittance (extension): NXHIP_SHADOWS_* — whether opacity and texture alpha attenuate shadow rays */
int nxs_pathtracer_set_shadow_transmittance(nxs_pathtracer *p, int mode);
/* PathTracer::SetFeatureBuffers (extension): albedo / normal / depth of the camera ray's hit, accumulated like the colour (nxhip_set_aov) */
int nxs_pathtracer_set_feature_buffers(nxs_pathtracer *p, int on);
/* PathTracer::SetDeviceBlasBuild (extension, off by default): meshes added to `s` from now on get their BVH8 from the device
 * builder (nxhip_build_blas) instead of the host's; switch it off, or destroy the scene, before `p` goes away. */
int nxs_pathtracer_set_device_blas_build(nxs_pathtracer *p, nxs_scene *s, int enable);
/* Extension (skinned meshes) — PathTracer::PoseMesh for mesh `meshId`: an immediate call, made before nxs_scene_update.  The skin goes to
 * the device on first use, the device blends the vertices and refits the mesh's BLAS (nxhip_pose_blas), the posed root box comes back
 * for the instances' bounds; nxs_scene_update and nxs_pathtracer_update_device_scene then proceed as for a deformed mesh. */
int nxs_pathtracer_pose_mesh(nxs_pathtracer *p, nxs_scene *s, uint32_t meshId, const float *palette, uint32_t jointCount);
/* Extension (morph targets) — the PathTracer::PoseMesh overload that takes weights, for mesh `meshId`: one weight per target and, where
 * the mesh is skinned too, its palette (NULL and 0 for an unskinned mesh).  Morph and skin go to the device on first use; the device adds
 * the active targets' deltas, blends the joints and refits the BLAS in one pass (nxhip_pose_blas_morph).  Made before nxs_scene_update. */
int nxs_pathtracer_pose_mesh_morph(nxs_pathtracer *p, nxs_scene *s, uint32_t meshId, const float *weights, uint32_t targetCount, const float *palette, uint32_t jointCount);
int nxs_pathtracer_update_device_scene(nxs_pathtracer *p, nxs_scene *s);
int nxs_pathtracer_render(nxs_pathtracer *p, nxs_scene *s);
int nxs_pathtracer_reset_frame_number(nxs_pathtracer *p);
uint32_t nxs_pathtracer_frame_number(const nxs_pathtracer *p);
int nxs_pathtracer_read_pixels(nxs_pathtracer *p, uint32_t *rgba8);
struct nxhip_ctx *nxs_pathtracer_device_context(nxs_pathtracer *p);

/* Scene::AddHDRMap(filePath, fileName) — Scene/Scene.cpp:93-97: environment map from a Radiance .hdr (or .png) file. */
int nxs_scene_add_hdr_map_file(nxs_scene *s, const char *path, const char *fileName);
/* Extension — Scene::AddHDRMapFloat(filePath, fileName): a Radiance .hdr file as linear float radiance (IMGLoader::LoadHDRFloat:
 * component = mantissa x 2^(e - 136), e = 0: 0) instead of the 8 bits nxs_scene_add_hdr_map_file reduces it to. */
int nxs_scene_add_hdr_map_file_float(nxs_scene *s, const char *path, const char *fileName);
/* IMGLoader::LoadHDRFloat on a file in memory: *width / *height, and into dstRgb (may be NULL: sizes only; dstCapacity in floats)
 * width x height x 3 floats. */
int nxh_decode_hdr_float(const uint8_t *data, size_t size, uint32_t *width, uint32_t *height, float *dstRgb, size_t dstCapacity);

/* ---- nexus::Renderer (include/nexus/Renderer.h): the reference's frame driver without its window ---------------------
 * Renderer::Render (Renderer/Renderer.cpp:41-77): scene.Update() + ResetFrameNumber when the scene is invalid, then
 * UpdateDeviceScene + PathTracer::Render; SaveScreenshot (Renderer.cpp:183-215): PNG with rows flipped. */
typedef struct nxs_renderer nxs_renderer;
int nxs_renderer_create(uint32_t width, uint32_t height, nxs_scene *scene, int device, nxs_renderer **out);
void nxs_renderer_destroy(nxs_renderer *r);
int nxs_renderer_render(nxs_renderer *r, nxs_scene *scene, float deltaTime);
int nxs_renderer_reset(nxs_renderer *r);
int nxs_renderer_on_resize(nxs_renderer *r, uint32_t width, uint32_t height);
int nxs_renderer_save_screenshot(nxs_renderer *r, const char *path);
int nxs_renderer_save_exr(nxs_renderer *r, const char *path); /* extension: float accumulation as OpenEXR */
uint32_t nxs_renderer_frame_number(const nxs_renderer *r);
double nxs_renderer_megasamples_per_second(const nxs_renderer *r); /* MetricsPanel.cpp:28-56 */
struct nxhip_ctx *nxs_renderer_device_context(nxs_renderer *r);
int nxs_renderer_set_modes(nxs_renderer *r, int rngMode, int compactMode, int conductorMode);
/* Renderer::SetDenoise / SaveDenoisedEXR / SaveFeatureEXR (extensions, include/nexus/Renderer.h): with denoise on the screenshot is the
 * a-trous filtered image (nxhip_denoise); the feature buffers go to <stem>.albedo.exr, <stem>.normal.exr and <stem>.depth.exr */
int nxs_renderer_set_denoise(nxs_renderer *r, int on);
int nxs_renderer_save_denoised_exr(nxs_renderer *r, const char *path);
int nxs_renderer_save_feature_exr(nxs_renderer *r, const char *path);
/* Renderer::SetAdaptive / RenderAdaptive / SaveSampleCountEXR and PathTracer::SetAdaptive (extensions; adaptive sampling of the device
 * layer, include/nexus_hip.h: per-pixel noise statistics, a per-block stop rule, passes over the unsettled blocks).  params == NULL: off.
 * framesRendered (may be NULL): frames the call issued. */
int nxs_renderer_set_adaptive(nxs_renderer *r, const nx_adaptive_params *params);
int nxs_renderer_render_adaptive(nxs_renderer *r, nxs_scene *scene, uint32_t maxFrames, uint32_t interval, uint32_t *framesRendered);
int nxs_renderer_save_sample_count_exr(nxs_renderer *r, const char *path);
int nxs_pathtracer_set_adaptive(nxs_pathtracer *p, const nx_adaptive_params *params);
/* Image writers without stb: PNG (RGBA8; the reference's stbi_write_png) and OpenEXR (scanline, uncompressed, float32 B G R).
 * flipVertically != 0 writes the last row first (the render buffer's row 0 is the bottom of the viewport). */
int nxh_write_png(const char *path, const uint32_t *rgba8, uint32_t width, uint32_t height, int flipVertically);
int nxh_write_exr(const char *path, const float *rgb, uint32_t width, uint32_t height, int flipVertically);

#ifdef __cplusplus
}
#endif
#endif
