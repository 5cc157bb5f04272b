// nexus/Assets.h — Material, Texture, Mesh, MeshInstance, Light, AssetManager of the kept API surface.
// Mirrors /root/reference/Nexus/src/Assets/{Material.h:5-72, Texture.h:5-27, Mesh.h:9-32, AssetManager.h:13-63},
// Scene/{MeshInstance.h:6-42, Light.h:4-33}.  Host Material / Light share the device POD layout (the reference copies
// them raw: DeviceVector<Material, D_Material> with no ToDevice, AssetManager.h:55).
#pragma once

#include <functional>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "BVH8.h"
#include "Math.h"

namespace nexus {

struct Material : nx_material {
    enum struct Type : int8_t { DIFFUSE = NX_MAT_DIFFUSE, DIELECTRIC = NX_MAT_DIELECTRIC, PLASTIC = NX_MAT_PLASTIC, CONDUCTOR = NX_MAT_CONDUCTOR,
                                 METALROUGH = NX_MAT_METALROUGH };  // (an extension: glTF's metallic-roughness model, nexus_hip.h)
    Material()
    {
        std::memset(static_cast<nx_material*>(this), 0, sizeof(nx_material));
        opacity = 1.0f;
        diffuseMapId = -1;
        emissiveMapId = -1;
        type = NX_MAT_DIFFUSE;
    }
};
static_assert(sizeof(Material) == sizeof(nx_material), "Material must alias nx_material");

struct Light : nx_light {
    enum struct Type : int8_t { POINT_LIGHT = NX_LIGHT_POINT, AREA_LIGHT = NX_LIGHT_AREA, MESH_LIGHT = NX_LIGHT_MESH };
    Light() { std::memset(static_cast<nx_light*>(this), 0, sizeof(nx_light)); }
};
static_assert(sizeof(Light) == sizeof(nx_light), "Light must alias nx_light");

// Extension: a light that is no geometry — point, sphere, spot, sun (nx_analytic_light of nexus_pod.h; the sampling rule: nexus_hip.h).
// Scene::AddAnalyticLight places one; the .glb reader makes one of every KHR_lights_punctual light a node carries.
struct AnalyticLight : nx_analytic_light {
    AnalyticLight()
    {
        std::memset(static_cast<nx_analytic_light*>(this), 0, sizeof(nx_analytic_light));
        direction[2] = -1.0f;  // glTF's convention: a light looks down its node's -Z
        colour[0] = colour[1] = colour[2] = 1.0f;
        intensity = 1.0f;
        outerConeAngle = 0.78539816339744830962f;
    }
};
static_assert(sizeof(AnalyticLight) == sizeof(nx_analytic_light), "AnalyticLight must alias nx_analytic_light");

// Extension: fog — one homogeneous participating medium in a world-space box (nx_medium of nexus_pod.h; the rule: nexus_hip.h).
// Scene::SetMedium places it.  The default is a unit box of no extinction (sigmaT 0: no medium), white albedo, isotropic.
struct Medium : nx_medium {
    Medium()
    {
        std::memset(static_cast<nx_medium*>(this), 0, sizeof(nx_medium));
        boxMax[0] = boxMax[1] = boxMax[2] = 1.0f;
        albedo[0] = albedo[1] = albedo[2] = 1.0f;
    }
};
static_assert(sizeof(Medium) == sizeof(nx_medium), "Medium must alias nx_medium");

// Extension: the detail maps of one material (nx_material_detail of nexus_pod.h; the shading rule: nexus_hip.h).  Ids are those
// AssetManager::AddTexture returned for a NORMAL / a ROUGHNESS texture; -1: none.  AssetManager::SetMaterialDetail attaches one to a material.
struct MaterialDetail : nx_material_detail {
    MaterialDetail()
    {
        normalMapId = roughnessMapId = -1;
        normalScale = 1.0f;
        pad_ = 0u;
    }
};
static_assert(sizeof(MaterialDetail) == sizeof(nx_material_detail), "MaterialDetail must alias nx_material_detail");

struct Texture {
    // (NORMAL and ROUGHNESS hold linear data: a tangent-space normal map; glTF's metallic-roughness image, whose G channel is read)
    enum struct Type { DIFFUSE, ROUGHNESS, METALLIC, EMISSIVE, NORMAL };
    Texture() = default;
    Texture(uint32_t w, uint32_t h, uint32_t c, const unsigned char* d) : width(w), height(h), channels(c), pixels(d, d + static_cast<size_t>(w) * h * 4) {}
    uint32_t width = 0, height = 0, channels = 0;
    std::vector<unsigned char> pixels;  // RGBA8, row 0 first
    Type type = Type::DIFFUSE;
};

// A float image: linear RGB radiance, nothing clamped (IMGLoader::LoadHDRFloat, Scene::AddHDRMapFloat)
struct FloatImage {
    uint32_t width = 0, height = 0;
    std::vector<float> pixels;  // RGB, width x height x 3, row 0 first
};

// Extension: a fog density grid (Scene::SetMediumDensity, nxhip_set_medium_density; IMGLoader::LoadNPYGrid reads one from a .npy file):
// nz x ny x nx voxels over the medium's box, x fastest.  Empty: none.
struct DensityGrid {
    uint32_t nx = 0, ny = 0, nz = 0;
    std::vector<float> voxels;
};

// Extension (skinned meshes; the blending rule: nexus_hip.h, nxhip_pose_blas): the skin of one mesh as the .glb reader finds it
// (LoadOptions::skins) — per triangle corner four joints and weights, de-indexed like the positions; the skin's joints as indices into
// Scene::GetNodes(); their inverse bind matrices (row major, binary64); the node that carries the mesh.  Scene::JointPalette evaluates a
// pose from it, PathTracer::PoseMesh sends it to the device on first use.
struct Skin {
    std::vector<nx_skin_corner> corners;  // 3 per triangle: corner 3 i + v is vertex v of triangle i
    std::vector<int> joints;
    std::vector<double> inverseBind;      // 16 per joint
    int meshNode = -1;
    bool onDevice = false;                // nxhip_set_blas_skin has been called for the mesh's BLAS
};

// Extension (morph targets; the rule: nexus_hip.h, nxhip_pose_blas_morph): the blend shapes of one mesh as the .glb reader finds them
// (LoadOptions::morphs) — per target and triangle corner a position and a normal delta, de-indexed like the positions, target-major; the
// default weights (the placing node's, else the mesh's, else zeros); extras.targetNames; the node that carries the mesh.
// Scene::MorphWeights samples an animation's weights from it, PathTracer::PoseMesh sends it to the device on first use.
struct Morph {
    std::vector<nx_morph_corner> deltas;  // targets x (3 per triangle): record t x corners + 3 i + v is vertex v of triangle i under target t
    uint32_t targets = 0;
    std::vector<float> weights;           // one per target: the file's defaults
    std::vector<std::string> names;       // extras.targetNames, or empty
    int meshNode = -1;
    bool onDevice = false;                // nxhip_set_blas_morph has been called for the mesh's BLAS
};

// ... a node of a loaded file's tree (parent and rest TRS), and a joint animation as channels
struct SceneNode {
    std::string name;
    int parent = -1;  // index into Scene::GetNodes(); -1: a root
    double translation[3] = {0, 0, 0}, rotation[4] = {0, 0, 0, 1}, scale[3] = {1, 1, 1};
    bool hasMatrix = false;  // the file gave a matrix instead of a TRS: used as it is unless a channel animates the node
    double matrix[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // row major
};
struct AnimationChannel {
    enum Path { TRANSLATION = 0, ROTATION = 1, SCALE = 2, WEIGHTS = 3 };  // WEIGHTS: morph targets (LoadOptions::morphs only)
    int node = -1;
    Path path = TRANSLATION;
    bool step = false;            // STEP; else LINEAR (rotations: shortest-arc slerp).  CUBICSPLINE is read as LINEAR over the keys' values
    std::vector<double> times;    // ascending
    std::vector<double> values;   // 3 (4 for rotations; the target count for weights) per key
};
struct Animation {
    std::string name;
    std::vector<AnimationChannel> channels;
};

struct Mesh {
    Mesh() = default;
    Mesh(const std::string& n, int32_t bId = -1, int32_t mId = -1, float3 p = make_float3(0.0f), float3 r = make_float3(0.0f), float3 s = make_float3(1.0f))
        : bvhId(bId), position(p), rotation(r), scale(s), materialId(mId), name(n)
    {
    }
    int32_t bvhId = -1;
    float3 position = make_float3(0.0f), rotation = make_float3(0.0f), scale = make_float3(1.0f);
    int32_t materialId = -1;
    std::string name;
    std::shared_ptr<Skin> skin;  // empty: the mesh is not skinned
    std::shared_ptr<Morph> morph;  // empty: the mesh has no morph targets
};

struct MeshInstance {
    MeshInstance() = default;
    MeshInstance(const Mesh& mesh, int bvhInstIdx, int mId = -1)
        : name(mesh.name), bvhInstanceIdx(bvhInstIdx), materialId(mId), rotation(mesh.rotation), scale(mesh.scale), position(mesh.position)
    {
    }
    void SetPosition(float3 p) { position = p; }
    void SetScale(float s) { scale = make_float3(s); }
    void SetScale(float3 s) { scale = s; }
    void SetTransform(float3 p, float3 r, float3 s) { position = p; rotation = r; scale = s; }
    void AssignMaterial(int mId) { materialId = mId; }

    std::string name;
    int bvhInstanceIdx = 0;
    int materialId = -1;
    float3 rotation = make_float3(0.0f), scale = make_float3(1.0f), position = make_float3(0.0f);
};

class AssetManager {
public:
    void Reset();
    int32_t CreateBVH(const std::vector<Triangle>& triangles);  // BVH8Builder(tris).Init().Build(), or the installed builder
    // Extension: who builds a mesh's BVH8.  Default (empty): the host builder, as the reference.  PathTracer::SetDeviceBlasBuild
    // installs one that builds on the GPU (nxhip_build_blas) and returns the tree with deviceBlasId set; `index` is the id the
    // new BVH will have in GetBVHs().
    using BlasBuilder = std::function<BVH8(const std::vector<Triangle>& triangles, size_t index)>;
    void SetBlasBuilder(BlasBuilder builder) { m_BlasBuilder = std::move(builder); }
    // The BVHs of all meshes of a file at once (OBJLoader::LoadOBJ; the reference calls CreateBVH per aiMesh,
    // Assets/OBJLoader.cpp:213-239): returns the id of the first, the others follow.  With a batch builder installed
    // (PathTracer::SetDeviceBlasBuild: nxhip_build_blas_batch, one device build for the whole file) they are built together,
    // otherwise one by one through CreateBVH.  `firstIndex` is the id the first new BVH will have.
    using BlasBatchBuilder = std::function<std::vector<BVH8>(const std::vector<std::vector<Triangle>>& meshes, size_t firstIndex)>;
    void SetBlasBatchBuilder(BlasBatchBuilder builder) { m_BlasBatchBuilder = std::move(builder); }
    int32_t CreateBVHs(const std::vector<std::vector<Triangle>>& meshes);
    int32_t AddMesh(Mesh&& mesh);
    // Extension (deforming meshes; the reference builds a new BVH for a changed mesh, Assets/AssetManager.cpp:23-37): the same
    // triangles of BVH `bvhId`, in the same order, at new positions.  The host tree is refitted (BVH8::Refit); Scene::Update then
    // re-derives the world bounds of the mesh's instances and brings the TLAS up to date, and PathTracer::UpdateDeviceScene
    // sends the mesh through nxhip_update_blas — no new BLAS id, no new instances.  Throws on another triangle count.
    void UpdateMeshTriangles(int32_t bvhId, const std::vector<Triangle>& triangles);
    // Extension (skinned meshes): BVH `bvhId` was posed on the device (PathTracer::PoseMesh) and its root now encodes [lo, hi].
    // BVHInstance::SetTransform uses that box for the mesh's instances from here on, and the mesh joins the set Scene::Update consumes —
    // but NOT `deformedBvhs`: the host's triangles are the bind pose, and sending them would overwrite the pose.
    void SetPosedBounds(int32_t bvhId, const float lo[3], const float hi[3]);
    // BVH ids changed by UpdateMeshTriangles or SetPosedBounds since Scene::Update last asked (it re-places their instances)
    std::set<int32_t> TakeDeformedBvhs();
    void AddMaterial();
    int AddMaterial(const Material& material);
    std::vector<Material>& GetMaterials() { return m_Materials; }
    const std::vector<Material>& GetMaterials() const { return m_Materials; }
    void InvalidateMaterial(uint32_t index) { m_InvalidMaterials.insert(index); }
    std::vector<BVH8>& GetBVHs() { return m_Bvhs; }
    const std::vector<BVH8>& GetBVHs() const { return m_Bvhs; }
    std::vector<Mesh>& GetMeshes() { return m_Meshes; }
    int AddTexture(const Texture& texture);  // -1 if it has no pixels; id within its kind (diffuse / emissive / normal / roughness)
    // Extension: the detail maps of material `materialId` (throws on an id that does not exist).  GetMaterialDetails: one record per
    // material, in the materials' order — empty while no material was ever given one, or after ClearMaterialDetails (the device then
    // has no table at all: PathTracer::UpdateDeviceScene sends count 0).
    void SetMaterialDetail(int materialId, const MaterialDetail& detail);
    void ClearMaterialDetails();
    std::vector<MaterialDetail> GetMaterialDetails() const;
    // Extension: how the alpha of material `materialId` is read (nx_material_alpha: NX_ALPHA_BLEND / MASK + cutoff / OPAQUE; the rule:
    // nexus_hip.h, nxhip_set_material_alpha; throws on an id that does not exist).  GetMaterialAlphas: one record per material — materials
    // never given one are BLEND — or empty while no material was ever given one, or after ClearMaterialAlphas (count 0 on the device).
    void SetMaterialAlpha(int materialId, const nx_material_alpha& alpha);
    void ClearMaterialAlphas();
    std::vector<nx_material_alpha> GetMaterialAlphas() const;
    const std::vector<Texture>& GetNormalMaps() const { return m_NormalMaps; }
    const std::vector<Texture>& GetRoughnessMaps() const { return m_RoughnessMaps; }
    void ApplyTextureToMaterial(int materialId, int diffuseMapId);
    const std::vector<Texture>& GetDiffuseMaps() const { return m_DiffuseMaps; }
    const std::vector<Texture>& GetEmissiveMaps() const { return m_EmissiveMaps; }
    bool SendDataToDevice();  // clears the invalid-material set; returns whether anything changed
    bool IsInvalid() const { return !m_InvalidMaterials.empty() || !m_DeformedBvhs.empty(); }

    // what the device still has to receive (consumed by PathTracer::UpdateDeviceScene)
    bool materialsDirty = true, texturesDirty = true, detailsDirty = false, alphasDirty = false;
    size_t uploadedBvhs = 0;
    std::set<int32_t> deformedBvhs;  // changed by UpdateMeshTriangles and not yet sent through nxhip_update_blas

private:
    std::vector<Material> m_Materials;
    std::set<uint32_t> m_InvalidMaterials;
    std::set<int32_t> m_DeformedBvhs;
    std::vector<Texture> m_DiffuseMaps, m_EmissiveMaps;
    std::vector<Texture> m_NormalMaps, m_RoughnessMaps;
    std::vector<MaterialDetail> m_MaterialDetails;  // sparse: shorter than m_Materials while later materials have none
    std::vector<nx_material_alpha> m_MaterialAlphas;  // likewise
    std::vector<BVH8> m_Bvhs;
    std::vector<Mesh> m_Meshes;
    BlasBuilder m_BlasBuilder;
    BlasBatchBuilder m_BlasBatchBuilder;
};

}  // namespace nexus
