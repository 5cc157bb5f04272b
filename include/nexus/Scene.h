// nexus/Scene.h — the scene graph of the kept API surface: assets, placed mesh instances, derived lights, TLAS.
// Public methods of /root/reference/Nexus/src/Scene/Scene.h:17-76 (Scene.cpp:10-176).  Differences in kind, not in API:
// there are no device members here — PathTracer::UpdateDeviceScene pushes what changed through the C-ABI and uses the
// `*Dirty` flags below to know what that is — and the HDR map is handed over as pixels, not as a file to decode.
#pragma once

#include <memory>
#include <set>
#include <string>
#include <vector>

#include "Assets.h"
#include "Camera.h"
#include "RenderSettings.h"
#include "TLAS.h"

namespace nexus {

class Scene {
public:
    Scene(uint32_t width, uint32_t height);
    void Reset();

    // ---- building the scene ------------------------------------------------------------------------------------
    // Load a .glb / .obj through OBJLoader::LoadOBJ: one BVH8 per mesh, one instance per (node, primitive) — Scene.cpp:83-91
    void CreateMeshInstanceFromFile(const std::string& path, const std::string& fileName);
    // Extension, off by default: the files loaded from here on read a .glb's materials as glTF's own metallic-roughness model
    // (Material::Type::METALROUGH; OBJLoader.h LoadOptions::metalRough) instead of the reference's PLASTIC
    void SetMetalRoughMaterials(bool on) { m_MetalRoughMaterials = on; }
    bool GetMetalRoughMaterials() const { return m_MetalRoughMaterials; }
    // Extension, off by default: the files loaded from here on hand their materials' glTF alphaMode / alphaCutoff to the AssetManager
    // (OBJLoader.h LoadOptions::alphaModes; AssetManager::SetMaterialAlpha), and PathTracer::UpdateDeviceScene sends the table
    // (nxhip_set_material_alpha): MASK cutouts are holes for every ray, OPAQUE ignores an unused alpha channel.  Off: alpha blends.
    void SetMaterialAlphaModes(bool on) { m_MaterialAlphaModes = on; }
    bool GetMaterialAlphaModes() const { return m_MaterialAlphaModes; }
    // Extension, off by default: the files loaded from here on keep their glTF skins, joint animations and node tree (OBJLoader.h
    // LoadOptions::skins): Mesh::skin, GetAnimations(), GetNodes().  JointPalette evaluates a pose on the host in binary64 — it costs joints,
    // not vertices — and PathTracer::PoseMesh has the device blend the vertices and refit the mesh's BVH (nxhip_pose_blas).
    void SetSkins(bool on) { m_Skins = on; }
    bool GetSkins() const { return m_Skins; }
    // Extension, off by default: the files loaded from here on keep their glTF morph targets, the node tree and the animations with their
    // weights channels (OBJLoader.h LoadOptions::morphs): Mesh::morph.  MorphWeights evaluates the weights on the host, and the PoseMesh
    // overload that takes weights has the device blend the deltas — and the joints, on a skinned mesh — into the mesh's BVH.
    void SetMorphs(bool on) { m_Morphs = on; }
    bool GetMorphs() const { return m_Morphs; }
    // The weights of morphed mesh `meshId`: the file's defaults, or — where animation `animationIdx` (-1: none) has a weights channel on the
    // node that places the mesh — that channel sampled at time t by JointPalette's rule for STEP and LINEAR channels, in binary64, rounded
    // once.  The twin of nexus_amd/animation.py morph_weights.  Throws for a mesh without a morph or an animation that does not exist.
    std::vector<float> MorphWeights(uint32_t meshId, int animationIdx, double t) const;
    const std::vector<SceneNode>& GetNodes() const { return m_Nodes; }
    const std::vector<Animation>& GetAnimations() const { return m_Animations; }
    // (used by OBJLoader::LoadOBJ: a file's nodes and animations, their node indices already those of GetNodes())
    void AddNodes(const std::vector<SceneNode>& nodes) { m_Nodes.insert(m_Nodes.end(), nodes.begin(), nodes.end()); }
    void AddAnimation(const Animation& animation) { m_Animations.push_back(animation); }
    // The joint palette of skinned mesh `meshId` with animation `animationIdx` (-1: the rest pose) sampled at time t, clamped to each
    // channel's first and last key: jointCount x 12 floats, row j the row-major 3 x 4 matrix
    // inverse(meshNodeWorld) x jointWorld[j] x inverseBind[j] (glTF's formula; the instance's own matrix puts meshNodeWorld back), rounded
    // once to binary32.  STEP and LINEAR channels; rotations by shortest-arc slerp, normalised lerp when 1 - |q0 . q1| < 1e-9.  The twin of
    // nexus_amd/animation.py joint_palette.  Throws for a mesh without a skin or an animation that does not exist.
    std::vector<float> JointPalette(uint32_t meshId, int animationIdx, double t) const;
    // Place mesh `meshId` (AssetManager::AddMesh) with the mesh's own transform and material; a light is derived if its
    // material emits.  The returned reference is valid until the next instance is created.
    MeshInstance& CreateMeshInstance(uint32_t meshId);
    void AddMaterial(Material& material) { m_AssetManager.AddMaterial(material); }
    void AddHDRMap(const Texture& texture);
    void AddHDRMap(const std::string& filePath, const std::string& fileName);  // Scene.cpp:93-97: IMGLoader::LoadIMG (.hdr or .png)
    // Extension: the environment as linear float radiance (nxhip_upload_env_float) — a .hdr file decoded by IMGLoader::LoadHDRFloat, or
    // width x height x 3 floats, row 0 the top row.  Either kind of map replaces the other.
    void AddHDRMapFloat(const std::string& filePath, const std::string& fileName);
    void AddHDRMapFloat(uint32_t width, uint32_t height, const float* rgb);
    // Extension: the environment generated on the device from the sun-and-sky model (nx_sky, include/nexus_pod.h; the model is stated in
    // include/nexus_hip.h) by PathTracer::UpdateDeviceScene (nxhip_set_sky, which validates it).  It replaces a map of either kind and is
    // replaced by AddHDRMap / AddHDRMapFloat.  ClearSky: no environment (the textures are sent again without one).
    void SetSky(const nx_sky& sky);
    void ClearSky();
    const nx_sky* GetSky() const { return m_HasSky ? &m_Sky : nullptr; }  // nullptr: none
    size_t AddLight(const Light& light);
    void RemoveLight(size_t index);
    // Extension: lights that are no geometry (Assets.h AnalyticLight).  Sampled by the light sample only: invisible to camera and bounce rays.
    size_t AddAnalyticLight(const AnalyticLight& light);
    void RemoveAnalyticLight(size_t index);
    // Extension: fog (Assets.h Medium) — one homogeneous medium in a world-space box, uploaded by PathTracer::UpdateDeviceScene
    // (nxhip_set_medium, which validates it).  ClearMedium removes it: the device is then what it was without one.
    void SetMedium(const Medium& medium) { m_Medium = medium; m_HasMedium = true; mediumDirty = true; }
    void ClearMedium() { if (m_HasMedium) mediumDirty = true; m_HasMedium = false; }
    const Medium* GetMedium() const { return m_HasMedium ? &m_Medium : nullptr; }  // nullptr: none
    // Extension: the fog's density grid (Assets.h DensityGrid) — nz x ny x nx voxels over the medium's box, x fastest; the extinction at a
    // point becomes sigmaT x the trilinear lookup there.  Copied here, uploaded by PathTracer::UpdateDeviceScene under its own dirty flag
    // (nxhip_set_medium_density, which validates it); independent of SetMedium.  ClearMediumDensity: the medium is homogeneous again.
    void SetMediumDensity(const float* voxels, uint32_t nx, uint32_t ny, uint32_t nz)
    {
        m_MediumDensity.nx = nx; m_MediumDensity.ny = ny; m_MediumDensity.nz = nz;
        m_MediumDensity.voxels.assign(voxels, voxels + static_cast<size_t>(nx) * ny * nz);
        mediumDensityDirty = true;
    }
    void ClearMediumDensity() { if (!m_MediumDensity.voxels.empty()) mediumDensityDirty = true; m_MediumDensity = DensityGrid(); }
    const DensityGrid* GetMediumDensity() const { return m_MediumDensity.voxels.empty() ? nullptr : &m_MediumDensity; }  // nullptr: none

    // ---- editing: change a MeshInstance, then tell the scene which one --------------------------------------------
    std::vector<MeshInstance>& GetMeshInstances() { return m_MeshInstances; }
    void InvalidateMeshInstance(uint32_t instanceId) { m_InvalidMeshInstances.insert(instanceId); }
    void Invalidate() { m_Invalid = true; }
    // Extension, off by default: when only existing instances changed, refit the TLAS (O(n)) in Update() instead of the
    // reference's full agglomerative rebuild (Scene.cpp:29-55).
    void SetTlasRefit(bool enable) { m_TlasRefit = enable; }
    // Extension, off by default: leave the TLAS to the device.  Update() then builds no tree on the host when instances were
    // added or removed — PathTracer::UpdateDeviceScene has the device build it from the instances' world boxes
    // (nxhip_rebuild_tlas: the binned-SAH builder over the instance boxes, milliseconds where the reference's agglomerative
    // clustering takes seconds, and a tree rays enter fewer instances of) — and
    // moved instances are refitted on the device as with SetTlasRefit.  GetTLAS() holds no tree in this mode.
    void SetDeviceTlasBuild(bool enable) { m_DeviceTlas = enable; tlasDirty = true; }
    bool UsesDeviceTlasBuild() const { return m_DeviceTlas; }

    // ---- per frame -----------------------------------------------------------------------------------------------
    bool IsInvalid() const { return m_Invalid || !m_InvalidMeshInstances.empty() || m_Camera->IsInvalid() || m_AssetManager.IsInvalid(); }
    void Update();     // apply pending instance edits, refresh lights, bring the TLAS up to date
    void BuildTLAS();  // unconditional rebuild + BVH8 conversion

    // ---- read access ---------------------------------------------------------------------------------------------
    bool IsEmpty() const { return m_MeshInstances.empty(); }
    std::shared_ptr<Camera> GetCamera() const { return m_Camera; }
    std::shared_ptr<TLAS> GetTLAS() const { return m_Tlas; }
    AssetManager& GetAssetManager() { return m_AssetManager; }
    const AssetManager& GetAssetManager() const { return m_AssetManager; }
    std::vector<Material>& GetMaterials() { return m_AssetManager.GetMaterials(); }
    RenderSettings& GetRenderSettings() { return m_RenderSettings; }
    const RenderSettings& GetRenderSettings() const { return m_RenderSettings; }
    const std::vector<BVHInstance>& GetBVHInstances() const { return m_BVHInstances; }
    const std::vector<Light>& GetLights() const { return m_Lights; }
    const std::vector<AnalyticLight>& GetAnalyticLights() const { return m_AnalyticLights; }
    const Texture& GetHDRMap() const { return m_HdrMap; }
    const FloatImage& GetHDRMapFloat() const { return m_HdrMapFloat; }  // pixels empty: the map is GetHDRMap()'s, or there is none

    // what the device has not seen yet (set here, cleared by PathTracer::UpdateDeviceScene)
    mutable bool tlasDirty = true, lightsDirty = true, hdrDirty = false, analyticLightsDirty = false, mediumDirty = false, mediumDensityDirty = false;
    // With SetTlasRefit(true): BVH-instance ids whose transform (and nothing else) changed since the device last saw the TLAS.
    // PathTracer::UpdateDeviceScene hands them to nxhip_set_instance_transforms — inverse, bounds, traversal records and the
    // TLAS refit happen in HBM — instead of uploading the tree again.
    mutable std::vector<uint32_t> movedInstances;

private:
    // derive / drop the MESH_LIGHT of instance `index` from its material (Scene.cpp:142-176)
    void UpdateInstanceLighting(size_t index);

    AssetManager m_AssetManager;
    RenderSettings m_RenderSettings;
    std::shared_ptr<Camera> m_Camera;
    Texture m_HdrMap;
    FloatImage m_HdrMapFloat;
    nx_sky m_Sky{};
    bool m_HasSky = false;

    std::vector<MeshInstance> m_MeshInstances;  // what the user edits
    std::vector<BVHInstance> m_BVHInstances;    // what the TLAS and the device see, one per mesh instance
    std::vector<Light> m_Lights;
    std::vector<AnalyticLight> m_AnalyticLights;
    Medium m_Medium;
    bool m_HasMedium = false;
    bool m_MetalRoughMaterials = false;
    bool m_MaterialAlphaModes = false;
    bool m_Skins = false;
    bool m_Morphs = false;
    std::vector<SceneNode> m_Nodes;
    std::vector<Animation> m_Animations;
    DensityGrid m_MediumDensity;
    std::shared_ptr<TLAS> m_Tlas;

    std::set<uint32_t> m_InvalidMeshInstances;
    bool m_Invalid = true;
    bool m_TlasRefit = false;
    bool m_DeviceTlas = false;
    size_t m_TlasBuiltFor = 0;  // instance count of the last full TLAS build
};

}  // namespace nexus
