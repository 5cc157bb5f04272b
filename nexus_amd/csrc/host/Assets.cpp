// Assets.cpp — AssetManager (see include/nexus/Assets.h); behaviour of /root/reference/Nexus/src/Assets/AssetManager.cpp:12-116.
#include "nexus/Assets.h"

#include <stdexcept>

#include "nexus/BVH8Builder.h"

namespace nexus {

void AssetManager::Reset()
{
    m_Materials.clear();
    m_InvalidMaterials.clear();
    m_DiffuseMaps.clear();
    m_EmissiveMaps.clear();
    m_NormalMaps.clear();
    m_RoughnessMaps.clear();
    if (!m_MaterialDetails.empty()) detailsDirty = true;  // (the device must hear that the table is gone)
    m_MaterialDetails.clear();
    if (!m_MaterialAlphas.empty()) alphasDirty = true;
    m_MaterialAlphas.clear();
    m_Meshes.clear();
    m_Bvhs.clear();
    m_DeformedBvhs.clear();
    deformedBvhs.clear();
    uploadedBvhs = 0;
    materialsDirty = texturesDirty = true;
}

int32_t AssetManager::CreateBVH(const std::vector<Triangle>& triangles)
{
    if (m_BlasBuilder) {
        m_Bvhs.push_back(m_BlasBuilder(triangles, m_Bvhs.size()));
        return static_cast<int32_t>(m_Bvhs.size()) - 1;
    }
    BVH8Builder builder(triangles);
    builder.Init();
    m_Bvhs.push_back(builder.Build());
    return static_cast<int32_t>(m_Bvhs.size()) - 1;
}

int32_t AssetManager::CreateBVHs(const std::vector<std::vector<Triangle>>& meshes)
{
    const int32_t first = static_cast<int32_t>(m_Bvhs.size());
    if (m_BlasBatchBuilder && meshes.size() > 1) {
        std::vector<BVH8> built = m_BlasBatchBuilder(meshes, m_Bvhs.size());
        for (BVH8& b : built) m_Bvhs.push_back(std::move(b));
    } else {
        for (const std::vector<Triangle>& m : meshes) CreateBVH(m);
    }
    return first;
}

int32_t AssetManager::AddMesh(Mesh&& mesh)
{
    m_Meshes.push_back(std::move(mesh));
    return static_cast<int32_t>(m_Meshes.size()) - 1;
}

void AssetManager::UpdateMeshTriangles(int32_t bvhId, const std::vector<Triangle>& triangles)
{
    if (bvhId < 0 || static_cast<size_t>(bvhId) >= m_Bvhs.size()) throw std::runtime_error("AssetManager::UpdateMeshTriangles: no such BVH");
    BVH8& bvh = m_Bvhs[static_cast<size_t>(bvhId)];
    if (triangles.size() != bvh.triangleIdx.size()) throw std::runtime_error("AssetManager::UpdateMeshTriangles: the triangle count differs from the mesh's (a refit keeps the topology)");
    bvh.Refit(triangles);  // (nodes and the tree's copy of the triangles)
    bvh.posed = false;     // (the host's shape is the mesh's shape again)
    m_DeformedBvhs.insert(bvhId);
    deformedBvhs.insert(bvhId);
}

void AssetManager::SetPosedBounds(int32_t bvhId, const float lo[3], const float hi[3])
{
    if (bvhId < 0 || static_cast<size_t>(bvhId) >= m_Bvhs.size()) throw std::runtime_error("AssetManager::SetPosedBounds: no such BVH");
    BVH8& bvh = m_Bvhs[static_cast<size_t>(bvhId)];
    bvh.posed = true;
    for (int a = 0; a < 3; a++) { bvh.posedMin[a] = lo[a]; bvh.posedMax[a] = hi[a]; }
    m_DeformedBvhs.insert(bvhId);  // (Scene::Update re-places the instances; the triangles stay where they are: on the device)
}

std::set<int32_t> AssetManager::TakeDeformedBvhs()
{
    std::set<int32_t> out;
    out.swap(m_DeformedBvhs);
    return out;
}

void AssetManager::AddMaterial()
{
    Material material;
    material.diffuse.albedo[0] = material.diffuse.albedo[1] = material.diffuse.albedo[2] = 0.2f;
    AddMaterial(material);
}

int AssetManager::AddMaterial(const Material& material)
{
    m_Materials.push_back(material);
    materialsDirty = true;
    return static_cast<int>(m_Materials.size()) - 1;
}

int AssetManager::AddTexture(const Texture& texture)
{
    if (texture.pixels.empty()) return -1;
    texturesDirty = true;
    if (texture.type == Texture::Type::DIFFUSE) {
        m_DiffuseMaps.push_back(texture);
        return static_cast<int>(m_DiffuseMaps.size()) - 1;
    }
    if (texture.type == Texture::Type::EMISSIVE) {
        m_EmissiveMaps.push_back(texture);
        return static_cast<int>(m_EmissiveMaps.size()) - 1;
    }
    if (texture.type == Texture::Type::NORMAL) {
        m_NormalMaps.push_back(texture);
        return static_cast<int>(m_NormalMaps.size()) - 1;
    }
    if (texture.type == Texture::Type::ROUGHNESS) {
        m_RoughnessMaps.push_back(texture);
        return static_cast<int>(m_RoughnessMaps.size()) - 1;
    }
    return -1;
}

void AssetManager::SetMaterialDetail(int materialId, const MaterialDetail& detail)
{
    if (materialId < 0 || static_cast<size_t>(materialId) >= m_Materials.size()) throw std::runtime_error("AssetManager::SetMaterialDetail: no such material");
    if (m_MaterialDetails.size() <= static_cast<size_t>(materialId)) m_MaterialDetails.resize(static_cast<size_t>(materialId) + 1);
    m_MaterialDetails[static_cast<size_t>(materialId)] = detail;
    detailsDirty = true;
}

void AssetManager::ClearMaterialDetails()
{
    m_MaterialDetails.clear();
    detailsDirty = true;
}

std::vector<MaterialDetail> AssetManager::GetMaterialDetails() const
{
    std::vector<MaterialDetail> out = m_MaterialDetails;
    if (!out.empty()) out.resize(m_Materials.size());  // (materials added since carry no maps)
    return out;
}

void AssetManager::SetMaterialAlpha(int materialId, const nx_material_alpha& alpha)
{
    if (materialId < 0 || static_cast<size_t>(materialId) >= m_Materials.size()) throw std::runtime_error("AssetManager::SetMaterialAlpha: no such material");
    if (m_MaterialAlphas.size() <= static_cast<size_t>(materialId)) m_MaterialAlphas.resize(static_cast<size_t>(materialId) + 1, nx_material_alpha{NX_ALPHA_BLEND, 0.5f});
    m_MaterialAlphas[static_cast<size_t>(materialId)] = alpha;
    alphasDirty = true;
}

void AssetManager::ClearMaterialAlphas()
{
    m_MaterialAlphas.clear();
    alphasDirty = true;
}

std::vector<nx_material_alpha> AssetManager::GetMaterialAlphas() const
{
    std::vector<nx_material_alpha> out = m_MaterialAlphas;
    if (!out.empty()) out.resize(m_Materials.size(), nx_material_alpha{NX_ALPHA_BLEND, 0.5f});  // (materials added since blend)
    return out;
}

void AssetManager::ApplyTextureToMaterial(int materialId, int diffuseMapId)
{
    m_Materials[materialId].diffuseMapId = diffuseMapId;
    InvalidateMaterial(materialId);
}

bool AssetManager::SendDataToDevice()
{
    const bool invalid = !m_InvalidMaterials.empty();
    if (invalid) materialsDirty = true;
    m_InvalidMaterials.clear();
    return invalid;
}

}  // namespace nexus
