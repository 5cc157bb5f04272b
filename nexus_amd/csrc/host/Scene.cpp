// Scene.cpp — see include/nexus/Scene.h.  Behaviour of /root/reference/Nexus/src/Scene/Scene.cpp:10-176: default camera
// (0,4,14) looking down -z, 60 degree horizontal FOV, focus 5; an instance becomes a MESH_LIGHT when its material has an
// emissive map or intensity * max(emissive) > 0; the TLAS is rebuilt whenever an instance changed.
#include "nexus/Scene.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "nexus/IMGLoader.h"
#include "nexus/OBJLoader.h"

namespace nexus {

Scene::Scene(uint32_t width, uint32_t height)
    : m_Camera(std::make_shared<Camera>(make_float3(0.0f, 4.0f, 14.0f), make_float3(0.0f, 0.0f, -1.0f), 60.0f, width, height, 5.0f, 0.0f))
{
}

void Scene::Reset()
{
    m_Invalid = true;
    m_BVHInstances.clear();
    m_InvalidMeshInstances.clear();
    m_MeshInstances.clear();
    m_Lights.clear();
    if (!m_AnalyticLights.empty()) analyticLightsDirty = true;  // (the device must hear that they are gone)
    m_AnalyticLights.clear();
    ClearMedium();
    ClearMediumDensity();
    m_AssetManager.Reset();
    m_Nodes.clear();
    m_Animations.clear();
    m_Camera->Invalidate();
    m_TlasBuiltFor = 0;
    tlasDirty = lightsDirty = true;
}

// Scene::Update — Scene.cpp:29-55: push pending instance edits into the BVH instances, refresh lights, then bring the TLAS
// up to date (a full agglomerative rebuild as in the reference, or the O(n) refit extension when only existing instances
// changed and it is enabled).
void Scene::Update()
{
    m_Camera->SetInvalid(false);
    m_AssetManager.SendDataToDevice();
    // Deformed meshes (AssetManager::UpdateMeshTriangles refitted their BVH8): their instances are placed again, as they are —
    // SetTransform below re-derives the world bounds from the new root frame — and the TLAS follows by the mode in force.
    for (const int32_t bvhId : m_AssetManager.TakeDeformedBvhs())
        for (size_t id = 0; id < m_MeshInstances.size(); id++) {
            const BVHInstance& placed = m_BVHInstances[static_cast<size_t>(m_MeshInstances[id].bvhInstanceIdx)];
            if (m_AssetManager.GetMeshes()[placed.GetBvhIdx()].bvhId == bvhId) m_InvalidMeshInstances.insert(static_cast<uint32_t>(id));
        }
    if (m_InvalidMeshInstances.empty()) {
        m_Invalid = false;
        return;
    }

    const std::vector<Mesh>& meshes = m_AssetManager.GetMeshes();
    std::vector<BVH8>& blases = m_AssetManager.GetBVHs();
    std::vector<uint32_t> moved;
    bool onlyTransforms = true;  // nothing but the placement of existing instances changed
    for (const uint32_t id : m_InvalidMeshInstances) {
        const MeshInstance& edited = m_MeshInstances[id];
        BVHInstance& placed = m_BVHInstances[static_cast<size_t>(edited.bvhInstanceIdx)];
        placed.SetBvh(&blases[static_cast<size_t>(meshes[placed.GetBvhIdx()].bvhId)]);  // the vector may have grown since
        placed.SetTransform(edited.position, edited.rotation, edited.scale);
        moved.push_back(static_cast<uint32_t>(edited.bvhInstanceIdx));
        if (edited.materialId == -1) continue;
        if (placed.GetMaterialId() != edited.materialId) onlyTransforms = false;
        placed.AssignMaterial(edited.materialId);
        UpdateInstanceLighting(id);
    }
    m_InvalidMeshInstances.clear();

    const bool sameInstances = m_TlasBuiltFor == m_BVHInstances.size();
    if (m_DeviceTlas) {
        // the tree lives on the device only: same instances moved -> refit there; anything else -> rebuilt there
        if (sameInstances && onlyTransforms && !tlasDirty) movedInstances.insert(movedInstances.end(), moved.begin(), moved.end());
        else {
            tlasDirty = true;
            movedInstances.clear();
        }
        m_TlasBuiltFor = m_BVHInstances.size();
        m_Invalid = false;
        return;
    }
    if (!m_Tlas) m_Tlas = std::make_shared<TLAS>(m_BVHInstances);
    m_Tlas->SetBVHInstances(m_BVHInstances);
    if (m_TlasRefit && sameInstances && m_Tlas->Refit()) {
        // the host copy of the tree is refitted too (O(n)), so that it stays what the device holds; the device is told
        // only which instances moved, unless it has yet to see this tree at all
        if (onlyTransforms && !tlasDirty) movedInstances.insert(movedInstances.end(), moved.begin(), moved.end());
        else tlasDirty = true;
    } else {
        m_Tlas->Build();
        m_Tlas->Convert();
        m_TlasBuiltFor = m_BVHInstances.size();
        tlasDirty = true;
    }
    if (tlasDirty) movedInstances.clear();
    m_Invalid = false;
}

void Scene::BuildTLAS()
{
    m_Tlas = std::make_shared<TLAS>(m_BVHInstances);
    m_Tlas->Build();
    m_Tlas->Convert();
    m_TlasBuiltFor = m_BVHInstances.size();
    tlasDirty = true;
}

MeshInstance& Scene::CreateMeshInstance(uint32_t meshId)
{
    const Mesh& mesh = m_AssetManager.GetMeshes()[meshId];
    const BVH8& bvh8 = m_AssetManager.GetBVHs()[mesh.bvhId];
    m_BVHInstances.push_back(BVHInstance(meshId, &bvh8));  // bvhIdx := meshId, as the reference (Scene.cpp:69)
    m_MeshInstances.push_back(MeshInstance(mesh, static_cast<int>(m_BVHInstances.size()) - 1, mesh.materialId));
    const size_t instanceId = m_MeshInstances.size() - 1;
    UpdateInstanceLighting(instanceId);
    InvalidateMeshInstance(static_cast<uint32_t>(instanceId));
    return m_MeshInstances[instanceId];
}

void Scene::CreateMeshInstanceFromFile(const std::string& path, const std::string& fileName)
{
    LoadOptions options;
    options.metalRough = m_MetalRoughMaterials;
    options.alphaModes = m_MaterialAlphaModes;
    options.skins = m_Skins;
    options.morphs = m_Morphs;
    OBJLoader::LoadOBJ(path, fileName, this, &m_AssetManager, options);
    Invalidate();  // the TLAS is rebuilt by the next Update()
}

// ---- pose evaluation (skinned meshes): binary64 throughout, one rounding at the end ---------------------------------------------
namespace {

struct D4 {
    double m[4][4];
};

D4 d4_identity()
{
    D4 r;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) r.m[i][j] = i == j ? 1.0 : 0.0;
    return r;
}

D4 d4_mul(const D4& a, const D4& b)
{
    D4 r;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int k = 0; k < 4; k++) s += a.m[i][k] * b.m[k][j];
            r.m[i][j] = s;
        }
    return r;
}

// Gauss-Jordan with partial pivoting; throws on a singular matrix (a mesh node scaled to nothing cannot carry a skin)
D4 d4_inverse(const D4& a)
{
    double w[4][8];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            w[i][j] = a.m[i][j];
            w[i][4 + j] = i == j ? 1.0 : 0.0;
        }
    for (int c = 0; c < 4; c++) {
        int p = c;
        for (int r = c + 1; r < 4; r++)
            if (std::fabs(w[r][c]) > std::fabs(w[p][c])) p = r;
        if (w[p][c] == 0.0) throw std::runtime_error("Scene::JointPalette: the mesh node's world matrix is singular");
        if (p != c)
            for (int j = 0; j < 8; j++) std::swap(w[p][j], w[c][j]);
        const double d = w[c][c];
        for (int j = 0; j < 8; j++) w[c][j] /= d;
        for (int r = 0; r < 4; r++) {
            if (r == c) continue;
            const double f = w[r][c];
            if (f == 0.0) continue;
            for (int j = 0; j < 8; j++) w[r][j] -= f * w[c][j];
        }
    }
    D4 out;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) out.m[i][j] = w[i][4 + j];
    return out;
}

void quat_normalise(double q[4])
{
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 4; k++) q[k] /= n;
}

// a channel's value at time t, clamped to its first and last key (out: 4 doubles; a weights channel: one per target)
void sample_channel(const AnimationChannel& c, double t, double* out)
{
    const size_t keys = c.times.size();
    const int width = c.path == AnimationChannel::ROTATION ? 4 : c.path == AnimationChannel::WEIGHTS ? static_cast<int>(c.values.size() / keys) : 3;
    auto key = [&](size_t k, double* v) {
        for (int d = 0; d < width; d++) v[d] = c.values[static_cast<size_t>(width) * k + static_cast<size_t>(d)];
    };
    if (t <= c.times.front()) return key(0, out);
    if (t >= c.times.back()) return key(keys - 1, out);
    const size_t i = static_cast<size_t>(std::upper_bound(c.times.begin(), c.times.end(), t) - c.times.begin()) - 1;  // times[i] <= t < times[i + 1]
    if (c.step) return key(i, out);
    const double u = (t - c.times[i]) / (c.times[i + 1] - c.times[i]);
    if (c.path != AnimationChannel::ROTATION) {
        const double* a = c.values.data() + static_cast<size_t>(width) * i;
        const double* b = a + width;
        for (int d = 0; d < width; d++) out[d] = (1.0 - u) * a[d] + u * b[d];
        return;
    }
    double a[4], b[4];
    key(i, a);
    key(i + 1, b);
    // shortest-arc slerp; a normalised lerp where the arc is too short to divide by its sine
    double dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
    if (dot < 0.0) {
        dot = -dot;
        for (int d = 0; d < 4; d++) b[d] = -b[d];
    }
    if (1.0 - dot < 1e-9) {
        for (int d = 0; d < 4; d++) out[d] = (1.0 - u) * a[d] + u * b[d];
    } else {
        const double theta = std::acos(std::min(dot, 1.0));
        const double sa = std::sin((1.0 - u) * theta), sb = std::sin(u * theta), s = std::sin(theta);
        for (int d = 0; d < 4; d++) out[d] = (sa * a[d] + sb * b[d]) / s;
    }
    quat_normalise(out);
}

}  // namespace

std::vector<float> Scene::JointPalette(uint32_t meshId, int animationIdx, double t) const
{
    const std::vector<Mesh>& meshes = const_cast<AssetManager&>(m_AssetManager).GetMeshes();
    if (meshId >= meshes.size() || !meshes[meshId].skin) throw std::runtime_error("Scene::JointPalette: no such mesh, or the mesh has no skin");
    if (animationIdx < -1 || animationIdx >= static_cast<int>(m_Animations.size())) throw std::runtime_error("Scene::JointPalette: no such animation");
    const Skin& skin = *meshes[meshId].skin;
    // local TRS of every node: the rest pose, then what the animation's channels say at t
    struct Trs {
        double t[3], r[4], s[3];
        bool animated = false;
    };
    std::vector<Trs> trs(m_Nodes.size());
    for (size_t i = 0; i < m_Nodes.size(); i++) {
        std::copy(m_Nodes[i].translation, m_Nodes[i].translation + 3, trs[i].t);
        std::copy(m_Nodes[i].rotation, m_Nodes[i].rotation + 4, trs[i].r);
        std::copy(m_Nodes[i].scale, m_Nodes[i].scale + 3, trs[i].s);
    }
    if (animationIdx >= 0)
        for (const AnimationChannel& c : m_Animations[static_cast<size_t>(animationIdx)].channels) {
            if (c.path == AnimationChannel::WEIGHTS) continue;  // (MorphWeights)
            Trs& n = trs[static_cast<size_t>(c.node)];
            double v[4] = {0, 0, 0, 0};
            sample_channel(c, t, v);
            std::copy(v, v + (c.path == AnimationChannel::ROTATION ? 4 : 3), c.path == AnimationChannel::TRANSLATION ? n.t : c.path == AnimationChannel::ROTATION ? n.r : n.s);
            n.animated = true;
        }
    auto local = [&](size_t i) {
        D4 m = d4_identity();
        if (m_Nodes[i].hasMatrix && !trs[i].animated) {
            for (int a = 0; a < 4; a++)
                for (int b = 0; b < 4; b++) m.m[a][b] = m_Nodes[i].matrix[4 * a + b];
            return m;
        }
        double q[4] = {trs[i].r[0], trs[i].r[1], trs[i].r[2], trs[i].r[3]};
        quat_normalise(q);
        const double x = q[0], y = q[1], z = q[2], w = q[3];
        const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                                {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                                {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) m.m[a][b] = R[a][b] * trs[i].s[b];
            m.m[a][3] = trs[i].t[a];
        }
        return m;
    };
    std::vector<D4> world(m_Nodes.size());
    std::vector<char> done(m_Nodes.size(), 0);
    auto resolve = [&](size_t i) {
        // (iterative: up to the first resolved ancestor, then back down)
        std::vector<size_t> chain;
        for (size_t at = i; !done[at]; at = static_cast<size_t>(m_Nodes[at].parent)) {
            chain.push_back(at);
            if (m_Nodes[at].parent < 0) break;
            if (chain.size() > m_Nodes.size()) throw std::runtime_error("Scene::JointPalette: the node tree has a cycle");
        }
        for (size_t k = chain.size(); k-- > 0;) {
            const size_t at = chain[k];
            world[at] = m_Nodes[at].parent < 0 ? local(at) : d4_mul(world[static_cast<size_t>(m_Nodes[at].parent)], local(at));
            done[at] = 1;
        }
    };
    resolve(static_cast<size_t>(skin.meshNode));
    const D4 toMesh = d4_inverse(world[static_cast<size_t>(skin.meshNode)]);
    std::vector<float> palette(skin.joints.size() * 12);
    for (size_t k = 0; k < skin.joints.size(); k++) {
        resolve(static_cast<size_t>(skin.joints[k]));
        D4 ibm;
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) ibm.m[a][b] = skin.inverseBind[16 * k + 4 * static_cast<size_t>(a) + static_cast<size_t>(b)];
        const D4 m = d4_mul(d4_mul(toMesh, world[static_cast<size_t>(skin.joints[k])]), ibm);
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 4; b++) palette[12 * k + 4 * static_cast<size_t>(a) + static_cast<size_t>(b)] = static_cast<float>(m.m[a][b]);
    }
    return palette;
}

std::vector<float> Scene::MorphWeights(uint32_t meshId, int animationIdx, double t) const
{
    const std::vector<Mesh>& meshes = const_cast<AssetManager&>(m_AssetManager).GetMeshes();
    if (meshId >= meshes.size() || !meshes[meshId].morph) throw std::runtime_error("Scene::MorphWeights: no such mesh, or the mesh has no morph targets");
    if (animationIdx < -1 || animationIdx >= static_cast<int>(m_Animations.size())) throw std::runtime_error("Scene::MorphWeights: no such animation");
    const Morph& morph = *meshes[meshId].morph;
    if (animationIdx >= 0)
        for (const AnimationChannel& c : m_Animations[static_cast<size_t>(animationIdx)].channels) {
            if (c.path != AnimationChannel::WEIGHTS || c.node != morph.meshNode) continue;
            if (c.values.size() != c.times.size() * morph.targets) throw std::runtime_error("Scene::MorphWeights: the weights channel does not have one value per target and key");
            std::vector<double> w(std::max<size_t>(morph.targets, 4));
            sample_channel(c, t, w.data());
            std::vector<float> out(morph.targets);
            for (size_t k = 0; k < out.size(); k++) out[k] = static_cast<float>(w[k]);
            return out;
        }
    return morph.weights;
}

void Scene::SetSky(const nx_sky& sky)
{
    m_Sky = sky;
    m_HasSky = true;
    m_HdrMap = Texture();
    m_HdrMapFloat = FloatImage();
    hdrDirty = true;
}

void Scene::ClearSky()
{
    if (!m_HasSky) return;
    m_HasSky = false;
    m_AssetManager.texturesDirty = true;  // (only nxhip_clear_textures removes an environment: the textures go up again, without one)
    hdrDirty = true;
}

void Scene::AddHDRMap(const Texture& texture)
{
    m_HdrMap = texture;
    m_HdrMapFloat = FloatImage();
    m_HasSky = false;
    hdrDirty = true;
}

void Scene::AddHDRMapFloat(uint32_t width, uint32_t height, const float* rgb)
{
    if (!rgb || width == 0 || height == 0) throw std::runtime_error("Scene::AddHDRMapFloat: empty image");
    m_HdrMapFloat.width = width;
    m_HdrMapFloat.height = height;
    m_HdrMapFloat.pixels.assign(rgb, rgb + static_cast<size_t>(width) * height * 3);
    m_HdrMap = Texture();
    m_HasSky = false;
    hdrDirty = true;
}

void Scene::AddHDRMapFloat(const std::string& filePath, const std::string& fileName)
{
    const FloatImage img = IMGLoader::LoadHDRFloat(filePath + fileName);
    AddHDRMapFloat(img.width, img.height, img.pixels.data());
}

void Scene::AddHDRMap(const std::string& filePath, const std::string& fileName) { AddHDRMap(IMGLoader::LoadIMG(filePath + fileName)); }

size_t Scene::AddLight(const Light& light)
{
    m_Lights.push_back(light);
    lightsDirty = true;
    return m_Lights.size() - 1;
}

size_t Scene::AddAnalyticLight(const AnalyticLight& light)
{
    m_AnalyticLights.push_back(light);
    analyticLightsDirty = true;
    return m_AnalyticLights.size() - 1;
}

void Scene::RemoveAnalyticLight(size_t index)
{
    if (index >= m_AnalyticLights.size()) throw std::out_of_range("Scene::RemoveAnalyticLight: no such light");
    m_AnalyticLights.erase(m_AnalyticLights.begin() + static_cast<std::ptrdiff_t>(index));
    analyticLightsDirty = true;
}

void Scene::RemoveLight(size_t index)
{
    m_Lights.erase(m_Lights.begin() + static_cast<std::ptrdiff_t>(index));
    lightsDirty = true;
}

namespace {

// Scene.cpp:142-176 in two predicates.  An instance *becomes* a light when its material has an emissive map or
// intensity * max(emissive) > 0; an existing light is *dropped* only when max(emissive * intensity) is exactly 0 (so a
// textured emitter with a black emissive factor keeps its light — the reference's asymmetry, kept).
bool starts_emitting(const Material& m) { return m.emissiveMapId != -1 || m.intensity * fmaxf(make_float3(m.emissive)) > 0.0f; }
bool stops_emitting(const Material& m) { return fmaxf(make_float3(m.emissive) * m.intensity) == 0.0f; }

}  // namespace

void Scene::UpdateInstanceLighting(size_t index)
{
    const int materialId = m_MeshInstances[index].materialId;
    if (materialId == -1) return;
    const Material& material = m_AssetManager.GetMaterials()[static_cast<size_t>(materialId)];

    size_t existing = m_Lights.size();
    for (size_t i = 0; i < m_Lights.size() && existing == m_Lights.size(); i++)
        if (m_Lights[i].type == NX_LIGHT_MESH && m_Lights[i].mesh.meshId == index) existing = i;

    if (existing != m_Lights.size()) {
        if (stops_emitting(material)) RemoveLight(existing);
    } else if (starts_emitting(material)) {
        Light meshLight;
        meshLight.type = NX_LIGHT_MESH;
        meshLight.mesh.meshId = static_cast<uint32_t>(index);
        AddLight(meshLight);
    }
}

}  // namespace nexus
