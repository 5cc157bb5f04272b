// nexus_scene_capi.cpp — flat C wrappers over nexus::Scene / nexus::PathTracer (see include/nexus_host.h).
#include <cstring>
#include <exception>
#include <memory>
#include <stdexcept>
#include <string>

#include "nexus/IMGLoader.h"
#include "nexus/OBJLoader.h"
#include "nexus/Renderer.h"
#include "nexus/PathTracer.h"
#include "nexus/Scene.h"
#include "nexus_host.h"

using namespace nexus;

struct nxs_scene {
    Scene scene;
    nxs_scene(uint32_t w, uint32_t h) : scene(w, h) {}
};
struct nxh_loaded_scene {
    LoadedScene ls;
};
struct nxs_pathtracer {
    PathTracer pt;
    nxs_pathtracer(uint32_t w, uint32_t h, int dev) : pt(w, h, dev) {}
};
struct nxs_renderer {
    Renderer r;
    nxs_renderer(uint32_t w, uint32_t h, Scene* s, int dev) : r(w, h, s, dev) {}
};

namespace {
thread_local std::string g_err;
template <typename F> int guarded(F&& f)
{
    try {
        f();
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return 1;
    }
}
}  // namespace

extern "C" {

const char* nxs_last_error(void) { return g_err.c_str(); }

int nxs_scene_create(uint32_t width, uint32_t height, nxs_scene** out)
{
    return guarded([&] { *out = new nxs_scene(width, height); });
}
void nxs_scene_destroy(nxs_scene* s) { delete s; }

int nxs_scene_add_material(nxs_scene* s, const nx_material* m, int32_t* materialId)
{
    return guarded([&] {
        Material mat;
        std::memcpy(static_cast<nx_material*>(&mat), m, sizeof(nx_material));
        const int id = s->scene.GetAssetManager().AddMaterial(mat);
        if (materialId) *materialId = id;
    });
}

int nxs_scene_add_texture(nxs_scene* s, int kind, const uint8_t* rgba8, uint32_t w, uint32_t h, int32_t* texId)
{
    return guarded([&] {
        Texture t(w, h, 4, rgba8);
        t.type = kind == 1 ? Texture::Type::EMISSIVE : kind == 3 ? Texture::Type::NORMAL : kind == 4 ? Texture::Type::ROUGHNESS : Texture::Type::DIFFUSE;
        const int id = s->scene.GetAssetManager().AddTexture(t);
        if (texId) *texId = id;
    });
}

int nxs_scene_set_hdr_map(nxs_scene* s, const uint8_t* rgba8, uint32_t w, uint32_t h)
{
    return guarded([&] { s->scene.AddHDRMap(Texture(w, h, 4, rgba8)); });
}

int nxs_scene_add_mesh(nxs_scene* s, const nx_triangle* tris, uint32_t triCount, int32_t materialId, int32_t* meshId)
{
    return guarded([&] {
        std::vector<Triangle> v;
        v.reserve(triCount);
        for (uint32_t i = 0; i < triCount; i++) v.emplace_back(tris[i]);
        AssetManager& am = s->scene.GetAssetManager();
        const int32_t bvhId = am.CreateBVH(v);
        const int32_t id = am.AddMesh(Mesh("mesh" + std::to_string(bvhId), bvhId, materialId));
        if (meshId) *meshId = id;
    });
}

int nxs_scene_create_instance(nxs_scene* s, uint32_t meshId, int32_t materialId, const float pos[3], const float rotDeg[3], const float scale[3],
                              int32_t* instanceId)
{
    return guarded([&] {
        MeshInstance& mi = s->scene.CreateMeshInstance(meshId);
        mi.AssignMaterial(materialId);
        mi.SetTransform(make_float3(pos), make_float3(rotDeg), make_float3(scale));
        if (instanceId) *instanceId = static_cast<int32_t>(s->scene.GetMeshInstances().size()) - 1;
    });
}

int nxs_scene_update_mesh(nxs_scene* s, uint32_t meshId, const nx_triangle* tris, uint32_t triCount)
{
    return guarded([&] {
        AssetManager& am = s->scene.GetAssetManager();
        if (!tris || meshId >= am.GetMeshes().size()) throw std::runtime_error("nxs_scene_update_mesh: no such mesh, or null triangles");
        std::vector<Triangle> v;
        v.reserve(triCount);
        for (uint32_t i = 0; i < triCount; i++) v.emplace_back(tris[i]);
        am.UpdateMeshTriangles(am.GetMeshes()[meshId].bvhId, v);
    });
}

int nxs_scene_assign_material(nxs_scene* s, uint32_t instanceId, int32_t materialId)
{
    return guarded([&] {
        if (instanceId >= s->scene.GetMeshInstances().size()) throw std::runtime_error("nxs_scene_assign_material: no such instance");
        s->scene.GetMeshInstances()[instanceId].AssignMaterial(materialId);
        s->scene.InvalidateMeshInstance(instanceId);
    });
}

int nxh_load_scene_file(const char* file, nxh_loaded_scene** out)
{
    return guarded([&] {
        if (!file || !out) throw std::runtime_error("nxh_load_scene_file: null argument");
        std::unique_ptr<nxh_loaded_scene> p(new nxh_loaded_scene);
        p->ls = OBJLoader::Parse(file);
        *out = p.release();
    });
}
int nxh_load_scene_file_ex(const char* file, uint32_t flags, nxh_loaded_scene** out)
{
    return guarded([&] {
        if (!file || !out) throw std::runtime_error("nxh_load_scene_file_ex: null argument");
        if (flags & ~(uint32_t)(NXH_LOAD_METAL_ROUGH | NXH_LOAD_ALPHA_MODES | NXH_LOAD_SKINS | NXH_LOAD_MORPHS)) throw std::runtime_error("nxh_load_scene_file_ex: unknown flag");
        std::unique_ptr<nxh_loaded_scene> p(new nxh_loaded_scene);
        LoadOptions options;
        options.metalRough = (flags & NXH_LOAD_METAL_ROUGH) != 0;
        options.alphaModes = (flags & NXH_LOAD_ALPHA_MODES) != 0;
        options.skins = (flags & NXH_LOAD_SKINS) != 0;
        options.morphs = (flags & NXH_LOAD_MORPHS) != 0;
        p->ls = OBJLoader::Parse(file, options);
        *out = p.release();
    });
}
void nxh_loaded_scene_free(nxh_loaded_scene* s) { delete s; }
uint32_t nxh_loaded_mesh_count(const nxh_loaded_scene* s) { return static_cast<uint32_t>(s->ls.meshes.size()); }
uint32_t nxh_loaded_mesh_triangle_count(const nxh_loaded_scene* s, uint32_t mesh)
{
    return mesh < s->ls.meshes.size() ? static_cast<uint32_t>(s->ls.meshes[mesh].size()) : 0u;
}
int nxh_loaded_mesh_triangles(const nxh_loaded_scene* s, uint32_t mesh, nx_triangle* dst)
{
    return guarded([&] {
        if (mesh >= s->ls.meshes.size() || !dst) throw std::runtime_error("nxh_loaded_mesh_triangles: bad arguments");
        for (size_t i = 0; i < s->ls.meshes[mesh].size(); i++) dst[i] = Triangle::ToDevice(s->ls.meshes[mesh][i]);
    });
}
uint32_t nxh_loaded_material_count(const nxh_loaded_scene* s) { return static_cast<uint32_t>(s->ls.materials.size()); }
int nxh_loaded_materials(const nxh_loaded_scene* s, nx_material* dst)
{
    return guarded([&] {
        if (!dst) throw std::runtime_error("nxh_loaded_materials: null destination");
        for (size_t i = 0; i < s->ls.materials.size(); i++) dst[i] = static_cast<const nx_material&>(s->ls.materials[i]);
    });
}
uint32_t nxh_loaded_instance_count(const nxh_loaded_scene* s) { return static_cast<uint32_t>(s->ls.instances.size()); }
int nxh_loaded_instances(const nxh_loaded_scene* s, nx_loaded_instance* dst)
{
    return guarded([&] {
        if (!dst) throw std::runtime_error("nxh_loaded_instances: null destination");
        for (size_t i = 0; i < s->ls.instances.size(); i++) {
            const LoadedInstance& in = s->ls.instances[i];
            dst[i].mesh = in.mesh;
            dst[i].material = in.material;
            store(dst[i].position, in.position);
            store(dst[i].rotation, in.rotation);
            store(dst[i].scale, in.scale);
        }
    });
}

uint32_t nxh_loaded_texture_count(const nxh_loaded_scene* s) { return static_cast<uint32_t>(s->ls.textures.size()); }
int nxh_loaded_texture_info(const nxh_loaded_scene* s, uint32_t index, uint32_t* width, uint32_t* height, int32_t* kind)
{
    return guarded([&] {
        if (index >= s->ls.textures.size()) throw std::runtime_error("nxh_loaded_texture_info: no such texture");
        const Texture& t = s->ls.textures[index];
        if (width) *width = t.width;
        if (height) *height = t.height;
        if (kind) *kind = t.type == Texture::Type::EMISSIVE ? 1 : 0;
    });
}
int nxh_loaded_texture_pixels(const nxh_loaded_scene* s, uint32_t index, uint8_t* dstRgba8)
{
    return guarded([&] {
        if (index >= s->ls.textures.size() || !dstRgba8) throw std::runtime_error("nxh_loaded_texture_pixels: bad argument");
        const Texture& t = s->ls.textures[index];
        std::memcpy(dstRgba8, t.pixels.data(), t.pixels.size());
    });
}
int nxh_loaded_material_textures(const nxh_loaded_scene* s, int32_t* diffuseTexture, int32_t* emissiveTexture)
{
    return guarded([&] {
        if (!diffuseTexture || !emissiveTexture) throw std::runtime_error("nxh_loaded_material_textures: null destination");
        for (size_t i = 0; i < s->ls.materials.size(); i++) {
            diffuseTexture[i] = s->ls.materialDiffuseTexture[i];
            emissiveTexture[i] = s->ls.materialEmissiveTexture[i];
        }
    });
}
uint32_t nxh_loaded_detail_texture_count(const nxh_loaded_scene* s) { return static_cast<uint32_t>(s->ls.detailTextures.size()); }
int nxh_loaded_detail_texture_info(const nxh_loaded_scene* s, uint32_t index, uint32_t* width, uint32_t* height, int32_t* kind)
{
    return guarded([&] {
        if (index >= s->ls.detailTextures.size()) throw std::runtime_error("nxh_loaded_detail_texture_info: no such texture");
        const Texture& t = s->ls.detailTextures[index];
        if (width) *width = t.width;
        if (height) *height = t.height;
        if (kind) *kind = t.type == Texture::Type::NORMAL ? 3 : 4;
    });
}
int nxh_loaded_detail_texture_pixels(const nxh_loaded_scene* s, uint32_t index, uint8_t* dstRgba8)
{
    return guarded([&] {
        if (index >= s->ls.detailTextures.size() || !dstRgba8) throw std::runtime_error("nxh_loaded_detail_texture_pixels: bad argument");
        const Texture& t = s->ls.detailTextures[index];
        std::memcpy(dstRgba8, t.pixels.data(), t.pixels.size());
    });
}
int nxh_loaded_material_detail(const nxh_loaded_scene* s, int32_t* normalTexture, int32_t* roughnessTexture, float* normalScale)
{
    return guarded([&] {
        if (!normalTexture || !roughnessTexture || !normalScale) throw std::runtime_error("nxh_loaded_material_detail: null destination");
        for (size_t i = 0; i < s->ls.materials.size(); i++) {
            normalTexture[i] = s->ls.materialNormalTexture[i];
            roughnessTexture[i] = s->ls.materialRoughnessTexture[i];
            normalScale[i] = s->ls.materialNormalScale[i];
        }
    });
}
int nxh_loaded_material_alpha(const nxh_loaded_scene* s, nx_material_alpha* dst, uint32_t capacity, uint32_t* count)
{
    return guarded([&] {
        if (!s || !count) throw std::runtime_error("nxh_loaded_material_alpha: null argument");
        *count = static_cast<uint32_t>(s->ls.materialAlpha.size());
        for (size_t i = 0; dst && i < s->ls.materialAlpha.size() && i < capacity; i++) dst[i] = s->ls.materialAlpha[i];
    });
}
uint32_t nxh_loaded_analytic_light_count(const nxh_loaded_scene* s) { return static_cast<uint32_t>(s->ls.analyticLights.size()); }
int nxh_loaded_analytic_lights(const nxh_loaded_scene* s, nx_analytic_light* dst)
{
    return guarded([&] {
        if (!dst) throw std::runtime_error("nxh_loaded_analytic_lights: null destination");
        for (size_t i = 0; i < s->ls.analyticLights.size(); i++) dst[i] = s->ls.analyticLights[i];
    });
}
int nxh_loaded_skin(const nxh_loaded_scene* s, uint32_t mesh, nx_skin_corner* dst, uint32_t capacity, uint32_t* cornerCount, uint32_t* jointCount)
{
    return guarded([&] {
        if (!s || !cornerCount || !jointCount || mesh >= s->ls.meshes.size()) throw std::runtime_error("nxh_loaded_skin: null argument, or no such mesh");
        const Skin* skin = mesh < s->ls.skins.size() ? s->ls.skins[mesh].get() : nullptr;
        *cornerCount = skin ? static_cast<uint32_t>(skin->corners.size()) : 0u;
        *jointCount = skin ? static_cast<uint32_t>(skin->joints.size()) : 0u;
        for (size_t i = 0; skin && dst && i < skin->corners.size() && i < capacity; i++) dst[i] = skin->corners[i];
    });
}
int nxh_loaded_morph(const nxh_loaded_scene* s, uint32_t mesh, nx_morph_corner* dst, uint32_t capacity, uint32_t* cornerCount, uint32_t* targetCount, float* defaultWeights)
{
    return guarded([&] {
        if (!s || !cornerCount || !targetCount || mesh >= s->ls.meshes.size()) throw std::runtime_error("nxh_loaded_morph: null argument, or no such mesh");
        const Morph* morph = mesh < s->ls.morphs.size() ? s->ls.morphs[mesh].get() : nullptr;
        *targetCount = morph ? morph->targets : 0u;
        *cornerCount = morph ? static_cast<uint32_t>(morph->deltas.size() / morph->targets) : 0u;
        for (size_t i = 0; morph && dst && i < morph->deltas.size() && i < capacity; i++) dst[i] = morph->deltas[i];
        for (size_t i = 0; morph && defaultWeights && i < morph->weights.size(); i++) defaultWeights[i] = morph->weights[i];
    });
}
uint32_t nxh_loaded_animation_count(const nxh_loaded_scene* s) { return static_cast<uint32_t>(s->ls.animations.size()); }
uint32_t nxh_loaded_warning_count(const nxh_loaded_scene* s) { return static_cast<uint32_t>(s->ls.warnings.size()); }
const char* nxh_loaded_warning(const nxh_loaded_scene* s, uint32_t index) { return index < s->ls.warnings.size() ? s->ls.warnings[index].c_str() : ""; }

int nxh_decode_png(const uint8_t* data, size_t size, uint32_t* width, uint32_t* height, uint32_t* channels, uint8_t* dstRgba8, size_t dstCapacity)
{
    return guarded([&] {
        if (!data || !width || !height) throw std::runtime_error("nxh_decode_png: null argument");
        const Texture t = IMGLoader::LoadIMG(data, size);
        *width = t.width;
        *height = t.height;
        if (channels) *channels = t.channels;
        if (dstRgba8) {
            if (dstCapacity < t.pixels.size()) throw std::runtime_error("nxh_decode_png: destination too small");
            std::memcpy(dstRgba8, t.pixels.data(), t.pixels.size());
        }
    });
}

int nxh_decode_hdr_float(const uint8_t* data, size_t size, uint32_t* width, uint32_t* height, float* dstRgb, size_t dstCapacity)
{
    return guarded([&] {
        if (!data || !width || !height) throw std::runtime_error("nxh_decode_hdr_float: null argument");
        const FloatImage img = IMGLoader::LoadHDRFloat(data, size);
        *width = img.width;
        *height = img.height;
        if (dstRgb) {
            if (dstCapacity < img.pixels.size()) throw std::runtime_error("nxh_decode_hdr_float: destination too small");
            std::memcpy(dstRgb, img.pixels.data(), img.pixels.size() * sizeof(float));
        }
    });
}

int nxs_scene_set_sky(nxs_scene* s, const nx_sky* sky)
{
    return guarded([&] {
        if (!sky) throw std::runtime_error("nxs_scene_set_sky: null argument");
        s->scene.SetSky(*sky);
    });
}

int nxs_scene_clear_sky(nxs_scene* s)
{
    return guarded([&] { s->scene.ClearSky(); });
}

int nxs_scene_set_hdr_map_float(nxs_scene* s, const float* rgb, uint32_t w, uint32_t h)
{
    return guarded([&] { s->scene.AddHDRMapFloat(w, h, rgb); });
}

int nxs_scene_add_hdr_map_file_float(nxs_scene* s, const char* path, const char* fileName)
{
    return guarded([&] {
        if (!path || !fileName) throw std::runtime_error("nxs_scene_add_hdr_map_file_float: null argument");
        s->scene.AddHDRMapFloat(path, fileName);
    });
}

int nxs_scene_set_instance_transform(nxs_scene* s, uint32_t instanceId, const float pos[3], const float rotDeg[3], const float scale[3])
{
    return guarded([&] {
        if (instanceId >= s->scene.GetMeshInstances().size()) throw std::runtime_error("nxs_scene_set_instance_transform: no such instance");
        s->scene.GetMeshInstances()[instanceId].SetTransform(make_float3(pos), make_float3(rotDeg), make_float3(scale));
        s->scene.InvalidateMeshInstance(instanceId);  // what the viewer's transform panel does (SceneHierarchyPanel.cpp)
    });
}

int nxs_scene_set_tlas_refit(nxs_scene* s, int enable)
{
    return guarded([&] { s->scene.SetTlasRefit(enable != 0); });
}

int nxs_scene_set_device_tlas(nxs_scene* s, int enable)
{
    return guarded([&] { s->scene.SetDeviceTlasBuild(enable != 0); });
}

int nxs_scene_load_file(nxs_scene* s, const char* path, const char* fileName)
{
    return guarded([&] {
        if (!path || !fileName) throw std::runtime_error("nxs_scene_load_file: null argument");
        s->scene.CreateMeshInstanceFromFile(path, fileName);
    });
}

int nxs_scene_set_metal_rough(nxs_scene* s, int on)
{
    return guarded([&] { s->scene.SetMetalRoughMaterials(on != 0); });
}

int nxs_scene_set_material_alpha_modes(nxs_scene* s, int on)
{
    return guarded([&] { s->scene.SetMaterialAlphaModes(on != 0); });
}
int nxs_scene_material_alphas(const nxs_scene* s, nx_material_alpha* dst, uint32_t capacity, uint32_t* count)
{
    return guarded([&] {
        if (!s || !count) throw std::runtime_error("nxs_scene_material_alphas: null argument");
        const std::vector<nx_material_alpha> a = s->scene.GetAssetManager().GetMaterialAlphas();
        *count = static_cast<uint32_t>(a.size());
        for (size_t i = 0; dst && i < a.size() && i < capacity; i++) dst[i] = a[i];
    });
}

int nxs_scene_set_skins(nxs_scene* s, int on)
{
    return guarded([&] { s->scene.SetSkins(on != 0); });
}
uint32_t nxs_scene_mesh_count(const nxs_scene* s) { return static_cast<uint32_t>(const_cast<nxs_scene*>(s)->scene.GetAssetManager().GetMeshes().size()); }
uint32_t nxs_scene_animation_count(const nxs_scene* s) { return static_cast<uint32_t>(s->scene.GetAnimations().size()); }
uint32_t nxs_scene_mesh_joint_count(const nxs_scene* s, uint32_t meshId)
{
    const std::vector<Mesh>& meshes = const_cast<nxs_scene*>(s)->scene.GetAssetManager().GetMeshes();
    return meshId < meshes.size() && meshes[meshId].skin ? static_cast<uint32_t>(meshes[meshId].skin->joints.size()) : 0u;
}
int nxs_scene_joint_palette(const nxs_scene* s, uint32_t meshId, int32_t animationIdx, double t, float* dst, uint32_t capacity, uint32_t* jointCount)
{
    return guarded([&] {
        if (!s || !jointCount) throw std::runtime_error("nxs_scene_joint_palette: null argument");
        const std::vector<float> p = s->scene.JointPalette(meshId, animationIdx, t);
        *jointCount = static_cast<uint32_t>(p.size() / 12);
        if (dst) {
            if (capacity < *jointCount) throw std::runtime_error("nxs_scene_joint_palette: destination too small");
            std::memcpy(dst, p.data(), p.size() * sizeof(float));
        }
    });
}

int nxs_scene_set_morphs(nxs_scene* s, int on)
{
    return guarded([&] { s->scene.SetMorphs(on != 0); });
}
uint32_t nxs_scene_mesh_target_count(const nxs_scene* s, uint32_t meshId)
{
    const std::vector<Mesh>& meshes = const_cast<nxs_scene*>(s)->scene.GetAssetManager().GetMeshes();
    return meshId < meshes.size() && meshes[meshId].morph ? meshes[meshId].morph->targets : 0u;
}
int nxs_scene_morph_weights(const nxs_scene* s, uint32_t meshId, int32_t animationIdx, double t, float* dst, uint32_t capacity, uint32_t* targetCount)
{
    return guarded([&] {
        if (!s || !targetCount) throw std::runtime_error("nxs_scene_morph_weights: null argument");
        const std::vector<float> w = s->scene.MorphWeights(meshId, animationIdx, t);
        *targetCount = static_cast<uint32_t>(w.size());
        if (dst) {
            if (capacity < w.size()) throw std::runtime_error("nxs_scene_morph_weights: destination too small");
            std::memcpy(dst, w.data(), w.size() * sizeof(float));
        }
    });
}

int nxs_scene_set_camera(nxs_scene* s, const float pos[3], const float forward[3], float hfov, float focusDist, float defocusAngle)
{
    return guarded([&] {
        Camera& c = *s->scene.GetCamera();
        c.LookAt(make_float3(pos), make_float3(forward));
        c.SetHorizontalFOV(hfov);
        c.GetFocusDist() = focusDist;
        c.GetDefocusAngle() = defocusAngle;
    });
}

int nxs_scene_set_render_settings(nxs_scene* s, const nx_render_settings* settings)
{
    return guarded([&] {
        std::memcpy(&s->scene.GetRenderSettings(), settings, sizeof(nx_render_settings));
        s->scene.Invalidate();
    });
}

int nxs_scene_update(nxs_scene* s)
{
    return guarded([&] { s->scene.Update(); });
}

int nxs_scene_set_material_detail(nxs_scene* s, int32_t materialId, const nx_material_detail* detail)
{
    return guarded([&] {
        if (!detail) throw std::runtime_error("nxs_scene_set_material_detail: null record");
        MaterialDetail d;
        static_cast<nx_material_detail&>(d) = *detail;
        s->scene.GetAssetManager().SetMaterialDetail(materialId, d);
    });
}
int nxs_scene_clear_material_details(nxs_scene* s) { return guarded([&] { s->scene.GetAssetManager().ClearMaterialDetails(); }); }
uint32_t nxs_scene_material_detail_count(const nxs_scene* s) { return static_cast<uint32_t>(s->scene.GetAssetManager().GetMaterialDetails().size()); }
int nxs_scene_material_details(const nxs_scene* s, nx_material_detail* dst, uint32_t capacity)
{
    return guarded([&] {
        const std::vector<MaterialDetail> d = s->scene.GetAssetManager().GetMaterialDetails();
        if (capacity < d.size() || (!dst && !d.empty())) throw std::runtime_error("nxs_scene_material_details: destination too small");
        for (size_t i = 0; i < d.size(); i++) dst[i] = d[i];
    });
}
uint32_t nxs_scene_light_count(const nxs_scene* s) { return static_cast<uint32_t>(s->scene.GetLights().size()); }
int nxs_scene_add_analytic_light(nxs_scene* s, const nx_analytic_light* light, uint32_t* index)
{
    return guarded([&] {
        if (!light) throw std::runtime_error("nxs_scene_add_analytic_light: null light");
        AnalyticLight l;
        static_cast<nx_analytic_light&>(l) = *light;
        const size_t at = s->scene.AddAnalyticLight(l);
        if (index) *index = static_cast<uint32_t>(at);
    });
}
int nxs_scene_remove_analytic_light(nxs_scene* s, uint32_t index) { return guarded([&] { s->scene.RemoveAnalyticLight(index); }); }
uint32_t nxs_scene_analytic_light_count(const nxs_scene* s) { return static_cast<uint32_t>(s->scene.GetAnalyticLights().size()); }
int nxs_scene_analytic_lights(const nxs_scene* s, nx_analytic_light* dst, uint32_t capacity)
{
    return guarded([&] {
        if (!dst && capacity) throw std::runtime_error("nxs_scene_analytic_lights: null destination");
        const std::vector<AnalyticLight>& al = s->scene.GetAnalyticLights();
        for (size_t i = 0; i < al.size() && i < capacity; i++) dst[i] = al[i];
    });
}
int nxs_scene_set_medium(nxs_scene* s, const nx_medium* medium)
{
    return guarded([&] {
        if (!medium) throw std::runtime_error("nxs_scene_set_medium: null medium (nxs_scene_clear_medium removes it)");
        Medium m;
        static_cast<nx_medium&>(m) = *medium;
        s->scene.SetMedium(m);
    });
}
int nxs_scene_clear_medium(nxs_scene* s) { return guarded([&] { s->scene.ClearMedium(); }); }
int nxs_scene_medium(const nxs_scene* s, nx_medium* dst, int* has)
{
    return guarded([&] {
        if (!has) throw std::runtime_error("nxs_scene_medium: null has");
        const Medium* m = s->scene.GetMedium();
        *has = m ? 1 : 0;
        if (m && dst) *dst = *m;
    });
}
int nxs_scene_set_medium_density(nxs_scene* s, const float* rho, uint32_t nx, uint32_t ny, uint32_t nz)
{
    return guarded([&] {
        if (!rho) throw std::runtime_error("nxs_scene_set_medium_density: null grid (nxs_scene_clear_medium_density removes it)");
        if (nx == 0 || ny == 0 || nz == 0 || nx > 512 || ny > 512 || nz > 512) throw std::runtime_error("nxs_scene_set_medium_density: every dimension must lie in 1 .. 512");
        s->scene.SetMediumDensity(rho, nx, ny, nz);
    });
}
int nxs_scene_clear_medium_density(nxs_scene* s) { return guarded([&] { s->scene.ClearMediumDensity(); }); }
int nxs_scene_medium_density(const nxs_scene* s, uint32_t dims[3], float* dst, size_t dstCapacity)
{
    return guarded([&] {
        if (!dims) throw std::runtime_error("nxs_scene_medium_density: null dims");
        const DensityGrid* g = s->scene.GetMediumDensity();
        dims[0] = g ? g->nx : 0u;
        dims[1] = g ? g->ny : 0u;
        dims[2] = g ? g->nz : 0u;
        if (g && dst) {
            if (dstCapacity < g->voxels.size()) throw std::runtime_error("nxs_scene_medium_density: destination too small");
            std::memcpy(dst, g->voxels.data(), g->voxels.size() * sizeof(float));
        }
    });
}
int nxh_decode_npy_grid(const uint8_t* data, size_t size, uint32_t dims[3], float* dst, size_t dstCapacity)
{
    return guarded([&] {
        if (!data || !dims) throw std::runtime_error("nxh_decode_npy_grid: null argument");
        const DensityGrid g = IMGLoader::LoadNPYGrid(data, size);
        dims[0] = g.nx;
        dims[1] = g.ny;
        dims[2] = g.nz;
        if (dst) {
            if (dstCapacity < g.voxels.size()) throw std::runtime_error("nxh_decode_npy_grid: destination too small");
            std::memcpy(dst, g.voxels.data(), g.voxels.size() * sizeof(float));
        }
    });
}
uint32_t nxs_scene_instance_count(const nxs_scene* s) { return static_cast<uint32_t>(s->scene.GetBVHInstances().size()); }

int nxs_pathtracer_create(uint32_t width, uint32_t height, int device, nxs_pathtracer** out)
{
    return guarded([&] { *out = new nxs_pathtracer(width, height, device); });
}
void nxs_pathtracer_destroy(nxs_pathtracer* p) { delete p; }
int nxs_pathtracer_set_modes(nxs_pathtracer* p, int rngMode, int compactMode, int conductorMode)
{
    return guarded([&] { p->pt.SetModes(rngMode, compactMode, conductorMode); });
}
int nxs_pathtracer_set_frames_per_pass(nxs_pathtracer* p, uint32_t frames) { return guarded([&] { p->pt.SetFramesPerPass(frames); }); }
int nxs_pathtracer_set_passes_in_flight(nxs_pathtracer* p, uint32_t passes) { return guarded([&] { p->pt.SetPassesInFlight(passes); }); }
int nxs_pathtracer_set_pixel_order(nxs_pathtracer* p, int order) { return guarded([&] { p->pt.SetPixelOrder(order); }); }
int nxs_pathtracer_set_entry_points(nxs_pathtracer* p, int on) { return guarded([&] { p->pt.SetEntryPoints(on != 0); }); }
int nxs_pathtracer_set_light_sampling(nxs_pathtracer* p, int mode) { return guarded([&] { p->pt.SetLightSampling(mode); }); }
int nxs_pathtracer_set_light_importance(nxs_pathtracer* p, int importance) { return guarded([&] { p->pt.SetLightImportance(importance); }); }
int nxs_pathtracer_set_shadow_transmittance(nxs_pathtracer* p, int mode) { return guarded([&] { p->pt.SetShadowTransmittance(mode); }); }
int nxs_pathtracer_set_feature_buffers(nxs_pathtracer* p, int on) { return guarded([&] { p->pt.SetFeatureBuffers(on != 0); }); }
int nxs_pathtracer_set_device_blas_build(nxs_pathtracer* p, nxs_scene* s, int enable)
{
    return guarded([&] { p->pt.SetDeviceBlasBuild(s->scene, enable != 0); });
}
int nxs_pathtracer_pose_mesh(nxs_pathtracer* p, nxs_scene* s, uint32_t meshId, const float* palette, uint32_t jointCount)
{
    return guarded([&] {
        if (!p || !s || !palette) throw std::runtime_error("nxs_pathtracer_pose_mesh: null argument");
        const std::vector<Mesh>& meshes = s->scene.GetAssetManager().GetMeshes();
        if (meshId >= meshes.size()) throw std::runtime_error("nxs_pathtracer_pose_mesh: no such mesh");
        p->pt.PoseMesh(s->scene, meshes[meshId].bvhId, std::vector<float>(palette, palette + static_cast<size_t>(jointCount) * 12));
    });
}
int nxs_pathtracer_pose_mesh_morph(nxs_pathtracer* p, nxs_scene* s, uint32_t meshId, const float* weights, uint32_t targetCount, const float* palette, uint32_t jointCount)
{
    return guarded([&] {
        if (!p || !s || !weights || (!palette && jointCount)) throw std::runtime_error("nxs_pathtracer_pose_mesh_morph: null argument");
        const std::vector<Mesh>& meshes = s->scene.GetAssetManager().GetMeshes();
        if (meshId >= meshes.size()) throw std::runtime_error("nxs_pathtracer_pose_mesh_morph: no such mesh");
        p->pt.PoseMesh(s->scene, meshes[meshId].bvhId, std::vector<float>(weights, weights + targetCount),
                       palette ? std::vector<float>(palette, palette + static_cast<size_t>(jointCount) * 12) : std::vector<float>());
    });
}
int nxs_pathtracer_update_device_scene(nxs_pathtracer* p, nxs_scene* s)
{
    return guarded([&] { p->pt.UpdateDeviceScene(s->scene); });
}
int nxs_pathtracer_render(nxs_pathtracer* p, nxs_scene* s)
{
    return guarded([&] { p->pt.Render(s->scene); });
}
int nxs_pathtracer_reset_frame_number(nxs_pathtracer* p)
{
    return guarded([&] { p->pt.ResetFrameNumber(); });
}
uint32_t nxs_pathtracer_frame_number(const nxs_pathtracer* p) { return p->pt.GetFrameNumber(); }
int nxs_pathtracer_read_pixels(nxs_pathtracer* p, uint32_t* rgba8)
{
    return guarded([&] {
        const std::vector<uint32_t>& px = p->pt.GetPixelBuffer();
        std::memcpy(rgba8, px.data(), px.size() * 4);
    });
}
struct nxhip_ctx* nxs_pathtracer_device_context(nxs_pathtracer* p) { return p->pt.GetDeviceContext(); }

int nxs_scene_add_hdr_map_file(nxs_scene* s, const char* path, const char* fileName)
{
    return guarded([&] {
        if (!path || !fileName) throw std::runtime_error("nxs_scene_add_hdr_map_file: null argument");
        s->scene.AddHDRMap(path, fileName);
    });
}

int nxs_renderer_create(uint32_t width, uint32_t height, nxs_scene* scene, int device, nxs_renderer** out)
{
    return guarded([&] {
        if (!scene || !out) throw std::runtime_error("nxs_renderer_create: null argument");
        *out = new nxs_renderer(width, height, &scene->scene, device);
    });
}
void nxs_renderer_destroy(nxs_renderer* r) { delete r; }
int nxs_renderer_render(nxs_renderer* r, nxs_scene* scene, float deltaTime)
{
    return guarded([&] { r->r.Render(scene->scene, deltaTime); });
}
int nxs_renderer_reset(nxs_renderer* r) { return guarded([&] { r->r.Reset(); }); }
int nxs_renderer_on_resize(nxs_renderer* r, uint32_t width, uint32_t height) { return guarded([&] { r->r.OnResize(width, height); }); }
int nxs_renderer_save_screenshot(nxs_renderer* r, const char* path)
{
    return guarded([&] {
        if (!path || !r->r.SaveScreenshot(path)) throw std::runtime_error(std::string("cannot write ") + (path ? path : "(null)"));
    });
}
int nxs_renderer_save_exr(nxs_renderer* r, const char* path)
{
    return guarded([&] {
        if (!path || !r->r.SaveAccumulationEXR(path)) throw std::runtime_error(std::string("cannot write ") + (path ? path : "(null)"));
    });
}
uint32_t nxs_renderer_frame_number(const nxs_renderer* r) { return r->r.GetFrameNumber(); }
double nxs_renderer_megasamples_per_second(const nxs_renderer* r) { return r->r.GetMegaSamplesPerSecond(); }
struct nxhip_ctx* nxs_renderer_device_context(nxs_renderer* r) { return r->r.GetPathTracer().GetDeviceContext(); }
int nxs_renderer_set_modes(nxs_renderer* r, int rngMode, int compactMode, int conductorMode)
{
    return guarded([&] { r->r.GetPathTracer().SetModes(rngMode, compactMode, conductorMode); });
}
int nxs_renderer_set_denoise(nxs_renderer* r, int on) { return guarded([&] { r->r.SetDenoise(on != 0); }); }
int nxs_renderer_save_denoised_exr(nxs_renderer* r, const char* path)
{
    return guarded([&] {
        if (!path || !r->r.SaveDenoisedEXR(path)) throw std::runtime_error(std::string("cannot write the denoised image to ") + (path ? path : "(null)") + " (is denoise on?)");
    });
}
int nxs_renderer_save_feature_exr(nxs_renderer* r, const char* path)
{
    return guarded([&] {
        if (!path || !r->r.SaveFeatureEXR(path)) throw std::runtime_error(std::string("cannot write the feature buffers to ") + (path ? path : "(null)") + " (are they on?)");
    });
}
int nxs_renderer_set_adaptive(nxs_renderer* r, const nx_adaptive_params* params) { return guarded([&] { r->r.SetAdaptive(params); }); }
int nxs_renderer_render_adaptive(nxs_renderer* r, nxs_scene* scene, uint32_t maxFrames, uint32_t interval, uint32_t* framesRendered)
{
    return guarded([&] {
        const uint32_t frames = r->r.RenderAdaptive(scene->scene, maxFrames, interval);
        if (framesRendered) *framesRendered = frames;
    });
}
int nxs_renderer_save_sample_count_exr(nxs_renderer* r, const char* path)
{
    return guarded([&] {
        if (!path || !r->r.SaveSampleCountEXR(path)) throw std::runtime_error(std::string("cannot write the sample counts to ") + (path ? path : "(null)") + " (is adaptive sampling on?)");
    });
}
int nxs_pathtracer_set_adaptive(nxs_pathtracer* p, const nx_adaptive_params* params) { return guarded([&] { p->pt.SetAdaptive(params); }); }

int nxh_write_png(const char* path, const uint32_t* rgba8, uint32_t width, uint32_t height, int flipVertically)
{
    return guarded([&] {
        if (!path || !WritePNG(path, rgba8, width, height, flipVertically != 0)) throw std::runtime_error("nxh_write_png: cannot write the file");
    });
}
int nxh_write_exr(const char* path, const float* rgb, uint32_t width, uint32_t height, int flipVertically)
{
    return guarded([&] {
        if (!path || !WriteEXR(path, rgb, width, height, flipVertically != 0)) throw std::runtime_error("nxh_write_exr: cannot write the file");
    });
}

}  // extern "C"
