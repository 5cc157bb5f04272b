// nexus/OBJLoader.h — scene ingestion of the kept API surface without Assimp.
// Mirrors /root/reference/Nexus/src/Assets/OBJLoader.h:13-20 (OBJLoader::LoadOBJ(path, filename, scene, assetManager)) and
// what OBJLoader.cpp:8-239 yields through Assimp for the files the reference ships: one mesh + BVH per glTF primitive,
// one instance per (node, primitive) placed with the node's TRS decomposed to Euler degrees, the material heuristics of
// OBJLoader.cpp:71-163, aiProcess_FlipUVs.  Reads binary glTF 2.0 (.glb) and triangulated / polygonal Wavefront .obj.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "Assets.h"
#include "Triangle.h"

namespace nexus {

class Scene;

struct LoadedInstance {
    int mesh = 0, material = 0;
    float3 position = make_float3(0.0f), rotation = make_float3(0.0f), scale = make_float3(1.0f);  // rotation: Euler XYZ, degrees
    std::string name;
};

struct LoadedScene {
    std::vector<std::vector<Triangle>> meshes;
    std::vector<std::string> meshNames;
    std::vector<Material> materials;
    std::vector<LoadedInstance> instances;
    // Images the materials refer to, decoded to RGBA8 (glTF baseColorTexture -> DIFFUSE, emissiveTexture -> EMISSIVE, as
    // Assimp presents them to OBJLoader.cpp:115-160), and per material the index into `textures` (-1: none).  The
    // materials' diffuseMapId / emissiveMapId stay -1 here: ids are handed out by the AssetManager in LoadOBJ.
    std::vector<Texture> textures;
    std::vector<int> materialDiffuseTexture, materialEmissiveTexture;
    // Detail maps (glTF normalTexture and pbrMetallicRoughness.metallicRoughnessTexture -> NORMAL, ROUGHNESS: linear data), in a list of
    // their own — `textures` and its order are what they were — and per material the index into it (-1: none) and normalTexture.scale.
    // texCoord sets other than 0 and KHR_texture_transform are not carried: the map is used with set 0 as it is, with a warning.
    std::vector<Texture> detailTextures;
    std::vector<int> materialNormalTexture, materialRoughnessTexture;
    std::vector<float> materialNormalScale;
    // glTF alphaMode / alphaCutoff per material (nx_material_alpha of nexus_pod.h; the rule: nexus_hip.h) — filled only when asked for
    // (LoadOptions::alphaModes), else empty: every material's alpha is a stochastic blend, as it has always been
    std::vector<nx_material_alpha> materialAlpha;
    std::vector<AnalyticLight> analyticLights;  // glTF KHR_lights_punctual: one per node that carries a light, in world space
    // glTF skins, joint animations and the node tree — filled only when asked for (LoadOptions::skins), else empty.  skins[i] belongs to
    // meshes[i] (empty pointer: not skinned); node indices are the file's.
    std::vector<std::shared_ptr<Skin>> skins;
    // glTF morph targets — filled only when asked for (LoadOptions::morphs, which fills nodes and animations too and keeps the animations'
    // weights channels), else empty.  morphs[i] belongs to meshes[i] (empty pointer: no targets).
    std::vector<std::shared_ptr<Morph>> morphs;
    std::vector<SceneNode> nodes;
    std::vector<Animation> animations;
    std::vector<std::string> warnings;  // images that could not be decoded (the reference prints and carries on, IMGLoader.cpp:24-25)
};

// How a file's materials are read.  metalRough (off by default: glTF's default metallicFactor is 1, so it would turn every existing
// file into metal): a .glb material without transmission becomes an NX_MAT_METALROUGH — albedo = baseColorFactor.rgb, roughness =
// roughnessFactor as it stands (default 1), metallic = metallicFactor (default 1), ior from KHR_materials_ior (default 1.5) —
// instead of the reference's PLASTIC; a material with transmissionFactor > 0 stays the DIELECTRIC it is, and .obj files do not change.
// alphaModes (off by default, so every existing scene renders as before): a .glb material's alphaMode — OPAQUE when the file says nothing,
// glTF's default — and alphaCutoff (default 0.5) are read into LoadedScene::materialAlpha, and LoadOBJ hands them to the AssetManager
// (SetMaterialAlpha).  A MASK material whose alphaCutoff lies outside [0, 1] is refused by the reader, with the material's number.  .obj files
// carry no such mode: their materials stay blends.
// skins (off by default, so every existing scene loads as before): a .glb's skins, JOINTS_0 / WEIGHTS_0, joint animations and node tree are
// read into LoadedScene::skins / animations / nodes, and LoadOBJ hands them to the meshes and the scene.  JOINTS_1 is ignored with a
// warning, and so are morph targets unless `morphs` is on; a CUBICSPLINE sampler is read as its keys' values and interpolated linearly,
// with a warning.
// morphs (off by default): a .glb's morph targets — POSITION and NORMAL, float VEC3, sparse accessors included; all primitives of a mesh
// with the same number of them — are read into LoadedScene::morphs, the node tree and the animations as under `skins`, and the animations'
// `weights` channels are kept.  TANGENT deltas are not read: the 96-byte triangle has no tangents.
struct LoadOptions {
    bool metalRough = false;
    bool alphaModes = false;
    bool skins = false;
    bool morphs = false;
};

class OBJLoader {
public:
    // Parse a file into meshes / materials / instances; throws std::runtime_error with a message on malformed input.
    static LoadedScene Parse(const std::string& file, const LoadOptions& options = LoadOptions());
    // Scene::CreateMeshInstanceFromFile's worker (Scene.cpp:83-91): adds the file's materials, builds one BVH8 per mesh,
    // registers the meshes and creates one mesh instance per loaded instance.
    static void LoadOBJ(const std::string& path, const std::string& filename, Scene* scene, AssetManager* assetManager, const LoadOptions& options = LoadOptions());
};

}  // namespace nexus
