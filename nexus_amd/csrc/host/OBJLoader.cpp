// OBJLoader.cpp — binary glTF 2.0 and Wavefront .obj ingestion without Assimp (see nexus/OBJLoader.h).
// What the reference obtains through Assimp (/root/reference/Nexus/src/Assets/OBJLoader.cpp:8-239) is reproduced for the
// subset of the formats its demo assets use; the numbers (TRS decomposition, roughness mapping) are computed in double
// and stored as float, like the Python reader in nexus_amd/loaders.py that the tests compare against.
#include "nexus/OBJLoader.h"

#include "nexus/IMGLoader.h"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>

#include "nexus/Scene.h"

namespace nexus {

namespace {

[[noreturn]] void fail(const std::string& what) { throw std::runtime_error("OBJLoader: " + what); }

// ---- a small JSON reader (objects, arrays, strings, numbers, true / false / null) ----------------------------------
struct Json {
    enum Kind { Null, Bool, Number, String, Array, Object } kind = Null;
    bool b = false;
    double num = 0.0;
    std::string str;
    std::vector<Json> arr;
    std::vector<std::pair<std::string, Json>> obj;

    const Json* find(const std::string& key) const
    {
        if (kind != Object) return nullptr;
        for (const auto& kv : obj)
            if (kv.first == key) return &kv.second;
        return nullptr;
    }
    const Json& at(const std::string& key) const
    {
        const Json* j = find(key);
        if (!j) fail("glTF JSON: missing key \"" + key + "\"");
        return *j;
    }
    const Json& at(size_t i) const
    {
        if (kind != Array || i >= arr.size()) fail("glTF JSON: array index out of range");
        return arr[i];
    }
    double number(const std::string& key, double dflt) const
    {
        const Json* j = find(key);
        return (j && j->kind == Number) ? j->num : dflt;
    }
    size_t size() const { return kind == Array ? arr.size() : 0; }
};

class JsonParser {
public:
    JsonParser(const char* p, size_t n) : m_P(p), m_End(p + n) {}
    Json parse()
    {
        Json j = value();
        skip();
        return j;
    }

private:
    const char* m_P;
    const char* m_End;
    void skip()
    {
        while (m_P < m_End && (*m_P == ' ' || *m_P == '\n' || *m_P == '\r' || *m_P == '\t')) m_P++;
    }
    char peek()
    {
        skip();
        if (m_P >= m_End) fail("glTF JSON: unexpected end");
        return *m_P;
    }
    void expect(char c)
    {
        if (peek() != c) fail(std::string("glTF JSON: expected '") + c + "'");
        m_P++;
    }
    Json value()
    {
        const char c = peek();
        Json j;
        if (c == '{') {
            j.kind = Json::Object;
            m_P++;
            if (peek() == '}') { m_P++; return j; }
            for (;;) {
                Json k = string();
                expect(':');
                j.obj.emplace_back(std::move(k.str), value());
                if (peek() == ',') { m_P++; continue; }
                expect('}');
                return j;
            }
        }
        if (c == '[') {
            j.kind = Json::Array;
            m_P++;
            if (peek() == ']') { m_P++; return j; }
            for (;;) {
                j.arr.push_back(value());
                if (peek() == ',') { m_P++; continue; }
                expect(']');
                return j;
            }
        }
        if (c == '"') return string();
        if (c == 't' || c == 'f' || c == 'n') {
            const char* words[3] = {"true", "false", "null"};
            for (int w = 0; w < 3; w++) {
                const size_t len = std::strlen(words[w]);
                if (static_cast<size_t>(m_End - m_P) >= len && std::strncmp(m_P, words[w], len) == 0) {
                    m_P += len;
                    if (w < 2) { j.kind = Json::Bool; j.b = (w == 0); }
                    return j;
                }
            }
            fail("glTF JSON: bad literal");
        }
        // number
        char* end = nullptr;
        const std::string tmp(m_P, std::min<size_t>(static_cast<size_t>(m_End - m_P), 64));
        const double v = std::strtod(tmp.c_str(), &end);
        if (end == tmp.c_str()) fail("glTF JSON: bad number");
        m_P += end - tmp.c_str();
        j.kind = Json::Number;
        j.num = v;
        return j;
    }
    Json string()
    {
        expect('"');
        Json j;
        j.kind = Json::String;
        while (m_P < m_End && *m_P != '"') {
            if (*m_P == '\\') {
                m_P++;
                if (m_P >= m_End) break;
                switch (*m_P) {
                case 'n': j.str += '\n'; break;
                case 't': j.str += '\t'; break;
                case 'r': j.str += '\r'; break;
                case 'b': j.str += '\b'; break;
                case 'f': j.str += '\f'; break;
                case 'u':  // names only: keep ASCII, replace the rest
                    if (m_End - m_P >= 5) {
                        const unsigned long cp = std::strtoul(std::string(m_P + 1, 4).c_str(), nullptr, 16);
                        j.str += cp < 128 ? static_cast<char>(cp) : '?';
                        m_P += 4;
                    }
                    break;
                default: j.str += *m_P; break;
                }
                m_P++;
            } else {
                j.str += *m_P++;
            }
        }
        if (m_P >= m_End) fail("glTF JSON: unterminated string");
        m_P++;
        return j;
    }
};

// ---- 4x4 double matrices, row major ----------------------------------------------------------------------------------
struct M4 {
    double m[4][4];
    static M4 identity()
    {
        M4 r;
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) r.m[i][j] = (i == j) ? 1.0 : 0.0;
        return r;
    }
    M4 operator*(const M4& o) const
    {
        M4 r;
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) {
                double s = 0.0;
                for (int k = 0; k < 4; k++) s += m[i][k] * o.m[k][j];
                r.m[i][j] = s;
            }
        return r;
    }
};

M4 node_local_matrix(const Json& node)
{
    M4 r = M4::identity();
    if (const Json* mat = node.find("matrix")) {  // glTF stores column major
        if (mat->size() != 16) fail("glTF node matrix must have 16 entries");
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) r.m[i][j] = mat->at(static_cast<size_t>(j * 4 + i)).num;
        return r;
    }
    double q[4] = {0, 0, 0, 1}, s[3] = {1, 1, 1}, t[3] = {0, 0, 0};
    if (const Json* j = node.find("rotation"))
        for (size_t k = 0; k < 4 && k < j->size(); k++) q[k] = j->at(k).num;
    if (const Json* j = node.find("scale"))
        for (size_t k = 0; k < 3 && k < j->size(); k++) s[k] = j->at(k).num;
    if (const Json* j = node.find("translation"))
        for (size_t k = 0; k < 3 && k < j->size(); k++) t[k] = j->at(k).num;
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                            {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) r.m[i][j] = R[i][j] * s[j];
        r.m[i][3] = t[i];
    }
    return r;
}

// aiMatrix4x4::Decompose as the reference consumes it: position, Euler XYZ in degrees, scale
void decompose_trs(const M4& m, float3& pos, float3& rotDeg, float3& scale)
{
    double c[3][3];  // columns
    for (int k = 0; k < 3; k++)
        for (int i = 0; i < 3; i++) c[k][i] = m.m[i][k];
    double sc[3];
    for (int k = 0; k < 3; k++) sc[k] = std::sqrt(c[k][0] * c[k][0] + c[k][1] * c[k][1] + c[k][2] * c[k][2]);
    const double det = m.m[0][0] * (m.m[1][1] * m.m[2][2] - m.m[1][2] * m.m[2][1]) - m.m[0][1] * (m.m[1][0] * m.m[2][2] - m.m[1][2] * m.m[2][0]) +
                       m.m[0][2] * (m.m[1][0] * m.m[2][1] - m.m[1][1] * m.m[2][0]);
    if (det < 0)
        for (int k = 0; k < 3; k++) sc[k] = -sc[k];
    for (int k = 0; k < 3; k++)
        if (sc[k] != 0)
            for (int i = 0; i < 3; i++) c[k][i] /= sc[k];
    const double eps = 1e-10;
    const double ry = std::asin(-c[0][2]);
    const double cy = std::cos(ry);
    double rx, rz;
    if (std::fabs(cy) > eps) {
        rx = std::atan2(c[1][2], c[2][2]);
        rz = std::atan2(c[0][1], c[0][0]);
    } else {
        rx = 0.0;
        rz = std::atan2(-c[1][0], c[1][1]);
    }
    const double deg = 180.0 / 3.141592653589793238462643383279502884;
    pos = make_float3(static_cast<float>(m.m[0][3]), static_cast<float>(m.m[1][3]), static_cast<float>(m.m[2][3]));
    rotDeg = make_float3(static_cast<float>(rx * deg), static_cast<float>(ry * deg), static_cast<float>(rz * deg));
    scale = make_float3(static_cast<float>(sc[0]), static_cast<float>(sc[1]), static_cast<float>(sc[2]));
}

std::vector<unsigned char> read_file(const std::string& file)
{
    std::ifstream f(file, std::ios::binary);
    if (!f) fail("cannot open " + file);
    std::vector<unsigned char> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    return data;
}

uint32_t rd32(const std::vector<unsigned char>& d, size_t off)
{
    if (off + 4 > d.size()) fail("glb: truncated file");
    uint32_t v;
    std::memcpy(&v, d.data() + off, 4);
    return v;
}

void set_albedo_like(Material& m, const double rgb[3], double roughness, double ior)
{
    m.plastic.albedo[0] = static_cast<float>(rgb[0]);
    m.plastic.albedo[1] = static_cast<float>(rgb[1]);
    m.plastic.albedo[2] = static_cast<float>(rgb[2]);
    m.plastic.roughness = static_cast<float>(roughness);
    m.plastic.ior = static_cast<float>(ior);
}

// OBJLoader.cpp:71-163 through Assimp's glTF importer
Material gltf_material(const Json& m, const LoadOptions& options)
{
    static const Json empty;
    const Json* pbr = m.find("pbrMetallicRoughness");
    const Json* ext = m.find("extensions");
    double base[4] = {1, 1, 1, 1};
    if (pbr)
        if (const Json* b = pbr->find("baseColorFactor"))
            for (size_t k = 0; k < 4 && k < b->size(); k++) base[k] = b->at(k).num;
    const double rough = pbr ? pbr->number("roughnessFactor", 1.0) : 1.0;
    const double shininess = (1.0 - rough) * (1.0 - rough) * 1000.0;  // Assimp: roughness -> shininess
    double roughness = 1.0 - std::sqrt(shininess) / 31.62278;         // the reference maps it back
    roughness = std::min(1.0, std::max(0.0, roughness));
    auto ext_number = [&](const char* e, const char* key, double dflt) {
        if (!ext) return dflt;
        const Json* j = ext->find(e);
        return j ? j->number(key, dflt) : dflt;
    };
    const double ior = ext_number("KHR_materials_ior", "ior", 1.45);
    const double transmission = ext_number("KHR_materials_transmission", "transmissionFactor", 0.0);
    Material out;
    out.type = transmission > 0.0 ? NX_MAT_DIELECTRIC : NX_MAT_PLASTIC;
    set_albedo_like(out, base, roughness, ior);
    if (options.metalRough && !(transmission > 0.0)) {
        // glTF's own model (LoadOptions::metalRough): the raw factors, the spec's defaults
        out.type = NX_MAT_METALROUGH;
        set_albedo_like(out, base, rough, ext_number("KHR_materials_ior", "ior", 1.5));
        out.metalrough.metallic = static_cast<float>(pbr ? pbr->number("metallicFactor", 1.0) : 1.0);
    }
    if (const Json* e = m.find("emissiveFactor"))
        for (size_t k = 0; k < 3 && k < e->size(); k++) out.emissive[k] = static_cast<float>(e->at(k).num);
    out.intensity = static_cast<float>(ext_number("KHR_materials_emissive_strength", "emissiveStrength", 1.0));
    out.opacity = static_cast<float>(base[3]);
    return out;
}

float3 face_normal(float3 p0, float3 p1, float3 p2)
{
    const float3 fn = cross(p1 - p0, p2 - p0);
    const float ln = std::sqrt(fn.x * fn.x + fn.y * fn.y + fn.z * fn.z);
    if (!(ln > 0.0f)) return make_float3(0.0f, 0.0f, 1.0f);
    const float d = std::max(ln, 1e-30f);
    return make_float3(fn.x / d, fn.y / d, fn.z / d);
}

struct Accessor {
    const unsigned char* base = nullptr;
    size_t stride = 0, count = 0;
    int componentType = 0, ncomp = 0;
    double get(size_t i, int c) const
    {
        const unsigned char* p = base + i * stride;
        switch (componentType) {
        case 5120: { int8_t v; std::memcpy(&v, p + c, 1); return v; }
        case 5121: { uint8_t v; std::memcpy(&v, p + c, 1); return v; }
        case 5122: { int16_t v; std::memcpy(&v, p + 2 * c, 2); return v; }
        case 5123: { uint16_t v; std::memcpy(&v, p + 2 * c, 2); return v; }
        case 5125: { uint32_t v; std::memcpy(&v, p + 4 * c, 4); return v; }
        case 5126: { float v; std::memcpy(&v, p + 4 * c, 4); return v; }
        default: fail("glb: unsupported accessor component type");
        }
    }
};

// LoadOptions::skins: the node tree (parents and rest TRS), the skin of every skinned primitive (the corner records are there already:
// the primitive loop of parse_glb) and the joint animations as channels.  The twin of nexus_amd/loaders.py _read_skins.
template <class AccessorOf>
void read_skins(const Json& doc, const AccessorOf& accessor, const std::map<std::pair<size_t, size_t>, std::pair<int, int>>& primMesh, LoadedScene& out, const LoadOptions& options)
{
    const Json& nodes = doc.at("nodes");
    out.nodes.resize(nodes.size());
    for (size_t ni = 0; ni < nodes.size(); ni++) {
        const Json& node = nodes.at(ni);
        SceneNode& n = out.nodes[ni];
        if (const Json* name = node.find("name")) n.name = name->str;
        if (const Json* j = node.find("translation"))
            for (size_t k = 0; k < 3 && k < j->size(); k++) n.translation[k] = j->at(k).num;
        if (const Json* j = node.find("rotation"))
            for (size_t k = 0; k < 4 && k < j->size(); k++) n.rotation[k] = j->at(k).num;
        if (const Json* j = node.find("scale"))
            for (size_t k = 0; k < 3 && k < j->size(); k++) n.scale[k] = j->at(k).num;
        if (node.find("matrix")) {
            n.hasMatrix = true;
            const M4 m = node_local_matrix(node);
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 4; j++) n.matrix[4 * i + j] = m.m[i][j];
        }
        if (const Json* ch = node.find("children"))
            for (size_t k = 0; k < ch->size(); k++) {
                const size_t c = static_cast<size_t>(ch->at(k).num);
                if (c >= nodes.size()) fail("glb: a node names a child that does not exist");
                out.nodes[c].parent = static_cast<int>(ni);
            }
    }
    for (size_t ni = 0; ni < nodes.size(); ni++) {
        const Json& node = nodes.at(ni);
        const Json* meshRef = node.find("mesh");
        const Json* skinRef = node.find("skin");
        if (!options.skins || !meshRef || !skinRef) continue;
        const Json& skin = doc.at("skins").at(static_cast<size_t>(skinRef->num));
        const Json& joints = skin.at("joints");
        std::vector<int> jointNodes;
        for (size_t k = 0; k < joints.size(); k++) {
            if (joints.at(k).num < 0 || joints.at(k).num >= static_cast<double>(nodes.size())) fail("glb: a skin names a joint node that does not exist");
            jointNodes.push_back(static_cast<int>(joints.at(k).num));
        }
        std::vector<double> inverseBind(jointNodes.size() * 16, 0.0);
        for (size_t k = 0; k < jointNodes.size(); k++)
            for (int d = 0; d < 4; d++) inverseBind[16 * k + 5 * static_cast<size_t>(d)] = 1.0;
        if (const Json* ibm = skin.find("inverseBindMatrices")) {
            const Accessor a = accessor(static_cast<size_t>(ibm->num));
            if (a.ncomp != 16 || a.count != jointNodes.size()) fail("glb: a skin's inverse bind matrices do not fit its joints");
            for (size_t k = 0; k < a.count; k++)
                for (int i = 0; i < 4; i++)
                    for (int j = 0; j < 4; j++) inverseBind[16 * k + 4 * static_cast<size_t>(i) + static_cast<size_t>(j)] = a.get(k, j * 4 + i);  // glTF stores column major
        }
        for (const auto& kv : primMesh) {
            if (kv.first.first != static_cast<size_t>(meshRef->num)) continue;
            Skin* s = out.skins[static_cast<size_t>(kv.second.first)].get();
            if (!s || s->meshNode >= 0) continue;  // (no JOINTS_0 / WEIGHTS_0; or placed by an earlier node: that one's skin holds)
            for (const nx_skin_corner& c : s->corners)
                for (int k = 0; k < 4; k++)
                    if (c.weight[k] != 0.0f && c.joint[k] >= jointNodes.size()) fail("glb: a primitive names a joint its skin does not have");
            s->joints = jointNodes;
            s->inverseBind = inverseBind;
            s->meshNode = static_cast<int>(ni);
        }
    }
    for (std::shared_ptr<Skin>& s : out.skins)
        if (s && s->meshNode < 0) s.reset();  // (joints and weights on a mesh no skinned node places: nothing to pose it with)
    const Json* anims = doc.find("animations");
    for (size_t ai = 0; anims && ai < anims->size(); ai++) {
        const Json& anim = anims->at(ai);
        Animation A;
        if (const Json* name = anim.find("name")) A.name = name->str;
        const Json* channels = anim.find("channels");
        for (size_t ci = 0; channels && ci < channels->size(); ci++) {
            const Json& ch = channels->at(ci);
            const Json* target = ch.find("target");
            if (!target || !target->find("node") || !target->find("path")) continue;
            const std::string& path = target->at("path").str;
            const bool weights = options.morphs && path == "weights";
            if (path != "translation" && path != "rotation" && path != "scale" && !weights) continue;  // (weights without LoadOptions::morphs: ignored with the primitive's warning)
            AnimationChannel c;
            c.node = static_cast<int>(target->at("node").num);
            if (c.node < 0 || static_cast<size_t>(c.node) >= nodes.size()) fail("glb: an animation channel names a node that does not exist");
            c.path = weights ? AnimationChannel::WEIGHTS : path == "translation" ? AnimationChannel::TRANSLATION : path == "rotation" ? AnimationChannel::ROTATION : AnimationChannel::SCALE;
            const Json& sampler = anim.at("samplers").at(static_cast<size_t>(ch.at("sampler").num));
            const Accessor in = accessor(static_cast<size_t>(sampler.at("input").num)), val = accessor(static_cast<size_t>(sampler.at("output").num));
            const Json* ip = sampler.find("interpolation");
            const std::string interpolation = ip ? ip->str : "LINEAR";
            size_t perKey = 1, valueAt = 0;
            if (interpolation == "CUBICSPLINE") {
                out.warnings.push_back("animation " + std::to_string(ai) + ": a CUBICSPLINE sampler is read as its keys' values and interpolated linearly");
                perKey = 3;  // (in-tangent, value, out-tangent) per key
                valueAt = 1;
            } else if (interpolation == "STEP") {
                c.step = true;
            } else if (interpolation != "LINEAR") {
                fail("glb: animation " + std::to_string(ai) + " has an unknown interpolation");
            }
            if (weights) {  // scalars, (keys, targets) row by row: a CUBICSPLINE key is its three rows of targets
                const size_t rows = in.count * perKey;
                if (in.count == 0 || val.ncomp != 1 || val.count == 0 || val.count % rows != 0) fail("glb: animation " + std::to_string(ai) + " has a sampler whose keys and values differ in number");
                const size_t targets = val.count / rows;
                const double unit = val.componentType == 5120 ? 127.0 : val.componentType == 5121 ? 255.0 : val.componentType == 5122 ? 32767.0 : val.componentType == 5123 ? 65535.0 : 1.0;
                for (size_t k = 0; k < in.count; k++) {
                    c.times.push_back(in.get(k, 0));
                    for (size_t d = 0; d < targets; d++) {
                        const double v = val.get((perKey * k + valueAt) * targets + d, 0);
                        c.values.push_back(unit == 1.0 ? v : std::max(v / unit, -1.0));
                    }
                }
                A.channels.push_back(std::move(c));
                continue;
            }
            const int width = c.path == AnimationChannel::ROTATION ? 4 : 3;
            if (in.count == 0 || val.count != in.count * perKey || val.ncomp != width) fail("glb: animation " + std::to_string(ai) + " has a sampler whose keys and values differ in number");
            // (normalised integers: glTF allows them for rotations)
            const double unit = val.componentType == 5120 ? 127.0 : val.componentType == 5121 ? 255.0 : val.componentType == 5122 ? 32767.0 : val.componentType == 5123 ? 65535.0 : 1.0;
            for (size_t k = 0; k < in.count; k++) {
                c.times.push_back(in.get(k, 0));
                for (int d = 0; d < width; d++) c.values.push_back(unit == 1.0 ? val.get(perKey * k + valueAt, d) : std::max(val.get(perKey * k + valueAt, d) / unit, -1.0));
            }
            A.channels.push_back(std::move(c));
        }
        out.animations.push_back(std::move(A));
    }
}

// LoadOptions::morphs: which node places each morphed mesh, and the default weights — the node's, else the mesh's, else zeros.  The twin of
// nexus_amd/loaders.py _read_morphs.
void read_morphs(const Json& doc, const std::map<std::pair<size_t, size_t>, std::pair<int, int>>& primMesh, LoadedScene& out)
{
    const Json& nodes = doc.at("nodes");
    for (size_t ni = 0; ni < nodes.size(); ni++) {
        const Json& node = nodes.at(ni);
        const Json* meshRef = node.find("mesh");
        if (!meshRef) continue;
        const Json& mesh = doc.at("meshes").at(static_cast<size_t>(meshRef->num));
        for (const auto& kv : primMesh) {
            if (kv.first.first != static_cast<size_t>(meshRef->num)) continue;
            Morph* m = out.morphs[static_cast<size_t>(kv.second.first)].get();
            if (!m || m->meshNode >= 0) continue;  // (no targets; or placed by an earlier node: that one holds)
            m->meshNode = static_cast<int>(ni);
            const Json* w = node.find("weights");
            if (!w) w = mesh.find("weights");
            if (w) {
                if (w->size() != m->targets) fail("glb: mesh " + std::to_string(kv.first.first) + " has " + std::to_string(m->targets) + " morph targets and " + std::to_string(w->size()) + " default weights");
                for (size_t k = 0; k < w->size(); k++) m->weights[k] = static_cast<float>(w->at(k).num);
            }
            if (const Json* extras = mesh.find("extras"))
                if (extras->kind == Json::Object)
                    if (const Json* names = extras->find("targetNames"))
                        for (size_t k = 0; k < names->size(); k++) m->names.push_back(names->at(k).str);
        }
    }
    for (std::shared_ptr<Morph>& m : out.morphs)
        if (m && m->meshNode < 0) m.reset();  // (a mesh no node places: the Python reader lists none either)
}

LoadedScene parse_glb(const std::string& file, const LoadOptions& options)
{
    const std::vector<unsigned char> data = read_file(file);
    if (data.size() < 20 || rd32(data, 0) != 0x46546C67u || rd32(data, 4) != 2u) fail(file + " is not a glTF 2.0 binary file");
    size_t off = 12;
    const unsigned char* jsonChunk = nullptr;
    size_t jsonLen = 0;
    const unsigned char* blob = nullptr;
    size_t blobLen = 0;
    while (off + 8 <= data.size()) {
        const uint32_t clen = rd32(data, off), ctype = rd32(data, off + 4);
        if (off + 8 + clen > data.size()) fail("glb: chunk runs past the end of the file");
        if (ctype == 0x4E4F534Au) { jsonChunk = data.data() + off + 8; jsonLen = clen; }
        else if (ctype == 0x004E4942u) { blob = data.data() + off + 8; blobLen = clen; }
        off += 8 + static_cast<size_t>(clen);
    }
    if (!jsonChunk) fail("glb without a JSON chunk");
    const Json doc = JsonParser(reinterpret_cast<const char*>(jsonChunk), jsonLen).parse();

    auto accessor = [&](size_t index) {
        const Json& a = doc.at("accessors").at(index);
        const Json& bv = doc.at("bufferViews").at(static_cast<size_t>(a.at("bufferView").num));
        Accessor acc;
        acc.componentType = static_cast<int>(a.at("componentType").num);
        const std::string& type = a.at("type").str;
        acc.ncomp = type == "SCALAR" ? 1 : type == "VEC2" ? 2 : type == "VEC3" ? 3 : type == "VEC4" ? 4 : type == "MAT4" ? 16 : 0;
        if (!acc.ncomp) fail("glb: unsupported accessor type " + type);
        const size_t csize = (acc.componentType == 5120 || acc.componentType == 5121) ? 1 : (acc.componentType == 5122 || acc.componentType == 5123) ? 2 : 4;
        const size_t start = static_cast<size_t>(bv.number("byteOffset", 0)) + static_cast<size_t>(a.number("byteOffset", 0));
        const size_t stride = static_cast<size_t>(bv.number("byteStride", 0));
        acc.stride = stride ? stride : csize * static_cast<size_t>(acc.ncomp);
        acc.count = static_cast<size_t>(a.at("count").num);
        if (!blob || (acc.count && start + (acc.count - 1) * acc.stride + csize * static_cast<size_t>(acc.ncomp) > blobLen)) fail("glb: accessor runs past the binary chunk");
        acc.base = blob + start;
        return acc;
    };

    // a morph target's attribute, 3 floats per vertex: the accessor's bufferView (zeros without one) with its sparse part written over it
    auto target_values = [&](size_t index, const std::string& what) {
        const Json& a = doc.at("accessors").at(index);
        if (static_cast<int>(a.at("componentType").num) != 5126 || a.at("type").str != "VEC3") fail("glb: " + what + ": a morph target attribute must be a float VEC3 accessor");
        const size_t count = static_cast<size_t>(a.at("count").num);
        std::vector<float> v(count * 3, 0.0f);
        if (a.find("bufferView")) {
            const Accessor acc = accessor(index);
            for (size_t i = 0; i < count; i++)
                for (int c = 0; c < 3; c++) v[3 * i + static_cast<size_t>(c)] = static_cast<float>(acc.get(i, c));
        }
        if (const Json* sparse = a.find("sparse")) {
            const size_t n = static_cast<size_t>(sparse->at("count").num);
            auto part = [&](const Json& ref, int componentType, int ncomp) {
                const Json& bv = doc.at("bufferViews").at(static_cast<size_t>(ref.at("bufferView").num));
                Accessor acc;
                acc.componentType = componentType;
                acc.ncomp = ncomp;
                const size_t csize = (componentType == 5120 || componentType == 5121) ? 1 : (componentType == 5122 || componentType == 5123) ? 2 : 4;
                const size_t start = static_cast<size_t>(bv.number("byteOffset", 0)) + static_cast<size_t>(ref.number("byteOffset", 0));
                acc.stride = csize * static_cast<size_t>(ncomp);
                acc.count = n;
                if (!blob || (n && start + n * acc.stride > blobLen)) fail("glb: a sparse accessor runs past the binary chunk");
                acc.base = blob + start;
                return acc;
            };
            const Accessor ind = part(sparse->at("indices"), static_cast<int>(sparse->at("indices").at("componentType").num), 1), val = part(sparse->at("values"), 5126, 3);
            for (size_t k = 0; k < n; k++) {
                const size_t at = static_cast<size_t>(ind.get(k, 0));
                if (at >= count) fail("glb: a sparse accessor names an element it does not have");
                for (int c = 0; c < 3; c++) v[3 * at + static_cast<size_t>(c)] = static_cast<float>(val.get(k, c));
            }
        }
        return v;
    };

    LoadedScene out;
    std::map<size_t, size_t> meshTargets;  // LoadOptions::morphs: mesh -> the target count of its primitives (all equal)
    // texture index -> decoded image, decoded once however many materials share it
    std::map<std::pair<size_t, int>, int> decoded;  // (glTF texture, kind) -> index into out.textures
    auto load_texture = [&](const Json& texRef, Texture::Type kind) -> int {
        const size_t ti = static_cast<size_t>(texRef.at("index").num);
        const bool detail = kind == Texture::Type::NORMAL || kind == Texture::Type::ROUGHNESS;
        std::vector<Texture>& store = detail ? out.detailTextures : out.textures;
        const auto key = std::make_pair(ti, kind == Texture::Type::DIFFUSE ? 0 : kind == Texture::Type::EMISSIVE ? 1 : kind == Texture::Type::NORMAL ? 2 : 3);
        const auto hit = decoded.find(key);
        if (hit != decoded.end()) return hit->second;
        int result = -1;
        try {
            const Json& tex = doc.at("textures").at(ti);
            const Json& img = doc.at("images").at(static_cast<size_t>(tex.at("source").num));
            Texture t;
            if (const Json* bvRef = img.find("bufferView")) {
                const Json& bv = doc.at("bufferViews").at(static_cast<size_t>(bvRef->num));
                const size_t start = static_cast<size_t>(bv.number("byteOffset", 0)), len = static_cast<size_t>(bv.at("byteLength").num);
                if (!blob || start + len > blobLen) fail("glb: image runs past the binary chunk");
                t = IMGLoader::LoadIMG(blob + start, len);
            } else if (const Json* uri = img.find("uri")) {
                if (uri->str.compare(0, 5, "data:") == 0) fail("glb: data: URIs are not supported for images");
                const size_t slash = file.find_last_of("/\\");
                t = IMGLoader::LoadIMG((slash == std::string::npos ? std::string() : file.substr(0, slash + 1)) + uri->str);
            } else {
                fail("glb: image without bufferView or uri");
            }
            t.type = kind;
            result = static_cast<int>(store.size());
            store.push_back(std::move(t));
        } catch (const std::exception& e) {
            out.warnings.push_back(std::string("texture ") + std::to_string(ti) + ": " + e.what());
        }
        decoded[key] = result;
        return result;
    };
    if (const Json* mats = doc.find("materials"))
        for (size_t i = 0; i < mats->size(); i++) {
            const Json& m = mats->at(i);
            out.materials.push_back(gltf_material(m, options));
            int dt = -1, et = -1;
            if (const Json* pbr = m.find("pbrMetallicRoughness"))
                if (const Json* t = pbr->find("baseColorTexture")) dt = load_texture(*t, Texture::Type::DIFFUSE);
            if (const Json* t = m.find("emissiveTexture")) et = load_texture(*t, Texture::Type::EMISSIVE);
            out.materialDiffuseTexture.push_back(dt);
            out.materialEmissiveTexture.push_back(et);
            // detail maps: set 0 and untransformed coordinates are all the triangles carry — the map is used with them, and the file's author is told
            const Json* nt = m.find("normalTexture");
            const Json* rt = nullptr;
            if (const Json* pbr = m.find("pbrMetallicRoughness")) rt = pbr->find("metallicRoughnessTexture");
            const std::pair<const Json*, const char*> refs[] = {{nt, "normalTexture"}, {rt, "metallicRoughnessTexture"}};
            for (const auto& ref : refs) {
                if (!ref.first) continue;
                const int set = static_cast<int>(ref.first->number("texCoord", 0));
                if (set != 0) out.warnings.push_back("material " + std::to_string(i) + ": " + ref.second + " uses texCoord " + std::to_string(set) + "; set 0 is used");
                if (const Json* ext = ref.first->find("extensions"))
                    if (ext->find("KHR_texture_transform")) out.warnings.push_back("material " + std::to_string(i) + ": " + ref.second + " carries KHR_texture_transform, which is ignored");
            }
            out.materialNormalTexture.push_back(nt ? load_texture(*nt, Texture::Type::NORMAL) : -1);
            out.materialRoughnessTexture.push_back(rt ? load_texture(*rt, Texture::Type::ROUGHNESS) : -1);
            out.materialNormalScale.push_back(nt ? static_cast<float>(nt->number("scale", 1.0)) : 1.0f);
            if (options.alphaModes) {
                nx_material_alpha a;
                a.mode = NX_ALPHA_OPAQUE;  // glTF's default
                if (const Json* mode = m.find("alphaMode")) {
                    if (mode->kind != Json::String || (mode->str != "OPAQUE" && mode->str != "MASK" && mode->str != "BLEND")) fail("glb: material " + std::to_string(i) + " has an unknown alphaMode");
                    a.mode = mode->str == "MASK" ? NX_ALPHA_MASK : mode->str == "BLEND" ? NX_ALPHA_BLEND : NX_ALPHA_OPAQUE;
                }
                a.cutoff = static_cast<float>(m.number("alphaCutoff", 0.5));
                // (glTF asks for >= 0 only; above 1 nothing would pass, which the device's table — cutoff in [0, 1] — cannot say: refused here,
                //  by the material's number, not at the device update)
                if (a.mode == NX_ALPHA_MASK && !(a.cutoff >= 0.0f && a.cutoff <= 1.0f))
                    fail("glb: material " + std::to_string(i) + " has alphaMode MASK with an alphaCutoff outside [0, 1]");
                out.materialAlpha.push_back(a);
            }
        }
    if (out.materials.empty()) {
        Material m;  // pod.make_material() defaults
        m.diffuse.albedo[0] = m.diffuse.albedo[1] = m.diffuse.albedo[2] = 0.8f;
        m.plastic.ior = 1.45f;
        out.materials.push_back(m);
        out.materialDiffuseTexture.push_back(-1);
        out.materialEmissiveTexture.push_back(-1);
        out.materialNormalTexture.push_back(-1);
        out.materialRoughnessTexture.push_back(-1);
        out.materialNormalScale.push_back(1.0f);
        if (options.alphaModes) out.materialAlpha.push_back(nx_material_alpha{NX_ALPHA_OPAQUE, 0.5f});  // (no map: the same thing as a blend)
    }

    // one mesh per primitive (what Assimp hands the reference, OBJLoader.cpp:165-181)
    std::map<std::pair<size_t, size_t>, std::pair<int, int>> primMesh;  // (mesh, primitive) -> (loaded mesh, material)
    const Json* meshes = doc.find("meshes");
    for (size_t mi = 0; meshes && mi < meshes->size(); mi++) {
        const Json& mesh = meshes->at(mi);
        const Json& prims = mesh.at("primitives");
        for (size_t pi = 0; pi < prims.size(); pi++) {
            const Json& prim = prims.at(pi);
            if (static_cast<int>(prim.number("mode", 4)) != 4) continue;
            const Json& attrs = prim.at("attributes");
            const Accessor pos = accessor(static_cast<size_t>(attrs.at("POSITION").num));
            const bool hasN = attrs.find("NORMAL") != nullptr, hasUV = attrs.find("TEXCOORD_0") != nullptr;
            Accessor nrm, uv, idx;
            if (hasN) nrm = accessor(static_cast<size_t>(attrs.at("NORMAL").num));
            if (hasUV) uv = accessor(static_cast<size_t>(attrs.at("TEXCOORD_0").num));
            const bool indexed = prim.find("indices") != nullptr;
            if (indexed) idx = accessor(static_cast<size_t>(prim.at("indices").num));
            const size_t corners = indexed ? idx.count : pos.count;
            std::vector<Triangle> tris;
            tris.reserve(corners / 3);
            for (size_t t = 0; t + 2 < corners; t += 3) {
                size_t v[3];
                for (int k = 0; k < 3; k++) {
                    v[k] = indexed ? static_cast<size_t>(idx.get(t + k, 0)) : t + k;
                    if (v[k] >= pos.count) fail("glb: vertex index out of range");
                }
                float3 p[3], n[3];
                float2 tc[3];
                for (int k = 0; k < 3; k++) {
                    p[k] = make_float3(static_cast<float>(pos.get(v[k], 0)), static_cast<float>(pos.get(v[k], 1)), static_cast<float>(pos.get(v[k], 2)));
                    n[k] = hasN ? make_float3(static_cast<float>(nrm.get(v[k], 0)), static_cast<float>(nrm.get(v[k], 1)), static_cast<float>(nrm.get(v[k], 2))) : make_float3(0.0f);
                    // aiProcess_FlipUVs, OBJLoader.cpp:219-220
                    tc[k] = hasUV ? make_float2(static_cast<float>(uv.get(v[k], 0)), 1.0f - static_cast<float>(uv.get(v[k], 1))) : make_float2(0.0f, 0.0f);
                }
                tris.emplace_back(p[0], p[1], p[2], n[0], n[1], n[2], tc[0], tc[1], tc[2]);
            }
            primMesh[{mi, pi}] = {static_cast<int>(out.meshes.size()), static_cast<int>(prim.number("material", 0))};
            if (options.skins) {
                const std::string what = "mesh " + std::to_string(mi) + " primitive " + std::to_string(pi);
                if (const Json* targets = prim.find("targets"))
                    if (targets->size() > 0 && !options.morphs) out.warnings.push_back(what + ": morph targets are ignored");
                if (attrs.find("JOINTS_1")) out.warnings.push_back(what + ": more than four influences per vertex (JOINTS_1) are ignored; JOINTS_0 / WEIGHTS_0 are used");
                std::shared_ptr<Skin> skin;
                if (attrs.find("JOINTS_0") && attrs.find("WEIGHTS_0")) {
                    const Accessor jt = accessor(static_cast<size_t>(attrs.at("JOINTS_0").num)), wt = accessor(static_cast<size_t>(attrs.at("WEIGHTS_0").num));
                    if (jt.ncomp != 4 || wt.ncomp != 4 || jt.count != pos.count || wt.count != pos.count) fail("glb: " + what + " has JOINTS_0 / WEIGHTS_0 that do not fit its vertices");
                    // (normalised integers: glTF's UNSIGNED_BYTE / UNSIGNED_SHORT weights)
                    const double unit = wt.componentType == 5121 ? 255.0 : wt.componentType == 5123 ? 65535.0 : 1.0;
                    skin = std::make_shared<Skin>();
                    skin->corners.resize(corners / 3 * 3);
                    for (size_t c = 0; c < skin->corners.size(); c++) {  // corner 3 i + v = vertex v of triangle i, de-indexed like the positions
                        const size_t v = indexed ? static_cast<size_t>(idx.get(c, 0)) : c;
                        for (int k = 0; k < 4; k++) {
                            const double j = jt.get(v, k);
                            if (j < 0 || j > 65535) fail("glb: " + what + " names a joint that does not fit 16 bits");
                            skin->corners[c].joint[k] = static_cast<uint16_t>(j);
                            skin->corners[c].weight[k] = unit == 1.0 ? static_cast<float>(wt.get(v, k)) : static_cast<float>(wt.get(v, k) / unit);
                        }
                    }
                }
                out.skins.push_back(std::move(skin));
            }
            if (options.morphs) {
                const std::string what = "mesh " + std::to_string(mi) + " primitive " + std::to_string(pi);
                const Json* targets = prim.find("targets");
                const size_t count = targets ? targets->size() : 0;
                if (!meshTargets.count(mi)) meshTargets[mi] = count;
                if (meshTargets[mi] != count) fail("glb: mesh " + std::to_string(mi) + " has primitives with different numbers of morph targets");
                std::shared_ptr<Morph> morph;
                if (count) {
                    morph = std::make_shared<Morph>();
                    morph->targets = static_cast<uint32_t>(count);
                    morph->weights.assign(count, 0.0f);
                    const size_t used = corners / 3 * 3;
                    morph->deltas.assign(count * used, nx_morph_corner{{0, 0, 0}, {0, 0, 0}});
                    for (size_t t = 0; t < count; t++) {
                        const Json& tg = targets->at(t);
                        const std::pair<const char*, int> attrsOf[] = {{"POSITION", 0}, {"NORMAL", 1}};
                        for (const auto& at : attrsOf) {
                            const Json* ref = tg.find(at.first);
                            if (!ref) continue;
                            const std::vector<float> v = target_values(static_cast<size_t>(ref->num), what);
                            if (v.size() != pos.count * 3) fail("glb: " + what + " has a morph target that does not fit its vertices");
                            for (size_t c = 0; c < used; c++) {  // corner 3 i + v = vertex v of triangle i, de-indexed like the positions
                                const size_t vi = indexed ? static_cast<size_t>(idx.get(c, 0)) : c;
                                nx_morph_corner& d = morph->deltas[t * used + c];
                                std::memcpy(at.second == 0 ? d.dPosition : d.dNormal, v.data() + 3 * vi, 12);
                            }
                        }
                    }
                }
                out.morphs.push_back(std::move(morph));
            }
            out.meshes.push_back(std::move(tris));
            const Json* name = mesh.find("name");
            out.meshNames.push_back(name ? name->str : "mesh" + std::to_string(mi));
        }
    }

    // KHR_lights_punctual: the light list of the root extension; a node names one by index (walk below).  Radiometric as written —
    // colour x intensity goes to the record unconverted (no 683 lm/W) —, `range` is ignored, radius and angular radius are 0.
    std::vector<AnalyticLight> punctual;
    if (const Json* ext = doc.find("extensions"))
        if (const Json* khr = ext->find("KHR_lights_punctual"))
            if (const Json* list = khr->find("lights"))
                for (size_t i = 0; i < list->size(); i++) {
                    const Json& l = list->at(i);
                    AnalyticLight a;
                    const std::string& type = l.at("type").str;
                    if (type == "point") a.type = NX_ALIGHT_POINT;
                    else if (type == "spot") a.type = NX_ALIGHT_SPOT;
                    else if (type == "directional") a.type = NX_ALIGHT_DIRECTIONAL;
                    else fail("glb: KHR_lights_punctual light of unknown type " + type);
                    if (const Json* c = l.find("color"))
                        for (size_t k = 0; k < 3 && k < c->size(); k++) a.colour[k] = static_cast<float>(c->at(k).num);
                    a.intensity = static_cast<float>(l.number("intensity", 1.0));
                    a.innerConeAngle = a.outerConeAngle = 0.0f;
                    if (a.type == NX_ALIGHT_SPOT) {
                        static const Json none;
                        const Json* spot = l.find("spot");
                        a.innerConeAngle = static_cast<float>((spot ? *spot : none).number("innerConeAngle", 0.0));
                        a.outerConeAngle = static_cast<float>((spot ? *spot : none).number("outerConeAngle", 0.78539816339744830962));
                    }
                    punctual.push_back(a);
                }

    const Json& nodes = doc.at("nodes");
    struct Walker {
        const Json& nodes;
        const std::vector<AnalyticLight>& punctual;
        const std::map<std::pair<size_t, size_t>, std::pair<int, int>>& primMesh;
        LoadedScene& out;
        int depth = 0;
        void walk(size_t ni, const M4& parent)
        {
            if (++depth > 256) fail("glb: node hierarchy too deep (cycle?)");
            const Json& node = nodes.at(ni);
            const M4 m = parent * node_local_matrix(node);
            if (const Json* meshRef = node.find("mesh")) {
                LoadedInstance inst;
                decompose_trs(m, inst.position, inst.rotation, inst.scale);
                if (const Json* name = node.find("name")) inst.name = name->str;
                const size_t mi = static_cast<size_t>(meshRef->num);
                for (const auto& kv : primMesh)
                    if (kv.first.first == mi) {
                        inst.mesh = kv.second.first;
                        inst.material = kv.second.second;
                        out.instances.push_back(inst);
                    }
            }
            if (const Json* ext = node.find("extensions"))
                if (const Json* khr = ext->find("KHR_lights_punctual")) {
                    const size_t li = static_cast<size_t>(khr->at("light").num);
                    if (li >= punctual.size()) fail("glb: a node refers to a KHR_lights_punctual light that does not exist");
                    AnalyticLight a = punctual[li];
                    // position: the node's world translation; direction: its -Z axis (the length is the device layer's to normalise)
                    for (int i = 0; i < 3; i++) {
                        a.position[i] = static_cast<float>(m.m[i][3]);
                        a.direction[i] = static_cast<float>(-m.m[i][2]);
                    }
                    out.analyticLights.push_back(a);
                }
            if (const Json* ch = node.find("children"))
                for (size_t k = 0; k < ch->size(); k++) walk(static_cast<size_t>(ch->at(k).num), m);
            depth--;
        }
    } walker{nodes, punctual, primMesh, out};
    const Json& scenes = doc.at("scenes");
    const Json& scene = scenes.at(static_cast<size_t>(doc.number("scene", 0)));
    const Json& roots = scene.at("nodes");
    for (size_t k = 0; k < roots.size(); k++) walker.walk(static_cast<size_t>(roots.at(k).num), M4::identity());
    for (const LoadedInstance& inst : out.instances)
        if (inst.material < 0 || static_cast<size_t>(inst.material) >= out.materials.size()) fail("glb: primitive refers to a material that does not exist");
    if (options.skins || options.morphs) read_skins(doc, accessor, primMesh, out, options);
    if (options.morphs) read_morphs(doc, primMesh, out);
    return out;
}

// Triangulated / polygonal Wavefront .obj (v / vn / vt / f, fan triangulation), one mesh, Assimp's default material
LoadedScene parse_obj(const std::string& file)
{
    std::ifstream f(file);
    if (!f) fail("cannot open " + file);
    std::vector<float3> v, vn;
    std::vector<float2> vt;
    struct Corner { long vi, ti, ni; };
    std::vector<Corner> faces;  // 3 per triangle
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        std::string tag;
        if (!(ss >> tag)) continue;
        if (tag == "v" || tag == "vn") {
            float3 p;
            if (!(ss >> p.x >> p.y >> p.z)) fail("obj: malformed " + tag + " line");
            (tag == "v" ? v : vn).push_back(p);
        } else if (tag == "vt") {
            float2 t;
            if (!(ss >> t.x >> t.y)) fail("obj: malformed vt line");
            vt.push_back(t);
        } else if (tag == "f") {
            std::vector<Corner> corners;
            std::string tok;
            while (ss >> tok) {
                Corner c{0, 0, 0};
                const size_t s1 = tok.find('/');
                c.vi = std::strtol(tok.substr(0, s1).c_str(), nullptr, 10);
                if (s1 != std::string::npos) {
                    const size_t s2 = tok.find('/', s1 + 1);
                    const std::string t = tok.substr(s1 + 1, s2 == std::string::npos ? std::string::npos : s2 - s1 - 1);
                    if (!t.empty()) c.ti = std::strtol(t.c_str(), nullptr, 10);
                    if (s2 != std::string::npos) {
                        const std::string n = tok.substr(s2 + 1);
                        if (!n.empty()) c.ni = std::strtol(n.c_str(), nullptr, 10);
                    }
                }
                corners.push_back(c);
            }
            for (size_t k = 1; k + 1 < corners.size(); k++) {
                faces.push_back(corners[0]);
                faces.push_back(corners[k]);
                faces.push_back(corners[k + 1]);
            }
        }
    }
    auto fix = [](long i, size_t n) -> size_t {
        const long r = i > 0 ? i - 1 : static_cast<long>(n) + i;
        if (r < 0 || static_cast<size_t>(r) >= n) fail("obj: index out of range");
        return static_cast<size_t>(r);
    };
    bool allN = !vn.empty(), allT = !vt.empty();
    for (const Corner& c : faces) {
        if (!c.ni) allN = false;
        if (!c.ti) allT = false;
    }
    std::vector<Triangle> tris;
    tris.reserve(faces.size() / 3);
    for (size_t t = 0; t + 2 < faces.size(); t += 3) {
        float3 p[3], n[3];
        float2 tc[3];
        for (int k = 0; k < 3; k++) p[k] = v[fix(faces[t + k].vi, v.size())];
        const float3 fn = allN ? make_float3(0.0f) : face_normal(p[0], p[1], p[2]);
        for (int k = 0; k < 3; k++) {
            n[k] = allN ? vn[fix(faces[t + k].ni, vn.size())] : fn;
            tc[k] = make_float2(0.0f, 0.0f);
            if (allT) {
                const float2 uv = vt[fix(faces[t + k].ti, vt.size())];
                tc[k] = make_float2(uv.x, 1.0f - uv.y);
            }
        }
        tris.emplace_back(p[0], p[1], p[2], n[0], n[1], n[2], tc[0], tc[1], tc[2]);
    }
    if (tris.empty()) fail("obj: " + file + " holds no faces");
    LoadedScene out;
    out.meshes.push_back(std::move(tris));
    out.meshNames.push_back(file);
    Material m;
    m.type = NX_MAT_PLASTIC;
    const double grey[3] = {0.6, 0.6, 0.6};
    set_albedo_like(m, grey, 1.0 - std::sqrt(20.0) / 31.62278, 1.45);
    m.intensity = 0.0f;
    out.materials.push_back(m);
    out.materialDiffuseTexture.push_back(-1);
    out.materialEmissiveTexture.push_back(-1);
    out.materialNormalTexture.push_back(-1);
    out.materialRoughnessTexture.push_back(-1);
    out.materialNormalScale.push_back(1.0f);
    LoadedInstance inst;
    inst.name = file;
    out.instances.push_back(inst);
    return out;
}

bool ends_with(const std::string& s, const char* suffix)
{
    const size_t n = std::strlen(suffix);
    if (s.size() < n) return false;
    for (size_t i = 0; i < n; i++)
        if (std::tolower(static_cast<unsigned char>(s[s.size() - n + i])) != suffix[i]) return false;
    return true;
}

}  // namespace

LoadedScene OBJLoader::Parse(const std::string& file, const LoadOptions& options)
{
    if (ends_with(file, ".glb")) return parse_glb(file, options);
    if (ends_with(file, ".obj")) return parse_obj(file);
    fail("unsupported file type (only .glb and .obj): " + file);
}

void OBJLoader::LoadOBJ(const std::string& path, const std::string& filename, Scene* scene, AssetManager* assetManager, const LoadOptions& options)
{
    const LoadedScene ls = Parse(path + filename, options);
    const int materialBase = static_cast<int>(assetManager->GetMaterials().size());
    // textures first: a material carries the id its map got in the manager's diffuse / emissive list (OBJLoader.cpp:134-135, 157-158)
    std::vector<int> textureIds(ls.textures.size(), -1);
    for (size_t i = 0; i < ls.textures.size(); i++) textureIds[i] = assetManager->AddTexture(ls.textures[i]);
    std::vector<int> detailIds(ls.detailTextures.size(), -1);
    for (size_t i = 0; i < ls.detailTextures.size(); i++) detailIds[i] = assetManager->AddTexture(ls.detailTextures[i]);
    for (size_t i = 0; i < ls.materials.size(); i++) {
        Material m = ls.materials[i];
        if (ls.materialDiffuseTexture[i] >= 0) m.diffuseMapId = textureIds[static_cast<size_t>(ls.materialDiffuseTexture[i])];
        if (ls.materialEmissiveTexture[i] >= 0) m.emissiveMapId = textureIds[static_cast<size_t>(ls.materialEmissiveTexture[i])];
        const int id = assetManager->AddMaterial(m);
        // detail maps: the ids their textures get in the manager's normal / roughness lists
        if (ls.materialNormalTexture[i] >= 0 || ls.materialRoughnessTexture[i] >= 0) {
            MaterialDetail d;
            if (ls.materialNormalTexture[i] >= 0) d.normalMapId = detailIds[static_cast<size_t>(ls.materialNormalTexture[i])];
            if (ls.materialRoughnessTexture[i] >= 0) d.roughnessMapId = detailIds[static_cast<size_t>(ls.materialRoughnessTexture[i])];
            d.normalScale = ls.materialNormalScale[i];
            assetManager->SetMaterialDetail(id, d);
        }
        if (i < ls.materialAlpha.size()) assetManager->SetMaterialAlpha(id, ls.materialAlpha[i]);
    }
    // one BVH8 per mesh of the file (OBJLoader.cpp:213-239) — created together, so that a device builder can build them in one go
    std::vector<int32_t> meshIds;
    const int32_t firstBvh = assetManager->CreateBVHs(ls.meshes);
    // skins, nodes and animations (LoadOptions::skins): the file's node indices become the scene's, behind the nodes of the files before it
    const int nodeBase = static_cast<int>(scene->GetNodes().size());
    if (!ls.nodes.empty()) {
        std::vector<SceneNode> nodes = ls.nodes;
        for (SceneNode& n : nodes)
            if (n.parent >= 0) n.parent += nodeBase;
        scene->AddNodes(nodes);
        for (Animation a : ls.animations) {
            for (AnimationChannel& c : a.channels) c.node += nodeBase;
            scene->AddAnimation(a);
        }
    }
    for (size_t i = 0; i < ls.meshes.size(); i++) {
        Mesh mesh(ls.meshNames[i], firstBvh + static_cast<int32_t>(i), -1);
        if (i < ls.skins.size() && ls.skins[i]) {
            mesh.skin = std::make_shared<Skin>(*ls.skins[i]);
            for (int& j : mesh.skin->joints) j += nodeBase;
            mesh.skin->meshNode += nodeBase;
        }
        if (i < ls.morphs.size() && ls.morphs[i]) {
            mesh.morph = std::make_shared<Morph>(*ls.morphs[i]);
            mesh.morph->meshNode += nodeBase;
        }
        meshIds.push_back(assetManager->AddMesh(std::move(mesh)));
    }
    for (const LoadedInstance& inst : ls.instances) {
        MeshInstance& mi = scene->CreateMeshInstance(static_cast<uint32_t>(meshIds[static_cast<size_t>(inst.mesh)]));
        mi.name = inst.name.empty() ? ls.meshNames[static_cast<size_t>(inst.mesh)] : inst.name;
        mi.AssignMaterial(materialBase + inst.material);
        mi.SetTransform(inst.position, inst.rotation, inst.scale);
    }
    for (const AnalyticLight& l : ls.analyticLights) scene->AddAnalyticLight(l);
}

}  // namespace nexus
