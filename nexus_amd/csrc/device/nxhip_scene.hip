// nxhip_scene.hip — scene upload: BLASes and the TLAS (uploaded, device-built, refitted), materials, lights, textures, environment tables.
// (the C-ABI device layer declared in include/nexus_hip.h; helpers shared with the other nxhip_*.hip units: nx_host.h)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "nx_host.h"

using namespace nxd;

extern "C" {

// ---- scene upload -----------------------------------------------------------------------------------

// 80-byte nodes at a stride of kNodeStride 16-byte chunks (5 = packed as uploaded)
static std::vector<uint4> pad_nodes(const nx_bvh8_node* nodes, uint32_t nodeCount)
{
    std::vector<uint4> out((size_t)nodeCount * kNodeStride, make_uint4(0u, 0u, 0u, 0u));
    for (uint32_t i = 0; i < nodeCount; i++) std::memcpy(&out[(size_t)i * kNodeStride], &nodes[i], sizeof(nx_bvh8_node));
    return out;
}

// The shading copy of a BLAS's triangles when they are kept one per kShadeTriStride bytes (nx_device.h): a strided device copy
// of the packed array.
static int make_shade_tris(BlasHost& b)
{
    if (kShadeTriStride == (int)sizeof(nx_triangle)) return NXHIP_OK;
    NX_ALLOC(b.shadeTris, (size_t)b.triCount * kShadeTriStride);
    NX_HIP(hipMemset(b.shadeTris.p, 0, (size_t)b.triCount * kShadeTriStride));
    NX_HIP(hipMemcpy2D(b.shadeTris.p, kShadeTriStride, b.tris.p, sizeof(nx_triangle), sizeof(nx_triangle), b.triCount, hipMemcpyDeviceToDevice));
    return NXHIP_OK;
}

static int refresh_blas_table(nxhip_ctx* c)
{
    std::vector<BlasDev> table(std::max<size_t>(1, c->blas.size()));
    std::memset(table.data(), 0, table.size() * sizeof(BlasDev));
    for (size_t i = 0; i < c->blas.size(); i++) {
        const BlasHost& b = c->blas[i];
        table[i].nodes = b.nodes.as<uint4>();
        table[i].isect = b.isect.as<float4>();
        table[i].tris = kShadeTriStride == (int)sizeof(nx_triangle) ? b.tris.as<nx_triangle>() : b.shadeTris.as<nx_triangle>();
        table[i].triIdx = b.triIdx.as<uint32_t>();
        table[i].nodeCount = b.nodeCount;
        table[i].triCount = b.triCount;
    }
    NX_SYNC_ALL(c);  // nothing may still read the old table
    NX_ALLOC(c->blasTable, table.size() * sizeof(BlasDev));
    NX_HIP(hipMemcpy(c->blasTable.p, table.data(), table.size() * sizeof(BlasDev), hipMemcpyHostToDevice));
    c->h.blas = c->blasTable.as<BlasDev>();
    c->stateDirty = true;
    c->shadeInstDirty = true;  // (the records hold the BLASes' triangle arrays)
    entry_inputs_changed(c);
    return NXHIP_OK;
}

}  // extern "C"

// The shading records of the instances (nx_device.h ShadeInst) from the instance, BLAS and material tables.  Called before a
// render when one of them has changed (shadeInstDirty); the cross-table indices have been checked by then (check_scene_ready).
// The matrices come from the DEVICE's instance table: nxhip_set_instance_transforms computes the inverses there.
// See-through for a shadow ray of NXHIP_SHADOWS_TRANSMIT (include/nexus_hip.h): `opacity < 1` — a NaN opacity is opaque, as in the
// material kernel — or a diffuse map that has a texel with alpha < 255.  (A map id without its texture: opaque by the map; no pass
// or hook launches with such a table — check_scene_ready.)
bool nxd::material_see_through(const nxhip_ctx* c, const nx_material& m)
{
    if (m.opacity < 1.0f) return true;
    return m.diffuseMapId >= 0 && (size_t)m.diffuseMapId < c->diffuseMaps.size() && c->diffuseMaps[(size_t)m.diffuseMapId].hasAlpha;
}

// After anything that can change the answer above: the material table, a diffuse texture upload, nxhip_clear_textures.
void nxd::refresh_see_through(nxhip_ctx* c)
{
    c->materialsSeeThrough = false;
    for (const nx_material& m : c->hostMaterials) c->materialsSeeThrough = c->materialsSeeThrough || material_see_through(c, m);
    c->shadeInstDirty = true;  // (ShadeInst::seeThrough)
}

// After anything that changes the detail table (nxhip_set_material_detail): does some material name a normal or a roughness map
// (kFlavorDetail reads the fact at every pass), and the per-instance records follow (refresh_shade_inst).
void nxd::refresh_detail_maps(nxhip_ctx* c)
{
    c->materialsNameDetail = false;
    for (const nx_material_detail& d : c->hostMaterialDetail) c->materialsNameDetail = c->materialsNameDetail || d.normalMapId != -1 || d.roughnessMapId != -1;
    c->shadeInstDirty = true;
}

// After anything that changes the alpha table (nxhip_set_material_alpha): is some material NX_ALPHA_MASK (kFlavorAlphaTest and the ray-batch
// hooks read the fact), is some material not NX_ALPHA_BLEND (kFlavorSolid), and the per-instance records follow (refresh_shade_inst: ShadeInst::alphaMode / alphaCutoff).
void nxd::refresh_alpha_modes(nxhip_ctx* c)
{
    c->materialsAlphaMask = c->materialsAlphaSolid = false;
    for (const nx_material_alpha& a : c->hostMaterialAlpha) {
        c->materialsAlphaMask = c->materialsAlphaMask || a.mode == (uint32_t)NX_ALPHA_MASK;
        c->materialsAlphaSolid = c->materialsAlphaSolid || a.mode != (uint32_t)NX_ALPHA_BLEND;
    }
    c->shadeInstDirty = true;
}

// What a render and the ray-batch hooks refuse about the alpha table: a count that is not the material count, and a MASK material on an
// instance that is a mesh light (the light sampler would pick points inside the holes).  Instance and material ids have been checked.
int nxd::check_alpha_table(const nxhip_ctx* c)
{
    if (c->hostMaterialAlpha.empty()) return NXHIP_OK;
    if (c->hostMaterialAlpha.size() != c->hostMaterials.size())
        return fail_invalid("the material alpha table does not have one entry per material (nxhip_set_material_alpha)");
    for (const nx_light& l : c->hostLights) {
        if (l.type != NX_LIGHT_MESH || l.mesh.meshId >= c->hostInstances.size()) continue;
        const int32_t m = c->hostInstances[l.mesh.meshId].materialId;
        if (m >= 0 && (size_t)m < c->hostMaterialAlpha.size() && c->hostMaterialAlpha[(size_t)m].mode == (uint32_t)NX_ALPHA_MASK)
            return fail_invalid("a mesh light's material is NX_ALPHA_MASK: holes in emitters are not supported (nxhip_set_material_alpha)");
    }
    return NXHIP_OK;
}

// The grid's words of the state block, from the context's grid and the medium's box: all 0 unless a medium with sigmaT > 0 AND a grid are
// set, so a grid alone, or a medium alone, leaves the block what it was.  vscale and bscale in binary64, rounded once.
void nxd::refresh_medium_grid(nxhip_ctx* c)
{
    DeviceState& h = c->h;
    h.mediumRho = nullptr;
    h.mediumBricks = nullptr;
    for (int k = 0; k < 3; k++) {
        h.mediumN[k] = h.mediumNb[k] = 0u;
        h.mediumVscale[k] = h.mediumBscale[k] = 0.0f;
    }
    h.padGrid0_ = h.padGrid1_ = 0u;
    h.padGrid2_ = h.padGrid3_ = 0.0f;
    if (h.mediumOn && c->mediumRho.p) {
        h.mediumRho = c->mediumRho.as<float>();
        h.mediumBricks = c->mediumBricks.as<float>();
        for (int k = 0; k < 3; k++) {
            const double extent = (double)h.medium.boxMax[k] - (double)h.medium.boxMin[k];
            h.mediumN[k] = c->mediumGridN[k];
            h.mediumNb[k] = (c->mediumGridN[k] + 7u) / 8u;
            h.mediumVscale[k] = (float)((double)c->mediumGridN[k] / extent);
            h.mediumBscale[k] = (float)((double)c->mediumGridN[k] / (8.0 * extent));
        }
    }
    c->stateDirty = true;  // (the pass graphs follow by their flavor: kFlavorMediumGrid)
}

// A render, and the hooks that walk, refuse a medium whose box is too deep for the walk's bound of 4096 iterations to stay out of reach.
int nxd::check_medium_grid(const nxhip_ctx* c, const char* who)
{
    if (!c->h.mediumOn || !c->h.mediumRho) return NXHIP_OK;
    double diag = 0.0;
    for (int k = 0; k < 3; k++) {
        const double e = (double)c->h.medium.boxMax[k] - (double)c->h.medium.boxMin[k];
        diag += e * e;
    }
    const double thickness = (double)c->h.medium.sigmaT * (double)c->mediumRhoMax * std::sqrt(diag);
    if (thickness > 512.0)
        return fail_invalid(std::string(who) + ": the medium's density grid is too thick: sigmaT x max(rho) x |boxMax - boxMin| = " + std::to_string(thickness) +
                            " exceeds 512 mean free paths (the tracking loop is bounded) - lower sigmaT, scale the grid's values down or shrink the box");
    return NXHIP_OK;
}

int nxd::refresh_shade_inst(nxhip_ctx* c)
{
    const size_t n = c->hostInstances.size();
    if (!c->hostMaterialDetail.empty() && c->hostMaterialDetail.size() != c->hostMaterialsDev.size())
        return fail_invalid("the material detail table does not have one entry per material (nxhip_set_material_detail)");
    if (!c->hostMaterialAlpha.empty() && c->hostMaterialAlpha.size() != c->hostMaterialsDev.size())
        return fail_invalid("the material alpha table does not have one entry per material (nxhip_set_material_alpha)");
    std::vector<nx_bvh_instance> inst(n);
    NX_SYNC_ALL(c);
    if (n) NX_HIP(hipMemcpy(inst.data(), c->instances.p, n * sizeof(nx_bvh_instance), hipMemcpyDeviceToHost));
    std::vector<ShadeInst> rec(std::max<size_t>(1, n));
    std::memset(rec.data(), 0, rec.size() * sizeof(ShadeInst));
    for (size_t i = 0; i < n; i++) {
        const nx_bvh_instance& in = inst[i];
        if (in.bvhIdx >= c->blas.size()) return fail_invalid("instance refers to a BLAS id that has not been uploaded");
        if (in.materialId < 0 || (size_t)in.materialId >= c->hostMaterialsDev.size()) return fail_invalid("an instance refers to a material id that has not been set");
        const BlasHost& b = c->blas[in.bvhIdx];
        std::memcpy(rec[i].transform, in.transform.cell, sizeof rec[i].transform);
        std::memcpy(rec[i].invTransform, in.invTransform.cell, sizeof rec[i].invTransform);
        rec[i].tris = kShadeTriStride == (int)sizeof(nx_triangle) ? b.tris.as<nx_triangle>() : b.shadeTris.as<nx_triangle>();
        rec[i].triCount = b.triCount;
        rec[i].materialId = in.materialId;
        rec[i].material = c->hostMaterialsDev[(size_t)in.materialId];
        rec[i].seeThrough = material_see_through(c, rec[i].material) ? 1u : 0u;
        if (!c->hostMaterialAlpha.empty()) {  // (none: NX_ALPHA_BLEND, cutoff 0 — the memset above)
            rec[i].alphaMode = c->hostMaterialAlpha[(size_t)in.materialId].mode;
            rec[i].alphaCutoff = c->hostMaterialAlpha[(size_t)in.materialId].cutoff;
            // (an OPAQUE material's crossing ends a TRANSMIT shadow ray with no fetch: the instance's existing test; a MASK material's
            //  is decided by the ALPHA_TEST instance before it looks here)
            if (rec[i].alphaMode == (uint32_t)NX_ALPHA_OPAQUE) rec[i].seeThrough = 0u;
        }
    }
    NX_ALLOC(c->shadeInst, rec.size() * sizeof(ShadeInst));
    NX_HIP(hipMemcpy(c->shadeInst.p, rec.data(), rec.size() * sizeof(ShadeInst), hipMemcpyHostToDevice));
    c->h.shadeInst = c->shadeInst.as<ShadeInst>();
    // the parallel array of detail records: entry i = the detail record of instance i's material; none while there is no table
    // (... unless a material is an NX_MAT_METALROUGH: its kernels are DETAIL instances and read the array, which then names no map)
    // (... or the SOLID instances are in use, which are DETAIL instances as well: materialsAlphaSolid)
    const bool metal = ((c->materialTypeMask >> NX_MAT_METALROUGH) & 1u) != 0u;
    if (c->hostMaterialDetail.empty() && !metal && !c->materialsAlphaSolid) {
        c->shadeDetail = DevBuf();
        c->h.shadeDetail = nullptr;
    } else {
        std::vector<nx_material_detail> det(std::max<size_t>(1, n), nx_material_detail{-1, -1, 1.0f, 0u});
        if (!c->hostMaterialDetail.empty())
            for (size_t i = 0; i < n; i++) det[i] = c->hostMaterialDetail[(size_t)rec[i].materialId];
        NX_ALLOC(c->shadeDetail, det.size() * sizeof(nx_material_detail));
        NX_HIP(hipMemcpy(c->shadeDetail.p, det.data(), det.size() * sizeof(nx_material_detail), hipMemcpyHostToDevice));
        c->h.shadeDetail = c->shadeDetail.as<nx_material_detail>();
    }
    c->stateDirty = true;
    c->shadeInstDirty = false;
    // the traversal records' material codes follow the shading records (nx_refit.hip inst_code_kernel)
    if (c->instTrav.p && !c->hostInstIdx.empty()) {
        entry_inputs_changed(c);  // (an entry state carries its instance's index + material code: InstTrav::instIdx)
        const uint32_t count = (uint32_t)c->hostInstIdx.size();
        NX_HIP(launch_untimed(kernels::inst_code(metal), (count + 255u) / 256u, 256, c->stream, c->dState.as<DeviceState>(), c->instTrav.as<InstTrav>(), c->shadeInst.as<ShadeInst>(), count));
        NX_HIP(hipStreamSynchronize(c->stream));
    }
    return NXHIP_OK;
}

extern "C" {

static int refresh_inst_trav(nxhip_ctx* c)
{
    // one record per TLAS leaf, in leaf order
    const size_t n = c->hostInstIdx.size();
    std::vector<InstTrav> trav(std::max<size_t>(1, n));
    std::memset(trav.data(), 0, trav.size() * sizeof(InstTrav));
    bool allIdentity = n > 0;
    for (size_t k = 0; k < n; k++) {
        const uint32_t i = c->hostInstIdx[k];
        const nx_bvh_instance& inst = c->hostInstances[i];
        if (inst.bvhIdx >= c->blas.size()) return fail_invalid("instance refers to a BLAS id that has not been uploaded");
        const float* m = inst.invTransform.cell;
        trav[k].r0 = make_float4(m[0], m[1], m[2], m[3]);
        trav[k].r1 = make_float4(m[4], m[5], m[6], m[7]);
        trav[k].r2 = make_float4(m[8], m[9], m[10], m[11]);
        BlasHost& b = c->blas[inst.bvhIdx];
        if (!b.rootKnown) {
            if (b.nodeCount) NX_HIP(hipMemcpy(b.root, b.nodes.p, sizeof b.root, hipMemcpyDeviceToHost));
            b.rootKnown = true;
        }
        trav[k].nodes = b.nodes.as<uint4>();
        trav[k].isect = b.isect.as<float4>();
        trav[k].instIdx = i;
        trav[k].flags = rows_are_identity(m) ? kInstIdentity : 0u;
        allIdentity = allIdentity && trav[k].flags != 0u;
        for (int q = 0; q < 5; q++) trav[k].root[q] = b.root[q];
    }
    NX_SYNC_ALL(c);
    NX_ALLOC(c->instTrav, trav.size() * sizeof(InstTrav));
    NX_HIP(hipMemcpy(c->instTrav.p, trav.data(), trav.size() * sizeof(InstTrav), hipMemcpyHostToDevice));
    c->h.instTrav = c->instTrav.as<InstTrav>();
    c->h.sceneFlags = allIdentity ? kSceneAllIdentity : 0u;
    c->stateDirty = true;
    entry_inputs_changed(c);
    c->shadeInstDirty = true;  // (the records' material codes are written when the shading records are rebuilt: refresh_shade_inst)
    return NXHIP_OK;
}

// What the traversal kernels assume of 8-wide nodes, checked before anything reaches the GPU (BLAS: primitives = triangles of
// the leaf-ordered list; TLAS: instances).  The kernels decode a slot from its META byte alone — bits 3 and 4 both set: an
// inner child whose hit bit goes to position 24 .. 31 and whose node is childBaseIdx + (imask bits below its slot); otherwise
// a leaf whose (meta >> 5) bits go to position (meta & 31) ... of the 24-bit primitive mask — so the check follows the meta
// bytes: an inner slot must be announced in imask and carry exactly one bit (more would land on other slots' positions and
// index one node past the children), a leaf's bits must stay below position 24 (beyond it they read as inner hits) and
// inside the primitive list, children must exist and follow their parent (no cycles: the traversal would never end).
static const char* wide_node_defect(const nx_bvh8_node& n, uint32_t i, uint32_t nodeCount, uint32_t primCount, bool childrenMustFollow)
{
    int inner = 0, prims = 0;
    for (int s = 0; s < 8; s++) {
        const uint32_t m = n.meta[s];
        if (n.imask & (1u << s)) inner++;
        if ((m & 0x18u) == 0x18u && (m >> 5) != 0u) {  // decoded as an inner child
            if (!(n.imask & (1u << s))) return "a slot is encoded as an inner child but not announced in imask";
            if ((m >> 5) != 1u) return "an inner slot carries more than one hit bit";
            if ((m & 0x07u) != (uint32_t)s) return "an inner slot is encoded with another slot's number";
        } else if (m >> 5) {  // decoded as a leaf of 1 .. 3 primitives at offset (m & 31)
            const int top = 32 - __builtin_clz(m >> 5);
            if ((int)(m & 0x1fu) + top > 24) return "a leaf slot's primitive bits leave the 24-bit primitive mask";
            prims = std::max(prims, (int)(m & 0x1fu) + top);
        }
    }
    if (inner && (uint64_t)n.childBaseIdx + (uint64_t)inner > nodeCount) return "child index out of range";
    if (childrenMustFollow && inner && n.childBaseIdx <= i) return "child nodes must follow their parent";
    if (prims && (uint64_t)n.triangleBaseIdx + (uint64_t)prims > primCount) return "leaf range out of range";
    return nullptr;
}
static const char* wide_nodes_defect(const nx_bvh8_node* nodes, uint32_t nodeCount, uint32_t primCount)
{
    for (uint32_t i = 0; i < nodeCount; i++)
        if (const char* defect = wide_node_defect(nodes[i], i, nodeCount, primCount, true)) return defect;
    return nullptr;
}

int nxhip_upload_blas(nxhip_ctx* c, const nx_bvh8_node* nodes, uint32_t nodeCount, const nx_triangle* tris, uint32_t triCount,
                      const uint32_t* triIdx, int32_t* blasId)
try {
    NX_CHECK_CTX(c);
    if (!nodes || !tris || !triIdx || nodeCount == 0 || triCount == 0) return fail_invalid("nxhip_upload_blas: empty input");
    NX_HIP(hipSetDevice(c->device));
    // validate what the kernels assume before anything reaches the GPU: indices in range
    for (uint32_t i = 0; i < triCount; i++)
        if (triIdx[i] >= triCount) return fail_invalid("nxhip_upload_blas: triangle index out of range");
    if (const char* defect = wide_nodes_defect(nodes, nodeCount, triCount)) return fail_invalid(std::string("nxhip_upload_blas: ") + defect);
    BlasHost b;
    b.nodeCount = nodeCount;
    b.triCount = triCount;
    // leaf-ordered intersection stream: {p0 | original index}, {edge0}, {edge1}; the edges are the same float
    // subtractions the reference performs per test (Triangle.cuh:55-56), done once here
    std::vector<float4> isect((size_t)triCount * kTriStride, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint32_t k = 0; k < triCount; k++) {
        const uint32_t t = triIdx[k];
        const nx_triangle& tr = tris[t];
        float idBits;
        std::memcpy(&idBits, &t, 4);
        isect[kTriStride * (size_t)k + 0] = make_float4(tr.pos0[0], tr.pos0[1], tr.pos0[2], idBits);
        isect[kTriStride * (size_t)k + 1] = make_float4(tr.pos1[0] - tr.pos0[0], tr.pos1[1] - tr.pos0[1], tr.pos1[2] - tr.pos0[2], 0.0f);
        isect[kTriStride * (size_t)k + 2] = make_float4(tr.pos2[0] - tr.pos0[0], tr.pos2[1] - tr.pos0[1], tr.pos2[2] - tr.pos0[2], 0.0f);
    }
    std::vector<uint4> padded = pad_nodes(nodes, nodeCount);
    NX_ALLOC(b.nodes, padded.size() * sizeof(uint4));
    NX_ALLOC(b.isect, isect.size() * sizeof(float4));
    NX_ALLOC(b.tris, (size_t)triCount * sizeof(nx_triangle));
    NX_ALLOC(b.triIdx, (size_t)triCount * 4);
    NX_HIP(hipMemcpy(b.nodes.p, padded.data(), padded.size() * sizeof(uint4), hipMemcpyHostToDevice));
    NX_HIP(hipMemcpy(b.isect.p, isect.data(), isect.size() * sizeof(float4), hipMemcpyHostToDevice));
    NX_HIP(hipMemcpy(b.tris.p, tris, (size_t)triCount * sizeof(nx_triangle), hipMemcpyHostToDevice));
    NX_HIP(hipMemcpy(b.triIdx.p, triIdx, (size_t)triCount * 4, hipMemcpyHostToDevice));
    if (const int rcs = make_shade_tris(b)) return rcs;
    c->blas.push_back(std::move(b));
    if (blasId) *blasId = (int32_t)c->blas.size() - 1;
    return refresh_blas_table(c);
} NX_CATCH("nxhip_upload_blas")

int nxhip_build_blas(nxhip_ctx* c, const nx_triangle* tris, uint32_t triCount, int32_t* blasId)
try {
    NX_CHECK_CTX(c);
    if (!tris || triCount == 0) return fail_invalid("nxhip_build_blas: empty input");
    if (kNodeStride != 5) return fail_invalid("nxhip_build_blas: built with padded node records");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    BlasHost b;
    b.triCount = triCount;
    NX_ALLOC(b.tris, (size_t)triCount * sizeof(nx_triangle));
    NX_HIP(hipMemcpy(b.tris.p, tris, (size_t)triCount * sizeof(nx_triangle), hipMemcpyHostToDevice));
    DevBuf wide;
    uint32_t nodeCount = 0;
    NX_TRY(lbvh_build(c, b.tris.as<nx_triangle>(), triCount, c->deviceBuilderRadius, wide, b.triIdx, b.isect, &nodeCount));
    NX_ALLOC(b.nodes, (size_t)nodeCount * sizeof(nx_bvh8_node));  // the builder's array is sized for the worst case
    NX_HIP(hipMemcpy(b.nodes.p, wide.p, (size_t)nodeCount * sizeof(nx_bvh8_node), hipMemcpyDeviceToDevice));
    b.nodeCount = nodeCount;
    if (const int rcs = make_shade_tris(b)) return rcs;
    c->blas.push_back(std::move(b));
    if (blasId) *blasId = (int32_t)c->blas.size() - 1;
    return refresh_blas_table(c);
} NX_CATCH("nxhip_build_blas")

int nxhip_build_blas_batch(nxhip_ctx* c, const nx_triangle* const* tris, const uint32_t* triCounts, uint32_t meshCount, int32_t* blasIds)
try {
    NX_CHECK_CTX(c);
    if (!tris || !triCounts || meshCount == 0) return fail_invalid("nxhip_build_blas_batch: empty input");
    if (kNodeStride != 5) return fail_invalid("nxhip_build_blas_batch: built with padded node records");
    uint64_t total = 0;
    for (uint32_t m = 0; m < meshCount; m++) {
        if (!tris[m] || triCounts[m] == 0) return fail_invalid("nxhip_build_blas_batch: a mesh without triangles");
        total += triCounts[m];
    }
    if (total > 0x7fffffffull) return fail_invalid("nxhip_build_blas_batch: more than 2^31 triangles in one batch");
    if (c->deviceBuilderRadius != NXHIP_BUILDER_SAH || meshCount == 1) {
        // the other builders (radix tree, clustering) have no forest form: one build per mesh
        for (uint32_t m = 0; m < meshCount; m++) {
            int32_t id = -1;
            NX_TRY(nxhip_build_blas(c, tris[m], triCounts[m], &id));
            if (blasIds) blasIds[m] = id;
        }
        return NXHIP_OK;
    }
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    // NX_TUNING_KNOBS=1 NX_BATCH_TIMING=1: where the call's time goes, to stderr (tools / tests only)
    const bool timing = std::getenv("NX_TUNING_KNOBS") && std::atoi(std::getenv("NX_TUNING_KNOBS")) == 1 && std::getenv("NX_BATCH_TIMING");
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto lap = [&](const char* what, std::chrono::steady_clock::time_point& t0) {
        if (!timing) return;
        (void)hipStreamSynchronize(c->stream);
        const auto t1 = now();
        std::fprintf(stderr, "[nxhip_build_blas_batch] %-34s %7.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    };
    auto tLap = now();
    // the triangles of all meshes, concatenated, through a pinned staging buffer the context keeps (one transfer instead of one
    // per mesh)
    const size_t bytes = (size_t)total * sizeof(nx_triangle);
    constexpr size_t kHalf = (size_t)16 << 20;  // two halves of a 32 MiB pinned buffer, allocated once per context: a staging buffer
                                                // as large as the batch would cost more to pin than the transfer takes
    if (!c->hostStaging) {
        NX_HIP(hipHostMalloc(&c->hostStaging, 2 * kHalf, hipHostMallocDefault));
        c->hostStagingBytes = 2 * kHalf;
        NX_HIP(hipEventCreateWithFlags(&c->stagingDone[0], hipEventDisableTiming));
        NX_HIP(hipEventCreateWithFlags(&c->stagingDone[1], hipEventDisableTiming));
    }
    std::vector<uint32_t> counts(triCounts, triCounts + meshCount);
    auto trisPool = std::make_shared<DevBuf>();
    auto nodesPool = std::make_shared<DevBuf>(), idxPool = std::make_shared<DevBuf>(), isectPool = std::make_shared<DevBuf>();
    if (!trisPool->alloc(bytes)) return NXHIP_ERR_HIP;
    {
        // the meshes as one byte stream through the two halves: while one half is on its way to the device the other is filled
        size_t sent = 0, inHalf = 0;
        int half = 0;
        bool used[2] = {false, false};
        char* const base = static_cast<char*>(c->hostStaging);
        auto flush = [&]() -> int {
            if (inHalf == 0) return NXHIP_OK;
            NX_HIP(hipMemcpyAsync(static_cast<char*>(trisPool->p) + sent, base + (size_t)half * kHalf, inHalf, hipMemcpyHostToDevice, c->stream));
            NX_HIP(hipEventRecord(c->stagingDone[half], c->stream));
            used[half] = true;
            sent += inHalf;
            inHalf = 0;
            half ^= 1;
            if (used[half]) NX_HIP(hipEventSynchronize(c->stagingDone[half]));  // the half about to be refilled has left
            return NXHIP_OK;
        };
        for (uint32_t m = 0; m < meshCount; m++) {
            const char* src = reinterpret_cast<const char*>(tris[m]);
            size_t left = (size_t)counts[m] * sizeof(nx_triangle);
            while (left) {
                const size_t take = std::min(left, kHalf - inHalf);
                std::memcpy(base + (size_t)half * kHalf + inHalf, src, take);
                inHalf += take;
                src += take;
                left -= take;
                if (inHalf == kHalf)
                    if (const int rcf = flush()) return rcf;
            }
        }
        if (const int rcf = flush()) return rcf;
    }
    std::vector<uint32_t> nodeFirst, nodeCounts;
    lap("triangles through pinned staging", tLap);
    NX_TRY(lbvh_build_batch(c, trisPool->as<nx_triangle>(), counts, *nodesPool, *idxPool, *isectPool, nodeFirst, nodeCounts));
    lap("device build", tLap);
    // every mesh's root node, for the instance records (refresh_inst_trav would otherwise fetch them one by one)
    std::vector<nx_bvh8_node> allNodes(nodesPool->bytes / sizeof(nx_bvh8_node));
    NX_HIP(hipMemcpy(allNodes.data(), nodesPool->p, allNodes.size() * sizeof(nx_bvh8_node), hipMemcpyDeviceToHost));
    size_t first = 0;
    for (uint32_t m = 0; m < meshCount; m++) {
        BlasHost b;
        b.triCount = counts[m];
        b.nodeCount = nodeCounts[m];
        b.nodes = DevBuf::view(nodesPool, (size_t)nodeFirst[m] * sizeof(nx_bvh8_node), (size_t)nodeCounts[m] * sizeof(nx_bvh8_node));
        b.isect = DevBuf::view(isectPool, first * kTriStride * sizeof(float4), (size_t)counts[m] * kTriStride * sizeof(float4));
        b.tris = DevBuf::view(trisPool, first * sizeof(nx_triangle), (size_t)counts[m] * sizeof(nx_triangle));
        b.triIdx = DevBuf::view(idxPool, first * 4, (size_t)counts[m] * 4);
        std::memcpy(b.root, &allNodes[nodeFirst[m]], sizeof b.root);
        b.rootKnown = true;
        if (const int rcs = make_shade_tris(b)) return rcs;
        c->blas.push_back(std::move(b));
        if (blasIds) blasIds[m] = (int32_t)c->blas.size() - 1;
        first += counts[m];
    }
    lap("roots read back, BLAS records", tLap);
    const int rcTable = refresh_blas_table(c);
    lap("BLAS table", tLap);
    return rcTable;
} NX_CATCH("nxhip_build_blas_batch")

int nxhip_read_blas_batch(nxhip_ctx* c, int32_t firstBlasId, uint32_t count, nx_bvh8_node* nodes, uint32_t nodeCapacity, uint32_t* nodeCounts, uint32_t* primIdx, uint32_t primCapacity)
{
    NX_CHECK_CTX(c);
    if (firstBlasId < 0 || (size_t)firstBlasId + count > c->blas.size()) return fail_invalid("nxhip_read_blas_batch: no such BLAS range");
    if (count == 0) return NXHIP_OK;
    if (kNodeStride != 5) return fail_invalid("nxhip_read_blas_batch: built with padded node records");
    uint64_t nodeTotal = 0, primTotal = 0;
    bool oneRun = true;  // the BLASes of one nxhip_build_blas_batch call lie back to back in their pools: one copy each for nodes and indices
    for (uint32_t k = 0; k < count; k++) {
        const BlasHost& b = c->blas[(size_t)firstBlasId + k];
        if (nodeCounts) nodeCounts[k] = b.nodeCount;
        if (k) {
            const BlasHost& a = c->blas[(size_t)firstBlasId + k - 1];
            oneRun = oneRun && a.nodes.pool && a.nodes.pool == b.nodes.pool && static_cast<char*>(a.nodes.p) + a.nodes.bytes == b.nodes.p &&
                     a.triIdx.pool == b.triIdx.pool && static_cast<char*>(a.triIdx.p) + a.triIdx.bytes == b.triIdx.p;
        }
        nodeTotal += b.nodeCount;
        primTotal += b.triCount;
    }
    if ((nodes && nodeCapacity < nodeTotal) || (primIdx && primCapacity < primTotal)) return fail_invalid("nxhip_read_blas_batch: destination too small");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    const BlasHost& b0 = c->blas[(size_t)firstBlasId];
    if (oneRun) {
        if (nodes) NX_HIP(hipMemcpy(nodes, b0.nodes.p, (size_t)nodeTotal * sizeof(nx_bvh8_node), hipMemcpyDeviceToHost));
        if (primIdx) NX_HIP(hipMemcpy(primIdx, b0.triIdx.p, (size_t)primTotal * 4, hipMemcpyDeviceToHost));
        return NXHIP_OK;
    }
    size_t nodeAt = 0, primAt = 0;
    for (uint32_t k = 0; k < count; k++) {
        const BlasHost& b = c->blas[(size_t)firstBlasId + k];
        if (nodes) NX_HIP(hipMemcpy(nodes + nodeAt, b.nodes.p, (size_t)b.nodeCount * sizeof(nx_bvh8_node), hipMemcpyDeviceToHost));
        if (primIdx) NX_HIP(hipMemcpy(primIdx + primAt, b.triIdx.p, (size_t)b.triCount * 4, hipMemcpyDeviceToHost));
        nodeAt += b.nodeCount;
        primAt += b.triCount;
    }
    return NXHIP_OK;
}

int nxhip_set_device_builder(nxhip_ctx* c, int clusteringRadius)
{
    NX_CHECK_CTX(c);
    if (clusteringRadius < NXHIP_BUILDER_SAH || clusteringRadius > 256) return fail_invalid("nxhip_set_device_builder: NXHIP_BUILDER_SAH (-1), 0 (radix tree) or a clustering radius up to 256");
    c->deviceBuilderRadius = clusteringRadius;
    return NXHIP_OK;
}

int nxhip_read_blas(nxhip_ctx* c, int32_t blasId, nx_bvh8_node* nodes, uint32_t nodeCapacity, uint32_t* primIdx, uint32_t primCapacity, uint32_t* nodeCount)
{
    NX_CHECK_CTX(c);
    if (blasId < 0 || (size_t)blasId >= c->blas.size()) return fail_invalid("nxhip_read_blas: no such BLAS");
    const BlasHost& b = c->blas[(size_t)blasId];
    if (nodeCount) *nodeCount = b.nodeCount;
    if ((nodes && nodeCapacity < b.nodeCount) || (primIdx && primCapacity < b.triCount)) return fail_invalid("nxhip_read_blas: destination too small");
    if (kNodeStride != 5) return fail_invalid("nxhip_read_blas: built with padded node records");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    if (nodes) NX_HIP(hipMemcpy(nodes, b.nodes.p, (size_t)b.nodeCount * sizeof(nx_bvh8_node), hipMemcpyDeviceToHost));
    if (primIdx) NX_HIP(hipMemcpy(primIdx, b.triIdx.p, (size_t)b.triCount * 4, hipMemcpyDeviceToHost));
    return NXHIP_OK;
}

int nxhip_debug_write_blas_node(nxhip_ctx* c, int32_t blasId, uint32_t nodeIdx, const nx_bvh8_node* node)
{
    NX_DEBUG_HOOK("nxhip_debug_write_blas_node");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    if (!node || blasId < 0 || (size_t)blasId >= c->blas.size()) return fail_invalid("nxhip_debug_write_blas_node: no such BLAS");
    BlasHost& b = c->blas[(size_t)blasId];
    if (nodeIdx >= b.nodeCount) return fail_invalid("nxhip_debug_write_blas_node: no such node");
    // the upload checks, as the traversal decodes a node (meta bytes), minus "children follow their parent": a node that points back
    // at itself is what the hook exists for (the stall guard's test); everything that could index past an array is refused
    if (const char* defect = wide_node_defect(*node, nodeIdx, b.nodeCount, b.triCount, false)) return fail_invalid(std::string("nxhip_debug_write_blas_node: ") + defect);
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    NX_HIP(hipMemcpy(b.nodes.as<uint4>() + (size_t)nodeIdx * kNodeStride, node, sizeof(nx_bvh8_node), hipMemcpyHostToDevice));
    entry_inputs_changed(c);
    if (nodeIdx == 0) {  // the root is also embedded in the instance records
        std::memcpy(b.root, node, sizeof b.root);
        b.rootKnown = true;
        if (!c->hostInstIdx.empty()) return refresh_inst_trav(c);
    }
    return NXHIP_OK;
}

int nxhip_debug_set_scan_epoch(nxhip_ctx* c, uint32_t epoch)
{
    NX_DEBUG_HOOK("nxhip_debug_set_scan_epoch");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    NX_SYNC_ALL(c);
    for (uint32_t k = 0; k < slot_count(c); k++) slot_at(c, k)->scanEpoch = std::min(epoch, kScanEpochLimit - 1u);
    return NXHIP_OK;
}

int nxhip_debug_keep_binary_tree(nxhip_ctx* c, int on)
try {
    NX_DEBUG_HOOK("nxhip_debug_keep_binary_tree");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    c->keepBinaryTree = on != 0;
    if (!on) c->binaryTree = nxhip_ctx::BinaryTreeStash{};
    return NXHIP_OK;
} NX_CATCH("nxhip_debug_keep_binary_tree")

int nxhip_debug_read_binary_tree(nxhip_ctx* c, uint32_t capacity, uint32_t* n, float* primCost, int32_t* builder, int32_t* left, int32_t* right, int32_t* parent, int32_t* count,
                                 float* box6, uint32_t* leafOrder, uint64_t* eval)
try {
    NX_DEBUG_HOOK("nxhip_debug_read_binary_tree");  // (first: a release library refuses whatever it is handed)
    NX_CHECK_CTX(c);
    if (!n) return fail_invalid("nxhip_debug_read_binary_tree: null n");
    const nxhip_ctx::BinaryTreeStash& s = c->binaryTree;
    if (!s.valid) return fail_invalid("nxhip_debug_read_binary_tree: no binary tree is stashed (nxhip_debug_keep_binary_tree, then a single build)");
    *n = s.n;
    if (primCost) *primCost = s.primCost;
    if (builder) *builder = s.builder;
    if (s.n == 0) return NXHIP_OK;
    if (capacity < s.n) return fail_invalid("nxhip_debug_read_binary_tree: capacity too small (*n holds the primitives of the stashed tree)");
    if (!left || !right || !parent || !count || !box6 || !leafOrder || !eval) return fail_invalid("nxhip_debug_read_binary_tree: null destination");
    std::memcpy(left, s.left.data(), s.left.size() * 4);
    std::memcpy(right, s.right.data(), s.right.size() * 4);
    std::memcpy(parent, s.parent.data(), s.parent.size() * 4);
    std::memcpy(count, s.count.data(), s.count.size() * 4);
    std::memcpy(box6, s.box.data(), s.box.size() * 4);
    std::memcpy(leafOrder, s.leafOrder.data(), s.leafOrder.size() * 4);
    std::memcpy(eval, s.eval.data(), s.eval.size() * 8);
    return NXHIP_OK;
} NX_CATCH("nxhip_debug_read_binary_tree")

int nxhip_clear_blas(nxhip_ctx* c)
try {
    NX_CHECK_CTX(c);
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    c->blas.clear();  // (with their refit plans)
    c->blasRefreshPending = false;
    c->tlasTightBoxes.release();
    c->hostInstances.clear();
    c->hostInstIdx.clear();
    c->h.tlasNodes = nullptr;
    c->h.instanceCount = 0;
    return refresh_blas_table(c);
} NX_CATCH("nxhip_clear_blas")

int nxhip_set_tlas(nxhip_ctx* c, const nx_bvh8_node* nodes, uint32_t nodeCount, const uint32_t* instanceIdx, const nx_bvh_instance* instances,
                   uint32_t instanceCount)
try {
    NX_CHECK_CTX(c);
    if (!nodes || !instanceIdx || !instances || nodeCount == 0 || instanceCount == 0) return fail_invalid("nxhip_set_tlas: empty input");
    if (instanceCount > kHitInstMask) return fail_invalid("nxhip_set_tlas: more than 2^29 - 1 instances (a hit record keeps the instance in 29 bits)");
    NX_HIP(hipSetDevice(c->device));
    for (uint32_t i = 0; i < instanceCount; i++) {
        if (instanceIdx[i] >= instanceCount) return fail_invalid("nxhip_set_tlas: instance index out of range");
        if (instances[i].bvhIdx >= c->blas.size()) return fail_invalid("nxhip_set_tlas: instance refers to a BLAS id that has not been uploaded");
    }
    // (checked here, before the context is touched: a failure must leave the previous TLAS and its traversal records in place)
    if (const char* defect = wide_nodes_defect(nodes, nodeCount, instanceCount)) return fail_invalid(std::string("nxhip_set_tlas: ") + defect);
    NX_SYNC_ALL(c);
    c->tlasTightBoxes.release();  // (a tree from outside: its boxes are the records')
    std::vector<uint4> padded = pad_nodes(nodes, nodeCount);
    NX_ALLOC(c->tlasNodes, padded.size() * sizeof(uint4));
    NX_ALLOC(c->tlasInstIdx, (size_t)instanceCount * 4);
    NX_ALLOC(c->instances, (size_t)instanceCount * sizeof(nx_bvh_instance));
    NX_HIP(hipMemcpy(c->tlasNodes.p, padded.data(), padded.size() * sizeof(uint4), hipMemcpyHostToDevice));
    NX_HIP(hipMemcpy(c->tlasInstIdx.p, instanceIdx, (size_t)instanceCount * 4, hipMemcpyHostToDevice));
    NX_HIP(hipMemcpy(c->instances.p, instances, (size_t)instanceCount * sizeof(nx_bvh_instance), hipMemcpyHostToDevice));
    c->hostInstances.assign(instances, instances + instanceCount);
    c->hostInstIdx.assign(instanceIdx, instanceIdx + instanceCount);
    c->h.tlasNodes = c->tlasNodes.as<uint4>();
    c->h.tlasInstIdx = c->tlasInstIdx.as<uint32_t>();
    c->h.instances = c->instances.as<nx_bvh_instance>();
    c->h.instanceCount = instanceCount;
    c->stateDirty = true;
    c->shadeInstDirty = true;
    c->lightTableDirty = true;
    entry_inputs_changed(c);
    {
        // schedule of the device-side refit (nxhip_set_instance_transforms): node indices grouped by depth, deepest first
        std::vector<uint32_t> depth(nodeCount, 0u);
        uint32_t maxDepth = 0;
        for (uint32_t i = 0; i < nodeCount; i++) {  // children follow their parent in the array: one ascending sweep
            const nx_bvh8_node& n = nodes[i];
            const uint32_t inner = (uint32_t)__builtin_popcount(n.imask);
            for (uint32_t k = 0; k < inner; k++) {
                depth[n.childBaseIdx + k] = depth[i] + 1;
                maxDepth = std::max(maxDepth, depth[i] + 1);
            }
        }
        std::vector<uint32_t> levelStart(maxDepth + 2, 0u), order(nodeCount);
        for (uint32_t i = 0; i < nodeCount; i++) levelStart[(maxDepth - depth[i]) + 1]++;
        for (uint32_t l = 0; l <= maxDepth; l++) levelStart[l + 1] += levelStart[l];
        std::vector<uint32_t> cursor(levelStart.begin(), levelStart.end() - 1);
        for (uint32_t i = 0; i < nodeCount; i++) order[cursor[maxDepth - depth[i]]++] = i;
        std::vector<uint32_t> leafOf(instanceCount, 0u);
        for (uint32_t k = 0; k < instanceCount; k++) leafOf[instanceIdx[k]] = k;
        NX_ALLOC(c->refitOrder, (size_t)nodeCount * 4);
        NX_ALLOC(c->refitLevelStart, levelStart.size() * 4);
        NX_ALLOC(c->leafOfInstance, (size_t)instanceCount * 4);
        NX_ALLOC(c->refitBoxes, (size_t)nodeCount * 24);
        NX_HIP(hipMemcpy(c->refitOrder.p, order.data(), order.size() * 4, hipMemcpyHostToDevice));
        NX_HIP(hipMemcpy(c->refitLevelStart.p, levelStart.data(), levelStart.size() * 4, hipMemcpyHostToDevice));
        NX_HIP(hipMemcpy(c->leafOfInstance.p, leafOf.data(), leafOf.size() * 4, hipMemcpyHostToDevice));
        c->h.leafOfInstance = c->leafOfInstance.as<uint32_t>();  // (also what a handed-over ray names its instance record by: ThinState::leaf)
        c->refitLevels = maxDepth + 1;
        c->tlasNodeCount = nodeCount;
    }
    return refresh_inst_trav(c);
} NX_CATCH("nxhip_set_tlas")

int nxhip_rebuild_tlas(nxhip_ctx* c, const nx_bvh_instance* instances, uint32_t instanceCount)
try {
    NX_CHECK_CTX(c);
    if (!instances || instanceCount == 0) return fail_invalid("nxhip_rebuild_tlas: empty input");
    if (kNodeStride != 5) return fail_invalid("nxhip_rebuild_tlas: built with padded node records");
    for (uint32_t i = 0; i < instanceCount; i++)
        if (instances[i].bvhIdx >= c->blas.size()) return fail_invalid("nxhip_rebuild_tlas: instance refers to a BLAS id that has not been uploaded");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    DevBuf dInst, wide, primIdx, boxes;
    bool boxesAreTight = false;
    NX_ALLOC(dInst, (size_t)instanceCount * sizeof(nx_bvh_instance));
    NX_HIP(hipMemcpy(dInst.p, instances, (size_t)instanceCount * sizeof(nx_bvh_instance), hipMemcpyHostToDevice));
    uint32_t nodeCount = 0;
    NX_TRY(lbvh_build_tlas(c, dInst.as<nx_bvh_instance>(), instanceCount, c->deviceBuilderRadius, wide, primIdx, boxes, &boxesAreTight, &nodeCount));
    // The tree is a few hundred nodes per thousand instances: it comes back once so that nxhip_set_tlas — range checks, the
    // traversal records in leaf order, the schedule of the device-side refit — installs it like any other TLAS.
    std::vector<nx_bvh8_node> nodes(nodeCount);
    std::vector<uint32_t> idx(instanceCount);
    NX_HIP(hipMemcpy(nodes.data(), wide.p, (size_t)nodeCount * sizeof(nx_bvh8_node), hipMemcpyDeviceToHost));
    NX_HIP(hipMemcpy(idx.data(), primIdx.p, (size_t)instanceCount * 4, hipMemcpyDeviceToHost));
    const int rc = nxhip_set_tlas(c, nodes.data(), nodeCount, idx.data(), instances, instanceCount);
    // the boxes the tree was built from stay with it: the device-side refit keeps using them instead of the records' looser ones
    if (rc == NXHIP_OK && boxesAreTight) c->tlasTightBoxes = std::move(boxes);
    return rc;
} NX_CATCH("nxhip_rebuild_tlas")

int nxhip_read_tlas_index(nxhip_ctx* c, uint32_t* instanceIdx, uint32_t capacity, uint32_t* nodeCount)
{
    NX_CHECK_CTX(c);
    if (!c->h.tlasNodes) return fail_invalid("nxhip_read_tlas_index: no TLAS has been set");
    if (nodeCount) *nodeCount = c->tlasNodeCount;
    if (instanceIdx) {
        if (capacity < c->hostInstIdx.size()) return fail_invalid("nxhip_read_tlas_index: destination too small");
        std::memcpy(instanceIdx, c->hostInstIdx.data(), c->hostInstIdx.size() * 4);
    }
    return NXHIP_OK;
}

// The two launches of the device-side refit, on the context's stream: BVHInstance::SetTransform for the `count` instances listed
// in `ids` (device; matrices in c->refitMatrices; blasRefresh: each keeps its own and only what follows its BLAS's root is redone),
// then the bottom-up sweep of the TLAS (nx_refit.hip).
static int launch_instance_transform(nxhip_ctx* c, const uint32_t* ids, uint32_t count, bool blasRefresh)
{
    // (the shading records follow the matrices when they are current; a stale set is rebuilt from the device's instance table)
    ShadeInst* shadeInst = c->shadeInstDirty ? nullptr : c->shadeInst.as<ShadeInst>();
    const unsigned grid = std::min<unsigned>((count + 255u) / 256u, (unsigned)c->wideBlocks);
    NX_HIP(launch_untimed(kernels::instance_transform(), grid, 256, c->stream, c->dState.as<DeviceState>(), c->instances.as<nx_bvh_instance>(), c->instTrav.as<InstTrav>(),
                          c->leafOfInstance.as<uint32_t>(), ids, c->refitMatrices.as<float>(), count, c->tlasTightBoxes.p, shadeInst, blasRefresh ? 1u : 0u));
    return NXHIP_OK;
}

static int launch_tlas_refit(nxhip_ctx* c)
{
    NX_HIP(launch_untimed(kernels::tlas_refit(), 1, 1024, c->stream, c->tlasNodes.as<nx_bvh8_node>(), c->tlasInstIdx.as<uint32_t>(), c->instances.as<nx_bvh_instance>(),
                          c->refitOrder.as<uint32_t>(), c->refitLevelStart.as<uint32_t>(), c->refitLevels, c->refitBoxes.p, c->tlasTightBoxes.p));
    return NXHIP_OK;
}

}  // extern "C"

// What follows a BLAS's root, brought up to date after nxhip_update_blas refitted some BLASes: for every instance of one of them
// (its matrix as it is) the world bounds, the tight box and the root-node copy of its traversal record, then ONE refit of the TLAS.
// Deferred to the next call that needs the scene — a render, the ray-batch hooks, nxhip_read_tlas — so that ten meshes updated in
// a frame pay it once; running it again changes nothing.  Works on a TLAS from nxhip_set_tlas and on a device-built one alike
// (the refit schedule and the tight boxes are the ones nxhip_set_instance_transforms uses).
int nxd::refresh_updated_blas(nxhip_ctx* c)
{
    if (!c->blasRefreshPending) return NXHIP_OK;
    if (!c->h.tlasNodes || c->refitLevels == 0 || c->hostInstances.empty()) return NXHIP_OK;  // (no TLAS yet: nxhip_set_tlas reads the new roots)
    std::vector<uint32_t> ids;
    for (size_t i = 0; i < c->hostInstances.size(); i++) {
        const uint32_t b = c->hostInstances[i].bvhIdx;
        if (b < c->blas.size() && c->blas[b].refreshPending) ids.push_back((uint32_t)i);
    }
    for (BlasHost& b : c->blas) b.refreshPending = false;
    c->blasRefreshPending = false;
    const uint32_t count = (uint32_t)ids.size();
    if (count == 0) return NXHIP_OK;
    NX_TRY(upload_state(c));
    // the list goes up when it differs from the last refresh's (the same meshes deforming frame after frame: never again)
    if (ids != c->blasRefreshIds || !c->blasRefreshIdsDev.p) {
        NX_SYNC_ALL(c);
        if (c->blasRefreshIdsDev.bytes < (size_t)count * 4) NX_ALLOC(c->blasRefreshIdsDev, (size_t)count * 4);
        NX_HIP(hipMemcpy(c->blasRefreshIdsDev.p, ids.data(), (size_t)count * 4, hipMemcpyHostToDevice));
        c->blasRefreshIds.swap(ids);
    }
    NX_TRY(launch_instance_transform(c, c->blasRefreshIdsDev.as<uint32_t>(), count, true));
    NX_TRY(launch_tlas_refit(c));
    entry_inputs_changed(c);  // (the instances' root copies and the TLAS's boxes)
    // passes on the other slots' streams must not start on the old bounds
    if (slot_count(c) > 1) NX_HIP(hipStreamSynchronize(c->stream));
    return NXHIP_OK;
}

extern "C" {

int nxhip_set_instance_transforms(nxhip_ctx* c, const uint32_t* instanceIds, const float* transforms16, uint32_t count)
try {
    NX_CHECK_CTX(c);
    if (count == 0) return NXHIP_OK;
    if (!instanceIds || !transforms16) return fail_invalid("nxhip_set_instance_transforms: null argument");
    if (!c->h.tlasNodes || c->refitLevels == 0) return fail_invalid("nxhip_set_instance_transforms: no TLAS has been set");
    for (uint32_t i = 0; i < count; i++)
        if (instanceIds[i] >= c->h.instanceCount) return fail_invalid("nxhip_set_instance_transforms: instance id out of range");
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(upload_state(c));
    if (slot_count(c) > 1) NX_SYNC_ALL(c);  // passes on the other slots' streams still traverse the old placement
    if (c->refitIds.bytes < (size_t)count * 4) NX_ALLOC(c->refitIds, (size_t)count * 4);
    if (c->refitMatrices.bytes < (size_t)count * 64) NX_ALLOC(c->refitMatrices, (size_t)count * 64);
    // stream order does the rest: a frame already in flight finishes with the old placement, the next one sees the new
    NX_HIP(hipMemcpyAsync(c->refitIds.p, instanceIds, (size_t)count * 4, hipMemcpyHostToDevice, c->stream));
    NX_HIP(hipMemcpyAsync(c->refitMatrices.p, transforms16, (size_t)count * 64, hipMemcpyHostToDevice, c->stream));
    NX_TRY(launch_instance_transform(c, c->refitIds.as<uint32_t>(), count, false));
    NX_TRY(launch_tlas_refit(c));
    entry_inputs_changed(c);  // (the instance records, their identity flags, the TLAS's boxes)
    // pageable host arrays: the copies above are staged before hipMemcpyAsync returns on this runtime, but that is not a
    // documented guarantee — wait, the call is not on the per-frame path
    NX_SYNC_ALL(c);
    for (uint32_t i = 0; i < count; i++) std::memcpy(c->hostInstances[instanceIds[i]].transform.cell, transforms16 + 16 * (size_t)i, 64);
    c->lightTableDirty = true;  // (a scale changes areas)
    // The kernel has set each moved record's identity flag from the inverse it computed.  The scene-wide "no instance transforms
    // a ray" flag is the host's to keep: it survives only if every new matrix is the identity itself (whose inverse, by the
    // cofactor formula, is the identity bit for bit).
    if (c->h.sceneFlags & kSceneAllIdentity) {
        bool still = true;
        for (uint32_t i = 0; i < count && still; i++) {
            const float* m = transforms16 + 16 * (size_t)i;
            still = rows_are_identity(m) && m[12] == 0.0f && m[13] == 0.0f && m[14] == 0.0f && m[15] == 1.0f;
        }
        if (!still) {
            c->h.sceneFlags &= ~kSceneAllIdentity;
            c->stateDirty = true;
        }
    }
    return NXHIP_OK;
} NX_CATCH("nxhip_set_instance_transforms")

// The refit plan of a BLAS (BlasHost::refitOrder ...): the one place where the tree comes back to the host, once per BLAS.  Depth is
// derived from the tree itself, root down — a device-built tree need not number children after their parents.
static int ensure_blas_refit_plan(nxhip_ctx* c, BlasHost& b)
{
    if (!b.refitLevels.empty()) return NXHIP_OK;
    if (kNodeStride != 5) return fail_invalid("nxhip_update_blas: built with padded node records");
    NX_SYNC_ALL(c);
    std::vector<nx_bvh8_node> nodes(b.nodeCount);
    NX_HIP(hipMemcpy(nodes.data(), b.nodes.p, (size_t)b.nodeCount * sizeof(nx_bvh8_node), hipMemcpyDeviceToHost));
    constexpr uint32_t kUnseen = 0xffffffffu;
    std::vector<uint32_t> depth(b.nodeCount, kUnseen), queue;
    queue.reserve(b.nodeCount);
    queue.push_back(0u);
    depth[0] = 0;
    uint32_t maxDepth = 0;
    for (size_t at = 0; at < queue.size(); at++) {  // breadth first: `queue` ends up sorted by depth
        const uint32_t i = queue[at];
        // (what the kernel will index with, checked like an upload: nothing it reads may lie outside the BLAS's arrays)
        if (const char* defect = wide_node_defect(nodes[i], i, b.nodeCount, b.triCount, false)) return fail_invalid(std::string("nxhip_update_blas: ") + defect);
        const uint32_t inner = (uint32_t)__builtin_popcount(nodes[i].imask);
        for (uint32_t k = 0; k < inner; k++) {
            const uint32_t child = nodes[i].childBaseIdx + k;
            if (depth[child] != kUnseen) return fail_invalid("nxhip_update_blas: the BLAS is not a tree (a node has two parents)");
            depth[child] = depth[i] + 1;
            maxDepth = std::max(maxDepth, depth[child]);
            queue.push_back(child);
        }
    }
    // deepest level first; nodes no parent names (none in a builder's output) are left alone
    std::vector<uint32_t> levelStart(maxDepth + 2, 0u), order(queue.size());
    for (const uint32_t i : queue) levelStart[(maxDepth - depth[i]) + 1]++;
    for (uint32_t l = 0; l <= maxDepth; l++) levelStart[l + 1] += levelStart[l];
    std::vector<uint32_t> cursor(levelStart.begin(), levelStart.end() - 1);
    for (const uint32_t i : queue) order[cursor[maxDepth - depth[i]]++] = i;
    NX_ALLOC(b.refitOrder, order.size() * 4);
    NX_ALLOC(b.refitLevelStart, levelStart.size() * 4);
    NX_ALLOC(b.refitBoxes, (size_t)b.nodeCount * 32);
    NX_HIP(hipMemcpy(b.refitOrder.p, order.data(), order.size() * 4, hipMemcpyHostToDevice));
    NX_HIP(hipMemcpy(b.refitLevelStart.p, levelStart.data(), levelStart.size() * 4, hipMemcpyHostToDevice));
    b.refitLevels = std::move(levelStart);
    return NXHIP_OK;
}

// A level of more than kBlasRefitWide nodes gets a grid launch of its own: below that a single 256-thread workgroup covers it
// in at most four strides, and a launch (~5 us of latency between dependent kernels) costs more than the stride it would save.
constexpr uint32_t kBlasRefitWide = 1024, kBlasRefitBlock = 256;

// What follows new triangles in b.tris and b.isect, whoever wrote them (update_blas: a copy and isect_kernel; nxhip_pose_blas: the
// pose kernel): the nodes refitted level by level on the context's stream, and everything that embeds the BLAS marked stale.
static int refit_blas_nodes(nxhip_ctx* c, BlasHost& b)
{
    const uint32_t levels = (uint32_t)b.refitLevels.size() - 1u;
    auto width = [&](uint32_t l) { return b.refitLevels[l + 1] - b.refitLevels[l]; };
    for (uint32_t first = 0; first < levels;) {
        uint32_t count = 1;
        unsigned grid = 1;
        if (width(first) > kBlasRefitWide) {
            grid = std::min<unsigned>((width(first) + kBlasRefitBlock - 1u) / kBlasRefitBlock, (unsigned)(8 * std::max(1, c->numCUs)));
        } else {
            while (first + count < levels && width(first + count) <= kBlasRefitWide) count++;  // the run of narrow levels: one workgroup
        }
        NX_HIP(launch_untimed(kernels::blas_refit(), grid, kBlasRefitBlock, c->stream, b.nodes.as<uint4>(), b.triIdx.as<uint32_t>(), b.tris.as<nx_triangle>(),
                              b.refitOrder.as<uint32_t>(), b.refitLevelStart.as<uint32_t>(), first, count, b.refitBoxes.p));
        first += count;
    }
    b.rootKnown = false;  // (read again by whoever next needs the host copy: refresh_inst_trav)
    b.refreshPending = true;
    entry_inputs_changed(c);  // (the BLAS's nodes and triangle records; the deferred refresh bumps again for what follows its root)
    c->blasRefreshPending = true;
    c->lightTableDirty = true;
    return NXHIP_OK;
}

static int update_blas(nxhip_ctx* c, int32_t blasId, const void* tris, uint32_t triCount, bool fromDevice, const char* who)
{
    NX_CHECK_CTX(c);
    if (blasId < 0 || (size_t)blasId >= c->blas.size()) return fail_invalid(std::string(who) + ": no such BLAS");
    if (!tris) return fail_invalid(std::string(who) + ": null triangles");
    BlasHost& b = c->blas[(size_t)blasId];
    if (triCount != b.triCount) return fail_invalid(std::string(who) + ": the triangle count differs from the BLAS's (a refit keeps the topology)");
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(ensure_blas_refit_plan(c, b));
    if (slot_count(c) > 1) NX_SYNC_ALL(c);  // passes on the other slots' streams still traverse the old shape
    // stream order does the rest: a pass already issued finishes with the old triangles, the next one sees the new
    const size_t bytes = (size_t)triCount * sizeof(nx_triangle);
    NX_HIP(hipMemcpyAsync(b.tris.p, tris, bytes, fromDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    if (kShadeTriStride != (int)sizeof(nx_triangle))
        NX_HIP(hipMemcpy2DAsync(b.shadeTris.p, kShadeTriStride, b.tris.p, sizeof(nx_triangle), sizeof(nx_triangle), triCount, hipMemcpyDeviceToDevice, c->stream));
    NX_TRY(lbvh_write_isect(c, b.tris.as<nx_triangle>(), b.triIdx.as<uint32_t>(), triCount, b.isect.as<float4>()));
    NX_TRY(refit_blas_nodes(c, b));
    // a pageable host array: see nxhip_set_instance_transforms
    if (!fromDevice) NX_HIP(hipStreamSynchronize(c->stream));
    return NXHIP_OK;
}

int nxhip_update_blas(nxhip_ctx* c, int32_t blasId, const nx_triangle* tris, uint32_t triCount)
try {
    return update_blas(c, blasId, tris, triCount, false, "nxhip_update_blas");
} NX_CATCH("nxhip_update_blas")

int nxhip_update_blas_device(nxhip_ctx* c, int32_t blasId, const void* trisDevice, uint32_t triCount)
try {
    return update_blas(c, blasId, trisDevice, triCount, true, "nxhip_update_blas_device");
} NX_CATCH("nxhip_update_blas_device")

// ---- skinned meshes and morph targets (nx_skin.hip) ------------------------------------------------------
// The bind copy (BlasHost::bindTris) belongs to the skin and the morph together: the one that is set on a BLAS with neither takes it from
// the current triangles (and so does a skin set again on a BLAS that has only a skin, a morph on one that has only a morph); the one that
// finds the other present keeps it, so that both describe one shape; the last of the two to go frees it.

int nxhip_set_blas_skin(nxhip_ctx* c, int32_t blasId, const nx_skin_corner* corners, uint32_t cornerCount, uint32_t jointCount)
try {
    NX_CHECK_CTX(c);
    if (blasId < 0 || (size_t)blasId >= c->blas.size()) return fail_invalid("nxhip_set_blas_skin: no such BLAS");
    BlasHost& b = c->blas[(size_t)blasId];
    NX_HIP(hipSetDevice(c->device));
    if (!corners) {  // the skin goes; triangles and nodes stay as they are
        NX_SYNC_ALL(c);  // (a pose in flight still reads the buffers)
        if (b.morphTargets == 0) b.bindTris.release();
        b.skinTris.release();
        b.palette.release();
        b.skinJoints = 0;
        return NXHIP_OK;
    }
    if ((uint64_t)cornerCount != 3ull * b.triCount) return fail_invalid("nxhip_set_blas_skin: the corner count is not 3 x the BLAS's triangle count");
    if (jointCount == 0 || jointCount > 65536u) return fail_invalid("nxhip_set_blas_skin: the joint count must be 1 .. 65536");
    // everything the kernel will index with, and the weights it will use, before anything is allocated
    std::vector<SkinTri> packed(b.triCount);
    std::memset(packed.data(), 0, packed.size() * sizeof(SkinTri));
    for (uint32_t i = 0; i < cornerCount; i++) {
        const nx_skin_corner& s = corners[i];
        double sum = 0.0;
        for (int k = 0; k < 4; k++) {
            if (!std::isfinite(s.weight[k]) || s.weight[k] < 0.0f) return fail_invalid("nxhip_set_blas_skin: corner " + std::to_string(i) + " has a weight that is negative or not finite");
            if (s.weight[k] != 0.0f && s.joint[k] >= jointCount) return fail_invalid("nxhip_set_blas_skin: corner " + std::to_string(i) + " names joint " + std::to_string(s.joint[k]) + " of " + std::to_string(jointCount));
            sum += (double)s.weight[k];
        }
        if (!(sum > 0.0)) return fail_invalid("nxhip_set_blas_skin: the weights of corner " + std::to_string(i) + " sum to 0");
        SkinTri& t = packed[i / 3];
        for (int k = 0; k < 4; k++) {
            t.weight[i % 3][k] = (float)((double)s.weight[k] / sum);  // sum 1 in binary64, rounded once
            t.joint[i % 3][k] = s.weight[k] != 0.0f ? s.joint[k] : (uint16_t)0;  // (read unconditionally by the kernel)
        }
    }
    DevBuf bind, skin, palette;
    const bool takeBind = b.morphTargets == 0;  // (a morph is there: its deltas are relative to the copy it holds)
    const size_t triBytes = (size_t)b.triCount * sizeof(nx_triangle), skinBytes = packed.size() * sizeof(SkinTri);
    if ((takeBind && !bind.alloc(triBytes)) || !skin.alloc(skinBytes) || !palette.alloc((size_t)jointCount * 48)) return NXHIP_ERR_HIP;
    // the bind copy: the triangles as they are behind everything issued so far (an update or a pose on the stream included)
    if (takeBind) NX_HIP(hipMemcpyAsync(bind.p, b.tris.p, triBytes, hipMemcpyDeviceToDevice, c->stream));
    NX_HIP(hipMemcpyAsync(skin.p, packed.data(), skinBytes, hipMemcpyHostToDevice, c->stream));
    NX_HIP(hipStreamSynchronize(c->stream));  // (`packed` is pageable; and a previous skin's buffers are read by this stream only)
    if (takeBind) b.bindTris = std::move(bind);
    b.skinTris = std::move(skin);
    b.palette = std::move(palette);
    b.skinJoints = jointCount;
    return NXHIP_OK;
} NX_CATCH("nxhip_set_blas_skin")

// What both pose calls issue behind their checks, in stream order as in update_blas: the palette (skinned: jointMatrices) and the active
// targets (morph: `active`, (index, weight) pairs), ONE pose kernel, the refit, and the wait for the pageable arrays.  A skinned pose with no
// active target is nxhip_pose_blas's kernel whoever asks: "the pose with all weights 0" has its bits by construction.
static int issue_pose(nxhip_ctx* c, BlasHost& b, const float* jointMatrices, const std::vector<uint2>* active)
{
    NX_HIP(hipSetDevice(c->device));
    NX_TRY(ensure_blas_refit_plan(c, b));
    if (slot_count(c) > 1) NX_SYNC_ALL(c);  // passes on the other slots' streams still traverse the old shape
    const bool skinned = jointMatrices != nullptr;
    const uint32_t jointCount = skinned ? b.skinJoints : 0u, activeCount = active ? (uint32_t)active->size() : 0u;
    if (skinned) NX_HIP(hipMemcpyAsync(b.palette.p, jointMatrices, (size_t)jointCount * 48, hipMemcpyHostToDevice, c->stream));
    if (activeCount) NX_HIP(hipMemcpyAsync(b.morphActive.p, active->data(), (size_t)activeCount * 8, hipMemcpyHostToDevice, c->stream));
    const bool lds = skinned && jointCount <= kSkinLdsJoints;
    constexpr unsigned kPoseBlock = 256;
    const unsigned grid = std::min<unsigned>((b.triCount + kPoseBlock - 1u) / kPoseBlock, (unsigned)(8 * std::max(1, c->numCUs)));
    uint4* const shade = kShadeTriStride == (int)sizeof(nx_triangle) ? nullptr : b.shadeTris.as<uint4>();
    const size_t ldsBytes = lds ? (size_t)jointCount * 48 : 0;
    if (skinned && activeCount == 0) {
        NX_HIP(launch_untimed_lds(kernels::pose(lds), grid, kPoseBlock, ldsBytes, c->stream, b.bindTris.as<uint4>(), b.skinTris.as<uint4>(), b.palette.as<float4>(), jointCount,
                                  b.triIdx.as<uint32_t>(), b.triCount, b.tris.as<uint4>(), shade, b.isect.as<float4>()));
    } else {  // (unskinned with no active target: the morph-only instance skips its stage and writes the bind copy back)
        NX_HIP(launch_untimed_lds(kernels::pose_morph(skinned, lds), grid, kPoseBlock, ldsBytes, c->stream, b.bindTris.as<uint4>(), b.skinTris.as<uint4>(), b.palette.as<float4>(),
                                  jointCount, b.triIdx.as<uint32_t>(), b.triCount, b.tris.as<uint4>(), shade, b.isect.as<float4>(), b.morphTris.as<uint4>(),
                                  b.morphActive.as<uint2>(), activeCount));
    }
    NX_TRY(refit_blas_nodes(c, b));
    NX_HIP(hipStreamSynchronize(c->stream));  // pageable host arrays: see nxhip_set_instance_transforms
    return NXHIP_OK;
}

// the joint matrices of a pose of skinned BLAS b, as both pose calls check them
static int check_palette(const BlasHost& b, const float* jointMatrices, uint32_t jointCount, const std::string& who)
{
    if (!jointMatrices) return fail_invalid(who + ": null matrices");
    if (jointCount != b.skinJoints) return fail_invalid(who + ": the joint count differs from the skin's");
    for (size_t i = 0; i < (size_t)jointCount * 12; i++)
        if (!std::isfinite(jointMatrices[i])) return fail_invalid(who + ": a matrix entry is not finite");
    return NXHIP_OK;
}

int nxhip_pose_blas(nxhip_ctx* c, int32_t blasId, const float* jointMatrices, uint32_t jointCount)
try {
    NX_CHECK_CTX(c);
    if (blasId < 0 || (size_t)blasId >= c->blas.size()) return fail_invalid("nxhip_pose_blas: no such BLAS");
    BlasHost& b = c->blas[(size_t)blasId];
    if (b.skinJoints == 0) return fail_invalid("nxhip_pose_blas: the BLAS has no skin (nxhip_set_blas_skin)");
    NX_TRY(check_palette(b, jointMatrices, jointCount, "nxhip_pose_blas"));
    return issue_pose(c, b, jointMatrices, nullptr);
} NX_CATCH("nxhip_pose_blas")

int nxhip_set_blas_morph(nxhip_ctx* c, int32_t blasId, const nx_morph_corner* deltas, uint32_t cornerCount, uint32_t targetCount)
try {
    NX_CHECK_CTX(c);
    if (blasId < 0 || (size_t)blasId >= c->blas.size()) return fail_invalid("nxhip_set_blas_morph: no such BLAS");
    BlasHost& b = c->blas[(size_t)blasId];
    NX_HIP(hipSetDevice(c->device));
    if (!deltas) {  // the morph goes; triangles and nodes stay as they are
        NX_SYNC_ALL(c);  // (a pose in flight still reads the buffers)
        if (b.skinJoints == 0) b.bindTris.release();
        b.morphTris.release();
        b.morphActive.release();
        b.morphTargets = 0;
        return NXHIP_OK;
    }
    if ((uint64_t)cornerCount != 3ull * b.triCount) return fail_invalid("nxhip_set_blas_morph: the corner count is not 3 x the BLAS's triangle count");
    if (targetCount == 0 || targetCount > kMorphMaxTargets) return fail_invalid("nxhip_set_blas_morph: the target count must be 1 .. " + std::to_string(kMorphMaxTargets));
    // every delta the kernel will add, before anything is allocated
    const size_t records = (size_t)targetCount * b.triCount;
    std::vector<MorphTri> packed(records);
    std::memset(packed.data(), 0, packed.size() * sizeof(MorphTri));
    for (size_t i = 0; i < (size_t)targetCount * cornerCount; i++) {
        const nx_morph_corner& d = deltas[i];
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(d.dPosition[a]) || !std::isfinite(d.dNormal[a]))
                return fail_invalid("nxhip_set_blas_morph: corner " + std::to_string(i % cornerCount) + " of target " + std::to_string(i / cornerCount) + " has a delta that is not finite");
        MorphTri& t = packed[i / 3];  // (cornerCount = 3 x triCount: record t * triCount + triangle)
        std::memcpy(t.dPosition[i % 3], d.dPosition, 12);
        std::memcpy(t.dNormal[i % 3], d.dNormal, 12);
    }
    DevBuf bind, morph, active;
    const bool takeBind = b.skinJoints == 0;  // (a skin is there: it is relative to the copy it holds)
    const size_t triBytes = (size_t)b.triCount * sizeof(nx_triangle), morphBytes = records * sizeof(MorphTri);
    if ((takeBind && !bind.alloc(triBytes)) || !morph.alloc(morphBytes) || !active.alloc((size_t)targetCount * 8)) return NXHIP_ERR_HIP;
    if (takeBind) NX_HIP(hipMemcpyAsync(bind.p, b.tris.p, triBytes, hipMemcpyDeviceToDevice, c->stream));
    NX_HIP(hipMemcpyAsync(morph.p, packed.data(), morphBytes, hipMemcpyHostToDevice, c->stream));
    NX_HIP(hipStreamSynchronize(c->stream));  // (`packed` is pageable; and a previous morph's buffers are read by this stream only)
    if (takeBind) b.bindTris = std::move(bind);
    b.morphTris = std::move(morph);
    b.morphActive = std::move(active);
    b.morphTargets = targetCount;
    return NXHIP_OK;
} NX_CATCH("nxhip_set_blas_morph")

int nxhip_pose_blas_morph(nxhip_ctx* c, int32_t blasId, const float* weights, uint32_t targetCount, const float* jointMatrices, uint32_t jointCount)
try {
    NX_CHECK_CTX(c);
    if (blasId < 0 || (size_t)blasId >= c->blas.size()) return fail_invalid("nxhip_pose_blas_morph: no such BLAS");
    BlasHost& b = c->blas[(size_t)blasId];
    if (b.morphTargets == 0) return fail_invalid("nxhip_pose_blas_morph: the BLAS has no morph (nxhip_set_blas_morph)");
    if (!weights) return fail_invalid("nxhip_pose_blas_morph: null weights");
    if (targetCount != b.morphTargets) return fail_invalid("nxhip_pose_blas_morph: the target count differs from the morph's");
    const bool skinned = b.skinJoints != 0;
    if (skinned) NX_TRY(check_palette(b, jointMatrices, jointCount, "nxhip_pose_blas_morph (the BLAS is skinned)"));
    else if (jointMatrices || jointCount != 0) return fail_invalid("nxhip_pose_blas_morph: the BLAS has no skin: the matrices must be NULL and their count 0");
    // the active targets: weight not 0, ascending index — the only ones the kernel visits
    std::vector<uint2> active;
    for (uint32_t t = 0; t < targetCount; t++) {
        if (!std::isfinite(weights[t])) return fail_invalid("nxhip_pose_blas_morph: weight " + std::to_string(t) + " is not finite");
        if (weights[t] != 0.0f) {
            uint32_t bits;
            std::memcpy(&bits, &weights[t], 4);
            active.push_back(make_uint2(t, bits));
        }
    }
    return issue_pose(c, b, skinned ? jointMatrices : nullptr, &active);
} NX_CATCH("nxhip_pose_blas_morph")

int nxhip_read_blas_triangles(nxhip_ctx* c, int32_t blasId, nx_triangle* out, uint32_t capacity)
{
    NX_CHECK_CTX(c);
    if (blasId < 0 || (size_t)blasId >= c->blas.size()) return fail_invalid("nxhip_read_blas_triangles: no such BLAS");
    const BlasHost& b = c->blas[(size_t)blasId];
    if (!out || capacity < b.triCount) return fail_invalid("nxhip_read_blas_triangles: destination too small");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    NX_HIP(hipMemcpy(out, b.tris.p, (size_t)b.triCount * sizeof(nx_triangle), hipMemcpyDeviceToHost));
    return NXHIP_OK;
}

int nxhip_read_blas_bounds(nxhip_ctx* c, int32_t blasId, float lo[3], float hi[3])
{
    NX_CHECK_CTX(c);
    if (blasId < 0 || (size_t)blasId >= c->blas.size()) return fail_invalid("nxhip_read_blas_bounds: no such BLAS");
    if (!lo || !hi) return fail_invalid("nxhip_read_blas_bounds: null destination");
    const BlasHost& b = c->blas[(size_t)blasId];
    NX_HIP(hipSetDevice(c->device));
    nx_bvh8_node root;
    NX_HIP(hipMemcpyAsync(&root, b.nodes.p, sizeof root, hipMemcpyDeviceToHost, c->stream));  // behind the refit, if one is on its way
    NX_HIP(hipStreamSynchronize(c->stream));
    // the root's quantisation frame, as nexus::BVHInstance::SetTransform decodes it (host/BVHInstance.cpp root_frame)
    const float steps = std::exp2(8.0f) - 1.0f;
    for (int a = 0; a < 3; a++) {
        lo[a] = root.p[a];
        hi[a] = root.p[a] + std::exp2(static_cast<float>(root.e[a] - 127)) * steps;
    }
    return NXHIP_OK;
}

int nxhip_read_tlas(nxhip_ctx* c, nx_bvh8_node* nodes, uint32_t nodeCapacity, nx_bvh_instance* instances, uint32_t instanceCapacity)
{
    NX_CHECK_CTX(c);
    if (!c->h.tlasNodes) return fail_invalid("nxhip_read_tlas: no TLAS has been set");
    if ((nodes && nodeCapacity < c->tlasNodeCount) || (instances && instanceCapacity < c->h.instanceCount)) return fail_invalid("nxhip_read_tlas: destination too small");
    NX_HIP(hipSetDevice(c->device));
    if (const int rcRefresh = refresh_updated_blas(c)) return rcRefresh;
    NX_SYNC_ALL(c);
    if (nodes) {
        if (kNodeStride == 5) NX_HIP(hipMemcpy(nodes, c->tlasNodes.p, (size_t)c->tlasNodeCount * sizeof(nx_bvh8_node), hipMemcpyDeviceToHost));
        else return fail_invalid("nxhip_read_tlas: built with padded node records");
    }
    if (instances) NX_HIP(hipMemcpy(instances, c->instances.p, (size_t)c->h.instanceCount * sizeof(nx_bvh_instance), hipMemcpyDeviceToHost));
    return NXHIP_OK;
}

int nxhip_set_materials(nxhip_ctx* c, const nx_material* materials, uint32_t count)
try {
    NX_CHECK_CTX(c);
    if (!materials || count == 0) return fail_invalid("nxhip_set_materials: empty input");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    NX_ALLOC(c->materials, (size_t)count * sizeof(nx_material));
    c->hostMaterials.assign(materials, materials + count);
    // The device copy carries one derived flag in the padding byte behind `type` (offset 57 of the 60-byte record): the
    // material can emit or let a path pass through, i.e. its shading may look at / must keep the path's previous vertex
    // (nx_wavefront.h keep_previous_vertex).  The logic kernel reads type and flag with the one load it already does.
    std::vector<nx_material> dev(materials, materials + count);
    for (nx_material& m : dev) {
        // "can emit" exactly as shade_path tests it: maxcomp3(emissive * intensity) > 0 (a negative intensity with a negative
        // component emits too)
        const bool flag = m.emissiveMapId != -1 || m.diffuseMapId != -1 || m.opacity < 1.0f ||
                          std::max(std::max(m.emissive[0] * m.intensity, m.emissive[1] * m.intensity), m.emissive[2] * m.intensity) > 0.0f;
        reinterpret_cast<unsigned char*>(&m)[kMaterialFlagOffset] = flag ? 1u : 0u;
    }
    NX_HIP(hipMemcpy(c->materials.p, dev.data(), (size_t)count * sizeof(nx_material), hipMemcpyHostToDevice));
    c->h.materials = c->materials.as<nx_material>();
    c->hostMaterialsDev = dev;
    c->materialsNameMaps = false;  // (the table as it is now, not what has been uploaded: a material may name a map id before its texture exists)
    for (const nx_material& m : dev) c->materialsNameMaps = c->materialsNameMaps || m.diffuseMapId != -1 || m.emissiveMapId != -1;
    c->stateDirty = true;
    refresh_see_through(c);    // (sets shadeInstDirty: the records hold a copy of their instance's material)
    c->lightTableDirty = true;
    uint32_t mask = 0u;
    for (const nx_material& m : dev)
        if (m.type >= NX_MAT_DIFFUSE && m.type <= NX_MAT_METALROUGH) mask |= 1u << m.type;
    if (mask != c->materialTypeMask) {  // the pass graphs hold one material kernel per type in use
        c->materialTypeMask = mask;
        invalidate_graph(c);
    }
    return NXHIP_OK;
} NX_CATCH("nxhip_set_materials")

// Detail maps (include/nexus_hip.h): the table is checked on the host before anything changes — a refused call leaves the previous table
// where it is.  Ids are checked against the uploaded textures, and the count against the material table, when a pass is about to
// follow them (check_scene_ready): a table may be set before its textures or its materials are.
int nxhip_set_material_detail(nxhip_ctx* c, const nx_material_detail* details, uint32_t count)
try {
    NX_CHECK_CTX(c);
    if (count && !details) return fail_invalid("nxhip_set_material_detail: null array");
    for (uint32_t i = 0; i < count; i++) {
        const std::string who = "nxhip_set_material_detail: entry " + std::to_string(i);
        if (details[i].normalMapId < -1 || details[i].roughnessMapId < -1) return fail_invalid(who + ": a map id below -1");
        if (!std::isfinite(details[i].normalScale)) return fail_invalid(who + ": normalScale is not finite");
    }
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    c->hostMaterialDetail.assign(details, details + (details ? count : 0));
    for (nx_material_detail& d : c->hostMaterialDetail) d.pad_ = 0u;
    refresh_detail_maps(c);  // (the pass graphs follow by their flavor: kFlavorDetail)
    return NXHIP_OK;
} NX_CATCH("nxhip_set_material_detail")

// Alpha modes (include/nexus_hip.h): checked on the host before anything changes, as the detail table is; the count against the material
// table and the mesh-light refusal when a pass or a hook is about to follow the table (check_alpha_table).
int nxhip_set_material_alpha(nxhip_ctx* c, const nx_material_alpha* alphas, uint32_t count)
try {
    NX_CHECK_CTX(c);
    if (count && !alphas) return fail_invalid("nxhip_set_material_alpha: null array");
    for (uint32_t i = 0; i < count; i++) {
        const std::string who = "nxhip_set_material_alpha: entry " + std::to_string(i);
        if (alphas[i].mode != (uint32_t)NX_ALPHA_BLEND && alphas[i].mode != (uint32_t)NX_ALPHA_MASK && alphas[i].mode != (uint32_t)NX_ALPHA_OPAQUE)
            return fail_invalid(who + ": unknown mode");
        if (alphas[i].mode == (uint32_t)NX_ALPHA_MASK && !(std::isfinite(alphas[i].cutoff) && alphas[i].cutoff >= 0.0f && alphas[i].cutoff <= 1.0f))
            return fail_invalid(who + ": a MASK cutoff must be finite and lie in [0, 1]");
    }
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    c->hostMaterialAlpha.assign(alphas, alphas + (alphas ? count : 0));
    refresh_alpha_modes(c);  // (the pass graphs follow by their flavor: kFlavorAlphaTest)
    return NXHIP_OK;
} NX_CATCH("nxhip_set_material_alpha")

int nxhip_set_lights(nxhip_ctx* c, const nx_light* lights, uint32_t count)
try {
    NX_CHECK_CTX(c);
    // (only a context with analytic lights can meet this: the light sample's pick among lightCount + A + 1 has 23 bits — nxhip_set_analytic_lights)
    if (c->h.alightCount && (uint64_t)count + (uint64_t)c->h.alightCount + 1u > (uint64_t)kLightGuideMax)
        return fail_invalid("nxhip_set_lights: lightCount + analytic lights + 1 may not exceed 2^23");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    NX_ALLOC(c->lights, std::max<size_t>(1, count) * sizeof(nx_light));
    if (count) NX_HIP(hipMemcpy(c->lights.p, lights, (size_t)count * sizeof(nx_light), hipMemcpyHostToDevice));
    c->hostLights.assign(lights, lights + (lights ? count : 0));
    c->h.lights = c->lights.as<nx_light>();
    c->h.lightCount = count;
    c->stateDirty = true;
    c->lightTableDirty = true;
    return NXHIP_OK;
} NX_CATCH("nxhip_set_lights")

// Analytic lights (include/nexus_hip.h): checked on the host before anything is allocated — a refused call leaves the previous table
// where it is —, the device records (nx_alights.h ALight) derived in binary64 and rounded once.
int nxhip_set_analytic_lights(nxhip_ctx* c, const nx_analytic_light* lights, uint32_t count)
try {
    NX_CHECK_CTX(c);
    if (count && !lights) return fail_invalid("nxhip_set_analytic_lights: null array");
    if ((uint64_t)c->h.lightCount + (uint64_t)count + 1u > (uint64_t)kLightGuideMax) return fail_invalid("nxhip_set_analytic_lights: lightCount + count + 1 may not exceed 2^23");
    const double halfPi = 1.57079632679489661923;
    std::vector<ALight> table(count);
    for (uint32_t i = 0; i < count; i++) {
        const nx_analytic_light& l = lights[i];
        const std::string who = "nxhip_set_analytic_lights: light " + std::to_string(i);
        const float fields[] = {l.position[0], l.position[1], l.position[2], l.radius, l.direction[0], l.direction[1], l.direction[2], l.angularRadius,
                                l.colour[0], l.colour[1], l.colour[2], l.intensity, l.innerConeAngle, l.outerConeAngle};
        for (const float f : fields)
            if (!std::isfinite(f)) return fail_invalid(who + ": a field is not finite");
        if (l.type != NX_ALIGHT_POINT && l.type != NX_ALIGHT_SPOT && l.type != NX_ALIGHT_DIRECTIONAL) return fail_invalid(who + ": unknown type");
        if (l.radius < 0.0f || l.intensity < 0.0f || l.colour[0] < 0.0f || l.colour[1] < 0.0f || l.colour[2] < 0.0f || l.angularRadius < 0.0f)
            return fail_invalid(who + ": radius, intensity, colour and angularRadius may not be negative");
        if (!((double)l.angularRadius < halfPi)) return fail_invalid(who + ": angularRadius must be below pi/2");
        const double dx = l.direction[0], dy = l.direction[1], dz = l.direction[2];
        const double len = std::sqrt(dx * dx + dy * dy + dz * dz);
        const bool spot = l.type == NX_ALIGHT_SPOT, directional = l.type == NX_ALIGHT_DIRECTIONAL;
        if (!(len > 0.0)) return fail_invalid(who + ": the direction has length 0");  // (every kind: a POINT light does not read it, the record stays one rule)
        if (spot && !(l.innerConeAngle >= 0.0f && l.innerConeAngle < l.outerConeAngle && (double)l.outerConeAngle <= halfPi + 1e-7))
            return fail_invalid(who + ": cone angles must satisfy 0 <= inner < outer <= pi/2");
        ALight& d = table[i];
        const float r = directional ? 0.0f : l.radius;
        d.v0 = directional ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(l.position[0], l.position[1], l.position[2], r);
        const double sinHalf = std::sin(0.5 * (double)l.angularRadius);
        d.v1 = make_float4((float)(dx / len), (float)(dy / len), (float)(dz / len), 0.0f);
        d.v1.w = directional ? (float)(2.0 * sinHalf * sinHalf) : 0.0f;
        d.v2 = make_float4((float)((double)l.colour[0] * (double)l.intensity), (float)((double)l.colour[1] * (double)l.intensity),
                           (float)((double)l.colour[2] * (double)l.intensity), directional ? 1.0f : 0.0f);
        double scale = 0.0, offset = 1.0;  // (falloff 1 for everything but a SPOT)
        if (spot) {
            const double ci = std::cos((double)l.innerConeAngle), co = std::cos((double)l.outerConeAngle);
            scale = 1.0 / std::max(1e-3, ci - co);
            offset = -co * scale;
        }
        d.v3 = make_float4((float)scale, (float)offset, (float)((double)r * (double)r), 0.0f);
    }
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    if (count) {
        DevBuf fresh;  // (the old table goes only once the new one is there)
        NX_ALLOC(fresh, (size_t)count * sizeof(ALight));
        NX_HIP(hipMemcpy(fresh.p, table.data(), (size_t)count * sizeof(ALight), hipMemcpyHostToDevice));
        c->alights = std::move(fresh);
    } else {
        c->alights = DevBuf();
    }
    c->h.alights = count ? c->alights.as<ALight>() : nullptr;
    c->h.alightCount = count;
    c->stateDirty = true;  // (the pass graphs follow by their flavor: kFlavorAnalytic)
    return NXHIP_OK;
} NX_CATCH("nxhip_set_analytic_lights")

// The medium (include/nexus_hip.h): checked on the host — a refused call leaves the previous medium where it is.  It rides in the state
// block; a medium with sigmaT == 0 is no medium: the block is then what it was before the first call.
int nxhip_set_medium(nxhip_ctx* c, const nx_medium* medium)
try {
    NX_CHECK_CTX(c);
    nx_medium m;
    std::memset(&m, 0, sizeof m);
    if (medium) {
        const float fields[] = {medium->boxMin[0], medium->boxMin[1], medium->boxMin[2], medium->sigmaT, medium->boxMax[0], medium->boxMax[1], medium->boxMax[2], medium->g,
                                medium->albedo[0], medium->albedo[1], medium->albedo[2]};
        for (const float f : fields)
            if (!std::isfinite(f)) return fail_invalid("nxhip_set_medium: a field is not finite");
        if (medium->sigmaT < 0.0f) return fail_invalid("nxhip_set_medium: sigmaT may not be negative");
        for (int k = 0; k < 3; k++) {
            if (medium->albedo[k] < 0.0f || medium->albedo[k] > 1.0f) return fail_invalid("nxhip_set_medium: every albedo component must lie in [0, 1]");
            if (!(medium->boxMin[k] < medium->boxMax[k])) return fail_invalid("nxhip_set_medium: boxMin must be below boxMax on every axis");
        }
        if (std::fabs(medium->g) > 0.99f) return fail_invalid("nxhip_set_medium: |g| may not exceed 0.99");
        if (medium->sigmaT > 0.0f) {
            m = *medium;
            m.pad = 0u;
        }
    }
    c->h.medium = m;
    c->h.mediumOn = m.sigmaT > 0.0f ? 1u : 0u;
    c->h.mediumG2 = m.g * m.g;  // (binary32, as the rule states them)
    c->h.mediumOneMinusG2 = c->h.mediumOn ? 1.0f - c->h.mediumG2 : 0.0f;
    c->h.padMedium_ = 0u;
    c->stateDirty = true;  // (the pass graphs follow by their flavor: kFlavorMedium)
    refresh_medium_grid(c);  // (the grid stays; its scales follow the new box)
    return NXHIP_OK;
} NX_CATCH("nxhip_set_medium")

// The density grid (include/nexus_hip.h): checked on the host before anything is allocated — a refused call leaves the previous grid where
// it is.  The voxels go to the device as they are; the majorant bricks are built there (medium_brick_kernel), on the context's stream.
int nxhip_set_medium_density(nxhip_ctx* c, const float* rho, uint32_t nx, uint32_t ny, uint32_t nz)
try {
    NX_CHECK_CTX(c);
    if (!rho) {
        NX_HIP(hipSetDevice(c->device));
        NX_SYNC_ALL(c);
        c->mediumRho = DevBuf();
        c->mediumBricks = DevBuf();
        c->mediumGridN[0] = c->mediumGridN[1] = c->mediumGridN[2] = 0u;
        c->mediumRhoMax = 0.0f;
        refresh_medium_grid(c);
        return NXHIP_OK;
    }
    if (nx == 0u || ny == 0u || nz == 0u) return fail_invalid("nxhip_set_medium_density: a dimension is 0");
    if (nx > 512u || ny > 512u || nz > 512u) return fail_invalid("nxhip_set_medium_density: a dimension exceeds 512");
    const uint64_t voxels = (uint64_t)nx * ny * nz;
    if (voxels > (1ull << 27)) return fail_invalid("nxhip_set_medium_density: more than 2^27 voxels");
    float top = 0.0f;
    for (uint64_t k = 0; k < voxels; k++) {
        if (!(rho[k] >= 0.0f && rho[k] <= 3.4028234e38f)) return fail_invalid("nxhip_set_medium_density: voxel " + std::to_string(k) + " is negative or not finite");
        top = std::max(top, rho[k]);
    }
    if (!(top > 0.0f)) return fail_invalid("nxhip_set_medium_density: the grid's maximum is 0 (NULL removes the grid)");
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    const uint32_t nbx = (nx + 7u) / 8u, nby = (ny + 7u) / 8u, nbz = (nz + 7u) / 8u;
    const uint32_t bricks = nbx * nby * nbz;
    DevBuf freshRho, freshBricks;  // (the old grid goes only once the new one is there)
    NX_ALLOC(freshRho, (size_t)voxels * 4);
    NX_ALLOC(freshBricks, (size_t)bricks * 4);
    NX_HIP(hipMemcpy(freshRho.p, rho, (size_t)voxels * 4, hipMemcpyHostToDevice));
    const int blocks = (int)std::min<uint32_t>((bricks + (uint32_t)kWideBlock - 1u) / (uint32_t)kWideBlock, 4096u);
    NX_HIP(launch_untimed(kernels::medium_brick(), blocks, kWideBlock, c->stream, freshRho.as<float>(), nx, ny, nz, nbx, nby, nbz, freshBricks.as<float>()));
    NX_HIP(hipStreamSynchronize(c->stream));  // (a setter, not the launch path: the other slots' streams may read the bricks next)
    c->mediumRho = std::move(freshRho);
    c->mediumBricks = std::move(freshBricks);
    c->mediumGridN[0] = nx; c->mediumGridN[1] = ny; c->mediumGridN[2] = nz;
    c->mediumRhoMax = top;
    refresh_medium_grid(c);
    return NXHIP_OK;
} NX_CATCH("nxhip_set_medium_density")

static int refresh_texture_tables(nxhip_ctx* c)
{
    auto build = [&](std::vector<TextureHost>& v, DevBuf& table, const TextureDev*& dst) -> int {
        std::vector<TextureDev> t(std::max<size_t>(1, v.size()));
        std::memset(t.data(), 0, t.size() * sizeof(TextureDev));
        for (size_t i = 0; i < v.size(); i++) t[i] = TextureDev{v[i].texels.as<uint32_t>(), v[i].width, v[i].height};
        NX_ALLOC(table, t.size() * sizeof(TextureDev));
        NX_HIP(hipMemcpy(table.p, t.data(), t.size() * sizeof(TextureDev), hipMemcpyHostToDevice));
        dst = table.as<TextureDev>();
        return NXHIP_OK;
    };
    NX_SYNC_ALL(c);
    NX_TRY(build(c->diffuseMaps, c->diffuseTable, c->h.diffuseMaps));
    NX_TRY(build(c->emissiveMaps, c->emissiveTable, c->h.emissiveMaps));
    NX_TRY(build(c->normalMaps, c->normalTable, c->h.normalMaps));
    NX_TRY(build(c->roughnessMaps, c->roughnessTable, c->h.roughnessMaps));
    c->h.hdrMap = TextureDev{c->hdrMap.texels.as<uint32_t>(), c->hdrMap.width, c->hdrMap.height};
    c->h.envFloat = c->hdrFloat ? c->hdrMap.texels.as<float4>() : nullptr;  // (a float map: hdrMap's pointer is tested, this one read)
    c->stateDirty = true;
    return NXHIP_OK;
}

// NX_TUNING_KNOBS=1 NX_ENV_TIMING=1: what a build of the tables takes, to stderr (tools only)
static bool env_timing()
{
    const char* on = std::getenv("NX_TUNING_KNOBS");
    return on && std::atoi(on) == 1 && std::getenv("NX_ENV_TIMING");
}

static int build_env_tables_float(nxhip_ctx* c);

// Sampling distribution of the environment map (see nx_wavefront.h, "Environment importance sampling"): texel weight =
// luminance of the sRGB-decoded texel x sin(polar angle of its row) + 1e-6, accumulated in double; cdfs as float ending in
// exactly 1; density = weight / total x width x height / (2 pi^2) = pdf per solid angle x cos(latitude).  (An 8-bit map; a float
// map's tables have the same layout and meaning and are built by build_env_tables_float below.)
static int build_env_tables(nxhip_ctx* c)
{
    const uint32_t W = c->hdrMap.width, H = c->hdrMap.height;
    if (c->envSampling && c->hdrFloat && c->hdrMap.texels.p && W && H) return build_env_tables_float(c);
    const auto tStart = std::chrono::steady_clock::now();
    if (!c->envSampling || W == 0 || H == 0 || c->hostHdr.size() != (size_t)W * H * 4) {
        c->h.envSampling = 0;
        c->h.envMarginalCdf = c->h.envRowCdf = c->h.envDensity = nullptr;
        c->h.envMarginalGuide = c->h.envRowGuide = nullptr;
        c->stateDirty = true;
        return NXHIP_OK;
    }
    float lut[256];
    for (int i = 0; i < 256; i++) {
        const float x = (float)i / 255.0f;
        lut[i] = x <= 0.04045f ? x / 12.92f : std::pow((x + 0.055f) / 1.055f, 2.4f);
    }
    const double pi = 3.14159265358979323846;
    std::vector<float> marginal(H), row((size_t)W * H), density((size_t)W * H);
    std::vector<double> rowSum(H);
    double total = 0.0;
    for (uint32_t y = 0; y < H; y++) {
        const double sinTheta = std::sin(pi * ((double)y + 0.5) / (double)H);
        double run = 0.0;
        for (uint32_t x = 0; x < W; x++) {
            const uint8_t* t = &c->hostHdr[4 * ((size_t)y * W + x)];
            const double lum = 0.2126 * (double)lut[t[0]] + 0.7152 * (double)lut[t[1]] + 0.0722 * (double)lut[t[2]];
            const double wgt = lum * sinTheta + 1e-6;
            density[(size_t)y * W + x] = (float)wgt;
            run += wgt;
            row[(size_t)y * W + x] = (float)run;
        }
        rowSum[y] = run;
        total += run;
    }
    double run = 0.0;
    for (uint32_t y = 0; y < H; y++) {
        for (uint32_t x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            row[i] = x == W - 1 ? 1.0f : (float)((double)row[i] / rowSum[y]);
            density[i] = (float)((double)density[i] / total * (double)W * (double)H / (2.0 * pi * pi));
        }
        run += rowSum[y];
        marginal[y] = y == H - 1 ? 1.0f : (float)(run / total);
    }
    // guides for the device's cdf inversion (nx_wavefront.h cdf_find): bracket per bucket of the random number
    auto make_guide = [](const float* cdf, uint32_t n, uint32_t* guide) {
        uint32_t idx = 0;
        for (int b = 0; b <= kEnvGuide; b++) {
            const float bound = (float)b / (float)kEnvGuide;
            while (idx < n - 1 && !(cdf[idx] > bound)) idx++;
            guide[b] = idx;
        }
    };
    std::vector<uint32_t> marginalGuide(kEnvGuide + 1), rowGuide((size_t)H * (kEnvGuide + 1));
    make_guide(marginal.data(), H, marginalGuide.data());
    for (uint32_t y = 0; y < H; y++) make_guide(&row[(size_t)y * W], W, &rowGuide[(size_t)y * (kEnvGuide + 1)]);
    const auto tLoops = std::chrono::steady_clock::now();
    NX_SYNC_ALL(c);
    NX_ALLOC(c->envMarginalGuide, marginalGuide.size() * 4);
    NX_ALLOC(c->envRowGuide, rowGuide.size() * 4);
    NX_HIP(hipMemcpy(c->envMarginalGuide.p, marginalGuide.data(), marginalGuide.size() * 4, hipMemcpyHostToDevice));
    NX_HIP(hipMemcpy(c->envRowGuide.p, rowGuide.data(), rowGuide.size() * 4, hipMemcpyHostToDevice));
    c->h.envMarginalGuide = c->envMarginalGuide.as<uint32_t>();
    c->h.envRowGuide = c->envRowGuide.as<uint32_t>();
    NX_ALLOC(c->envMarginalCdf, marginal.size() * 4);
    NX_ALLOC(c->envRowCdf, row.size() * 4);
    NX_ALLOC(c->envDensity, density.size() * 4);
    NX_HIP(hipMemcpy(c->envMarginalCdf.p, marginal.data(), marginal.size() * 4, hipMemcpyHostToDevice));
    NX_HIP(hipMemcpy(c->envRowCdf.p, row.data(), row.size() * 4, hipMemcpyHostToDevice));
    NX_HIP(hipMemcpy(c->envDensity.p, density.data(), density.size() * 4, hipMemcpyHostToDevice));
    c->h.envSampling = 1;
    c->h.envMarginalCdf = c->envMarginalCdf.as<float>();
    c->h.envRowCdf = c->envRowCdf.as<float>();
    c->h.envDensity = c->envDensity.as<float>();
    c->stateDirty = true;
    if (env_timing())
        std::fprintf(stderr, "[env tables] host build %u x %u: %.3f ms (the loops %.3f ms, allocations and uploads the rest)\n", W, H,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tStart).count(), std::chrono::duration<double, std::milli>(tLoops - tStart).count());
    return NXHIP_OK;
}

// The tables of a FLOAT map: the same five arrays, built on the device from the texels that are already there (nx_envmap.hip: the
// footprint weight, binary64 scans), on the context's stream.  No texel and no table comes back to the host.
static int build_env_tables_float(nxhip_ctx* c)
{
    const uint32_t W = c->hdrMap.width, H = c->hdrMap.height;
    NX_SYNC_ALL(c);  // nothing may still read the old tables
    NX_ALLOC(c->envMarginalGuide, (size_t)(kEnvGuide + 1) * 4);
    NX_ALLOC(c->envRowGuide, (size_t)H * (kEnvGuide + 1) * 4);
    NX_ALLOC(c->envMarginalCdf, (size_t)H * 4);
    NX_ALLOC(c->envRowCdf, (size_t)W * H * 4);
    NX_ALLOC(c->envDensity, (size_t)W * H * 4);
    NX_ALLOC(c->envBuildTemp, (size_t)H * 2 * sizeof(double));
    const bool timing = env_timing();
    struct Events {  // (destroyed on every way out, the early returns of NX_HIP / NX_TRY included)
        hipEvent_t t0 = nullptr, t1 = nullptr;
        ~Events()
        {
            if (t0) (void)hipEventDestroy(t0);
            if (t1) (void)hipEventDestroy(t1);
        }
    } ev;
    if (timing) {
        NX_HIP(hipEventCreate(&ev.t0));
        NX_HIP(hipEventCreate(&ev.t1));
        NX_HIP(hipEventRecord(ev.t0, c->stream));
    }
    NX_TRY(env_float_tables_build(c->stream, c->hdrMap.texels.as<float4>(), W, H, c->envBuildTemp.as<double>(), c->envMarginalCdf.as<float>(), c->envRowCdf.as<float>(),
                                  c->envDensity.as<float>(), c->envMarginalGuide.as<uint32_t>(), c->envRowGuide.as<uint32_t>()));
    if (timing) NX_HIP(hipEventRecord(ev.t1, c->stream));
    // passes on the other slots' streams must not start on half-built tables (not on the per-frame path)
    NX_HIP(hipStreamSynchronize(c->stream));
    if (timing) {
        float ms = 0.0f;
        NX_HIP(hipEventElapsedTime(&ms, ev.t0, ev.t1));
        std::fprintf(stderr, "[env tables] device build %u x %u: %.3f ms (events around the three launches)\n", W, H, ms);
    }
    c->h.envMarginalGuide = c->envMarginalGuide.as<uint32_t>();
    c->h.envRowGuide = c->envRowGuide.as<uint32_t>();
    c->h.envSampling = 1;
    c->h.envMarginalCdf = c->envMarginalCdf.as<float>();
    c->h.envRowCdf = c->envRowCdf.as<float>();
    c->h.envDensity = c->envDensity.as<float>();
    c->stateDirty = true;
    return NXHIP_OK;
}

int nxhip_set_env_sampling(nxhip_ctx* c, int enable)
try {
    NX_CHECK_CTX(c);
    NX_HIP(hipSetDevice(c->device));
    if (enable && !c->hdrMap.texels.p) return fail_invalid("nxhip_set_env_sampling: upload the environment map first (nxhip_upload_texture kind 2 or nxhip_upload_env_float)");
    c->envSampling = enable != 0;
    return build_env_tables(c);
} NX_CATCH("nxhip_set_env_sampling")

int nxhip_upload_texture(nxhip_ctx* c, int kind, const uint8_t* rgba8, uint32_t width, uint32_t height, int32_t* texId)
try {
    NX_CHECK_CTX(c);
    if (!rgba8 || width == 0 || height == 0 || kind < 0 || kind > 4) return fail_invalid("nxhip_upload_texture: bad arguments");
    NX_HIP(hipSetDevice(c->device));
    TextureHost t;
    t.width = width;
    t.height = height;
    NX_ALLOC(t.texels, (size_t)width * height * 4);
    NX_HIP(hipMemcpy(t.texels.p, rgba8, (size_t)width * height * 4, hipMemcpyHostToDevice));
    int32_t id = 0;
    if (kind == 0) {
        for (size_t i = 0; i < (size_t)width * height && !t.hasAlpha; i++) t.hasAlpha = rgba8[4 * i + 3] != 255u;
        c->diffuseMaps.push_back(std::move(t));
        id = (int32_t)c->diffuseMaps.size() - 1;
        refresh_see_through(c);  // (a material may have named this id before its texture existed)
    }
    else if (kind == 1) { c->emissiveMaps.push_back(std::move(t)); id = (int32_t)c->emissiveMaps.size() - 1; c->lightTableDirty = true; }
    else if (kind == 3) { c->normalMaps.push_back(std::move(t)); id = (int32_t)c->normalMaps.size() - 1; }
    else if (kind == 4) { c->roughnessMaps.push_back(std::move(t)); id = (int32_t)c->roughnessMaps.size() - 1; }
    else {
        NX_SYNC_ALL(c);
        c->hdrMap = std::move(t);
        c->hdrFloat = false;
        c->hostHdr.assign(rgba8, rgba8 + (size_t)width * height * 4);
    }
    if (texId) *texId = id;
    const int rc = refresh_texture_tables(c);
    if (rc != NXHIP_OK || kind != 2) return rc;
    return build_env_tables(c);  // a new map under an enabled sampler gets new tables
} NX_CATCH("nxhip_upload_texture")

int nxhip_upload_env_float(nxhip_ctx* c, const float* rgb, uint32_t width, uint32_t height)
try {
    NX_CHECK_CTX(c);
    if (!rgb || width == 0 || height == 0) return fail_invalid("nxhip_upload_env_float: bad arguments");
    if (width > 32768u || height > 32768u || (uint64_t)width * height > (1ull << 27)) return fail_invalid("nxhip_upload_env_float: at most 32768 texels per axis and 2^27 in all");
    // before anything is allocated: radiance is finite and not negative (a NaN would poison the sampler's sums, a negative weight its cdfs)
    const size_t texels = (size_t)width * height;
    for (size_t i = 0; i < texels * 3; i++)
        if (!(rgb[i] >= 0.0f && rgb[i] <= 3.402823466e38f)) return fail_invalid("nxhip_upload_env_float: components must be finite and not negative");
    NX_HIP(hipSetDevice(c->device));
    TextureHost t;
    t.width = width;
    t.height = height;
    NX_ALLOC(t.texels, texels * sizeof(float4));
    {
        std::vector<float4> staged(texels);  // one 16-byte tap per texel (w unused)
        for (size_t i = 0; i < texels; i++) staged[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.0f);
        NX_HIP(hipMemcpy(t.texels.p, staged.data(), texels * sizeof(float4), hipMemcpyHostToDevice));
    }
    NX_SYNC_ALL(c);
    c->hdrMap = std::move(t);
    c->hdrFloat = true;
    c->hostHdr.clear();
    NX_TRY(refresh_texture_tables(c));
    return build_env_tables(c);  // a new map under an enabled sampler gets new tables
} NX_CATCH("nxhip_upload_env_float")

int nxhip_sky_defaults(nx_sky* sky)
{
    if (!sky) return fail_invalid("nxhip_sky_defaults: sky is NULL");
    *sky = nx_sky();
    sky->sunDirection[0] = sky->sunDirection[1] = 0.70710678118654752f;  // 45 degrees of elevation along +x
    sky->sunAngularRadius = 0.004675f;
    sky->altitude = 1.0f;
    sky->rayleighScale = sky->mieScale = 1.0f;
    sky->mieG = 0.8f;
    for (int ch = 0; ch < 3; ch++) {
        sky->sunIrradiance[ch] = 1.0f;
        sky->groundAlbedo[ch] = 0.3f;
    }
    sky->width = 2048;
    sky->height = 1024;
    sky->viewSteps = 64;
    sky->lightSteps = 16;
    return NXHIP_OK;
}

int nxhip_sky_sun_light(const nx_sky* sky, nx_analytic_light* out)
try {
    SkyPlan plan;
    NX_TRY(sky_plan(sky, "nxhip_sky_sun_light", &plan));
    if (!out) return fail_invalid("nxhip_sky_sun_light: out is NULL");
    double T[3];
    sky_sun_transmittance(plan, 256, T);  // (0 when the sun is below the observer's geometric horizon)
    *out = nx_analytic_light();
    out->type = NX_ALIGHT_DIRECTIONAL;
    out->angularRadius = sky->sunAngularRadius;
    out->intensity = 1.0f;
    for (int ch = 0; ch < 3; ch++) {
        out->direction[ch] = (float)-plan.sun[ch];
        out->colour[ch] = (float)((double)sky->sunIrradiance[ch] * T[ch]);
    }
    return NXHIP_OK;
} NX_CATCH("nxhip_sky_sun_light")

// The sky as a float map: generated on the device into a new texel buffer (nx_sky.hip), then installed as nxhip_upload_env_float installs
// its own — the same steps in the same order, so that lookup, sampler and tables cannot tell the two apart.
int nxhip_set_sky(nxhip_ctx* c, const nx_sky* sky)
try {
    NX_CHECK_CTX(c);
    SkyPlan plan;
    NX_TRY(sky_plan(sky, "nxhip_set_sky", &plan));  // before anything is allocated
    SkyDisc disc;
    if (sky->sunDisc) NX_TRY(sky_disc_plan(sky, plan, "nxhip_set_sky", &disc));
    NX_HIP(hipSetDevice(c->device));
    TextureHost t;
    t.width = sky->width;
    t.height = sky->height;
    NX_ALLOC(t.texels, (size_t)sky->width * sky->height * sizeof(float4));
    const bool timing = env_timing();
    struct Events {  // (destroyed on every way out)
        hipEvent_t t0 = nullptr, t1 = nullptr;
        ~Events()
        {
            if (t0) (void)hipEventDestroy(t0);
            if (t1) (void)hipEventDestroy(t1);
        }
    } ev;
    if (timing) {
        NX_HIP(hipEventCreate(&ev.t0));
        NX_HIP(hipEventCreate(&ev.t1));
        NX_HIP(hipEventRecord(ev.t0, c->stream));
    }
    NX_TRY(sky_generate(c->stream, plan, sky->sunDisc ? &disc : nullptr, t.texels.as<float4>(), sky->width, sky->height));
    if (timing) NX_HIP(hipEventRecord(ev.t1, c->stream));
    NX_SYNC_ALL(c);  // the new texels are complete and nothing reads the old map any more
    if (timing) {
        float ms = 0.0f;
        NX_HIP(hipEventElapsedTime(&ms, ev.t0, ev.t1));
        std::fprintf(stderr, "[sky] device build %u x %u, steps %u x %u%s: %.3f ms (events around the launches)\n", sky->width, sky->height, sky->viewSteps, sky->lightSteps,
                     sky->sunDisc ? ", disc" : "", ms);
    }
    c->hdrMap = std::move(t);
    c->hdrFloat = true;
    c->hostHdr.clear();
    NX_TRY(refresh_texture_tables(c));
    return build_env_tables(c);  // a new map under an enabled sampler gets new tables
} NX_CATCH("nxhip_set_sky")

int nxhip_clear_textures(nxhip_ctx* c)
try {
    NX_CHECK_CTX(c);
    NX_HIP(hipSetDevice(c->device));
    NX_SYNC_ALL(c);
    c->diffuseMaps.clear();
    c->emissiveMaps.clear();
    c->normalMaps.clear();
    c->roughnessMaps.clear();
    refresh_see_through(c);
    c->lightMapMeans = 0;
    c->lightTableDirty = true;
    c->hdrMap = TextureHost();
    c->hdrFloat = false;
    c->hostHdr.clear();
    c->envSampling = false;
    NX_TRY(build_env_tables(c));
    return refresh_texture_tables(c);
} NX_CATCH("nxhip_clear_textures")

}  // extern "C"

uint64_t nxd::layout_stamp_scene() { return layout_stamp(); }
