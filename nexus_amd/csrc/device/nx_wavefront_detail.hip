// nx_wavefront_detail.hip — the DETAIL instances of the material kernels (normal and roughness maps: nxhip_set_material_detail).
//
// The kernels are the templates of nx_wavefront.hip, compiled here for DETAIL = true and for nothing else: a translation unit of its
// own, so that the instances of contexts without detail maps are built from the text and with the neighbours they had
// (profiles/analytic_lights.txt section 3 records what doubling the instances of ONE unit did to the build; profiles/detail_maps.txt
// what this one costs).  DETAIL implies the general material launch: there is no NO_MAPS form.
// Also here: the test hook's kernel over the same device function (nx_detail.h detail_shading_frame).
#define NX_WAVEFRONT_INSTANCES_ONLY 1
#include "nx_wavefront.hip"

namespace nxd {

// nxhip_shading_frame_batch: for hit k — triangle triIdx[k] of instance `instanceIdx` at barycentrics hitUv[2k..], reached along rayDir[3k..]
// — what shade_path hands its sampling code: the world-space shading normal after fallback and flip, the roughness the BSDF
// receives, and whether the fallback was taken.  The preamble (positions, normals, texture coordinates, parameters) is shade_path's.
template <int TYPE>
NXD void shading_frame_hook_one(const DeviceState* S, const NX_G ShadeInst* inst, const nx_material_detail d, const uint32_t triIdx, const float hu, const float hv,
                                const f3 rayDirection, f3& ns, float& roughness, bool& fellBack)
{
    const NX_G nx_triangle* tri = shade_tri(inst->tris, triIdx);
    const nx_material material = inst->material;
    MatParams mp = load_params(material);
    const NX_G float* T = inst->transform;
    const NX_G float* IT = inst->invTransform;
    const f3 tp0 = ld3(tri->pos0), tp1 = ld3(tri->pos1), tp2 = ld3(tri->pos2);
    f3 normal = bary3(ld3(tri->normal0), ld3(tri->normal1), ld3(tri->normal2), hu, hv);
    const f2 texUv = bary2(tri->texCoord0, tri->texCoord1, tri->texCoord2, hu, hv);
    normal = normalize3(mat_vec_transposed(IT, normal));
    f3 gNormal = normalize3(mat_vec_transposed(IT, cross3(tp1 - tp0, tp2 - tp0)));
    ns = detail_shading_frame<TYPE>(S, d, tri, T, tp0, tp1, tp2, texUv, rayDirection, normal, gNormal, mp.roughness, fellBack);
    roughness = mp.roughness;
}

__global__ void __launch_bounds__(kWideBlock) shading_frame_hook_kernel(const DeviceState* __restrict__ S, const uint32_t instanceIdx, const uint32_t* __restrict__ triIdx,
                                                                         const float* __restrict__ hitUv, const float* __restrict__ rayDir, const uint32_t count,
                                                                         float* __restrict__ normalOut, float* __restrict__ roughnessOut, uint32_t* __restrict__ fellBackOut)
{
    const NX_G ShadeInst* inst = &S->shadeInst[instanceIdx];
    // (a context without a detail table: every material names no map)
    nx_material_detail d{-1, -1, 1.0f, 0u};
    if (S->shadeDetail) d = S->shadeDetail[instanceIdx];
    const int type = (int)inst->material.type;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const f3 dir = mk3(rayDir[3 * k], rayDir[3 * k + 1], rayDir[3 * k + 2]);
        f3 ns;
        float roughness;
        bool fellBack;
        switch (type) {
        case NX_MAT_DIFFUSE: shading_frame_hook_one<NX_MAT_DIFFUSE>(S, inst, d, triIdx[k], hitUv[2 * k], hitUv[2 * k + 1], dir, ns, roughness, fellBack); break;
        case NX_MAT_DIELECTRIC: shading_frame_hook_one<NX_MAT_DIELECTRIC>(S, inst, d, triIdx[k], hitUv[2 * k], hitUv[2 * k + 1], dir, ns, roughness, fellBack); break;
        case NX_MAT_PLASTIC: shading_frame_hook_one<NX_MAT_PLASTIC>(S, inst, d, triIdx[k], hitUv[2 * k], hitUv[2 * k + 1], dir, ns, roughness, fellBack); break;
        default: shading_frame_hook_one<NX_MAT_CONDUCTOR>(S, inst, d, triIdx[k], hitUv[2 * k], hitUv[2 * k + 1], dir, ns, roughness, fellBack); break;
        }
        normalOut[3 * k] = ns.x; normalOut[3 * k + 1] = ns.y; normalOut[3 * k + 2] = ns.z;
        roughnessOut[k] = roughness;
        fellBackOut[k] = fellBack ? 1u : 0u;
    }
}

// the detail maps' lookup on arrays (nxhip_tex2d_batch kind 3 / 4)
__global__ void __launch_bounds__(kWideBlock) tex2d_linear_hook_kernel(const TextureDev t, const float* __restrict__ uv, const uint32_t count, float4* __restrict__ out)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) out[k] = tex2d_linear(t, uv[2 * k], uv[2 * k + 1]);
}

// (the instances only the pass graphs of a context with detail maps launch — nxhip_render.hip pass_flavor, kFlavorDetail)
using DetailSets = Instances<kMfPower | kMfAnalytic | kMfDetail, kMfAnalytic | kMfDetail, kMfPower | kMfDetail, kMfDetail>;
namespace wavefront_detail {
const void* shade(int type, unsigned set) { return shade_instance<DetailSets, NX_MAT_DIFFUSE, NX_MAT_DIELECTRIC, NX_MAT_PLASTIC, NX_MAT_CONDUCTOR>(type, set); }
// (the SCAN material launch alone has TREE forms: nx_variants.h)
using DetailScanSets = Instances<kMfTree | kMfPower | kMfAnalytic | kMfDetail, kMfPower | kMfAnalytic | kMfDetail, kMfAnalytic | kMfDetail, kMfTree | kMfPower | kMfDetail, kMfPower | kMfDetail, kMfDetail>;
const void* shade_scan(unsigned set) { return shade_scan_instance<DetailScanSets>(set); }
const void* tail(unsigned set) { return tail_instance<DetailSets>(set); }
}  // namespace wavefront_detail
const void* shading_frame_hook_kernel_ptr() { return (const void*)shading_frame_hook_kernel; }
const void* tex2d_linear_hook_kernel_ptr() { return (const void*)tex2d_linear_hook_kernel; }

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_wavefront_detail() { return layout_stamp(); }

}  // namespace nxd
