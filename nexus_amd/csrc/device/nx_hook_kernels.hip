// nx_hook_kernels.hip — the array test hooks' kernels: the product's own device functions (BSDFs, texture lookups, the environment sampler,
// the analytic lights' draw, the shading frame, a material's inputs) on plain arrays, for nxhip_hooks.hip's batch entry points.
//
// A unit of its own because no pass graph launches these kernels: they only call functions of the headers, so they need no material
// kernel as a neighbour, and the units that hold those (nx_wavefront.hip and its _detail / _metal siblings) are the build's longest
// compiles (profiles/analytic_lights.txt section 3, profiles/detail_maps.txt) — a change to a hook no longer recompiles a kernel family.
// (The medium's hooks call functions defined in nx_medium.hip and stay there.)
#define NX_KERNEL_TU 1
#include "nx_wavefront.h"

namespace nxd {

// ------------------------------------------------------------------------------------------------------
// Test hooks: the shading functions on plain arrays (nxhip_bsdf_*_batch, nxhip_tex2d_batch)

template <int TYPE>
NXD void bsdf_hook_one(const MatParams& mp, bool sample, const nx_bsdf_query& q, nx_bsdf_result& r)
{
    f3 wo = ld3(q.wo), thr = mk3(0.0f);
    float pdf = 0.0f;
    uint32_t rng = q.rng;
    const bool ok = sample ? Bsdf<TYPE>::sample(mp, ld3(q.wi), rng, wo, thr, pdf) : Bsdf<TYPE>::eval(mp, ld3(q.wi), wo, thr, pdf);
    r.wo[0] = wo.x; r.wo[1] = wo.y; r.wo[2] = wo.z;
    r.pdf = pdf;
    r.throughput[0] = thr.x; r.throughput[1] = thr.y; r.throughput[2] = thr.z;
    r.ok = ok ? 1u : 0u;
    r.rngOut = rng;
    r.pad_[0] = r.pad_[1] = r.pad_[2] = 0u;
}

__global__ void __launch_bounds__(kWideBlock) bsdf_hook_kernel(const nx_material* __restrict__ material, const nx_bsdf_query* __restrict__ q, const uint32_t count,
                                                                const int sample, nx_bsdf_result* __restrict__ out)
{
    const nx_material m = *material;
    const MatParams mp = load_params(m);
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        nx_bsdf_result r;
        switch (m.type) {
        case NX_MAT_DIFFUSE: bsdf_hook_one<NX_MAT_DIFFUSE>(mp, sample != 0, q[k], r); break;
        case NX_MAT_DIELECTRIC: bsdf_hook_one<NX_MAT_DIELECTRIC>(mp, sample != 0, q[k], r); break;
        case NX_MAT_PLASTIC: bsdf_hook_one<NX_MAT_PLASTIC>(mp, sample != 0, q[k], r); break;
        default: bsdf_hook_one<NX_MAT_CONDUCTOR>(mp, sample != 0, q[k], r); break;
        }
        out[k] = r;
    }
}

// nxhip_bsdf_*_batch for a material of type NX_MAT_METALROUGH (the four reference types keep bsdf_hook_kernel above)
__global__ void __launch_bounds__(kWideBlock) bsdf_hook_metal_kernel(const nx_material* __restrict__ material, const nx_bsdf_query* __restrict__ q, const uint32_t count,
                                                                      const int sample, nx_bsdf_result* __restrict__ out)
{
    const nx_material m = *material;
    const MatParams mp = load_params(m);
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const nx_bsdf_query qk = q[k];
        f3 wo = ld3(qk.wo), thr = mk3(0.0f);
        float pdf = 0.0f;
        uint32_t rng = qk.rng;
        const bool ok = sample ? Bsdf<NX_MAT_METALROUGH>::sample(mp, ld3(qk.wi), rng, wo, thr, pdf) : Bsdf<NX_MAT_METALROUGH>::eval(mp, ld3(qk.wi), wo, thr, pdf);
        nx_bsdf_result r;
        r.wo[0] = wo.x; r.wo[1] = wo.y; r.wo[2] = wo.z;
        r.pdf = pdf;
        r.throughput[0] = thr.x; r.throughput[1] = thr.y; r.throughput[2] = thr.z;
        r.ok = ok ? 1u : 0u;
        r.rngOut = rng;
        r.pad_[0] = r.pad_[1] = r.pad_[2] = 0u;
        out[k] = r;
    }
}

// include/nexus_fmath.h on arrays (nxhip_fmath_batch, a test hook like the two above)
__global__ void __launch_bounds__(kWideBlock) fmath_hook_kernel(const int op, const double* __restrict__ a, const double* __restrict__ b, const uint32_t count,
                                                                 double* __restrict__ out)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) out[k] = nxf_apply(op, a[k], b ? b[k] : 0.0);
}

// (the texture descriptor comes by value: selecting one of S->diffuseMaps[i] / S->emissiveMaps[i] / S->hdrMap with a
//  uniform three-way branch here was miscompiled by hipcc 7.2 — the third arm left the descriptor pointer unset)
__global__ void __launch_bounds__(kWideBlock) tex2d_hook_kernel(const TextureDev t, const float* __restrict__ srgbLut, const float* __restrict__ uv,
                                                                 const uint32_t count, float4* __restrict__ out)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x)
        out[k] = tex2d(t, srgbLut, uv[2 * k], uv[2 * k + 1]);
}

// ... and the float environment map's lookup (nxhip_tex2d_batch kind 2 on a float map)
__global__ void __launch_bounds__(kWideBlock) tex2d_float_hook_kernel(const float4* __restrict__ texels, const int W, const int H, const float* __restrict__ uv,
                                                                       const uint32_t count, float4* __restrict__ out)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x)
        out[k] = tex2d_float(texels, W, H, uv[2 * k], uv[2 * k + 1]);
}

// the detail maps' lookup on arrays (nxhip_tex2d_batch kind 3 / 4)
__global__ void __launch_bounds__(kWideBlock) tex2d_linear_hook_kernel(const TextureDev t, const float* __restrict__ uv, const uint32_t count, float4* __restrict__ out)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) out[k] = tex2d_linear(t, uv[2 * k], uv[2 * k + 1]);
}

// The environment lookup and its sampler on arrays (nxhip_env_sample_batch / nxhip_env_eval_batch): the product's own env_invert,
// env_direction, env_uv, env_pdf, env_texel and sample_background.  sample != 0: in = count x 2 random numbers; the direction
// drawn, its pdf formed as the NEE forms it (from env_uv of the direction) and the texel the inversion picked.  sample == 0: in =
// count x 3 directions; the background colour and — pdf / texel may be null: the host passes them only with the sampler on —
// the sampler's pdf and the texel of the direction's map coordinates.
__global__ void __launch_bounds__(kWideBlock) env_hook_kernel(const DeviceState* __restrict__ S, const int sample, const float* __restrict__ in, const uint32_t count,
                                                               float* __restrict__ vec, float* __restrict__ pdf, uint32_t* __restrict__ texel)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        if (sample) {
            const EnvPick p = env_invert(S, in[2 * k], in[2 * k + 1]);
            const f3 d = env_direction(p.u, p.v);
            vec[3 * k] = d.x; vec[3 * k + 1] = d.y; vec[3 * k + 2] = d.z;
            pdf[k] = env_pdf(S, d, env_uv(d));
            texel[k] = (uint32_t)p.y * S->hdrMap.width + (uint32_t)p.x;
        } else {
            const f3 d = mk3(in[3 * k], in[3 * k + 1], in[3 * k + 2]);
            const f3 c = sample_background(S, d);
            vec[3 * k] = c.x; vec[3 * k + 1] = c.y; vec[3 * k + 2] = c.z;
            const EnvUv uv = env_uv(d);
            if (pdf) pdf[k] = env_pdf(S, d, uv);
            if (texel) texel[k] = env_texel(S, uv);
        }
    }
}

// The analytic lights' draw on arrays (nxhip_analytic_light_sample_batch): the product's own alight_sample for light `index`, from the
// origins as given (the caller's business to offset them) with r = count x 2 random numbers.
__global__ void __launch_bounds__(kWideBlock) alight_hook_kernel(const DeviceState* __restrict__ S, const uint32_t index, const float* __restrict__ origin,
                                                                  const float* __restrict__ r, const uint32_t count, float* __restrict__ direction,
                                                                  float* __restrict__ tmax, float* __restrict__ factor, uint32_t* __restrict__ ok)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        f3 d, f;
        float t;
        const bool good = alight_sample(&S->alights[index], mk3(origin[3 * k], origin[3 * k + 1], origin[3 * k + 2]), r[2 * k], r[2 * k + 1], d, t, f);
        direction[3 * k] = d.x; direction[3 * k + 1] = d.y; direction[3 * k + 2] = d.z;
        tmax[k] = t;
        factor[3 * k] = f.x; factor[3 * k + 1] = f.y; factor[3 * k + 2] = f.z;
        ok[k] = good ? 1u : 0u;
    }
}

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

// nxhip_material_inputs_batch: for hit k — triangle triIdx[k] of instance `instanceIdx` at barycentrics hitUv[2k..] — the base colour c, the
// roughness r and the metalness m the BSDF of an NX_MAT_METALROUGH material receives there, formed by the device functions shade_path
// calls and in its order: the diffuse map's texel (tex2d), the roughness map's G and B channels (detail_shading_frame, one lookup),
// the clamp of m (metal_clamp01).  out[5k..] = c.r, c.g, c.b, r, m.
__global__ void __launch_bounds__(kWideBlock) material_inputs_hook_kernel(const DeviceState* __restrict__ S, const uint32_t instanceIdx, const uint32_t* __restrict__ triIdx,
                                                                           const float* __restrict__ hitUv, const uint32_t count, float* __restrict__ out)
{
    const NX_G ShadeInst* inst = &S->shadeInst[instanceIdx];
    nx_material_detail d{-1, -1, 1.0f, 0u};
    if (S->shadeDetail) d = S->shadeDetail[instanceIdx];
    const nx_material material = inst->material;
    const NX_G float* T = inst->transform;
    const NX_G float* IT = inst->invTransform;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const float hu = hitUv[2 * k], hv = hitUv[2 * k + 1];
        const NX_G nx_triangle* tri = shade_tri(inst->tris, triIdx[k]);
        MatParams mp = load_params(material);
        const f3 tp0 = ld3(tri->pos0), tp1 = ld3(tri->pos1), tp2 = ld3(tri->pos2);
        f3 normal = bary3(ld3(tri->normal0), ld3(tri->normal1), ld3(tri->normal2), hu, hv);
        const f2 texUv = bary2(tri->texCoord0, tri->texCoord1, tri->texCoord2, hu, hv);
        normal = normalize3(mat_vec_transposed(IT, normal));
        f3 gNormal = normalize3(mat_vec_transposed(IT, cross3(tp1 - tp0, tp2 - tp0)));
        if (material.diffuseMapId != -1) {
            const float4 color = tex2d(S->diffuseMaps[material.diffuseMapId], S->srgbLut, texUv.x, texUv.y);
            mp.albedo = mk3(color.x, color.y, color.z);
        }
        bool fellBack;
        detail_shading_frame<NX_MAT_METALROUGH>(S, d, tri, T, tp0, tp1, tp2, texUv, -gNormal, normal, gNormal, mp.roughness, fellBack, &mp.metallic);
        out[5 * k] = mp.albedo.x; out[5 * k + 1] = mp.albedo.y; out[5 * k + 2] = mp.albedo.z;
        out[5 * k + 3] = mp.roughness;
        out[5 * k + 4] = metal_clamp01(mp.metallic);
    }
}

const void* bsdf_hook_kernel_ptr() { return (const void*)bsdf_hook_kernel; }
const void* bsdf_hook_metal_kernel_ptr() { return (const void*)bsdf_hook_metal_kernel; }
const void* fmath_hook_kernel_ptr() { return (const void*)fmath_hook_kernel; }
const void* tex2d_hook_kernel_ptr() { return (const void*)tex2d_hook_kernel; }
const void* tex2d_float_hook_kernel_ptr() { return (const void*)tex2d_float_hook_kernel; }
const void* tex2d_linear_hook_kernel_ptr() { return (const void*)tex2d_linear_hook_kernel; }
const void* env_hook_kernel_ptr() { return (const void*)env_hook_kernel; }
const void* alight_hook_kernel_ptr() { return (const void*)alight_hook_kernel; }
const void* shading_frame_hook_kernel_ptr() { return (const void*)shading_frame_hook_kernel; }
const void* material_inputs_hook_kernel_ptr() { return (const void*)material_inputs_hook_kernel; }

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_hook_kernels() { return layout_stamp(); }

}  // namespace nxd
