// nx_skin.hip — skinned meshes on the device (nxhip_pose_blas): bind-pose triangles and a joint palette go in, and the BLAS's
// 96-byte triangles, their shading copy and the leaf-ordered intersection stream come out of ONE pass; the level-by-level node
// refit of nxhip_update_blas (nx_refit.hip blas_refit_kernel) runs behind it.  The kernel boundary orders the two, as the comment
// above blas_refit_kernel explains: no workgroup waits for another.
//
// The reference has nothing of the kind: its loader drops skins, a rigged mesh arrives frozen in its bind pose.  Without this
// kernel the route is a caller's own skinning kernel writing 96-byte records, nxhip_update_blas_device's device copy, the strided
// shading copy and isect_kernel's pass that reads every triangle again (nx_lbvh.hip).
//
// The blending rule is stated in include/nexus_hip.h (nxhip_pose_blas).  One lane per triangle, walking LEAF order like
// isect_kernel: k is the position in the stream, id = primIdx[k] the triangle.  Per lane: 96 B of bind triangle and 80 B of skin
// (SkinTri, nx_device.h) read with 16-byte loads, 96 B of triangle and 48 B of stream written with 16-byte stores; the stream's
// words are isect_kernel's expressions over the values just stored, so it is what lbvh_write_isect would make of them, bit for bit.
// The palette — 48 B per joint — is staged in the LDS up to kSkinLdsJoints joints and read from global memory above that: two
// instances of one template.  Neighbouring triangles mostly share their joints, so the LDS reads of a wave are largely broadcasts.
//
// Morph targets (nxhip_pose_blas_morph) are a stage in front of the joint blend in the same pass: for each ACTIVE target — weight not 0;
// the host compacts the weights into (index, weight) pairs, read here through a uniform pointer, so the loop is scalar-controlled and the
// targets the file has beyond the active ones cost nothing — a lane reads its triangle's 80-byte MorphTri with five 16-byte loads and adds
// the weighted deltas to the bind corners.  Three more instances: morph only, morph + skin with the palette in the LDS or in global memory.
#define NX_KERNEL_TU 1
#include "nx_device.h"
#include "nx_math.h"

namespace nxd {

constexpr int kPoseBlock = 256;  // (nxhip_scene.hip launches pose_kernel with the same figure)

struct Row3x4 {
    float4 r[3];
};

NXD float4 scaled(const float w, const float4 a) { return make_float4(w * a.x, w * a.y, w * a.z, w * a.w); }
NXD float4 plus(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// one corner: position p and normal n (in and out) under M = sum_k w[k] J[joint[k]]
template <class Palette> NXD void pose_corner(const Palette& J, const float4 w, const uint32_t j01, const uint32_t j23, float (&p)[3], float (&n)[3])
{
    const uint32_t j[4] = {j01 & 0xffffu, j01 >> 16, j23 & 0xffffu, j23 >> 16};
    Row3x4 M;
    for (int r = 0; r < 3; r++)
        M.r[r] = plus(plus(plus(scaled(w.x, J(j[0], r)), scaled(w.y, J(j[1], r))), scaled(w.z, J(j[2], r))), scaled(w.w, J(j[3], r)));
    const float m[3][3] = {{M.r[0].x, M.r[0].y, M.r[0].z}, {M.r[1].x, M.r[1].y, M.r[1].z}, {M.r[2].x, M.r[2].y, M.r[2].z}};
    const float q[3] = {p[0], p[1], p[2]};
    p[0] = m[0][0] * q[0] + m[0][1] * q[1] + m[0][2] * q[2] + M.r[0].w;
    p[1] = m[1][0] * q[0] + m[1][1] * q[1] + m[1][2] * q[2] + M.r[1].w;
    p[2] = m[2][0] * q[0] + m[2][1] * q[1] + m[2][2] * q[2] + M.r[2].w;
    if (n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) return;  // (a mesh without NORMAL: the loaders' zero stays)
    // the cofactor matrix of the upper 3 x 3: det * inverse transpose
    const float c[3][3] = {
        {m[1][1] * m[2][2] - m[1][2] * m[2][1], m[1][2] * m[2][0] - m[1][0] * m[2][2], m[1][0] * m[2][1] - m[1][1] * m[2][0]},
        {m[0][2] * m[2][1] - m[0][1] * m[2][2], m[0][0] * m[2][2] - m[0][2] * m[2][0], m[0][1] * m[2][0] - m[0][0] * m[2][1]},
        {m[0][1] * m[1][2] - m[0][2] * m[1][1], m[0][2] * m[1][0] - m[0][0] * m[1][2], m[0][0] * m[1][1] - m[0][1] * m[1][0]}};
    const float det = m[0][0] * c[0][0] + m[0][1] * c[0][1] + m[0][2] * c[0][2];
    float v[3];
    for (int r = 0; r < 3; r++) {
        v[r] = c[r][0] * n[0] + c[r][1] * n[1] + c[r][2] * n[2];
        if (det < 0.0f) v[r] = -v[r];
    }
    const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const bool ok = len > 0.0f && len < __uint_as_float(0x7f800000u);  // (false for NaN as well)
    for (int r = 0; r < 3; r++) n[r] = ok ? v[r] / len : 0.0f;
}

// the end of a corner's morph stage: the summed normal n + sum w_t dNormal_t normalised; a length of 0 or not finite gives (0, 0, 0)
NXD void morph_normalise(float (&n)[3])
{
    const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const bool ok = len > 0.0f && len < __uint_as_float(0x7f800000u);  // (false for NaN as well)
    for (int r = 0; r < 3; r++) n[r] = ok ? n[r] / len : 0.0f;
}

// The pass, in its five instances: kMorph — the active targets' deltas (MorphTri, nx_device.h) are added to the bind corner first;
// kSkin — the joint blend follows (kLds: its palette from the LDS).  pose_kernel<kLds> below is <kLds, false, true>: the kernel
// nxhip_pose_blas launches, with the code it had before there were morph targets.
// (kernel parameters are plain pointers: see instance_transform_kernel, nx_refit.hip)
template <bool kLds, bool kMorph, bool kSkin>
NXD void pose_pass(const uint4* bindArg, const uint4* skinArg, const float4* paletteArg, const uint32_t jointCount, const uint32_t* __restrict__ primIdx, const uint32_t n,
                   uint4* trisArg, uint4* shadeArg, float4* isectArg, const uint4* morphArg, const uint2* __restrict__ active, const uint32_t activeCount)
{
    extern __shared__ float4 ldsPalette[];  // kLds: 3 x jointCount rows (the launch gives the bytes)
    const NX_G uint4* bind = (const NX_G uint4*)bindArg;
    const NX_G uint4* skin = (const NX_G uint4*)skinArg;
    const NX_G float4* palette = (const NX_G float4*)paletteArg;
    const NX_G uint4* morph = (const NX_G uint4*)morphArg;
    NX_G uint4* tris = (NX_G uint4*)trisArg;
    NX_G char* shade = (NX_G char*)shadeArg;
    NX_G float4* isect = (NX_G float4*)isectArg;
    if constexpr (kLds) {
        for (uint32_t i = threadIdx.x; i < 3u * jointCount; i += blockDim.x) ldsPalette[i] = palette[i];
        __syncthreads();
    }
    auto J = [&](const uint32_t joint, const int r) -> float4 {
        if constexpr (kLds) return ldsPalette[3u * joint + (uint32_t)r];
        else return palette[3u * joint + (uint32_t)r];
    };
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const uint32_t id = primIdx[k];
        uint4 t[6], s[5];
        for (int i = 0; i < 6; i++) t[i] = bind[6 * (size_t)id + i];
        if constexpr (kSkin)
            for (int i = 0; i < 5; i++) s[i] = skin[5 * (size_t)id + i];
        // nx_triangle as 24 words: pos0 0..2, pos1 3..5, pos2 6..8, normal0 9..11, normal1 12..14, normal2 15..17, texCoords 18..23
        uint32_t word[24];
        for (int i = 0; i < 6; i++) { word[4 * i] = t[i].x; word[4 * i + 1] = t[i].y; word[4 * i + 2] = t[i].z; word[4 * i + 3] = t[i].w; }
        if constexpr (kMorph) {
            if (activeCount != 0u) {  // (no active target: the stage is absent — no sum of zeros, no renormalised normal)
                // words 0..17 as floats: the three positions, then the three normals — MorphTri's own order
                float acc[18];
                for (int i = 0; i < 18; i++) acc[i] = __uint_as_float(word[i]);
                for (uint32_t a = 0; a < activeCount; a++) {
                    const uint2 tw = active[a];  // (uniform over the grid: target index, weight)
                    const float w = __uint_as_float(tw.y);
                    const NX_G uint4* rec = morph + 5 * ((size_t)tw.x * (size_t)n + (size_t)id);
                    uint4 d[5];
                    for (int i = 0; i < 5; i++) d[i] = rec[i];
                    const uint32_t dw[20] = {d[0].x, d[0].y, d[0].z, d[0].w, d[1].x, d[1].y, d[1].z, d[1].w, d[2].x, d[2].y,
                                             d[2].z, d[2].w, d[3].x, d[3].y, d[3].z, d[3].w, d[4].x, d[4].y, d[4].z, d[4].w};
                    for (int i = 0; i < 18; i++) acc[i] = acc[i] + w * __uint_as_float(dw[i]);
                }
                for (int v = 0; v < 3; v++) {
                    for (int a = 0; a < 3; a++) word[3 * v + a] = __float_as_uint(acc[3 * v + a]);
                    // a bind normal of exactly (0, 0, 0) stays: its deltas are not applied
                    if (word[9 + 3 * v] << 1 == 0u && word[10 + 3 * v] << 1 == 0u && word[11 + 3 * v] << 1 == 0u) continue;
                    float nrm[3] = {acc[9 + 3 * v], acc[10 + 3 * v], acc[11 + 3 * v]};
                    morph_normalise(nrm);
                    for (int a = 0; a < 3; a++) word[9 + 3 * v + a] = __float_as_uint(nrm[a]);
                }
            }
        }
        if constexpr (kSkin) {
            const uint32_t joints[6] = {s[3].x, s[3].y, s[3].z, s[3].w, s[4].x, s[4].y};
            for (int v = 0; v < 3; v++) {
                float p[3], nrm[3];
                for (int a = 0; a < 3; a++) { p[a] = __uint_as_float(word[3 * v + a]); nrm[a] = __uint_as_float(word[9 + 3 * v + a]); }
                const float4 w = make_float4(__uint_as_float(s[v].x), __uint_as_float(s[v].y), __uint_as_float(s[v].z), __uint_as_float(s[v].w));
                pose_corner(J, w, joints[2 * v], joints[2 * v + 1], p, nrm);
                for (int a = 0; a < 3; a++) { word[3 * v + a] = __float_as_uint(p[a]); word[9 + 3 * v + a] = __float_as_uint(nrm[a]); }
            }
        }
        for (int i = 0; i < 6; i++) t[i] = make_uint4(word[4 * i], word[4 * i + 1], word[4 * i + 2], word[4 * i + 3]);
        for (int i = 0; i < 6; i++) tris[6 * (size_t)id + i] = t[i];
        if (kShadeTriStride != (int)sizeof(nx_triangle)) {
            NX_G uint4* dst = (NX_G uint4*)(shade + (size_t)id * (size_t)kShadeTriStride);
            for (int i = 0; i < 6; i++) dst[i] = t[i];
        }
        // isect_kernel's record (nx_lbvh.hip), from the values just stored
        const float p0[3] = {__uint_as_float(word[0]), __uint_as_float(word[1]), __uint_as_float(word[2])};
        const float p1[3] = {__uint_as_float(word[3]), __uint_as_float(word[4]), __uint_as_float(word[5])};
        const float p2[3] = {__uint_as_float(word[6]), __uint_as_float(word[7]), __uint_as_float(word[8])};
        isect[(size_t)kTriStride * k + 0] = make_float4(p0[0], p0[1], p0[2], __uint_as_float(id));
        isect[(size_t)kTriStride * k + 1] = make_float4(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2], 0.0f);
        isect[(size_t)kTriStride * k + 2] = make_float4(p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2], 0.0f);
    }
}

template <bool kLds>
__global__ void __launch_bounds__(kPoseBlock) pose_kernel(const uint4* bindArg, const uint4* skinArg, const float4* paletteArg, const uint32_t jointCount,
                                                          const uint32_t* __restrict__ primIdx, const uint32_t n, uint4* trisArg, uint4* shadeArg, float4* isectArg)
{
    pose_pass<kLds, false, true>(bindArg, skinArg, paletteArg, jointCount, primIdx, n, trisArg, shadeArg, isectArg, nullptr, nullptr, 0u);
}

// nxhip_pose_blas_morph's kernel: the list above, then the MorphTri records (target-major), the active (index, weight) pairs and their count
template <bool kLds, bool kSkin>
__global__ void __launch_bounds__(kPoseBlock) pose_morph_kernel(const uint4* bindArg, const uint4* skinArg, const float4* paletteArg, const uint32_t jointCount,
                                                                const uint32_t* __restrict__ primIdx, const uint32_t n, uint4* trisArg, uint4* shadeArg, float4* isectArg,
                                                                const uint4* morphArg, const uint2* __restrict__ active, const uint32_t activeCount)
{
    pose_pass<kLds, true, kSkin>(bindArg, skinArg, paletteArg, jointCount, primIdx, n, trisArg, shadeArg, isectArg, morphArg, active, activeCount);
}

const void* pose_kernel_ptr(bool lds) { return lds ? (const void*)pose_kernel<true> : (const void*)pose_kernel<false>; }
const void* pose_morph_kernel_ptr(bool skin, bool lds)
{
    if (!skin) return (const void*)pose_morph_kernel<false, false>;
    return lds ? (const void*)pose_morph_kernel<true, true> : (const void*)pose_morph_kernel<false, true>;
}

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_skin() { return layout_stamp(); }

}  // namespace nxd
