// nx_detail.h — detail maps in the material step: the roughness map's factor and the normal map's shading normal.
//
// The rule is stated in full in include/nexus_hip.h (nxhip_set_material_detail); this is its one device text, called by the DETAIL
// instances of the material kernels (nx_wavefront.h shade_path) and by the test hook (nxhip_shading_frame_batch).
// Tangents come from the triangle's positions and texture coordinates (set 0), per triangle: the 96-byte nx_triangle has no room for
// glTF's TANGENT attribute.
#pragma once

#include "nx_device.h"
#include "nx_math.h"
#include "nx_texture.h"

namespace nxd {

// a squared length that is a usable one: not 0, not infinite, not NaN
NXD bool usable_length2(float l2) { return l2 > 0.0f && l2 < __builtin_huge_valf(); }

// N, gNormal: the interpolated and the geometric world normal BEFORE the back-face flip; both come back flipped as the default
// instance flips them (dot(gNormal, rayDirection) > 0 && TYPE != DIELECTRIC).  roughness: multiplied by the roughness map's G channel
// when the material names one.  Returns the shading normal after fallback and flip — N itself when the material names no normal
// map; fellBack: a normal map was named and one of the fallback conditions took the result back to N.
// tri: the hit's shading triangle; T: rows 0..2 of the instance's forward transform; tp0..tp2: the triangle's object-space positions
// (the caller has them in registers); texUv: the hit's texture coordinates.
template <int TYPE, class Tri, class Mat>
NXD f3 detail_shading_frame(const DeviceState* S, const nx_material_detail d, Tri tri, Mat T, const f3 tp0, const f3 tp1, const f3 tp2, const f2 texUv, const f3 rayDirection,
                            f3& N, f3& gNormal, float& roughness, bool& fellBack, float* const metallic = nullptr)
{
    if constexpr (TYPE == NX_MAT_METALROUGH) {
        // metallic (NX_MAT_METALROUGH only, which always passes it): multiplied by the B channel of the SAME lookup
        if (d.roughnessMapId != -1) {
            const float4 mr = tex2d_linear(S->roughnessMaps[d.roughnessMapId], texUv.x, texUv.y);
            roughness = roughness * mr.y;
            *metallic = *metallic * mr.z;
        }
    } else {
        if (d.roughnessMapId != -1) roughness = roughness * tex2d_linear(S->roughnessMaps[d.roughnessMapId], texUv.x, texUv.y).y;
    }
    f3 ns = N;
    fellBack = false;
    if (d.normalMapId != -1) {
        fellBack = true;
        const float4 c = tex2d_linear(S->normalMaps[d.normalMapId], texUv.x, texUv.y);
        const float mx = (2.0f * c.x - 1.0f) * d.normalScale, my = (2.0f * c.y - 1.0f) * d.normalScale, mz = 2.0f * c.z - 1.0f;
        const float du1 = tri->texCoord1[0] - tri->texCoord0[0], dv1 = tri->texCoord1[1] - tri->texCoord0[1];
        const float du2 = tri->texCoord2[0] - tri->texCoord0[0], dv2 = tri->texCoord2[1] - tri->texCoord0[1];
        const float det = du1 * dv2 - du2 * dv1;
        if (fabsf(det) > 0.0f) {
            const float sg = det < 0.0f ? -1.0f : 1.0f;
            const f3 e1 = tp1 - tp0, e2 = tp2 - tp0;
            const f3 Tu = mat_vec(T, (e1 * dv2 - e2 * dv1) * sg), Tv = mat_vec(T, (e2 * du1 - e1 * du2) * sg);
            const f3 tp = Tu - N * dot3(N, Tu);
            const float tl2 = dot3(tp, tp);
            if (usable_length2(tl2)) {
                const f3 t = tp * (1.0f / sqrtf(tl2));
                f3 b = cross3(N, t);
                if (dot3(b, Tv) > 0.0f) b = -b;  // glTF's v runs down the image, green points up: b . (-Tv) >= 0
                const f3 raw = (t * mx + b * my) + N * mz;
                const float rl2 = dot3(raw, raw);
                if (usable_length2(rl2)) {
                    const f3 cand = raw * (1.0f / sqrtf(rl2));
                    // the view v = -rayDirection must be above the mapped horizon on the side it is above the interpolated one:
                    // (ns . v)(N . v) > 0, and the two signs of v cancel
                    if (dot3(cand, rayDirection) * dot3(N, rayDirection) > 0.0f) { ns = cand; fellBack = false; }
                }
            }
        }
    }
    if (dot3(gNormal, rayDirection) > 0.0f && TYPE != NX_MAT_DIELECTRIC) { N = -N; gNormal = -gNormal; ns = -ns; }
    return ns;
}

}  // namespace nxd
