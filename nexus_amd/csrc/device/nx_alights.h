// nx_alights.h — analytic lights (nxhip_set_analytic_lights): the light sample's draw for one of them (the record: nx_device.h ALight).
// The contract is the header's (include/nexus_hip.h, "Analytic lights"); this file is its one implementation on the device: the
// ANALYTIC instances of the material kernels (nx_wavefront.h next_event_estimation) and the test hook (alight_hook_kernel) both
// call alight_sample.
#pragma once

#include "nx_device.h"
#include "nx_math.h"

namespace nxd {

// The draw for light L from the (already offset) origin o with the two random numbers r1, r2: direction, the shadow ray's length and
// factor = colour x intensity x att x 2 / (d^2 (1 + cos thetaMax)), the radiance over the density of the uniform cone.  One rule for
// every kind — a point is a sphere of radius 0, a delta sun a disc of angle 0 — written as one straight-line path with selects on the
// kind: the lanes of a wave pick different lights.  false: the origin lies inside the sphere (d <= radius), no sample.
NXD bool alight_sample(const NX_G ALight* L, const f3 o, const float r1, const float r2, f3& dir, float& tmax, f3& factor)
{
    const float4 v0 = L->v0, v1 = L->v1, v2 = L->v2, v3 = L->v3;
    const bool directional = v2.w != 0.0f;
    const f3 axis = mk3(v1.x, v1.y, v1.z);
    const f3 toCentre = mk3(v0.x, v0.y, v0.z) - o;
    const float d2c = dot3(toCentre, toCentre);
    const float dc = sqrtf(d2c);
    const f3 a = directional ? -axis : toCentre / dc;
    const float d = directional ? 1.0f : dc, d2 = directional ? 1.0f : d2c;
    const float radius = v0.w, radius2 = v3.z;
    const bool ok = directional || dc > radius;
    // q = 1 - cos thetaMax.  Not 1 - sqrt(1 - s2): that cancels (7 % off at radius / d = 1e-3 in binary32); this form is good to 1e-7
    const float s2 = radius2 / d2;
    const float q = directional ? v1.w : s2 / (1.0f + sqrtf(fmaxf(1.0f - s2, 0.0f)));
    const float rq = r1 * q;
    const float cosT = 1.0f - rq, sin2 = rq * (2.0f - rq);  // (no 1 - cos^2)
    const float sinT = sqrtf(sin2);
    const float phi = 6.28318531f * r2;
    // an orthonormal frame about a without a branch (Duff et al. 2017, "Building an Orthonormal Basis, Revisited")
    const float sg = copysignf(1.0f, a.z);
    const float k = -1.0f / (sg + a.z);
    const float b = a.x * a.y * k;
    const f3 t0 = mk3(1.0f + sg * a.x * a.x * k, sg * b, -sg * a.x), t1 = mk3(b, sg + a.y * a.y * k, -a.y);
    dir = (t0 * (nxf_cosf(phi) * sinT) + t1 * (nxf_sinf(phi) * sinT)) + a * cosT;
    // the near intersection with the sphere
    tmax = directional ? 1e30f : d * cosT - sqrtf(fmaxf(radius2 - d2 * sin2, 0.0f));
    // the spot's falloff (KHR_lights_punctual), taken at the centre: cd = cosine between the axis and the direction from the centre to o
    const float fall = fminf(fmaxf(-dot3(axis, a) * v3.x + v3.y, 0.0f), 1.0f);
    factor = mk3(v2.x, v2.y, v2.z) * ((fall * fall) * (2.0f / (d2 * (2.0f - q))));
    return ok;
}

}  // namespace nxd
