// nx_sky.hip — the sun-and-sky environment (nxhip_set_sky; the model is stated in full in include/nexus_hip.h), generated on the device
// straight into the float4 texel buffer the passes read.
//
//   sky_map_kernel    one lane per texel, 256-lane workgroups, the grid sized by the texel count: the texel's direction, then sky_radiance
//   sky_disc_kernel   one lane per texel of the sun disc's bounding box (computed on the host): the coverage c of the texel's 8 x 8
//                     sub-positions in binary64, Lsun x c x k added to the texel
//   sky_hook_kernel   sky_radiance on arrays of directions (nxhip_sky_radiance_batch)
//
// Units and precision.  Lengths are kilometres on the device (Rg = 6360, scale heights 8 and 1.2, the betas per km), so nothing leaves
// binary32's comfortable range.  The height of a point at |p| = 6.4e3 km is the difference |p| - Rg, which binary32 gives to half a
// metre; so no position is ever formed.  A ray is carried as two scalars of its origin p and unit direction w,
//   q = |p|^2 - Rg^2      b = p . w
// and the point at parameter u along it has q(u) = q + u (2 b + u), |p(u)| = sqrt(Rg^2 + q(u)), height h(u) = q(u) / (|p(u)| + Rg): no
// cancellation (h inherits q's relative error; q's terms cancel only where the geometry does, near the ground, to 1e-7 km).  The
// observer's q is altitude x (2 Rg + altitude), from the host in binary64.  Exits and ground hits are the roots of u^2 + 2 b u + q - c =
// 0 in their cancellation-free forms.  Exponentials, square roots and reciprocals are the hardware's (v_exp_f32, v_sqrt_f32, v_rcp_f32:
// 1 ulp); the accuracy against binary64 is measured by tests/test_gpu_sky.py.
//
// Cost.  The inner loop is Nv x Nl steps per texel of one sqrt, one rcp, two exp and a dozen plain operations, nothing from memory: it
// is bound by vector issue, transcendentals at half rate.  Live state across it is eight accumulators and the ray's scalars, far below
// the 64 registers of full occupancy (profiles/sky_kernel_resources.txt: no scratch).  Measured: 1.60 ms at 2048 x 1024 with the default
// 64 x 16 steps, 6.30 ms at 4096 x 2048 (profiles/sky.txt).
#include <algorithm>
#include <cmath>
#include <string>

#include "nx_host.h"

namespace nxd {

namespace {

constexpr int kSkyBlock = 256;
constexpr float kRg = 6360.0f, kRg2 = 6360.0f * 6360.0f;  // km; Rg^2 = 40 449 600 is exact in binary32
constexpr float kShell = 6420.0f * 6420.0f - 6360.0f * 6360.0f;  // Rt^2 - Rg^2 = 766 800, exact
constexpr float kInvHR = 1.0f / 8.0f, kInvHM = 1.0f / 1.2f;

__device__ __forceinline__ float sky_exp(const float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }

// exp(-h / HR), exp(-h / HM) at the point whose |p|^2 - Rg^2 is q
__device__ __forceinline__ void sky_density(const float q, float& rhoR, float& rhoM)
{
    const float r = __builtin_amdgcn_sqrtf(kRg2 + q);
    const float h = q * __builtin_amdgcn_rcpf(r + kRg);
    rhoR = sky_exp(-h * kInvHR);
    rhoM = sky_exp(-h * kInvHM);
}

// distance to the Rt sphere along a ray (q, b) that starts inside it: the positive root of u^2 + 2 b u - c = 0, c = Rt^2 - |p|^2 >= 0
__device__ __forceinline__ float sky_exit(const float q, const float b)
{
    const float c = fmaxf(kShell - q, 0.0f);
    const float s = __builtin_amdgcn_sqrtf(b * b + c);
    return b > 0.0f ? c * __builtin_amdgcn_rcpf(b + s) : s - b;
}

// The light-ray rule from the point (q, b = p . sun): false when the ray hits the Rg sphere ahead of it; else the optical depths of nl
// quadratic segments to the Rt exit, midpoint rule.
__device__ __forceinline__ bool sky_light_ray(const float q, const float b, const uint32_t nl, const float invNl, float& tauR, float& tauM)
{
    if (b < 0.0f && b * b - q >= 0.0f) return false;
    const float uEnd = sky_exit(q, b), twoB = 2.0f * b;
    float aR = 0.0f, aM = 0.0f, u0 = 0.0f;
    for (uint32_t j = 1; j <= nl; j++) {
        const float f = (float)j * invNl, u1 = uEnd * (f * f), um = 0.5f * (u0 + u1);
        float rhoR, rhoM;
        sky_density(q + um * (twoB + um), rhoR, rhoM);
        aR += rhoR * (u1 - u0);
        aM += rhoM * (u1 - u0);
        u0 = u1;
    }
    tauR = aR;
    tauM = aM;
    return true;
}

// The sky term along the unit direction (dx, dy, dz): single scattering, and the sunlit ground where the view ray ends on the planet.
// The ONE function the map kernel and the hook call.
__device__ void sky_radiance(const SkyLaunch& P, const float dx, const float dy, const float dz, float& outR, float& outG, float& outB)
{
    const float q0 = P.q0, b0 = P.r0 * dy;
    const float mu = (dx * P.sun[0] + dy * P.sun[1]) + dz * P.sun[2];
    const float pSun0 = P.r0 * P.sun[1];  // observer . sun
    const float disc = b0 * b0 - q0;
    const bool ground = b0 < 0.0f && disc >= 0.0f;
    const float tEnd = ground ? q0 * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(disc) - b0) : sky_exit(q0, b0);
    const float invNv = 1.0f / (float)P.nv, invNl = 1.0f / (float)P.nl, twoB0 = 2.0f * b0;
    float tauR = 0.0f, tauM = 0.0f;                 // view optical depths up to the current segment's start
    float rR = 0.0f, rG = 0.0f, rB = 0.0f;          // sum of rhoR ds x attenuation, per channel
    float mR = 0.0f, mG = 0.0f, mB = 0.0f;          // ... of rhoM
    float t0 = 0.0f;
    for (uint32_t i = 1; i <= P.nv; i++) {
        const float f = (float)i * invNv, t1 = tEnd * (f * f), tm = 0.5f * (t0 + t1), ds = t1 - t0;
        const float q = q0 + tm * (twoB0 + tm);
        float rhoR, rhoM;
        sky_density(q, rhoR, rhoM);
        const float dR = rhoR * ds, dM = rhoM * ds;
        float lR, lM;
        if (sky_light_ray(q, pSun0 + tm * mu, P.nl, invNl, lR, lM)) {
            const float sR = (tauR + 0.5f * dR) + lR, sM = ((tauM + 0.5f * dM) + lM) * P.betaMe;
            const float aR = sky_exp(-(P.betaR[0] * sR + sM)), aG = sky_exp(-(P.betaR[1] * sR + sM)), aB = sky_exp(-(P.betaR[2] * sR + sM));
            rR += dR * aR; rG += dR * aG; rB += dR * aB;
            mR += dM * aR; mG += dM * aG; mB += dM * aB;
        }
        tauR += dR;
        tauM += dM;
        t0 = t1;
    }
    const float pi = 3.14159265358979323846f;
    const float g = P.g, g2 = g * g, mu2 = 1.0f + mu * mu;
    const float pr = (3.0f / (16.0f * pi)) * mu2;
    const float den = (1.0f + g2) - 2.0f * g * mu;
    const float pm = (3.0f / (8.0f * pi)) * (1.0f - g2) * mu2 / ((2.0f + g2) * (den * sqrtf(den)));
    const float wm = P.betaMs * pm;
    float oR = P.irradiance[0] * (P.betaR[0] * pr * rR + wm * mR);
    float oG = P.irradiance[1] * (P.betaR[1] * pr * rG + wm * mG);
    float oB = P.irradiance[2] * (P.betaR[2] * pr * rB + wm * mB);
    if (ground) {
        const float bg = pSun0 + tEnd * mu;  // ground point . sun = Rg (n . s)
        float lR, lM;
        if (bg > 0.0f && sky_light_ray(0.0f, bg, P.nl, invNl, lR, lM)) {
            const float sR = tauR + lR, sM = (tauM + lM) * P.betaMe;
            const float w = bg * (1.0f / kRg) * (1.0f / pi);
            oR += P.albedo[0] * w * P.irradiance[0] * sky_exp(-(P.betaR[0] * sR + sM));
            oG += P.albedo[1] * w * P.irradiance[1] * sky_exp(-(P.betaR[1] * sR + sM));
            oB += P.albedo[2] * w * P.irradiance[2] * sky_exp(-(P.betaR[2] * sR + sM));
        }
    }
    outR = oR; outG = oG; outB = oB;
}

__global__ void __launch_bounds__(kSkyBlock) sky_map_kernel(float4* __restrict__ texels, const uint32_t W, const uint32_t H, const SkyLaunch P)
{
    const uint32_t i = blockIdx.x * (uint32_t)kSkyBlock + threadIdx.x;  // (W x H <= 2^27)
    if (i >= W * H) return;
    const uint32_t y = i / W, x = i - y * W;
    const float pi = 3.14159265358979323846f;
    const float phi = 0.5f * pi - pi * (((float)y + 0.5f) / (float)H), theta = 2.0f * pi * (((float)x + 0.5f) / (float)W) - pi;
    const float cp = cosf(phi), sp = sinf(phi);
    float r, g, b;
    sky_radiance(P, cp * cosf(theta), sp, cp * sinf(theta), r, g, b);
    texels[i] = make_float4(r, g, b, 0.0f);
}

// coverage of one texel by the sun's cap: how many of its 8 x 8 sub-positions lie within alpha of the sun (|d - s|^2 <= 4 sin^2(alpha / 2))
__host__ __device__ inline uint32_t sky_disc_count(const uint32_t x, const uint32_t y, const uint32_t W, const uint32_t H, const double sx, const double sy, const double sz,
                                                   const double chord2)
{
    const double pi = 3.14159265358979323846;
    uint32_t n = 0;
    for (int j = 0; j < 8; j++) {
        const double phi = 0.5 * pi - pi * (((double)y + ((double)j + 0.5) / 8.0) / (double)H);
        const double sp = sin(phi), cp = cos(phi);
        for (int k = 0; k < 8; k++) {
            const double theta = 2.0 * pi * (((double)x + ((double)k + 0.5) / 8.0) / (double)W) - pi;
            const double ex = cp * cos(theta) - sx, ey = sp - sy, ez = cp * sin(theta) - sz;
            if ((ex * ex + ey * ey) + ez * ez <= chord2) n++;
        }
    }
    return n;
}

__global__ void __launch_bounds__(kSkyBlock) sky_disc_kernel(float4* __restrict__ texels, const uint32_t W, const uint32_t H, const SkyDisc D)
{
    const uint32_t i = blockIdx.x * (uint32_t)kSkyBlock + threadIdx.x;
    if (i >= D.w * D.h) return;
    const uint32_t by = i / D.w, bx = i - by * D.w;
    const uint32_t x = (D.x0 + bx) % W, y = D.y0 + by;  // (the box wraps over the u seam; y0 + h <= H)
    const uint32_t n = sky_disc_count(x, y, W, H, D.sun[0], D.sun[1], D.sun[2], D.chord2);
    if (n == 0) return;
    const float c = (float)n * (1.0f / 64.0f);
    float4 t = texels[(size_t)y * W + x];
    t.x += D.add[0] * c;
    t.y += D.add[1] * c;
    t.z += D.add[2] * c;
    texels[(size_t)y * W + x] = t;
}

__global__ void __launch_bounds__(kWideBlock) sky_hook_kernel(const SkyLaunch P, const float* __restrict__ dir, const uint32_t count, float* __restrict__ rgb)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x)
        sky_radiance(P, dir[3 * k], dir[3 * k + 1], dir[3 * k + 2], rgb[3 * k], rgb[3 * k + 1], rgb[3 * k + 2]);
}

// ---- the host's share, binary64, metres in and kilometres out -------------------------------------------

constexpr double kPi = 3.14159265358979323846;
constexpr double kRgKm = 6360.0, kShellKm = 766800.0;

bool finite_all(const float* x, int n)
{
    for (int k = 0; k < n; k++)
        if (!(x[k] >= -3.402823466e38f && x[k] <= 3.402823466e38f)) return false;
    return true;
}

// the light-ray rule in binary64 from the point (q, b): T per channel, 0 when the ray hits the planet
void light_ray_transmittance(const double q, const double b, const uint32_t n, const double betaR[3], const double betaMe, double T[3])
{
    T[0] = T[1] = T[2] = 0.0;
    if (b < 0.0 && b * b - q >= 0.0) return;
    const double c = std::max(kShellKm - q, 0.0), s = std::sqrt(b * b + c), uEnd = b > 0.0 ? c / (b + s) : s - b;
    double tauR = 0.0, tauM = 0.0, u0 = 0.0;
    for (uint32_t j = 1; j <= n; j++) {
        const double f = (double)j / (double)n, u1 = uEnd * f * f, um = 0.5 * (u0 + u1);
        const double qq = q + um * (2.0 * b + um), h = qq / (std::sqrt(kRgKm * kRgKm + qq) + kRgKm);
        tauR += std::exp(-h / 8.0) * (u1 - u0);
        tauM += std::exp(-h / 1.2) * (u1 - u0);
        u0 = u1;
    }
    for (int ch = 0; ch < 3; ch++) T[ch] = std::exp(-(betaR[ch] * tauR + betaMe * tauM));
}

}  // namespace

int sky_plan(const nx_sky* sky, const char* who, SkyPlan* out)
{
    const std::string name(who);
    if (!sky) return fail_invalid(name + ": sky is NULL");
    const nx_sky& s = *sky;
    if (!finite_all(s.sunDirection, 3) || !finite_all(&s.sunAngularRadius, 1) || !finite_all(s.sunIrradiance, 3) || !finite_all(&s.altitude, 1) ||
        !finite_all(&s.rayleighScale, 1) || !finite_all(&s.mieScale, 1) || !finite_all(&s.mieG, 1) || !finite_all(s.groundAlbedo, 3))
        return fail_invalid(name + ": every field must be finite");
    const double dx = s.sunDirection[0], dy = s.sunDirection[1], dz = s.sunDirection[2], len = std::sqrt(dx * dx + dy * dy + dz * dz);
    if (!(len > 0.0)) return fail_invalid(name + ": sunDirection is zero");
    for (int ch = 0; ch < 3; ch++) {
        if (s.sunIrradiance[ch] < 0.0f) return fail_invalid(name + ": sunIrradiance must not be negative");
        if (s.groundAlbedo[ch] < 0.0f || s.groundAlbedo[ch] > 1.0f) return fail_invalid(name + ": groundAlbedo must be in [0, 1]");
    }
    if (s.rayleighScale < 0.0f || s.mieScale < 0.0f) return fail_invalid(name + ": rayleighScale and mieScale must not be negative");
    if (!(std::fabs((double)s.mieG) < 1.0)) return fail_invalid(name + ": |mieG| must be below 1");
    if (s.altitude < 1.0f || s.altitude > 50000.0f) return fail_invalid(name + ": altitude must be in [1, 50000] metres");
    if (s.sunAngularRadius < 0.0f || !((double)s.sunAngularRadius < 0.5 * kPi)) return fail_invalid(name + ": sunAngularRadius must be in [0, pi/2)");
    if (s.width == 0 || s.height == 0 || s.width > 32768u || s.height > 32768u || (uint64_t)s.width * s.height > (1ull << 27))
        return fail_invalid(name + ": the map must have 1 to 32768 texels per axis and at most 2^27 in all");
    if (s.viewSteps < 1 || s.viewSteps > 1024 || s.lightSteps < 1 || s.lightSteps > 1024) return fail_invalid(name + ": viewSteps and lightSteps must be in [1, 1024]");
    if (s.sunDisc > 1) return fail_invalid(name + ": sunDisc must be 0 or 1");
    if (s.sunDisc == 1 && !(s.sunAngularRadius > 0.0f)) return fail_invalid(name + ": a sun disc needs sunAngularRadius > 0");

    SkyPlan& p = *out;
    p = SkyPlan();
    p.sun[0] = dx / len; p.sun[1] = dy / len; p.sun[2] = dz / len;
    p.alpha = (double)s.sunAngularRadius;
    const double h0 = (double)s.altitude * 1e-3;
    p.q0 = h0 * (2.0 * kRgKm + h0);
    p.r0 = kRgKm + h0;
    const double baseR[3] = {5.802e-3, 13.558e-3, 33.1e-3};  // per km
    for (int ch = 0; ch < 3; ch++) p.betaR[ch] = baseR[ch] * (double)s.rayleighScale;
    p.betaMs = 3.996e-3 * (double)s.mieScale;
    p.betaMe = p.betaMs / 0.9;
    SkyLaunch& l = p.launch;
    l.r0 = (float)p.r0;
    l.q0 = (float)p.q0;
    for (int ch = 0; ch < 3; ch++) {
        l.sun[ch] = (float)p.sun[ch];
        l.betaR[ch] = (float)p.betaR[ch];
        l.irradiance[ch] = s.sunIrradiance[ch];
        l.albedo[ch] = s.groundAlbedo[ch];
    }
    l.betaMs = (float)p.betaMs;
    l.betaMe = (float)p.betaMe;
    l.g = s.mieG;
    l.nv = s.viewSteps;
    l.nl = s.lightSteps;
    return NXHIP_OK;
}

void sky_sun_transmittance(const SkyPlan& p, uint32_t segments, double T[3]) { light_ray_transmittance(p.q0, p.r0 * p.sun[1], segments, p.betaR, p.betaMe, T); }

// The disc of a W x H map: its bounding box, Lsun x k per channel.  NXHIP_ERR_INVALID when no sub-position of any texel lies in the cap.
int sky_disc_plan(const nx_sky* sky, const SkyPlan& p, const char* who, SkyDisc* out)
{
    const uint32_t W = sky->width, H = sky->height;
    const double alpha = p.alpha, phiS = std::asin(std::max(-1.0, std::min(1.0, p.sun[1]))), thetaS = std::atan2(p.sun[2], p.sun[0]);
    SkyDisc& d = *out;
    d = SkyDisc();
    const double vLo = (0.5 * kPi - (phiS + alpha)) / kPi, vHi = (0.5 * kPi - (phiS - alpha)) / kPi;
    const long yLo = std::max(0l, (long)std::floor(vLo * (double)H) - 1l), yHi = std::min((long)H - 1l, (long)std::floor(vHi * (double)H) + 1l);
    d.y0 = (uint32_t)yLo;
    d.h = (uint32_t)(yHi - yLo + 1);
    d.x0 = 0;
    d.w = W;
    if (std::fabs(phiS) + alpha < 0.5 * kPi - 1e-9) {  // (the cap holds no pole: its longitudes are theta_s +- asin(sin alpha / cos phi_s))
        const double dTheta = std::asin(std::min(1.0, std::sin(alpha) / std::cos(phiS)));
        const double uc = (thetaS + kPi) / (2.0 * kPi), du = dTheta / (2.0 * kPi);
        const long xLo = (long)std::floor((uc - du) * (double)W) - 1l, xHi = (long)std::floor((uc + du) * (double)W) + 1l;
        if (xHi - xLo + 1 < (long)W) {
            d.x0 = (uint32_t)(((xLo % (long)W) + (long)W) % (long)W);
            d.w = (uint32_t)(xHi - xLo + 1);
        }
    }
    for (int ch = 0; ch < 3; ch++) d.sun[ch] = p.sun[ch];
    const double sh = std::sin(0.5 * alpha);
    d.chord2 = 4.0 * sh * sh;
    double sum = 0.0;  // of c x Omega over the box
    for (uint32_t by = 0; by < d.h; by++) {
        const uint32_t y = d.y0 + by;
        const double omega = (2.0 * kPi / (double)W) * (std::sin(0.5 * kPi - kPi * (double)y / (double)H) - std::sin(0.5 * kPi - kPi * ((double)y + 1.0) / (double)H));
        uint64_t n = 0;
        for (uint32_t bx = 0; bx < d.w; bx++) n += sky_disc_count((d.x0 + bx) % W, y, W, H, d.sun[0], d.sun[1], d.sun[2], d.chord2);
        sum += (double)n / 64.0 * omega;
    }
    if (!(sum > 0.0))
        return fail_invalid(std::string(who) + ": the sun's disc fell between the sub-positions of the map's texels: use a larger map or a larger sunAngularRadius");
    const double k = 2.0 * kPi * (2.0 * sh * sh) / sum;  // (1 - cos alpha = 2 sin^2(alpha / 2))
    double T[3];
    sky_sun_transmittance(p, sky->lightSteps, T);
    const double sa = std::sin(alpha);
    for (int ch = 0; ch < 3; ch++) d.add[ch] = (float)((double)sky->sunIrradiance[ch] * T[ch] / (kPi * sa * sa) * k);
    return NXHIP_OK;
}

// the map on the stream: texels = width x height float4 (w = 0); disc: nullptr for none
int sky_generate(hipStream_t st, const SkyPlan& p, const SkyDisc* disc, float4* texels, uint32_t width, uint32_t height)
{
    const uint32_t n = width * height;
    sky_map_kernel<<<(n + kSkyBlock - 1) / kSkyBlock, kSkyBlock, 0, st>>>(texels, width, height, p.launch);
    NX_HIP(hipGetLastError());
    if (disc) {
        const uint32_t m = disc->w * disc->h;
        sky_disc_kernel<<<(m + kSkyBlock - 1) / kSkyBlock, kSkyBlock, 0, st>>>(texels, width, height, *disc);
        NX_HIP(hipGetLastError());
    }
    return NXHIP_OK;
}

const void* sky_hook_kernel_ptr() { return (const void*)sky_hook_kernel; }

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_sky() { return layout_stamp(); }

}  // namespace nxd
