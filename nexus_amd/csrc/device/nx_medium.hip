// nx_medium.hip — fog: one homogeneous participating medium in a world-space box (nxhip_set_medium; the rule: include/nexus_hip.h).
//
// Two streaming kernels beside the existing ones, in the pass graphs only while a medium with sigmaT > 0 is set (kFlavorMedium):
//   medium_scatter_kernel  between the closest-hit level of bounce b - 1 and the material launch of bounce b: reads every record of the trace
//                          queue, decides by the free-flight draw whether the path scatters in front of its hit (or on its way out of the
//                          scene), and where it does takes the record away from the material launch (code kHitCodeMedium) and produces
//                          the vertex's light sample and continuation ray itself, into the queues the material launch appends to;
//   medium_shadow_kernel   between the material launch of bounce b and its any-hit launch: multiplies the radiance of every shadow request
//                          that crosses the box by the transmittance of the crossing.
// No material kernel changes: this unit includes their shared text (nx_wavefront.h) for its device functions and instantiates none of its
// kernels — the light sample is next_event_estimation itself, with the phase function as its "BSDF", the slots come from SlotAllocator.
// A unit of its own: contexts without a medium launch nothing of it, and it compiles beside the material families, not behind them.
// Also here: the two test hooks' kernels over the device functions this unit defines.
//
// The density grid (nxhip_set_medium_density; the rule: include/nexus_hip.h): extinction sigmaT x rho(p), rho a trilinear lookup in a voxel
// grid over the box.  Both kernels have a GRID instance beside the homogeneous one (medium_scatter_kernel<GRID = true, ..>, and the sibling
// medium_shadow_grid_kernel; in the pass graphs under kFlavorMediumGrid): a per-lane 3-D DDA over bricks of 8 x 8 x 8 voxels with a majorant
// each — delta tracking for the free flight, ratio tracking for the shadow requests.  The homogeneous instances keep their code, instruction
// for instruction (profiles/medium_grid.txt).  medium_brick_kernel builds the majorants on the device; three hooks (lookup, walk, majorants)
// for the tests.
#define NX_KERNEL_TU 1
#include "nx_wavefront.h"

namespace nxd {

// ------------------------------------------------------------------------------------------------------
// the segment of a ray inside the box, the free flight, the phase function

constexpr float kInfF = __builtin_huge_valf();
// The medium's stage of the pixel-keyed stream.  rng_init_keyed mixes bounce * 2 + stage + 1 into the key, which tells stages 0 and 1 of all
// bounces apart and nothing else: stage 2 of bounce b would BE stage 0 of bounce b + 1 — the free flight's number would come back as the
// roulette's number of the continuation ray (measured: MIS and naive estimates 6 % apart).  256 is past every value the other stages can
// form (bounces stay below NX_PATH_MAX_LENGTH = 100), so the medium's numbers come from a stream nobody else reads.
constexpr uint32_t kMediumStage = 256u;
// ... and the shadow requests' ratio tracking under a density grid draws from the stage after it (a path has at most one request per bounce)
constexpr uint32_t kMediumShadowStage = 257u;
static_assert(kMediumStage > 2u * NX_PATH_MAX_LENGTH + 2u && kMediumShadowStage > 2u * NX_PATH_MAX_LENGTH + 2u && kMediumShadowStage != kMediumStage,
              "the medium's stages may not collide with a roulette or material stage of any bounce, nor with each other");
constexpr float kInv4Pi = 0.0795774715f;

// one axis of the slab test: narrows [lo, hi]; an axis the ray runs along contributes (-inf, +inf) inside the slab, nothing outside it
NXD void medium_axis(const float bmin, const float bmax, const float o, const float d, float& lo, float& hi, bool& empty)
{
    const float a = (bmin - o) / d, b = (bmax - o) / d;
    const bool along = d == 0.0f;
    lo = along ? lo : fmaxf(lo, fminf(a, b));
    hi = along ? hi : fminf(hi, fmaxf(a, b));
    empty = empty || (along && !(bmin <= o && o <= bmax));
}

// t0 and L = t1 - t0 of the rule; L = -1 (and t0 = 0) for an empty segment
struct MediumSeg { float t0, L; };
NXD MediumSeg medium_segment(const nx_medium& m, const f3 o, const f3 d, const float tEnd)
{
    float lo = 0.0f, hi = tEnd;
    bool empty = false;
    medium_axis(m.boxMin[0], m.boxMax[0], o.x, d.x, lo, hi, empty);
    medium_axis(m.boxMin[1], m.boxMax[1], o.y, d.y, lo, hi, empty);
    medium_axis(m.boxMin[2], m.boxMax[2], o.z, d.z, lo, hi, empty);
    return empty ? MediumSeg{0.0f, -1.0f} : MediumSeg{lo, hi - lo};
}

NXD float medium_flight(const float sigmaT, const float xi) { return -nxf_logf(1.0f - xi) / sigmaT; }
NXD float medium_transmittance(const float sigmaT, const float L) { return nxf_expf(-sigmaT * L); }

// Henyey-Greenstein: p(c), c = cosine between the direction of travel and the scattered direction
NXD float phase_pdf(const float g, const float g2, const float oneMinusG2, const float c)
{
    const float t = (1.0f + g2) - (2.0f * g) * c;
    return (oneMinusG2 * kInv4Pi) / (t * sqrtf(t));
}

// the continuation's direction about d from (xi1, xi2), and its pdf
NXD f3 phase_sample(const float g, const float g2, const float oneMinusG2, const f3 d, const float xi1, const float xi2, float& pdf)
{
    float c;
    if (fabsf(g) < 1.0e-3f) c = 1.0f - 2.0f * xi1;
    else {
        const float q = oneMinusG2 / ((1.0f - g) + (2.0f * g) * xi1);
        c = ((1.0f + g2) - q * q) / (2.0f * g);
        c = fminf(fmaxf(c, -1.0f), 1.0f);
    }
    const float sinT = sqrtf(fmaxf(0.0f, 1.0f - c * c));
    const float phi = 6.28318531f * xi2;
    // an orthonormal frame about d without a branch (Duff et al. 2017: nx_alights.h)
    const float sg = copysignf(1.0f, d.z);
    const float k = -1.0f / (sg + d.z);
    const float b = d.x * d.y * k;
    const f3 t0 = mk3(1.0f + sg * d.x * d.x * k, sg * b, -sg * d.x), t1 = mk3(b, sg + d.y * d.y * k, -d.y);
    const f3 w = normalize3((t0 * (nxf_cosf(phi) * sinT) + t1 * (nxf_sinf(phi) * sinT)) + d * c);
    pdf = phase_pdf(g, g2, oneMinusG2, c);
    return w;
}

// The phase function as next_event_estimation's "BSDF": the function is handed the normal (0, 0, 1), whose frame rotation is the identity, so
// `wo` IS the sampled world direction; the direction of travel and the medium's constants ride in the parameter block (cIor: d; roughness: g;
// ior: g * g; cK.x: 1 - g * g).  Value and pdf are both p(c): no cosine, and phase / pdf = 1 for the continuation.
constexpr int kMatPhase = 8;
template <> struct Bsdf<kMatPhase> {
    static NXD bool eval(const MatParams& m, f3, f3 wo, f3& thr, float& pdf)
    {
        pdf = phase_pdf(m.roughness, m.ior, m.cK.x, dot3(m.cIor, wo));
        thr = mk3(pdf);
        return true;
    }
};

// ------------------------------------------------------------------------------------------------------
// the density grid: lookup, majorant bricks, the walk

constexpr int kBrick = 8;             // voxels per brick edge
constexpr int kGridWalkBound = 4096;  // iterations of one walk, brick steps and tentative collisions together (render_pass keeps it out of reach)

// one axis of the lookup: the two voxel indices, clamped to the edge, and the weight of the second
NXD void grid_axis(const float p, const float bmin, const float vscale, const uint32_t n, int& i0, int& i1, float& f)
{
    const float g = (p - bmin) * vscale - 0.5f;
    const float fl = floorf(g);
    f = g - fl;
    const float top = (float)(n - 1u);
    // (clamped as floats: a point far outside the box, or one that is no number, may not reach the conversion)
    i0 = (int)fminf(fmaxf(fl, 0.0f), top);
    i1 = (int)fminf(fmaxf(fl + 1.0f, 0.0f), top);
}

NXD float grid_lerp(const float a, const float b, const float f) { return a + f * (b - a); }

// rho(p): three nested lerps, x, then y, then z
NXD float grid_density(const DeviceState* S, const f3 p)
{
    const nx_medium& med = S->medium;
    const uint32_t nx = S->mediumN[0], ny = S->mediumN[1], nz = S->mediumN[2];
    int x0, x1, y0, y1, z0, z1;
    float fx, fy, fz;
    grid_axis(p.x, med.boxMin[0], S->mediumVscale[0], nx, x0, x1, fx);
    grid_axis(p.y, med.boxMin[1], S->mediumVscale[1], ny, y0, y1, fy);
    grid_axis(p.z, med.boxMin[2], S->mediumVscale[2], nz, z0, z1, fz);
    const NX_G float* rho = S->mediumRho;
    const size_t r00 = ((size_t)z0 * ny + (size_t)y0) * nx, r10 = ((size_t)z0 * ny + (size_t)y1) * nx;
    const size_t r01 = ((size_t)z1 * ny + (size_t)y0) * nx, r11 = ((size_t)z1 * ny + (size_t)y1) * nx;
    const float c00 = grid_lerp(rho[r00 + x0], rho[r00 + x1], fx), c10 = grid_lerp(rho[r10 + x0], rho[r10 + x1], fx);
    const float c01 = grid_lerp(rho[r01 + x0], rho[r01 + x1], fx), c11 = grid_lerp(rho[r11 + x0], rho[r11 + x1], fx);
    return grid_lerp(grid_lerp(c00, c10, fy), grid_lerp(c01, c11, fy), fz);
}

// the brick of a point in brick space, clamped to the grid (as floats first: see grid_axis)
NXD int grid_brick_of(const float u, const uint32_t nb) { return (int)fminf(fmaxf(floorf(u), 0.0f), (float)(nb - 1u)); }

// tNext of one axis, from the integer brick index: never accumulated
NXD float grid_next(const int b, const bool forward, const float bscale, const float bmin, const float o, const float d)
{
    return d == 0.0f ? kInfF : ((((float)(b + (forward ? 1 : 0))) / bscale + bmin) - o) / d;
}

// The walk over [t0, t1] of the ray (o, d), by the rule of nexus_hip.h.  RATIO = false: delta tracking — returns 1 with tOut = the parameter
// of a real collision, 0 if the segment is passed without one.  RATIO = true: ratio tracking — T is multiplied at every tentative
// collision, the return value is 0.  Either: 2 at the iteration bound.  `iters` counts iterations, `colls` the tentative collisions among
// them.  All state is scalars: the axis is chosen by selects, no array is indexed by a lane's value.
template <bool RATIO>
NXD int grid_walk(const DeviceState* S, const f3 o, const f3 d, const float t0, const float t1, uint32_t& rng, float& tOut, float& T, uint32_t& iters, uint32_t& colls)
{
    const float sigmaT = S->medium.sigmaT;
    const float minX = S->medium.boxMin[0], minY = S->medium.boxMin[1], minZ = S->medium.boxMin[2];
    const float bsX = S->mediumBscale[0], bsY = S->mediumBscale[1], bsZ = S->mediumBscale[2];
    const int nbX = (int)S->mediumNb[0], nbY = (int)S->mediumNb[1], nbZ = (int)S->mediumNb[2];
    const NX_G float* bricks = S->mediumBricks;
    const f3 p0 = o + d * t0;
    int bx = grid_brick_of((p0.x - minX) * bsX, (uint32_t)nbX), by = grid_brick_of((p0.y - minY) * bsY, (uint32_t)nbY), bz = grid_brick_of((p0.z - minZ) * bsZ, (uint32_t)nbZ);
    const bool fwX = d.x > 0.0f, fwY = d.y > 0.0f, fwZ = d.z > 0.0f;
    float tnX = grid_next(bx, fwX, bsX, minX, o.x, d.x), tnY = grid_next(by, fwY, bsY, minY, o.y, d.y), tnZ = grid_next(bz, fwZ, bsZ, minZ, o.z, d.z);
    float t = t0;
    float tau = -nxf_logf(1.0f - rng_next(rng));
    iters = 0u;
    colls = 0u;
    for (int it = 0; it < kGridWalkBound; it++) {
        iters++;
        const int ax = tnX <= tnY ? (tnX <= tnZ ? 0 : 2) : (tnY <= tnZ ? 1 : 2);
        const float tn = ax == 0 ? tnX : (ax == 1 ? tnY : tnZ);
        const float tExit = fminf(tn, t1);
        const float M = bricks[((size_t)bz * (size_t)nbY + (size_t)by) * (size_t)nbX + (size_t)bx];
        const float mu = sigmaT * M;
        const float depth = mu * (tExit - t);
        if (tau < depth) {
            t += tau / mu;
            const float r = grid_density(S, o + d * t);
            colls++;
            if (RATIO) {
                T *= fmaxf(0.0f, 1.0f - r / M);
                if (T == 0.0f) return 0;
            } else {
                const float zeta = rng_next(rng);
                if (zeta * M < r) {
                    tOut = t;
                    return 1;
                }
            }
            tau = -nxf_logf(1.0f - rng_next(rng));
        } else {
            tau -= fmaxf(depth, 0.0f);
            if (!(tn < t1)) return 0;
            t = tExit;
            if (ax == 0) {
                bx += fwX ? 1 : -1;
                if (bx < 0 || bx >= nbX) return 0;
                tnX = grid_next(bx, fwX, bsX, minX, o.x, d.x);
            } else if (ax == 1) {
                by += fwY ? 1 : -1;
                if (by < 0 || by >= nbY) return 0;
                tnY = grid_next(by, fwY, bsY, minY, o.y, d.y);
            } else {
                bz += fwZ ? 1 : -1;
                if (bz < 0 || bz >= nbZ) return 0;
                tnZ = grid_next(bz, fwZ, bsZ, minZ, o.z, d.z);
            }
        }
    }
    if (RATIO) T = 0.0f;
    return 2;
}

// medium_brick_kernel: M[b] = the maximum of rho over the voxels [8 b_i - 1, 8 b_i + 8] per axis, clamped to the grid — one lane per brick,
// at most 10^3 reads each, every index clamped before it is formed.  Runs once per nxhip_set_medium_density, on the context's stream.
__global__ void __launch_bounds__(kWideBlock) medium_brick_kernel(const float* __restrict__ rho, const uint32_t nx, const uint32_t ny, const uint32_t nz, const uint32_t nbx,
                                                                   const uint32_t nby, const uint32_t nbz, float* __restrict__ bricks)
{
    const uint32_t total = nbx * nby * nbz;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < total; k += gridDim.x * blockDim.x) {
        const uint32_t bx = k % nbx, by = (k / nbx) % nby, bz = k / (nbx * nby);
        const uint32_t x0 = bx ? bx * kBrick - 1u : 0u, x1 = min(bx * kBrick + kBrick, nx - 1u);
        const uint32_t y0 = by ? by * kBrick - 1u : 0u, y1 = min(by * kBrick + kBrick, ny - 1u);
        const uint32_t z0 = bz ? bz * kBrick - 1u : 0u, z1 = min(bz * kBrick + kBrick, nz - 1u);
        float m = 0.0f;  // (the voxels are >= 0: nxhip_set_medium_density)
        for (uint32_t z = z0; z <= z1; z++)
            for (uint32_t y = y0; y <= y1; y++) {
                const size_t row = ((size_t)z * ny + y) * nx;
                for (uint32_t x = x0; x <= x1; x++) m = fmaxf(m, rho[row + x]);
            }
        bricks[k] = m;
    }
}

// ------------------------------------------------------------------------------------------------------
// medium_scatter_kernel
//
// Workgroup w serves region w % 8 of the trace queue of bounce - 1 (as the material launch does) in tiles of 256 consecutive slots — every
// queue array is read at the ray's own slot, coalesced — and appends to the same region of bounce `bounce`'s queues through the racing
// SlotAllocator: a ray yields at most one shadow request and one continuation ray, and the material launch produces none for a record this
// kernel took, so a region holds no more than it could without a medium.  The code word is read first: records nobody shades (0), and
// every ray that does not cross the box, cost 4 + 32 bytes and leave.  No LDS beyond the allocator's, no spin, no wait; the tile loop is
// bounded by the region's size.
// GRID = false is the homogeneous kernel as it always was; GRID = true (kFlavorMediumGrid) finds the collision by the walk: lanes of a wave
// walk different numbers of bricks, so a tile costs what its longest walk costs.
// METAL (a context with an NX_MAT_METALROUGH material: kFlavorMetal): the fifth material type's code is a hit like the other four's; the
// instances with METAL = false are the code of a context without such a material.
template <bool GRID, unsigned F>  // (F: POWER, ANALYTIC — next_event_estimation — and METAL)
__global__ void __launch_bounds__(kShadeBlock) medium_scatter_kernel(const DeviceState* __restrict__ S, const int bounceArg)
{
    constexpr bool ANALYTIC = (F & kMfAnalytic) != 0u, METAL = (F & kMfMetal) != 0u;
    static_assert(medium_set_ok(F), "medium_scatter_kernel reads POWER, TREE, ANALYTIC and METAL alone (nx_variants.h)");
    const int bounce = bounceArg & 0xff;
    const bool dropEnded = (bounceArg & kShadeDropEnded) != 0;
    const int region = (int)(blockIdx.x & (kQueueShards - 1));
    const int rank = (int)(blockIdx.x >> 3), ranks = max(1, (int)(gridDim.x >> 3));
    Counters* C = S->counters;
    const int inRegion = C->region[region].traceSize[bounce - 1];
    if (rank * kShadeBlock >= inRegion) return;  // no tile for this workgroup: it leaves before any barrier
    const uint32_t frame = S->frame->frameNumber;
    const int regionBase = region * (int)S->queueShardCap;
    const TraceRays in = S->trace.rays[(bounce - 1) & 1], out = S->trace.rays[bounce & 1];
    const nx_medium& med = S->medium;  // (read where it is used: a copy held across the light sample spills scalar registers)
    const bool lastBounce = bounce == (int)S->settings.pathLength;
    const bool lightSample = ANALYTIC || S->settings.useMIS != 0;
    SlotAllocator<false, 2> slots;  // 0: shadow requests, 1: continuation rays
    static_assert(offsetof(RegionCounters, traceSize) + kMaxBounceSlots * sizeof(int32_t) == offsetof(RegionCounters, traceShadowSize), "traceShadowSize follows traceSize");
    slots.init(S, &C->region[0].traceShadowSize[bounce], -kMaxBounceSlots, 0, bounce, inRegion);
    int ended = 0;  // continuation rays of this wave that were not queued (dropEnded; uniform over the wave)
    for (int tile = rank * kShadeBlock; tile < inRegion; tile += ranks * kShadeBlock) {
        const int r = tile + (int)threadIdx.x;
        const int at = regionBase + r;
        bool wantShadow = false, wantTrace = false, survives = true;
        ShadowPayload sh;
        sh.origin = mk3(0.0f); sh.direction = mk3(0.0f); sh.radiance = mk3(0.0f); sh.distance = 0.0f;
        f3 x = mk3(0.0f), nextDir = mk3(0.0f), beta = mk3(0.0f);
        float nextPdf = 0.0f;
        uint32_t pixelIdx = 0;
        uint32_t word = 0u;
        if (r < inRegion) word = S->trace.hitInst[at];
        const uint32_t code = word >> kHitCodeShift;
        if (code != 0u && code != kHitCodeMedium && (code <= 4u || (METAL && code == kHitCodeMetalRough) || code == kHitCodeMiss)) {
            const float4 ro = in.rayO[at], rd = in.rayD[at];
            const f3 o = mk3(ro.x, ro.y, ro.z), d = mk3(rd.x, rd.y, rd.z);
            pixelIdx = __float_as_uint(rd.w);
            const float tEnd = code == kHitCodeMiss ? kInfF : S->trace.hit[at].x;
            const MediumSeg seg = medium_segment(med, o, d, tEnd);
            if (seg.L > 0.0f) {
                uint32_t rng = seed_for(S, (uint32_t)at, pixelIdx, (uint32_t)bounce, kMediumStage, frame);
                float tScatter = 0.0f;
                int event;  // 0: the segment is passed, 1: the path scatters at tScatter, 2: the walk's bound — the path ends, absorbed
                if (GRID) {
                    float T = 1.0f;
                    uint32_t iters, colls;
                    event = grid_walk<false>(S, o, d, seg.t0, seg.t0 + seg.L, rng, tScatter, T, iters, colls);
                } else {
                    const float s = medium_flight(med.sigmaT, rng_next(rng));
                    event = s < seg.L ? 1 : 0;
                    tScatter = seg.t0 + s;
                }
                if (event != 0) {
                    // the path scatters at x: the record leaves the material launch's reach
                    S->trace.hitInst[at] = (word & kHitInstMask) | (kHitCodeMedium << kHitCodeShift);
                    if (event == 1 && (__float_as_uint(ro.w) & kRaySurvives) != 0u && !lastBounce) {
                        x = o + d * tScatter;
                        beta = mk3(1.0f);
                        if (bounce != 1) {
                            const float4 tp = in.tp[at];
                            const f3 throughput = mk3(tp.x, tp.y, tp.z);
                            beta = throughput / maxcomp3(throughput);
                        }
                        beta = beta * ld3(med.albedo);
                        const float g = med.g, g2 = S->mediumG2, oneMinusG2 = S->mediumOneMinusG2;
                        if (lightSample) {
                            MatParams mp;
                            mp.albedo = mk3(0.0f);
                            mp.roughness = g;
                            mp.ior = g2;
                            mp.cIor = d;
                            mp.cK = mk3(oneMinusG2, 0.0f, 0.0f);
                            wantShadow = next_event_estimation<kMatPhase, F>(S, mk3(0.0f, 0.0f, 1.0f), mp, x, mk3(0.0f, 0.0f, 1.0f), mk3(0.0f), beta, rng, sh);
                        }
                        const float xi1 = rng_next(rng), xi2 = rng_next(rng);
                        nextDir = phase_sample(g, g2, oneMinusG2, d, xi1, xi2, nextPdf);
                        wantTrace = true;
                        // the next logic step's Russian roulette, drawn by the producer as the material launch draws it (pixel-keyed numbers:
                        // the draw needs no slot); dropEnded: a ray that lost it is counted, not queued
                        uint32_t roulette = seed_for(S, 0u, pixelIdx, (uint32_t)bounce + 1u, 0u, frame);
                        survives = rng_next(roulette) < maxcomp3(beta);
                    }
                }
            }
        }
        if (dropEnded) {
            ended += __popcll(__ballot(wantTrace && !survives));
            wantTrace = wantTrace && survives;
        }
        const bool want[2] = {wantShadow, wantTrace};
        int slot[2];
        slots.alloc(want, slot, 0, region);
        const int shadowSlot = regionBase + slot[0], traceSlot = regionBase + slot[1];
        if (wantShadow) {
            S->shadow.rayO[shadowSlot] = make_float4(sh.origin.x, sh.origin.y, sh.origin.z, sh.distance);
            S->shadow.rayD[shadowSlot] = make_float4(sh.direction.x, sh.direction.y, sh.direction.z, __uint_as_float(pixelIdx));
            S->shadow.radiance[shadowSlot] = make_float4(sh.radiance.x, sh.radiance.y, sh.radiance.z, 0.0f);
        }
        if (wantTrace) {
            // w: kRayPassThrough clear — x becomes the path's previous vertex (keep_previous_vertex)
            out.rayO[traceSlot] = make_float4(x.x, x.y, x.z, __uint_as_float(survives ? kRaySurvives : 0u));
            out.rayD[traceSlot] = make_float4(nextDir.x, nextDir.y, nextDir.z, __uint_as_float(pixelIdx));
            out.tp[traceSlot] = make_float4(beta.x, beta.y, beta.z, nextPdf);
        }
    }
    // the continuation rays this wave did not queue (the reference queues them: nxhip_read_queue_sizes adds them back)
    if (dropEnded && ended && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(&C->region[region].endedSize[bounce], ended);
}

// ------------------------------------------------------------------------------------------------------
// medium_shadow_kernel: the shadow queue of a bounce, every request at its own slot (32 B read; 16 B read and written where the box is crossed)

__global__ void __launch_bounds__(kWideBlock) medium_shadow_kernel(const DeviceState* __restrict__ S, const int bounce)
{
    const QueueView in = queue_view(&S->counters->region[0].traceShadowSize[bounce], S->queueShardCap);
    const nx_medium med = S->medium;
    for (int index = (int)(blockIdx.x * blockDim.x + threadIdx.x); index < in.total; index += (int)(gridDim.x * blockDim.x)) {
        const int at = in.slot(index);
        const float4 ro = S->shadow.rayO[at], rd = S->shadow.rayD[at];
        const MediumSeg seg = medium_segment(med, mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z), ro.w);
        if (seg.L > 0.0f) {
            const float T = medium_transmittance(med.sigmaT, seg.L);
            float4 r = S->shadow.radiance[at];
            r.x *= T; r.y *= T; r.z *= T;
            S->shadow.radiance[at] = r;
        }
    }
}

// the GRID instance: ratio tracking along the crossing, from a stream of the request's own (stage 257); a request that meets no tentative
// collision — no brick with M > 0 on its way, or tau outlasting them — keeps its bits.  The medium is read from the state block where it is
// used (a held copy beside the walk's state spills scalar registers: profiles/medium.txt section 1).
__global__ void __launch_bounds__(kWideBlock) medium_shadow_grid_kernel(const DeviceState* __restrict__ S, const int bounce)
{
    const QueueView in = queue_view(&S->counters->region[0].traceShadowSize[bounce], S->queueShardCap);
    const uint32_t frame = S->frame->frameNumber;
    for (int index = (int)(blockIdx.x * blockDim.x + threadIdx.x); index < in.total; index += (int)(gridDim.x * blockDim.x)) {
        const int at = in.slot(index);
        const float4 ro = S->shadow.rayO[at], rd = S->shadow.rayD[at];
        const f3 o = mk3(ro.x, ro.y, ro.z), d = mk3(rd.x, rd.y, rd.z);
        const MediumSeg seg = medium_segment(S->medium, o, d, ro.w);
        if (seg.L > 0.0f) {
            uint32_t rng = seed_for(S, (uint32_t)at, __float_as_uint(rd.w), (uint32_t)bounce, kMediumShadowStage, frame);
            float T = 1.0f, tUnused;
            uint32_t iters, colls;
            const int event = grid_walk<true>(S, o, d, seg.t0, seg.t0 + seg.L, rng, tUnused, T, iters, colls);
            if (colls != 0u || event == 2) {
                float4 r = S->shadow.radiance[at];
                r.x *= T; r.y *= T; r.z *= T;
                S->shadow.radiance[at] = r;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// Test hooks: the functions above on plain arrays (nxhip_medium_segment_batch, nxhip_medium_phase_batch)

__global__ void __launch_bounds__(kWideBlock) medium_segment_hook_kernel(const DeviceState* __restrict__ S, const float* __restrict__ origin, const float* __restrict__ dir,
                                                                          const float* __restrict__ tEnd, const float* __restrict__ xi, const uint32_t count,
                                                                          float* __restrict__ t0, float* __restrict__ length, float* __restrict__ transmittance,
                                                                          float* __restrict__ scatterT)
{
    const nx_medium med = S->medium;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const MediumSeg seg = medium_segment(med, mk3(origin[3 * k], origin[3 * k + 1], origin[3 * k + 2]), mk3(dir[3 * k], dir[3 * k + 1], dir[3 * k + 2]), tEnd[k]);
        const bool crosses = seg.L > 0.0f;
        const float s = medium_flight(med.sigmaT, xi[k]);
        t0[k] = crosses ? seg.t0 : 0.0f;
        length[k] = crosses ? seg.L : 0.0f;
        transmittance[k] = crosses ? medium_transmittance(med.sigmaT, seg.L) : 1.0f;
        scatterT[k] = (crosses && s < seg.L) ? seg.t0 + s : -1.0f;
    }
}

__global__ void __launch_bounds__(kWideBlock) medium_phase_hook_kernel(const DeviceState* __restrict__ S, const float* __restrict__ dirIn, const float* __restrict__ xi1,
                                                                        const float* __restrict__ xi2, const uint32_t count, float* __restrict__ dirOut, float* __restrict__ pdf)
{
    const float g = S->medium.g, g2 = S->mediumG2, oneMinusG2 = S->mediumOneMinusG2;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        float p;
        const f3 w = phase_sample(g, g2, oneMinusG2, mk3(dirIn[3 * k], dirIn[3 * k + 1], dirIn[3 * k + 2]), xi1[k], xi2[k], p);
        dirOut[3 * k] = w.x; dirOut[3 * k + 1] = w.y; dirOut[3 * k + 2] = w.z;
        pdf[k] = p;
    }
}

// The grid's hooks (nxhip_medium_density_batch, nxhip_medium_track_batch): the lookup with the majorant of the point's brick, and the walk
// in both modes from the caller's stream state — each mode starts from its own copy of seed[k].  steps2[2k] is the free flight's walk,
// steps2[2k + 1] the ratio tracking's: iterations | tentative collisions << 16 (the bound, 4096, fits 16 bits); both 0 where the ray does
// not cross the box.
__global__ void __launch_bounds__(kWideBlock) medium_density_hook_kernel(const DeviceState* __restrict__ S, const float* __restrict__ points, const uint32_t count,
                                                                          float* __restrict__ rho, float* __restrict__ majorant)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const f3 p = mk3(points[3 * k], points[3 * k + 1], points[3 * k + 2]);
        rho[k] = grid_density(S, p);
        const int bx = grid_brick_of((p.x - S->medium.boxMin[0]) * S->mediumBscale[0], S->mediumNb[0]);
        const int by = grid_brick_of((p.y - S->medium.boxMin[1]) * S->mediumBscale[1], S->mediumNb[1]);
        const int bz = grid_brick_of((p.z - S->medium.boxMin[2]) * S->mediumBscale[2], S->mediumNb[2]);
        majorant[k] = S->mediumBricks[((size_t)bz * S->mediumNb[1] + (size_t)by) * S->mediumNb[0] + (size_t)bx];
    }
}

__global__ void __launch_bounds__(kWideBlock) medium_track_hook_kernel(const DeviceState* __restrict__ S, const float* __restrict__ origin, const float* __restrict__ dir,
                                                                        const float* __restrict__ tEnd, const uint32_t* __restrict__ seed, const uint32_t count,
                                                                        float* __restrict__ scatterT, float* __restrict__ transmittance, uint32_t* __restrict__ steps2)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const f3 o = mk3(origin[3 * k], origin[3 * k + 1], origin[3 * k + 2]), d = mk3(dir[3 * k], dir[3 * k + 1], dir[3 * k + 2]);
        const MediumSeg seg = medium_segment(S->medium, o, d, tEnd[k]);
        float st = -1.0f, T = 1.0f;
        uint32_t w0 = 0u, w1 = 0u;
        if (seg.L > 0.0f) {
            uint32_t rng = seed[k], iters, colls;
            float t = 0.0f, unusedT = 1.0f;
            const int event = grid_walk<false>(S, o, d, seg.t0, seg.t0 + seg.L, rng, t, unusedT, iters, colls);
            st = event == 1 ? t : -1.0f;
            w0 = iters | (colls << 16);
            rng = seed[k];
            grid_walk<true>(S, o, d, seg.t0, seg.t0 + seg.L, rng, t, T, iters, colls);
            w1 = iters | (colls << 16);
        }
        scatterT[k] = st;
        transmittance[k] = T;
        steps2[2 * k] = w0;
        steps2[2 * k + 1] = w1;
    }
}

// (POWER and ANALYTIC: next_event_estimation's instances, chosen as the material launch's are — nxhip_render.hip; METAL: the fifth type's hit code)
using MediumSets = Instances<kMfTree | kMfPower | kMfAnalytic | kMfMetal, kMfPower | kMfAnalytic | kMfMetal, kMfAnalytic | kMfMetal, kMfTree | kMfPower | kMfMetal, kMfPower | kMfMetal, kMfMetal,
                             kMfTree | kMfPower | kMfAnalytic, kMfPower | kMfAnalytic, kMfAnalytic, kMfTree | kMfPower, kMfPower, 0u>;
template <bool GRID> const void* medium_scatter_instance(unsigned set)
{
    return MediumSets::find(set, [](auto f) { return (const void*)medium_scatter_kernel<GRID, decltype(f)::value>; });
}
const void* medium_scatter_kernel_of(bool grid, unsigned set) { return grid ? medium_scatter_instance<true>(set) : medium_scatter_instance<false>(set); }
const void* medium_shadow_grid_kernel_ptr() { return (const void*)medium_shadow_grid_kernel; }
const void* medium_brick_kernel_ptr() { return (const void*)medium_brick_kernel; }
const void* medium_density_hook_kernel_ptr() { return (const void*)medium_density_hook_kernel; }
const void* medium_track_hook_kernel_ptr() { return (const void*)medium_track_hook_kernel; }

const void* medium_shadow_kernel_ptr() { return (const void*)medium_shadow_kernel; }
const void* medium_segment_hook_kernel_ptr() { return (const void*)medium_segment_hook_kernel; }
const void* medium_phase_hook_kernel_ptr() { return (const void*)medium_phase_hook_kernel; }

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_medium() { return layout_stamp(); }

}  // namespace nxd
