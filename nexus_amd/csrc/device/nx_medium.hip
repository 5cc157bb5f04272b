// nx_medium.hip — fog: one homogeneous participating medium in a world-space box (nxhip_set_medium; the rule: include/nexus_hip.h).
//
// Two streaming kernels beside the existing ones, in the pass graphs only while a medium with sigmaT > 0 is set (kFlavorMedium):
//   medium_scatter_kernel  between the closest-hit level of bounce b - 1 and the material launch of bounce b: reads every record of the trace
//                          queue, decides by the free-flight draw whether the path scatters in front of its hit (or on its way out of the
//                          scene), and where it does takes the record away from the material launch (code kHitCodeMedium) and produces
//                          the vertex's light sample and continuation ray itself, into the queues the material launch appends to;
//   medium_shadow_kernel   between the material launch of bounce b and its any-hit launch: multiplies the radiance of every shadow request
//                          that crosses the box by the transmittance of the crossing.
// No kernel of nx_wavefront.hip changes: its text is compiled here for the templates and device functions alone (NX_WAVEFRONT_INSTANCES_ONLY,
// as nx_wavefront_detail.hip does) — the light sample is next_event_estimation itself, with the phase function as its "BSDF".
// Also here: the two test hooks' kernels over the same device functions.
#define NX_WAVEFRONT_INSTANCES_ONLY 1
#include "nx_wavefront.hip"

namespace nxd {

// ------------------------------------------------------------------------------------------------------
// the segment of a ray inside the box, the free flight, the phase function

constexpr float kInfF = __builtin_huge_valf();
// The medium's stage of the pixel-keyed stream.  rng_init_keyed mixes bounce * 2 + stage + 1 into the key, which tells stages 0 and 1 of all
// bounces apart and nothing else: stage 2 of bounce b would BE stage 0 of bounce b + 1 — the free flight's number would come back as the
// roulette's number of the continuation ray (measured: MIS and naive estimates 6 % apart).  256 is past every value the other stages can
// form (bounces stay below NX_PATH_MAX_LENGTH = 100), so the medium's numbers come from a stream nobody else reads.
constexpr uint32_t kMediumStage = 256u;
static_assert(kMediumStage > 2u * NX_PATH_MAX_LENGTH + 2u, "the medium's stage may not collide with a roulette or material stage of any bounce");
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
// medium_scatter_kernel
//
// Workgroup w serves region w % 8 of the trace queue of bounce - 1 (as the material launch does) in tiles of 256 consecutive slots — every
// queue array is read at the ray's own slot, coalesced — and appends to the same region of bounce `bounce`'s queues through the racing
// SlotAllocator: a ray yields at most one shadow request and one continuation ray, and the material launch produces none for a record this
// kernel took, so a region holds no more than it could without a medium.  The code word is read first: records nobody shades (0), and
// every ray that does not cross the box, cost 4 + 32 bytes and leave.  No LDS beyond the allocator's, no spin, no wait; the tile loop is
// bounded by the region's size.
template <bool POWER, bool ANALYTIC>
__global__ void __launch_bounds__(kShadeBlock) medium_scatter_kernel(const DeviceState* __restrict__ S, const int bounceArg)
{
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
        if (code != 0u && code != kHitCodeMedium && (code <= 4u || code == kHitCodeMiss)) {
            const float4 ro = in.rayO[at], rd = in.rayD[at];
            const f3 o = mk3(ro.x, ro.y, ro.z), d = mk3(rd.x, rd.y, rd.z);
            pixelIdx = __float_as_uint(rd.w);
            const float tEnd = code == kHitCodeMiss ? kInfF : S->trace.hit[at].x;
            const MediumSeg seg = medium_segment(med, o, d, tEnd);
            if (seg.L > 0.0f) {
                uint32_t rng = seed_for(S, (uint32_t)at, pixelIdx, (uint32_t)bounce, kMediumStage, frame);
                const float s = medium_flight(med.sigmaT, rng_next(rng));
                if (s < seg.L) {
                    // the path scatters at x: the record leaves the material launch's reach
                    S->trace.hitInst[at] = (word & kHitInstMask) | (kHitCodeMedium << kHitCodeShift);
                    if ((__float_as_uint(ro.w) & kRaySurvives) != 0u && !lastBounce) {
                        x = o + d * (seg.t0 + s);
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
                            wantShadow = next_event_estimation<kMatPhase, POWER, false, ANALYTIC>(S, mk3(0.0f, 0.0f, 1.0f), mp, x, mk3(0.0f, 0.0f, 1.0f), mk3(0.0f), beta, rng, sh);
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

// (the light sample's mode and analytic lights: next_event_estimation's instances, chosen as the material launch's are — nxhip_render.hip)
const void* medium_scatter_kernel_ptr(bool lightPower, bool analytic)
{
    if (analytic) return lightPower ? (const void*)medium_scatter_kernel<true, true> : (const void*)medium_scatter_kernel<false, true>;
    return lightPower ? (const void*)medium_scatter_kernel<true, false> : (const void*)medium_scatter_kernel<false, false>;
}
const void* medium_shadow_kernel_ptr() { return (const void*)medium_shadow_kernel; }
const void* medium_segment_hook_kernel_ptr() { return (const void*)medium_segment_hook_kernel; }
const void* medium_phase_hook_kernel_ptr() { return (const void*)medium_phase_hook_kernel; }

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_medium() { return layout_stamp(); }

}  // namespace nxd
