// nx_lights.hip — light sampling by emitted power (nxhip_set_light_sampling): the table of every emissive triangle of every mesh
// light, built on the device and rebuilt there when instances move or meshes deform.
//
// No counterpart in the reference, whose light sample takes one light uniformly and one of its triangles uniformly
// (PathTracer.cu:213-308: a candle as often as a ceiling panel, the smallest triangles of a tessellated emitter as often as the
// largest).  Here entry i — ordered by light, then by triangle — has the weight w = world-space area x luminance of what the
// light's material emits, and is picked with probability P(i) = cdf[i] - cdf[i - 1]:
//   light_map_mean_kernel   mean of an emissive map's sRGB-decoded texels (once per uploaded map): the (r, g, b) of a textured light
//   light_weight_kernel     one thread per entry: w in binary64 from the binary32 area the shading code computes (tri_area of the
//                           transformed corners, the instance's current matrix) and the light's luminance; the entry's light
//   (scan)                  inclusive prefix sums of w in binary64, rocPRIM's run-to-run deterministic scan: two contexts with the
//                           same scene hold the same table bit for bit
//   light_normalise_kernel  cdf[i] = binary32(prefix[i] / total), the last entry exactly 1; a total of 0 (or none that is finite)
//                           clears the header's `valid`
//   light_guide_kernel      thread k: the first entry whose cdf exceeds k / G (cut-point method; G = the power of two >= entries)
//   light_pick_kernel       the test hook's pick (nxhip_light_pick_batch): nx_lights.h light_pick on an array of u
// Nothing comes back to the host during a build.
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "nx_host.h"
#include "nx_lights.h"

namespace nxd {

namespace {

constexpr int kLightBlock = 256;
constexpr int kMeanBlock = 1024;

// One workgroup per map, a fixed order of additions: the same mean on every run.
__global__ void __launch_bounds__(kMeanBlock) light_map_mean_kernel(const TextureDev t, const float* __restrict__ srgbLut, float* __restrict__ mean4)
{
    __shared__ double sSum[3][kMeanBlock];
    const size_t texels = (size_t)t.width * t.height;
    double s[3] = {0.0, 0.0, 0.0};
    for (size_t i = threadIdx.x; i < texels; i += kMeanBlock) {
        const uint32_t p = t.texels[i];  // (alpha ignored)
        s[0] += (double)srgbLut[p & 0xffu];
        s[1] += (double)srgbLut[(p >> 8) & 0xffu];
        s[2] += (double)srgbLut[(p >> 16) & 0xffu];
    }
    for (int c = 0; c < 3; c++) sSum[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int step = kMeanBlock / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step)
            for (int c = 0; c < 3; c++) sSum[c][threadIdx.x] += sSum[c][threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x < 3) mean4[threadIdx.x] = texels ? (float)(sSum[threadIdx.x][0] / (double)texels) : 0.0f;
    if (threadIdx.x == 3) mean4[3] = 0.0f;
}

__global__ void __launch_bounds__(kLightBlock) light_weight_kernel(const LightBuild b)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.entries) return;
    // the light of entry i: the last one whose first entry is not behind i (lights without triangles share their successor's base)
    uint32_t lo = 0, hi = b.lightCount;  // lightBase[lo] <= i < lightBase[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) / 2u;
        if (b.lightBase[mid] <= i) lo = mid;
        else hi = mid;
    }
    const uint32_t tri = i - b.lightBase[lo];
    const ShadeInst* inst = &b.shadeInst[b.lights[lo].mesh.meshId];
    const nx_triangle* t = shade_tri(inst->tris, tri);
    const float* T = inst->transform;
    // the very expression of the light sample's density (nx_wavefront.hip next_event_estimation)
    const float area = tri_area(mat_point(T, ld3(t->pos0)), mat_point(T, ld3(t->pos1)), mat_point(T, ld3(t->pos2)));
    const nx_material* m = &inst->material;
    f3 e = ld3(m->emissive);
    if (m->emissiveMapId != -1) e = ld3(b.mapMean + 4 * (size_t)m->emissiveMapId);
    const float Y = m->intensity * ((0.2126f * e.x + 0.7152f * e.y) + 0.0722f * e.z);  // (the coefficients of adaptive sampling)
    double w = (double)area * (double)Y;
    if (!(w > 0.0) || !isfinite(w)) w = 0.0;  // negative or not finite: never picked
    b.weight[i] = w;
    b.table[i].light = lo;
}

__global__ void __launch_bounds__(kLightBlock) light_normalise_kernel(const LightBuild b)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.entries) return;
    const double total = b.prefix[b.entries - 1u];
    const bool valid = total > 0.0 && isfinite(total);
    if (i == 0u) {
        b.header->valid = valid ? 1u : 0u;
        b.header->pad_ = 0u;
        b.header->total = total;
    }
    // (an invalid table is all ones: whoever walks it all the same stops at once)
    b.table[i].cdf = (valid && i + 1u != b.entries) ? (float)(b.prefix[i] / total) : 1.0f;
}

__global__ void __launch_bounds__(kLightBlock) light_guide_kernel(const LightBuild b)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= b.guideSize) return;
    const float x = (float)k / (float)b.guideSize;  // exact: k < guideSize <= 2^23, a power of two
    uint32_t lo = 0, hi = b.entries - 1u;           // the answer is in [lo, hi]: cdf[entries - 1] = 1 > x
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (b.table[mid].cdf > x) hi = mid;
        else lo = mid + 1u;
    }
    b.guide[k] = lo;
}

__global__ void __launch_bounds__(kLightBlock) light_pick_kernel(const LightEntry* __restrict__ table, const uint32_t* __restrict__ guide, const uint32_t guideSize,
                                                                  const uint32_t entries, const float* __restrict__ u, const uint32_t count,
                                                                  uint32_t* __restrict__ entry, float* __restrict__ prob)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const LightPick p = light_pick(table, guide, guideSize, entries, u[k]);
        entry[k] = p.entry;
        prob[k] = p.prob;
    }
}

unsigned blocks_for(uint32_t n) { return (n + (uint32_t)kLightBlock - 1u) / (uint32_t)kLightBlock; }

}  // namespace

int light_scan_bytes(size_t entries, size_t* bytes)
{
    *bytes = 0;
    NX_HIP(rocprim::deterministic_inclusive_scan(nullptr, *bytes, (double*)nullptr, (double*)nullptr, entries, rocprim::plus<double>(), nullptr));
    return NXHIP_OK;
}

int light_map_mean(hipStream_t st, const TextureDev& t, const float* srgbLut, float* mean4)
{
    light_map_mean_kernel<<<1, kMeanBlock, 0, st>>>(t, srgbLut, mean4);
    NX_HIP(hipGetLastError());
    return NXHIP_OK;
}

// weights -> prefix sums -> cdf -> guide, in stream order (b.entries >= 1)
int light_table_build(hipStream_t st, const LightBuild& b, void* scanTemp, size_t scanBytes)
{
    light_weight_kernel<<<blocks_for(b.entries), kLightBlock, 0, st>>>(b);
    NX_HIP(hipGetLastError());
    NX_HIP(rocprim::deterministic_inclusive_scan(scanTemp, scanBytes, b.weight, b.prefix, (size_t)b.entries, rocprim::plus<double>(), st));
    light_normalise_kernel<<<blocks_for(b.entries), kLightBlock, 0, st>>>(b);
    NX_HIP(hipGetLastError());
    light_guide_kernel<<<blocks_for(b.guideSize), kLightBlock, 0, st>>>(b);
    NX_HIP(hipGetLastError());
    return NXHIP_OK;
}

const void* light_pick_kernel_ptr() { return (const void*)light_pick_kernel; }

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_lights() { return layout_stamp(); }

}  // namespace nxd
