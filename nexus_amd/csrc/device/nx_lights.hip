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
// Behind the table, with nxhip_set_light_importance(NXHIP_LIGHT_IMPORTANCE_POSITION): the light tree over the table's entries (its kernels
// are listed where they stand, below; the pick and the probability lookup: nx_lights.h).
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "nx_host.h"
#include "nx_lights.h"

namespace nxd {

namespace {

constexpr int kLightBlock = 256;
constexpr int kMeanBlock = 1024;

// One workgroup per map, a fixed order of additions: the same mean on every run.
__global__ void __launch_bounds__(kMeanBlock) light_map_mean_kernel(const TextureDev t, const float* __restrict__ srgbLut, float* __restrict__ mean4,
                                                                     double* __restrict__ mean64)
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
    if (threadIdx.x < 4) mean64[threadIdx.x] = (threadIdx.x < 3 && texels) ? sSum[threadIdx.x][0] / (double)texels : 0.0;  // (the light tree's weights: below)
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
    // the very expression of the light sample's density (nx_wavefront.h next_event_estimation)
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

// ---- the light tree (nxhip_set_light_importance): built behind the table, over the table's entries ------------------------------------
//   light_tree_bounds_kernel  min / max of the entries' centroids (ordered-integer atomics: the same six words whatever the order)
//   light_tree_key_kernel     key = 30-bit Morton code of the centroid within those bounds << 23 | entry: no two keys alike
//   (sort)                    rocPRIM's radix sort of the keys
//   light_tree_leaf_kernel    slot j: the box and the binary64 weight of entry order[j], both from corners transformed in binary64 (the
//                             binary32 inputs, every operation in binary64, rounded once: what float64 geometry gives); slots past
//                             the entries are empty
//   light_tree_level_kernel   one level of inner nodes from its children (levels of 256 nodes or more: one launch each) ...
//   light_tree_top_kernel     ... and the levels above them in one workgroup
//   light_tree_finish_kernel  w = binary32(W_node / W_root) in every node; a root weight of 0 or not finite: all w = 0, `valid` cleared
// min / max, a fixed tree shape and one addition per inner node: every value is independent of the order the threads run in.

constexpr uint32_t kTreeEntryBits = 23u;  // kLightTreeLeavesMax entries
constexpr uint32_t kTreeTopNodes = 128u;  // the level light_tree_top_kernel starts at (at most)

struct TriCorners {
    f3 a, b, c;
};
// the three corners the light sample itself computes (next_event_estimation: mat_point of the instance's current matrix)
__device__ TriCorners tree_corners(const LightTreeBuild& b, const uint32_t e)
{
    const uint32_t light = b.table[e].light;
    const ShadeInst* inst = &b.shadeInst[b.lights[light].mesh.meshId];
    const nx_triangle* t = shade_tri(inst->tris, e - b.lightBase[light]);
    const float* T = inst->transform;
    return TriCorners{mat_point(T, ld3(t->pos0)), mat_point(T, ld3(t->pos1)), mat_point(T, ld3(t->pos2))};
}
__device__ f3 tree_centroid(const TriCorners& t)
{
    const float third = 1.0f / 3.0f;
    return mk3(((t.a.x + t.b.x) + t.c.x) * third, ((t.a.y + t.b.y) + t.c.y) * third, ((t.a.z + t.b.z) + t.c.z) * third);
}
// a float as an integer that orders the same way, and back
__device__ uint32_t ordered_bits(const float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ float ordered_float(const uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ uint32_t spread10(uint32_t v)  // bit i of a 10-bit number to bit 3i
{
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__device__ uint32_t quantise10(const float x) { return x >= 1023.0f ? 1023u : (x > 0.0f ? (uint32_t)x : 0u); }  // (a NaN gives 0)

__global__ void __launch_bounds__(kLightBlock) light_tree_bounds_kernel(const LightTreeBuild b)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const float inf = __uint_as_float(0x7f800000u);
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    if (i < b.entries) {
        const f3 c = tree_centroid(tree_corners(b, i));
        lo[0] = hi[0] = c.x; lo[1] = hi[1] = c.y; lo[2] = hi[2] = c.z;
    }
    for (int a = 0; a < 3; a++) {
        for (int step = 32; step > 0; step >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], step));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], step));
        }
    }
    if ((threadIdx.x & 63u) == 0u) {
        for (int a = 0; a < 3; a++) {
            if (lo[a] <= hi[a]) {  // (a wave past the entries, or one of centroids that are all NaN, has nothing to say)
                atomicMin(&b.bounds[a], ordered_bits(lo[a]));
                atomicMax(&b.bounds[3 + a], ordered_bits(hi[a]));
            }
        }
    }
}

__global__ void __launch_bounds__(kLightBlock) light_tree_key_kernel(const LightTreeBuild b)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.entries) return;
    const f3 c = tree_centroid(tree_corners(b, i));
    const float lx = ordered_float(b.bounds[0]), ly = ordered_float(b.bounds[1]), lz = ordered_float(b.bounds[2]);
    const float ex = ordered_float(b.bounds[3]) - lx, ey = ordered_float(b.bounds[4]) - ly, ez = ordered_float(b.bounds[5]) - lz;
    // one scale for the three axes (the largest extent spans the 1 024 cells): a flat arrangement stays flat in the code
    const float extent = fmaxf(fmaxf(ex, ey), ez);
    const float scale = extent > 0.0f ? 1024.0f / extent : 0.0f;
    const uint32_t morton = (spread10(quantise10((c.x - lx) * scale)) << 2) | (spread10(quantise10((c.y - ly) * scale)) << 1) | spread10(quantise10((c.z - lz) * scale));
    b.keys[i] = ((uint64_t)morton << kTreeEntryBits) | (uint64_t)i;
}

// Corner k of entry e's triangle under its instance's matrix, in binary64, and the light's luminance in binary64: the leaves' boxes and
// weights come from these — not from the binary32 mat_point / tri_area of the light sample, whose rounding of a four-term sum is tens
// of ulps of a coordinate that cancels to near zero and 1e-5 of the area of a small triangle far from the origin.  The probabilities
// are the tree's own on both sides of the MIS weight, so nothing needs them to equal the table's.
struct TriCorners64 {
    double a[3], b[3], c[3];
    double Y;
};
__device__ void tree_point64(const float* T, const float* p, double* out)
{
    for (int r = 0; r < 3; r++)
        out[r] = (((double)T[4 * r] * (double)p[0] + (double)T[4 * r + 1] * (double)p[1]) + (double)T[4 * r + 2] * (double)p[2]) + (double)T[4 * r + 3];
}
__device__ TriCorners64 tree_corners64(const LightTreeBuild& b, const uint32_t e)
{
    const uint32_t light = b.table[e].light;
    const ShadeInst* inst = &b.shadeInst[b.lights[light].mesh.meshId];
    const nx_triangle* t = shade_tri(inst->tris, e - b.lightBase[light]);
    TriCorners64 c;
    tree_point64(inst->transform, t->pos0, c.a);
    tree_point64(inst->transform, t->pos1, c.b);
    tree_point64(inst->transform, t->pos2, c.c);
    const nx_material* m = &inst->material;
    double r = (double)m->emissive[0], g = (double)m->emissive[1], bl = (double)m->emissive[2];
    if (m->emissiveMapId != -1) {
        const double* mean = b.mapMean64 + 4 * (size_t)m->emissiveMapId;
        r = mean[0]; g = mean[1]; bl = mean[2];
    }
    c.Y = (double)m->intensity * ((0.2126 * r + 0.7152 * g) + 0.0722 * bl);
    return c;
}

__global__ void __launch_bounds__(kLightBlock) light_tree_leaf_kernel(const LightTreeBuild b)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= b.leaves) return;
    const float inf = __uint_as_float(0x7f800000u);
    LightNode n{{inf, inf, inf}, 0.0f, {-inf, -inf, -inf}, kNotALight};
    double w = 0.0;
    if (j < b.entries) {
        const uint32_t e = (uint32_t)(b.sorted[j] & (uint64_t)((1u << kTreeEntryBits) - 1u));
        const TriCorners64 t = tree_corners64(b, e);
        double e1[3], e2[3];
        for (int a = 0; a < 3; a++) {
            n.lo[a] = (float)fmin(fmin(t.a[a], t.b[a]), t.c[a]);
            n.hi[a] = (float)fmax(fmax(t.a[a], t.b[a]), t.c[a]);
            e1[a] = t.b[a] - t.a[a];
            e2[a] = t.c[a] - t.a[a];
        }
        const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
        n.entry = e;
        w = (0.5 * sqrt((cx * cx + cy * cy) + cz * cz)) * t.Y;
        if (!(w > 0.0) || !isfinite(w)) w = 0.0;  // negative or not finite: never picked (the table's rule)
        b.order[j] = e;
        b.slotOf[e] = j;
    }
    b.nodes[b.leaves + j] = n;
    b.nodeWeight[b.leaves + j] = w;
}

__device__ void tree_join(const LightTreeBuild& b, const uint32_t k)
{
    const LightNode l = b.nodes[2u * k], r = b.nodes[2u * k + 1u];
    LightNode n;
    for (int a = 0; a < 3; a++) { n.lo[a] = fminf(l.lo[a], r.lo[a]); n.hi[a] = fmaxf(l.hi[a], r.hi[a]); }
    n.w = 0.0f;
    n.entry = 0u;
    b.nodes[k] = n;
    b.nodeWeight[k] = b.nodeWeight[2u * k] + b.nodeWeight[2u * k + 1u];
}

// the level whose first node is `first` (a power of two): nodes first .. 2 first - 1
__global__ void __launch_bounds__(kLightBlock) light_tree_level_kernel(const LightTreeBuild b, const uint32_t first)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < first) tree_join(b, first + i);
}

// ... and every level from `first` (<= kTreeTopNodes) up to the root, one workgroup
__global__ void __launch_bounds__(kLightBlock) light_tree_top_kernel(const LightTreeBuild b, const uint32_t first)
{
    for (uint32_t level = first; level >= 1u; level >>= 1) {
        if (threadIdx.x < level) tree_join(b, level + threadIdx.x);
        __threadfence_block();
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kLightBlock) light_tree_finish_kernel(const LightTreeBuild b)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 2u * b.leaves) return;
    if (k == 0u) {  // (unused: zeroed so that a read-back is the same every time)
        b.nodes[0] = LightNode{{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, 0u};
        return;
    }
    const double total = b.nodeWeight[1];
    const bool valid = total > 0.0 && isfinite(total);
    b.nodes[k].w = valid ? (float)(b.nodeWeight[k] / total) : 0.0f;
    if (k == 1u && !valid) b.header->valid = 0u;  // (the table's rule; light_normalise_kernel has written the header ahead of this)
}

__global__ void __launch_bounds__(kLightBlock) light_tree_pick_kernel(const LightNode* __restrict__ nodes, const uint32_t leaves, const float* __restrict__ points,
                                                                       const float* __restrict__ u, const uint32_t count, uint32_t* __restrict__ entry, float* __restrict__ prob)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        uint32_t e = kNotALight;
        float P = 0.0f;
        if (!light_tree_pick(nodes, leaves, mk3(points[3 * k], points[3 * k + 1], points[3 * k + 2]), u[k], e, P)) { e = kNotALight; P = 0.0f; }
        entry[k] = e;
        prob[k] = P;
    }
}

__global__ void __launch_bounds__(kLightBlock) light_tree_prob_kernel(const LightNode* __restrict__ nodes, const uint32_t leaves, const uint32_t* __restrict__ slotOf,
                                                                       const float* __restrict__ points, const uint32_t* __restrict__ entry, const uint32_t count,
                                                                       float* __restrict__ prob)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x)
        prob[k] = light_tree_prob(nodes, leaves, mk3(points[3 * k], points[3 * k + 1], points[3 * k + 2]), slotOf[entry[k]]);
}

unsigned blocks_for(uint32_t n) { return (n + (uint32_t)kLightBlock - 1u) / (uint32_t)kLightBlock; }

}  // namespace

int light_tree_sort_bytes(size_t entries, size_t* bytes)
{
    *bytes = 0;
    NX_HIP(rocprim::radix_sort_keys(nullptr, *bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, entries, 0u, 30u + kTreeEntryBits, nullptr));
    return NXHIP_OK;
}

// bounds -> keys -> sort -> leaves -> inner levels -> w, in stream order behind light_table_build (b.entries >= 1; b.leaves a power of two >= entries)
int light_tree_build(hipStream_t st, const LightTreeBuild& b, void* sortTemp, size_t sortBytes)
{
    NX_HIP(hipMemsetAsync(b.bounds, 0xff, 3 * sizeof(uint32_t), st));
    NX_HIP(hipMemsetAsync(b.bounds + 3, 0, 3 * sizeof(uint32_t), st));
    light_tree_bounds_kernel<<<blocks_for(b.entries), kLightBlock, 0, st>>>(b);
    NX_HIP(hipGetLastError());
    light_tree_key_kernel<<<blocks_for(b.entries), kLightBlock, 0, st>>>(b);
    NX_HIP(hipGetLastError());
    NX_HIP(rocprim::radix_sort_keys(sortTemp, sortBytes, b.keys, const_cast<uint64_t*>(b.sorted), (size_t)b.entries, 0u, 30u + kTreeEntryBits, st));
    light_tree_leaf_kernel<<<blocks_for(b.leaves), kLightBlock, 0, st>>>(b);
    NX_HIP(hipGetLastError());
    uint32_t first = b.leaves / 2u;
    for (; first > kTreeTopNodes; first /= 2u) {
        light_tree_level_kernel<<<blocks_for(first), kLightBlock, 0, st>>>(b, first);
        NX_HIP(hipGetLastError());
    }
    if (first >= 1u) {
        light_tree_top_kernel<<<1, kLightBlock, 0, st>>>(b, first);
        NX_HIP(hipGetLastError());
    }
    light_tree_finish_kernel<<<blocks_for(2u * b.leaves), kLightBlock, 0, st>>>(b);
    NX_HIP(hipGetLastError());
    return NXHIP_OK;
}

const void* light_tree_pick_kernel_ptr() { return (const void*)light_tree_pick_kernel; }
const void* light_tree_prob_kernel_ptr() { return (const void*)light_tree_prob_kernel; }

int light_scan_bytes(size_t entries, size_t* bytes)
{
    *bytes = 0;
    NX_HIP(rocprim::deterministic_inclusive_scan(nullptr, *bytes, (double*)nullptr, (double*)nullptr, entries, rocprim::plus<double>(), nullptr));
    return NXHIP_OK;
}

int light_map_mean(hipStream_t st, const TextureDev& t, const float* srgbLut, float* mean4, double* mean64)
{
    light_map_mean_kernel<<<1, kMeanBlock, 0, st>>>(t, srgbLut, mean4, mean64);
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
