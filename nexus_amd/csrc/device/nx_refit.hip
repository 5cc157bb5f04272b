// nx_refit.hip — dynamic transforms on the device: new object-to-world matrices of existing instances go in, and the
// instance table, the traversal records and the TLAS BVH8 (same topology, refitted bounds) are updated in HBM without the
// scene or the tree making a round trip through the host.
//
// Reference behaviour being replaced: every edit re-runs MeshInstance::SetTransform -> BVHInstance::SetTransform
// (/root/reference/Nexus/src/Geometry/BVH/BVHInstance.cpp:4-29: inverse matrix, world bounds from the 8 transformed corners
// of the BLAS root's quantisation frame), then an O(n^2) agglomerative TLAS rebuild on the CPU and a full re-upload
// (Scene/Scene.cpp:29-55, Geometry/BVH/TLAS.cpp:13-100).  Here: one thread per moved instance does the SetTransform
// arithmetic (same operation order as the host classes: results are bit-identical to nexus::BVHInstance::SetTransform), then
// one workgroup sweeps the TLAS bottom-up level by level (levels are independent inside; a barrier between them),
// re-deriving each node's quantisation frame and child boxes exactly as nexus::collapse::Refit does on the host.
// Deforming meshes (nxhip_update_blas): the same sweep over a BLAS, many workgroups wide, its leaf boxes taken from the new
// triangles (blas_refit_kernel below); the arithmetic of a node is one function both sweeps call (refit_node_frame).
#define NX_KERNEL_TU 1
#include "nx_device.h"
#include "nx_instbox.h"
#include "nx_math.h"

namespace nxd {

constexpr int kRefitBlock = 1024;
constexpr int kBlasRefitBlock = 256;  // (nxhip_scene.hip launches blas_refit_kernel with the same figure)

struct Box {
    float lo[3], hi[3];
};

NXD void box_empty(Box& b)
{
    for (int a = 0; a < 3; a++) { b.lo[a] = 1e30f; b.hi[a] = -1e30f; }  // nexus::AABB's empty box
}
NXD void box_grow(Box& b, const float* lo, const float* hi)
{
    for (int a = 0; a < 3; a++) { b.lo[a] = fminf(b.lo[a], lo[a]); b.hi[a] = fmaxf(b.hi[a], hi[a]); }
}

// nexus::Mat4::Inverted (host/Math.cpp): cofactor expansion, every product and sum in the same order
NXD float cof(const float* m, int a, int b, int c) { return m[a] * m[b] * m[c]; }
// returns whether the matrix is singular (det == 0: the identity comes out, as nexus::Mat4's default)
NXD bool mat4_invert(const float* m, float* out)
{
    float inv[16];
    inv[0] = cof(m, 5, 10, 15) - cof(m, 5, 11, 14) - cof(m, 9, 6, 15) + cof(m, 9, 7, 14) + cof(m, 13, 6, 11) - cof(m, 13, 7, 10);
    inv[1] = -cof(m, 1, 10, 15) + cof(m, 1, 11, 14) + cof(m, 9, 2, 15) - cof(m, 9, 3, 14) - cof(m, 13, 2, 11) + cof(m, 13, 3, 10);
    inv[2] = cof(m, 1, 6, 15) - cof(m, 1, 7, 14) - cof(m, 5, 2, 15) + cof(m, 5, 3, 14) + cof(m, 13, 2, 7) - cof(m, 13, 3, 6);
    inv[3] = -cof(m, 1, 6, 11) + cof(m, 1, 7, 10) + cof(m, 5, 2, 11) - cof(m, 5, 3, 10) - cof(m, 9, 2, 7) + cof(m, 9, 3, 6);
    inv[4] = -cof(m, 4, 10, 15) + cof(m, 4, 11, 14) + cof(m, 8, 6, 15) - cof(m, 8, 7, 14) - cof(m, 12, 6, 11) + cof(m, 12, 7, 10);
    inv[5] = cof(m, 0, 10, 15) - cof(m, 0, 11, 14) - cof(m, 8, 2, 15) + cof(m, 8, 3, 14) + cof(m, 12, 2, 11) - cof(m, 12, 3, 10);
    inv[6] = -cof(m, 0, 6, 15) + cof(m, 0, 7, 14) + cof(m, 4, 2, 15) - cof(m, 4, 3, 14) - cof(m, 12, 2, 7) + cof(m, 12, 3, 6);
    inv[7] = cof(m, 0, 6, 11) - cof(m, 0, 7, 10) - cof(m, 4, 2, 11) + cof(m, 4, 3, 10) + cof(m, 8, 2, 7) - cof(m, 8, 3, 6);
    inv[8] = cof(m, 4, 9, 15) - cof(m, 4, 11, 13) - cof(m, 8, 5, 15) + cof(m, 8, 7, 13) + cof(m, 12, 5, 11) - cof(m, 12, 7, 9);
    inv[9] = -cof(m, 0, 9, 15) + cof(m, 0, 11, 13) + cof(m, 8, 1, 15) - cof(m, 8, 3, 13) - cof(m, 12, 1, 11) + cof(m, 12, 3, 9);
    inv[10] = cof(m, 0, 5, 15) - cof(m, 0, 7, 13) - cof(m, 4, 1, 15) + cof(m, 4, 3, 13) + cof(m, 12, 1, 7) - cof(m, 12, 3, 5);
    inv[11] = -cof(m, 0, 5, 11) + cof(m, 0, 7, 9) + cof(m, 4, 1, 11) - cof(m, 4, 3, 9) - cof(m, 8, 1, 7) + cof(m, 8, 3, 5);
    inv[12] = -cof(m, 4, 9, 14) + cof(m, 4, 10, 13) + cof(m, 8, 5, 14) - cof(m, 8, 6, 13) - cof(m, 12, 5, 10) + cof(m, 12, 6, 9);
    inv[13] = cof(m, 0, 9, 14) - cof(m, 0, 10, 13) - cof(m, 8, 1, 14) + cof(m, 8, 2, 13) + cof(m, 12, 1, 10) - cof(m, 12, 2, 9);
    inv[14] = -cof(m, 0, 5, 14) + cof(m, 0, 6, 13) + cof(m, 4, 1, 14) - cof(m, 4, 2, 13) - cof(m, 12, 1, 6) + cof(m, 12, 2, 5);
    inv[15] = cof(m, 0, 5, 10) - cof(m, 0, 6, 9) - cof(m, 4, 1, 10) + cof(m, 4, 2, 9) + cof(m, 8, 1, 6) - cof(m, 8, 2, 5);
    const float det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    if (det != 0) {
        const float invdet = 1.0f / det;
        for (int i = 0; i < 16; ++i) out[i] = inv[i] * invdet;
        return false;
    }
    for (int i = 0; i < 16; ++i) out[i] = (i % 5 == 0) ? 1.0f : 0.0f;  // nexus::Mat4's default: identity
    return true;
}

// BVHInstance::SetTransform for `count` instances: thread k handles instance ids[k] with matrix transforms[16 k .. 16 k + 15]
// (kernel parameters are plain pointers: an address-space qualifier in a kernel signature would mangle the device symbol
//  differently from the host stub, which is compiled without it)
// blasRefresh != 0 (after nxhip_update_blas refitted the instance's BLAS): the matrix is the record's own and stays, with its
// inverse and the shading record; what follows the BLAS root is redone — world bounds, tight box, the record's root-node copy.
__global__ void __launch_bounds__(256) instance_transform_kernel(const DeviceState* __restrict__ S, nx_bvh_instance* instancesArg, InstTrav* travArg,
                                                                 const uint32_t* __restrict__ leafOfInstance, const uint32_t* __restrict__ ids,
                                                                 const float* __restrict__ transforms, const uint32_t count, InstBox* __restrict__ tightBoxes,
                                                                 ShadeInst* shadeInstArg, const uint32_t blasRefresh)
{
    NX_G ShadeInst* shadeInst = (NX_G ShadeInst*)shadeInstArg;  // nullptr: the host rebuilds the shading records before the next render
    NX_G nx_bvh_instance* instances = (NX_G nx_bvh_instance*)instancesArg;
    NX_G InstTrav* trav = (NX_G InstTrav*)travArg;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const uint32_t id = ids[k];
        float m[16], inv[16];
        NX_G nx_bvh_instance* inst = &instances[id];
        for (int i = 0; i < 16; i++) m[i] = blasRefresh ? inst->transform.cell[i] : transforms[16 * (size_t)k + i];
        const bool singular = mat4_invert(m, inv);
        // world bounds: the 8 transformed corners of the BLAS root's quantisation frame [p, p + 2^(e-127) * 255]
        const NX_G uint4* root = S->blas[inst->bvhIdx].nodes;
        const uint4 n0 = root[0];
        const float lo[3] = {__uint_as_float(n0.x), __uint_as_float(n0.y), __uint_as_float(n0.z)};
        const float steps = 255.0f;
        float hi[3];
        for (int a = 0; a < 3; a++) hi[a] = lo[a] + ldexpf(1.0f, (int)((n0.w >> (8 * a)) & 0xffu) - 127) * steps;
        Box wb;
        box_empty(wb);
        for (int corner = 0; corner < 8; corner++) {
            const float cx = (corner & 1) ? hi[0] : lo[0], cy = (corner & 2) ? hi[1] : lo[1], cz = (corner & 4) ? hi[2] : lo[2];
            const float p[3] = {m[0] * cx + m[1] * cy + m[2] * cz + m[3] * 1.0f, m[4] * cx + m[5] * cy + m[6] * cz + m[7] * 1.0f,
                                m[8] * cx + m[9] * cy + m[10] * cz + m[11] * 1.0f};
            box_grow(wb, p, p);
        }
        if (!blasRefresh) {
            for (int i = 0; i < 16; i++) { inst->transform.cell[i] = m[i]; inst->invTransform.cell[i] = inv[i]; }
            if (shadeInst)
                for (int i = 0; i < 12; i++) { shadeInst[id].transform[i] = m[i]; shadeInst[id].invTransform[i] = inv[i]; }
        }
        for (int a = 0; a < 3; a++) { inst->boundsMin[a] = wb.lo[a]; inst->boundsMax[a] = wb.hi[a]; }
        if (tightBoxes && kNodeStride == 5) {  // a TLAS built on the device keeps its tighter boxes (nx_instbox.h) through the refit
            InstBox tb;
            for (int a = 0; a < 3; a++) { tb.lo[a] = wb.lo[a]; tb.hi[a] = wb.hi[a]; }
            tighten_instance_box(reinterpret_cast<const NX_G nx_bvh8_node*>(root), m, tb, singular);
            tightBoxes[id] = tb;
        }
        NX_G InstTrav* t = &trav[leafOfInstance[id]];
        if (blasRefresh) {
            for (int q = 0; q < 5; q++) t->root[q] = root[q];
            continue;
        }
        t->r0 = make_float4(inv[0], inv[1], inv[2], inv[3]);
        t->r1 = make_float4(inv[4], inv[5], inv[6], inv[7]);
        t->r2 = make_float4(inv[8], inv[9], inv[10], inv[11]);
        t->flags = rows_are_identity(inv) ? kInstIdentity : 0u;
    }
}

NXD uint32_t quantize(float v)  // nexus::collapse Quantize
{
    if (!(v == v)) return 0u;
    if (v <= 0.0f) return 0u;
    if (v >= 255.0f) return 255u;
    return (uint32_t)v;
}

// ceil(log2f(x)) as the host computes it (std::log2 on a float, then std::ceil).  glibc's log2f is within 0.75 ulp, the
// double-precision logarithm rounded to float is the correctly rounded value: the two agree except for arguments within a
// few float steps of a power of two whose logarithm falls near a rounding midpoint (probability ~1e-7 per call).
NXD float ceil_log2(float x) { return ceilf((float)log2((double)x)); }

// The arithmetic of one node of nexus::collapse::Refit, shared by the TLAS and the BLAS refit so that the two cannot drift: from the
// node's box `nb` (the union of its used children's boxes, grown in slot order by the caller) the exponent bytes of its quantisation
// frame (e[0] | e[1] << 8 | e[2] << 16; the frame's origin p is nb.lo) and, for every used slot s, the six quantised coordinates
// q[0..5][s] = qlox, qloy, qloz, qhix, qhiy, qhiz (floor / ceil of the offset in grid steps, clamped to a byte).  Unused slots of q
// are left as they are.
NXD void refit_node_frame(const Box& nb, const Box (&childBox)[8], const bool (&used)[8], uint32_t& ebytes, uint8_t (&q)[6][8])
{
    const float denom = 1.0f / 255.0f;
    float invScale[3];
    ebytes = 0;
    for (int a = 0; a < 3; a++) {
        float ex = ceil_log2((nb.hi[a] - nb.lo[a]) * denom);
        if (fabsf(ex) < 126.0f && 255.0f * ldexpf(1.0f, (int)ex) < nb.hi[a] - nb.lo[a]) ex += 1.0f;  // 255 * 2^e >= fl(extent), exactly
        // exponent byte of exp2f(ex): 0 below the normal range (and for -inf: a degenerate axis), 255 above it
        uint32_t e = 0;
        if (ex == ex && ex > -127.0f) e = ex >= 128.0f ? 255u : (uint32_t)((int)ex + 127);
        ebytes |= e << (8 * a);
        // 1 / 2^ex, exactly: inf for ex = -inf (degenerate axis), as 1.0f / std::pow(2.0f, ex)
        const float pw = ex == ex ? (ex < -200.0f ? 0.0f : (ex > 200.0f ? __uint_as_float(0x7f800000u) : ldexpf(1.0f, (int)ex))) : ex;
        invScale[a] = 1.0f / pw;
    }
    for (int s = 0; s < 8; s++) {
        if (!used[s]) continue;
        const Box& cb = childBox[s];
        for (int a = 0; a < 3; a++) {
            q[a][s] = (uint8_t)quantize(floorf((cb.lo[a] - nb.lo[a]) * invScale[a]));
            q[3 + a][s] = (uint8_t)quantize(ceilf((cb.hi[a] - nb.lo[a]) * invScale[a]));
        }
    }
}

// nexus::collapse::Refit on the device.  `order` lists the node indices grouped by depth, deepest level first;
// levelStart[l] .. levelStart[l + 1] is level l of that list.  One workgroup: levels are separated by a barrier.
__global__ void __launch_bounds__(kRefitBlock) tlas_refit_kernel(nx_bvh8_node* nodesArg, const uint32_t* __restrict__ primIdx,
                                                                 const nx_bvh_instance* instancesArg, const uint32_t* __restrict__ order,
                                                                 const uint32_t* __restrict__ levelStart, const uint32_t levels, Box* __restrict__ nodeBox,
                                                                 const InstBox* __restrict__ tightBoxes)
{
    NX_G nx_bvh8_node* nodes = (NX_G nx_bvh8_node*)nodesArg;
    const NX_G nx_bvh_instance* instances = (const NX_G nx_bvh_instance*)instancesArg;
    for (uint32_t l = 0; l < levels; l++) {
        for (uint32_t i = levelStart[l] + threadIdx.x; i < levelStart[l + 1]; i += blockDim.x) {
            const uint32_t k = order[i];
            NX_G nx_bvh8_node* node = &nodes[k];
            const uint32_t imask = node->imask, childBase = node->childBaseIdx, primBase = node->triangleBaseIdx;
            Box childBox[8], nb;
            bool used[8];
            box_empty(nb);
            for (int s = 0; s < 8; s++) {
                used[s] = false;
                Box cb;
                box_empty(cb);
                const uint32_t meta = node->meta[s];
                if (imask & (1u << s)) {
                    cb = nodeBox[childBase + (uint32_t)__popc(imask & ((1u << s) - 1u))];
                } else if (meta) {
                    const uint32_t first = primBase + (meta & 0x1fu);
                    const int cnt = __popc(meta >> 5);
                    for (int j = 0; j < cnt; j++) {
                        const uint32_t instanceId = primIdx[first + (uint32_t)j];
                        if (tightBoxes) {  // (a device-built TLAS: the boxes it was built from, kept up to date by the transform kernel)
                            const InstBox tb = tightBoxes[instanceId];
                            box_grow(cb, tb.lo, tb.hi);
                            continue;
                        }
                        const NX_G nx_bvh_instance* in = &instances[instanceId];
                        const float lo[3] = {in->boundsMin[0], in->boundsMin[1], in->boundsMin[2]}, hi[3] = {in->boundsMax[0], in->boundsMax[1], in->boundsMax[2]};
                        box_grow(cb, lo, hi);
                    }
                } else {
                    continue;
                }
                used[s] = true;
                childBox[s] = cb;
                box_grow(nb, cb.lo, cb.hi);
            }
            nodeBox[k] = nb;
            uint32_t ebytes;
            uint8_t q[6][8];
            refit_node_frame(nb, childBox, used, ebytes, q);
            node->p[0] = nb.lo[0]; node->p[1] = nb.lo[1]; node->p[2] = nb.lo[2];
            node->e[0] = (uint8_t)(ebytes & 0xffu); node->e[1] = (uint8_t)((ebytes >> 8) & 0xffu); node->e[2] = (uint8_t)((ebytes >> 16) & 0xffu);
            for (int s = 0; s < 8; s++) {
                if (!used[s]) continue;
                node->qlox[s] = q[0][s]; node->qloy[s] = q[1][s]; node->qloz[s] = q[2][s];
                node->qhix[s] = q[3][s]; node->qhiy[s] = q[4][s]; node->qhiz[s] = q[5][s];
            }
        }
        __syncthreads();  // the next (shallower) level reads the boxes just written; one workgroup, so this orders them
    }
}

// ---- BLAS refit (nxhip_update_blas): the same sweep over a mesh's BVH8, its leaf boxes taken from the new triangles.
// The reference has nothing of the kind: a changed mesh there is a new BVH8Builder run (Assets/AssetManager.cpp:23-37).
//
// `order` / `levelStart` as above.  A launch handles the levels firstLevel .. firstLevel + levelCount - 1.  A level wide
// enough to occupy the chip is given a launch of its own (levelCount == 1, any grid: the nodes of a level are independent);
// a run of narrow levels is one launch of ONE workgroup with a barrier between levels (levelCount > 1 requires gridDim.x == 1).
// No workgroup ever waits for another inside a launch — the per-XCD L2s are not coherent for plain loads, and a tree of
// some ten levels does not repay an agent-scope release / acquire per node: kernel boundaries order the levels.
// One thread per node, slots in sequence: the host's operation order, hence its bits.  A node is read as 5 x uint4 and
// written back as 4 (the word with the child / primitive indices and the meta bytes never changes); the per-node boxes live
// in a 32-byte record so that a child's box is two aligned 16-byte loads.
struct __attribute__((aligned(16))) NodeBox32 {
    float4 lo, hi;
};

NXD uint32_t byte_of(const uint32_t lo, const uint32_t hi, const int s) { return ((s < 4 ? lo : hi) >> (8 * (s & 3))) & 0xffu; }
NXD uint32_t pack4(const uint8_t (&b)[8], const int first)
{
    return (uint32_t)b[first] | ((uint32_t)b[first + 1] << 8) | ((uint32_t)b[first + 2] << 16) | ((uint32_t)b[first + 3] << 24);
}

__global__ void __launch_bounds__(kBlasRefitBlock) blas_refit_kernel(uint4* nodesArg, const uint32_t* __restrict__ triIdx, const nx_triangle* trisArg,
                                                                    const uint32_t* __restrict__ order, const uint32_t* __restrict__ levelStart,
                                                                    const uint32_t firstLevel, const uint32_t levelCount, NodeBox32* nodeBoxArg)
{
    NX_G uint4* nodes = (NX_G uint4*)nodesArg;
    const NX_G nx_triangle* tris = (const NX_G nx_triangle*)trisArg;
    NX_G NodeBox32* nodeBox = (NX_G NodeBox32*)nodeBoxArg;
    for (uint32_t l = firstLevel; l < firstLevel + levelCount; l++) {
        const uint32_t end = levelStart[l + 1];
        for (uint32_t i = levelStart[l] + blockIdx.x * blockDim.x + threadIdx.x; i < end; i += gridDim.x * blockDim.x) {
            const uint32_t k = order[i];
            NX_G uint4* node = nodes + (size_t)k * kNodeStride;
            const uint4 n0 = node[0], n1 = node[1];
            uint4 n2 = node[2], n3 = node[3], n4 = node[4];
            const uint32_t imask = n0.w >> 24, childBase = n1.x, primBase = n1.y;
            Box childBox[8], nb;
            bool used[8];
            box_empty(nb);
            for (int s = 0; s < 8; s++) {
                used[s] = false;
                Box cb;
                box_empty(cb);
                const uint32_t meta = byte_of(n1.z, n1.w, s);
                if (imask & (1u << s)) {
                    const NodeBox32 c = nodeBox[childBase + (uint32_t)__popc(imask & ((1u << s) - 1u))];
                    cb.lo[0] = c.lo.x; cb.lo[1] = c.lo.y; cb.lo[2] = c.lo.z;
                    cb.hi[0] = c.hi.x; cb.hi[1] = c.hi.y; cb.hi[2] = c.hi.z;
                } else if (meta) {
                    const uint32_t first = primBase + (meta & 0x1fu);
                    const int cnt = __popc(meta >> 5);
                    for (int j = 0; j < cnt; j++) {
                        // the triangle's box as BVH8::Refit makes it — pos0, pos1, pos2 grown from the empty box — then the slot's
                        const NX_G nx_triangle* t = &tris[triIdx[first + (uint32_t)j]];
                        const float p0[3] = {t->pos0[0], t->pos0[1], t->pos0[2]}, p1[3] = {t->pos1[0], t->pos1[1], t->pos1[2]}, p2[3] = {t->pos2[0], t->pos2[1], t->pos2[2]};
                        Box tb;
                        box_empty(tb);
                        box_grow(tb, p0, p0);
                        box_grow(tb, p1, p1);
                        box_grow(tb, p2, p2);
                        box_grow(cb, tb.lo, tb.hi);
                    }
                } else {
                    continue;
                }
                used[s] = true;
                childBox[s] = cb;
                box_grow(nb, cb.lo, cb.hi);
            }
            NodeBox32 out;
            out.lo = make_float4(nb.lo[0], nb.lo[1], nb.lo[2], 0.0f);
            out.hi = make_float4(nb.hi[0], nb.hi[1], nb.hi[2], 0.0f);
            nodeBox[k] = out;
            uint32_t ebytes;
            uint8_t q[6][8];
            const uint32_t oldLo[6] = {n2.x, n2.z, n3.x, n3.z, n4.x, n4.z}, oldHi[6] = {n2.y, n2.w, n3.y, n3.w, n4.y, n4.w};
            for (int c = 0; c < 6; c++)
                for (int s = 0; s < 8; s++) q[c][s] = (uint8_t)byte_of(oldLo[c], oldHi[c], s);  // (unused slots keep their bytes)
            refit_node_frame(nb, childBox, used, ebytes, q);
            node[0] = make_uint4(__float_as_uint(nb.lo[0]), __float_as_uint(nb.lo[1]), __float_as_uint(nb.lo[2]), (n0.w & 0xff000000u) | ebytes);
            n2 = make_uint4(pack4(q[0], 0), pack4(q[0], 4), pack4(q[1], 0), pack4(q[1], 4));
            n3 = make_uint4(pack4(q[2], 0), pack4(q[2], 4), pack4(q[3], 0), pack4(q[3], 4));
            n4 = make_uint4(pack4(q[4], 0), pack4(q[4], 4), pack4(q[5], 0), pack4(q[5], 4));
            node[2] = n2;
            node[3] = n3;
            node[4] = n4;
        }
        if (levelCount > 1) __syncthreads();  // (one workgroup: the next, shallower level reads the boxes just written)
    }
}

// The material code of every traversal record (nx_device.h, kHitCodeShift): record k — TLAS leaf order — belongs to instance
// instIdx, whose shading record holds a copy of its material; type + 1 goes above the instance index, where the closest-hit
// kernel finds it in the register that carries the hit's instance (nx_trace.hip, flush).  Run by the host after it has rebuilt
// the shading records (refresh_shade_inst: an instance, BLAS or material table changed).
__global__ void __launch_bounds__(256) inst_code_kernel(const DeviceState* __restrict__ S, InstTrav* travArg, const ShadeInst* shadeInstArg, const uint32_t count)
{
    NX_G InstTrav* trav = (NX_G InstTrav*)travArg;
    const NX_G ShadeInst* shadeInst = (const NX_G ShadeInst*)shadeInstArg;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const uint32_t inst = trav[k].instIdx & kHitInstMask;
        const int type = (int)shadeInst[inst].material.type;
        trav[k].instIdx = inst | ((type >= 0 && type <= 3) ? (uint32_t)(type + 1) << kHitCodeShift : 0u);
    }
}
// ... of a material table that holds an NX_MAT_METALROUGH, whose code is not type + 1 (nx_device.h hit_code_of_type); the kernel above stays
// the code of every other table
__global__ void __launch_bounds__(256) inst_code_metal_kernel(const DeviceState* __restrict__ S, InstTrav* travArg, const ShadeInst* shadeInstArg, const uint32_t count)
{
    NX_G InstTrav* trav = (NX_G InstTrav*)travArg;
    const NX_G ShadeInst* shadeInst = (const NX_G ShadeInst*)shadeInstArg;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const uint32_t inst = trav[k].instIdx & kHitInstMask;
        trav[k].instIdx = inst | (hit_code_of_type((int)shadeInst[inst].material.type) << kHitCodeShift);
    }
}

const void* inst_code_kernel_ptr() { return (const void*)inst_code_kernel; }
const void* inst_code_metal_kernel_ptr() { return (const void*)inst_code_metal_kernel; }
const void* instance_transform_kernel_ptr() { return (const void*)instance_transform_kernel; }
const void* tlas_refit_kernel_ptr() { return (const void*)tlas_refit_kernel; }
const void* blas_refit_kernel_ptr() { return (const void*)blas_refit_kernel; }

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_refit() { return layout_stamp(); }

}  // namespace nxd
