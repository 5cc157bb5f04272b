// nx_entry.hip — entry states of the primary rays (nx_device.h EntryState): the first steps of a run of 64 consecutive paths,
// walked once for the whole run.
//
// The reference starts every ray at the TLAS root (Cuda/BVH/BVH8Traversal.cuh:165-192).  The 64 primary rays of an 8 x 8 pixel
// tile then decode the same nodes and arrive at the same hit masks for their first four of ten node steps
// (tools/entry_point_probe.py: 40 % of the primary level's node steps).  Here eight lanes per run walk those steps with the run's
// ray BUNDLE — the pyramid from the camera through the bounding rectangle of the run's pixels, any sub-pixel position, any frame
// of the pass — and a conservative classification of every child box (lane c of the run's group: child slot c of the node):
//   hit by all   the four edge rays of the pyramid pass through the box shrunk by a margin (the directions from a point that hit
//                a convex body form a convex cone: four edge rays inside it put the whole pyramid inside it)
//   missed by all  the box grown by the margin lies outside one of the pyramid's four side planes, or behind its apex
//   undecided    anything else: the walk stops in front of this node
// The margin (1e-4 of the coordinates involved) is a hundred times the rounding of the kernel's float slab test, and a flat box
// (a quantisation axis with exponent 0, or equal bounds) is a plane both bounds of which the kernel computes with the same
// operands, so "hit by all" and "missed by all" are statements about what the kernel's own arithmetic returns for every ray of
// the bundle.  The walk mirrors the traversal loop's bookkeeping (nx_trace.hip: node step, instance entry + root test, triangle,
// pop, instance exit) and goes on through the triangles of a leaf: one every ray of the run misses is skipped, one every ray hits
// is CONSUMED — its record goes into the state, every ray computes its own hit for it when the state is installed, and the run's
// hit-distance interval bounds the box tests behind it.  It ends at an undecided child or triangle, at a second triangle every ray
// hits in front of the first, or at its depth limit.  What it leaves is a loop-top state of the traversal.
//
// The states depend on the camera, the pixel set and the scene — not on the frame number or the pass size — so a table outlives the
// pass: the host launches the walk on a slot's stream, in front of the slot's next pass, only after a call that changed one of its
// inputs (nxhip_render.hip walk_entry_states; the list: nx_context.h entryGeneration), and every pass until then reads the table.
//
// Conditions, checked here: pinhole camera (no lens: one origin), one octant for the whole bundle, an origin without negative zero,
// infinity, NaN or denormal components, and — to go through an instance — a scene of identity instances (the ray is then the
// same in the BLAS's frame; a transformed instance ends the walk in front of it).
#define NX_KERNEL_TU 1
#include "nx_device.h"
#include "nx_math.h"

namespace nxd {

namespace {

struct D3 { double x, y, z; };
NXD D3 dsub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
NXD D3 dcross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
NXD double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
NXD double dcomp(D3 a, int k) { return k == 0 ? a.x : (k == 1 ? a.y : a.z); }

struct Bundle {
    D3 org;
    D3 dir[4];    // edge rays, in order round the pyramid
    D3 plane[4];  // inward normals of the side planes
    D3 axis;      // sum of the edge directions
    // once the walk has consumed a triangle: its plane, as the unit normal pointing away from the apex and the offset hitN . p0, and
    // how far behind it a box or a triangle must lie to be missed by every ray (the rays' hits are on the plane)
    D3 hitN;
    double hitC, hitGap;
};

// the points with hitN . x >= hitC + hitGap are behind the consumed triangle's plane for every ray of the bundle
NXD bool behind_hit_plane(const Bundle& b, const double lo[3], const double hi[3])
{
    const double n[3] = {b.hitN.x, b.hitN.y, b.hitN.z};
    double nearest = 0.0;  // the box's smallest hitN . x
    for (int a = 0; a < 3; a++) nearest += n[a] >= 0.0 ? n[a] * lo[a] : n[a] * hi[a];
    return nearest >= b.hitC + b.hitGap;
}

enum { kMissAll = 0, kHitAll = 1, kUndecided = 2 };

// one child box [lo, hi] against the bundle.  [hitLo, hitHi]: what the rays' hit distances lie between once the walk has consumed
// a triangle every ray hits (1e300: no hit yet) — the kernel enters a child only while its entry distance is at or below the ray's
// hit distance.  A box is then "missed by all" when the grown box lies behind the consumed triangle's plane by a margin (every ray
// meets the plane, where its hit is, before any point of the box), "hit by all" when every ray enters the shrunk box in front of
// hitLo, undecided otherwise.  (b.dir are unit vectors: parameters are distances.)
NXD int classify(const Bundle& b, const double lo[3], const double hi[3], const double hitLo, const double hitHi)
{
    double m[3];
    bool flat[3];
    for (int a = 0; a < 3; a++) {
        const double o = dcomp(b.org, a);
        m[a] = 1.0e-4 * (fabs(o) + fabs(lo[a]) + fabs(hi[a]) + (hi[a] - lo[a]));
        flat[a] = hi[a] == lo[a];
    }
    // missed by all: a separating axis between the grown box and the pyramid (an unbounded cone: apex + t * edge, t >= 0).  Along
    // an axis n the cone covers [n.apex, +inf) when every edge has n.edge >= 0, (-inf, n.apex] when every edge has n.edge <= 0,
    // everything otherwise; the box covers [bmin, bmax].  Candidates: the pyramid's four side planes, the axis of the view
    // (behind the apex), the box's three face normals and the twelve cross products of a box edge with a pyramid edge — the last
    // are what separates a box that lies diagonally beside a thin bundle.
    {
        const double glo[3] = {lo[0] - m[0], lo[1] - m[1], lo[2] - m[2]}, ghi[3] = {hi[0] + m[0], hi[1] + m[1], hi[2] + m[2]};
        const auto separated = [&](const D3 n) {
            int nonNeg = 0, nonPos = 0;
            for (int k = 0; k < 4; k++) {
                const double c = ddot(n, b.dir[k]);
                nonNeg += c >= 0.0 ? 1 : 0;
                nonPos += c <= 0.0 ? 1 : 0;
            }
            if (nonNeg != 4 && nonPos != 4) return false;
            const double nx[3] = {n.x, n.y, n.z};
            double bmin = 0.0, bmax = 0.0;
            for (int a = 0; a < 3; a++) {
                bmin += nx[a] >= 0.0 ? nx[a] * glo[a] : nx[a] * ghi[a];
                bmax += nx[a] >= 0.0 ? nx[a] * ghi[a] : nx[a] * glo[a];
            }
            const double apex = ddot(n, b.org);
            const double slack = 1.0e-9 * (fabs(apex) + fabs(bmin) + fabs(bmax));
            if (nonNeg == 4 && bmax < apex - slack) return true;
            if (nonPos == 4 && bmin > apex + slack) return true;
            return false;
        };
        if (hitHi < 1.0e299 && behind_hit_plane(b, glo, ghi)) return kMissAll;
        for (int k = 0; k < 4; k++)
            if (separated(b.plane[k])) return kMissAll;
        if (separated(b.axis)) return kMissAll;
        if (separated(D3{1.0, 0.0, 0.0}) || separated(D3{0.0, 1.0, 0.0}) || separated(D3{0.0, 0.0, 1.0})) return kMissAll;
        for (int k = 0; k < 4; k++) {
            const D3 d = b.dir[k];
            if (separated(D3{0.0, -d.z, d.y}) || separated(D3{d.z, 0.0, -d.x}) || separated(D3{-d.y, d.x, 0.0})) return kMissAll;  // e_x, e_y, e_z cross d
        }
    }
    // hit by all: every edge ray through the shrunk box (a flat axis stays the plane it is; an axis too thin to shrink: undecided)
    for (int a = 0; a < 3; a++)
        if (!flat[a] && hi[a] - lo[a] <= 4.0 * m[a]) return kUndecided;
    double tnMin = 1.0e300, tnMax = 0.0;
    for (int k = 0; k < 4; k++) {
        double tn = 0.0, tf = 1.0e300;
        for (int a = 0; a < 3; a++) {
            const double o = dcomp(b.org, a), d = dcomp(b.dir[k], a);  // (d != 0: one octant, with a margin)
            const double l = flat[a] ? lo[a] : lo[a] + m[a], h = flat[a] ? hi[a] : hi[a] - m[a];
            const double t0 = (l - o) / d, t1 = (h - o) / d;
            tn = fmax(tn, fmin(t0, t1));
            tf = fmin(tf, fmax(t0, t1));
        }
        // (a clear pass: the entry and exit distances apart by more than rounding, unless a flat axis makes them one plane's)
        if (!(tn <= tf) || tf <= 0.0) return kUndecided;
        if (!(flat[0] || flat[1] || flat[2]) && !(tn < tf)) return kUndecided;
        tnMin = fmin(tnMin, tn);
        tnMax = fmax(tnMax, tn);
    }
    if (hitHi < 1.0e299) {
        // (the entry distance into the shrunk box — a maximum of three slab distances — is at most the largest of its values on the
        //  four edge rays up to second order in the bundle's opening angle, 1e-5 for a run of 64 pixels: the slack is a hundred times
        //  that; the real box is entered no later than the shrunk one.  Its SMALLEST value can lie inside the bundle, first order
        //  below the edge rays' where the bundle straddles an edge of the box: "missed by all" is the plane test above, not this.)
        const double slack = 1.0e-3 * (tnMax + m[0] + m[1] + m[2]) + 1.0e-6;
        if (tnMax + slack < hitLo) return kHitAll;
        return kUndecided;
    }
    return kHitAll;
}

// The eight lanes of a run's group combine their results with cross-lane operations (groups are aligned: xor 1, 2, 4 stays inside).
constexpr int kGroup = 8;
NXD uint32_t group_or(uint32_t v)
{
    v |= __shfl_xor(v, 1);
    v |= __shfl_xor(v, 2);
    v |= __shfl_xor(v, 4);
    return v;
}

// ChildTrace (nx_traverse.h child_trace) for the bundle, lane c of the group testing child slot c (node half c >> 2, byte c & 3):
// the hit mask every ray of it gets, or false when a child is undecided.  Every lane of the group returns the same.
NXD bool group_child_trace(const Bundle& b, const NX_G uint4* node, const uint32_t invOct4, const int c, const double hitLo, const double hitHi,
                           uint2& ng, uint2& tg)
{
    const uint4 n0 = node[0], n1 = node[1], n2 = node[2], n3 = node[3], n4 = node[4];
    const uint32_t e_imask = n0.w;
    const int i = c >> 2, j = c & 3;
    const uint32_t meta4 = i ? n1.w : n1.z;
    const uint32_t isInner4 = (meta4 & (meta4 << 1)) & 0x10101010u;
    const uint32_t innerMask4 = (isInner4 >> 4) * 0xffu;
    const uint32_t bitIndex4 = (meta4 ^ (invOct4 & innerMask4)) & 0x1f1f1f1fu;
    const uint32_t childBits = (((meta4 >> 5) & 0x07070707u) >> (8 * j)) & 0xffu;
    uint32_t mine = 0u, undecided = 0u;
    if (childBits != 0u) {  // (an empty slot sets no bit whatever its bounds say)
        const double p[3] = {(double)__uint_as_float(n0.x), (double)__uint_as_float(n0.y), (double)__uint_as_float(n0.z)};
        const double scale[3] = {(double)__uint_as_float((e_imask & 0xffu) << 23), (double)__uint_as_float((e_imask << 15) & 0x7f800000u),
                                 (double)__uint_as_float((e_imask << 7) & 0x7f800000u)};
        const uint32_t bitIndex = (bitIndex4 >> (8 * j)) & 0xffu;
        const uint32_t qlox = i ? n2.y : n2.x, qloy = i ? n2.w : n2.z, qloz = i ? n3.y : n3.x;
        const uint32_t qhix = i ? n3.w : n3.z, qhiy = i ? n4.y : n4.x, qhiz = i ? n4.w : n4.z;
        const double lo[3] = {p[0] + scale[0] * (double)((qlox >> (8 * j)) & 0xffu), p[1] + scale[1] * (double)((qloy >> (8 * j)) & 0xffu),
                              p[2] + scale[2] * (double)((qloz >> (8 * j)) & 0xffu)};
        const double hi[3] = {p[0] + scale[0] * (double)((qhix >> (8 * j)) & 0xffu), p[1] + scale[1] * (double)((qhiy >> (8 * j)) & 0xffu),
                              p[2] + scale[2] * (double)((qhiz >> (8 * j)) & 0xffu)};
        if (hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2]) {
            undecided = 1u;  // (an inverted slot: leave it to the kernel's own arithmetic)
        } else {
            const int cl = classify(b, lo, hi, hitLo, hitHi);
            if (cl == kUndecided) undecided = 1u;
            else if (cl == kHitAll) mine = childBits << bitIndex;
        }
    }
    const uint32_t hitMask = group_or(mine);
    if (group_or(undecided) != 0u) return false;
    ng = make_uint2(n1.x, (hitMask & 0xff000000u) | (e_imask >> 24));
    tg = make_uint2(n1.y, hitMask & 0x00ffffffu);
    return true;
}

// One triangle of the intersection stream (p0 | id, e0, e1: nx_device.h) against the bundle: hit by every ray (the four edge rays hit
// its plane at points whose barycentrics lie a margin inside: the pyramid's cut with the plane is their convex hull), missed by every
// ray (all four violate the same linear constraint, or the plane lies behind), or undecided.  Hit by all: [tLo, tHi] bounds the
// distance.
NXD int classify_triangle(const Bundle& b, const NX_G float4* rec, double& tLo, double& tHi)
{
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    const D3 p0{(double)r0.x, (double)r0.y, (double)r0.z}, e0{(double)r1.x, (double)r1.y, (double)r1.z}, e1{(double)r2.x, (double)r2.y, (double)r2.z};
    const D3 n = dcross(e0, e1);
    const double nn = ddot(n, n);
    if (!(nn > 0.0)) return kUndecided;
    const double rootNn = sqrt(nn);
    const double height = ddot(n, dsub(p0, b.org));
    const double mag = fabs(b.org.x) + fabs(b.org.y) + fabs(b.org.z) + fabs(p0.x) + fabs(p0.y) + fabs(p0.z);
    double u[4], v[4], t[4];
    int front = 0, behind = 0;
    for (int k = 0; k < 4; k++) {
        const double denom = ddot(n, b.dir[k]);
        if (!(fabs(denom) > 1.0e-4 * rootNn)) return kUndecided;  // grazing
        t[k] = height / denom;
        if (t[k] > 0.0) front++;
        if (t[k] < -1.0e-3 * mag) behind++;  // (clearly behind: the kernel's t cannot round to a positive value)
        const D3 q{b.org.x + t[k] * b.dir[k].x - p0.x, b.org.y + t[k] * b.dir[k].y - p0.y, b.org.z + t[k] * b.dir[k].z - p0.z};
        u[k] = ddot(dcross(q, e1), n) / nn;
        v[k] = ddot(dcross(e0, q), n) / nn;
    }
    if (behind == 4) return kMissAll;
    if (front != 4) return kUndecided;
    const double m = 2.0e-3;
    int in = 0, uLow = 0, vLow = 0, wHigh = 0;
    double lo = 1.0e300, hi = 0.0;
    for (int k = 0; k < 4; k++) {
        if (u[k] >= m && v[k] >= m && u[k] + v[k] <= 1.0 - m) in++;
        if (u[k] <= -m) uLow++;
        if (v[k] <= -m) vLow++;
        if (u[k] + v[k] >= 1.0 + m) wHigh++;
        lo = fmin(lo, t[k]);
        hi = fmax(hi, t[k]);
    }
    if (uLow == 4 || vLow == 4 || wHigh == 4) return kMissAll;
    if (in != 4) return kUndecided;
    if (!(lo > 1.0e-3 * mag)) return kUndecided;  // (a hit this close to the origin: leave it to the kernel's own t > 0)
    tLo = lo * (1.0 - 1.0e-3) - 1.0e-6 * mag;
    tHi = hi * (1.0 + 1.0e-3) + 1.0e-6 * mag;
    return kHitAll;
}

}  // namespace

// The state of run `run`, walked by the eight lanes of its group (c: this lane's place in it) and written to the run's table entry; the
// root's when a condition is not met.  The bookkeeping — stack, node group, leaf group, consumed triangle — is the same in every lane
// of the group, except that lane k holds stack entry k.
NXD void walk_run(const DeviceState* __restrict__ S, const uint32_t run, const int c, NX_G EntryState* __restrict__ out, Bundle* bundles)
{
    uint2 stk = make_uint2(0u, 0u);  // stack entry c
    uint2 ng = make_uint2(0u, 0x80000000u), tg = make_uint2(0u, 0u);
    int sp = 0, instSp = -1, leafSlot = -1, steps = 0;
    const NX_G uint4* leafNodes = nullptr;
    const NX_G float4* isect = nullptr;
    uint32_t instIdx = 0u;
    float triRec[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t triWord = 0u, triInst = 0xffffffffu, skipped = 0u;
    int triLeaf = -1;
    double hitLo = 1.0e300, hitHi = 1.0e300;  // the run's hit distances once a triangle has been consumed
    // (written on every way out: the root's state when the walk takes no step)
    const auto store = [&]() {
        if (c < kEntryMaxStack) out->stack[c] = stk;
        if (c == kGroup - 1) {
            *(NX_G uint4*)&out->ng = make_uint4(ng.x, ng.y, tg.x, tg.y);
            *(NX_G int4*)&out->sp = make_int4(sp, instSp, leafSlot, steps);
        } else if (c == kGroup - 2) {
            out->nodes = leafNodes;
            out->isect = isect;
            *(NX_G uint4*)&out->triInst = make_uint4(triInst, instIdx, __float_as_uint(hitHi < 1.0e299 ? (float)hitLo : 1e30f),
                                                      __float_as_uint(hitHi < 1.0e299 ? (float)hitHi : 1e30f));
        } else if (c == 0) {
            *(NX_G float4*)&out->triP0[0] = make_float4(triRec[0], triRec[1], triRec[2], __uint_as_float(triWord));
        } else if (c == 1) {
            *(NX_G float4*)&out->triE0[0] = make_float4(triRec[3], triRec[4], triRec[5], __int_as_float(triLeaf));
        } else if (c == 2) {
            *(NX_G float4*)&out->triE1[0] = make_float4(triRec[6], triRec[7], triRec[8], __uint_as_float(skipped));
        }
    };
    const int base = (int)(threadIdx.x & ~(unsigned)(kGroup - 1));
    const auto push = [&](const uint2 e) {
        if (c == sp) stk = e;
        sp++;
    };

    const bool walked = [&]() -> bool {
    const nx_camera cam = S->camera;
        if (cam.lensRadius != 0.0f) return false;
        // the run's pixels: their bounding rectangle, in pixels
        const uint32_t resX = cam.resolution[0], resY = cam.resolution[1];
        uint32_t imin = 0xffffffffu, imax = 0u, jmin = 0xffffffffu, jmax = 0u;
        for (uint32_t k = (uint32_t)c; k < 64u; k += kGroup) {  // (eight pixels per lane, then the group's extremes)
            const uint32_t lp = run * 64u + k;
            if (lp >= S->localCount) break;
            const uint32_t g = S->pixelMap ? S->pixelMap[lp] : lp;
            const uint32_t j = g / resX, i = g - j * resX;
            imin = min(imin, i); imax = max(imax, i); jmin = min(jmin, j); jmax = max(jmax, j);
        }
        for (int x = 1; x < kGroup; x <<= 1) {
            imin = min(imin, (uint32_t)__shfl_xor((int)imin, x)); imax = max(imax, (uint32_t)__shfl_xor((int)imax, x));
            jmin = min(jmin, (uint32_t)__shfl_xor((int)jmin, x)); jmax = max(jmax, (uint32_t)__shfl_xor((int)jmax, x));
        }
        if (imin > imax) return false;
        Bundle b;
        b.org = D3{(double)cam.position[0], (double)cam.position[1], (double)cam.position[2]};
        {
            // NaN, +-inf, -0, +-denormal.  (+0 is fine: such a ray is not "ordinary" for nx_traverse.h's enter_instance, which then takes it
            // through the identity's rows — 1 * x + 0 * y + 0 * z + 0 — and that returns x bit for bit unless x is a NEGATIVE zero)
            constexpr int kSpecial = 0x003 | 0x004 | 0x200 | 0x020 | 0x010 | 0x080;
            if (__builtin_amdgcn_classf(cam.position[0], kSpecial) || __builtin_amdgcn_classf(cam.position[1], kSpecial) || __builtin_amdgcn_classf(cam.position[2], kSpecial)) return false;
        }
        // The bundle's margin, in pixels.  generate_kernel computes a direction as (llc + vpX * x + vpY * y) - position in binary32: each
        // component carries a few roundings of its LARGEST operand — half an ulp each for the two products, the two sums and the
        // difference, so at most 8 x 2^-24 of M = max(|llc| + |vpX| + |vpY|, |position|) per component with room to spare — and that, over the
        // world-space size of a pixel on the view plane, is how far the kernel's ray can lie from the exact one through its sub-pixel position.
        // A camera near the origin: ~1e-4 pixel, the fixed 0.01 covers it (and the float x, y themselves).  A camera far from the origin with
        // a short focus distance (position ~1e3, a view plane of a few units at 4k): tenths of a pixel — the margin follows, and beyond a
        // quarter of a pixel the run starts at the root like a run that meets no other condition.
        double eps = 0.01;
        {
            double M = 0.0, px2 = 0.0, py2 = 0.0;
            for (int a = 0; a < 3; a++) {
                M = fmax(M, fmax(fabs((double)cam.lowerLeftCorner[a]) + fabs((double)cam.viewportX[a]) + fabs((double)cam.viewportY[a]), fabs((double)cam.position[a])));
                px2 += (double)cam.viewportX[a] * (double)cam.viewportX[a];
                py2 += (double)cam.viewportY[a] * (double)cam.viewportY[a];
            }
            const double pixel = fmin(sqrt(px2) / (double)resX, sqrt(py2) / (double)resY);  // world-space size of a pixel on the view plane
            if (!(pixel > 0.0)) return false;
            eps += 1.7320508 * 8.0 * 5.9604644775390625e-8 * M / pixel;
            if (!(eps <= 0.25)) return false;
        }
        const double xs[4] = {((double)imin - eps) / resX, ((double)imax + 1.0 + eps) / resX, ((double)imax + 1.0 + eps) / resX, ((double)imin - eps) / resX};
        const double ys[4] = {((double)jmin - eps) / resY, ((double)jmin - eps) / resY, ((double)jmax + 1.0 + eps) / resY, ((double)jmax + 1.0 + eps) / resY};
        b.axis = D3{0.0, 0.0, 0.0};
        for (int k = 0; k < 4; k++) {
            b.dir[k] = D3{(double)cam.lowerLeftCorner[0] + (double)cam.viewportX[0] * xs[k] + (double)cam.viewportY[0] * ys[k] - b.org.x,
                          (double)cam.lowerLeftCorner[1] + (double)cam.viewportX[1] * xs[k] + (double)cam.viewportY[1] * ys[k] - b.org.y,
                          (double)cam.lowerLeftCorner[2] + (double)cam.viewportX[2] * xs[k] + (double)cam.viewportY[2] * ys[k] - b.org.z};
            b.axis = D3{b.axis.x + b.dir[k].x, b.axis.y + b.dir[k].y, b.axis.z + b.dir[k].z};
        }
        // one octant, with a margin: every direction of the bundle is a combination of the four with non-negative weights
        uint32_t oct = 0;
        for (int a = 0; a < 3; a++) {
            const double len = sqrt(ddot(b.axis, b.axis)) * 0.25;
            int neg = 0, pos = 0;
            for (int k = 0; k < 4; k++) {
                const double c = dcomp(b.dir[k], a);
                if (c < -1.0e-6 * len) neg++;
                else if (c > 1.0e-6 * len) pos++;
            }
            if (neg != 4 && pos != 4) return false;
            if (neg == 4) oct |= (a == 0 ? 4u : (a == 1 ? 2u : 1u));
        }
        const uint32_t invOct4 = (7u - oct) * 0x01010101u;
        for (int k = 0; k < 4; k++) {  // unit edge rays from here on: parameters along them are distances, as the kernel's hit distances are
            const double len = sqrt(ddot(b.dir[k], b.dir[k]));
            b.dir[k] = D3{b.dir[k].x / len, b.dir[k].y / len, b.dir[k].z / len};
        }
        b.axis = D3{b.dir[0].x + b.dir[1].x + b.dir[2].x + b.dir[3].x, b.dir[0].y + b.dir[1].y + b.dir[2].y + b.dir[3].y, b.dir[0].z + b.dir[1].z + b.dir[2].z + b.dir[3].z};
        for (int k = 0; k < 4; k++) {
            b.plane[k] = dcross(b.dir[k], b.dir[(k + 1) & 3]);
            if (ddot(b.plane[k], b.axis) < 0.0) b.plane[k] = D3{-b.plane[k].x, -b.plane[k].y, -b.plane[k].z};
        }

        // (the bundle lives in LDS from here on, one copy per group — every lane stores the same bytes and reads its own — so that it
        //  does not hold 60 registers through the walk)
        Bundle& lb = bundles[threadIdx.x / (unsigned)kGroup];
        lb = b;
        asm volatile("" ::: "memory");
        const bool identityScene = (S->sceneFlags & kSceneAllIdentity) != 0u;
        const NX_G uint4* nodes = S->tlasNodes;
        // The traversal loop of nx_trace.hip, step by step, for the whole run at once: acquire (pop), then ONE of — a TLAS leaf (the first
        // pending instance + its BLAS's root), a triangle of a pending BLAS leaf, a node.  Every step taken has the outcome every ray
        // of the run gets; the walk stops in front of the first step it cannot decide.
        for (;;) {
            if (steps >= 12 || sp >= kEntryMaxStack - 2) break;
            if (tg.y == 0u && (ng.y & 0xff000000u) == 0u) {
                // out of work: the next stack entry (none left: the rays are finished — nothing the walk needs to say)
                if (sp == 0) break;
                if (sp == instSp) {  // leaving the (identity) instance
                    nodes = S->tlasNodes;
                    instSp = -1;
                    leafSlot = -1;
                    leafNodes = nullptr;
                    isect = nullptr;
                    instIdx = 0u;
                }
                const uint2 e = make_uint2((uint32_t)__shfl((int)stk.x, base + sp - 1), (uint32_t)__shfl((int)stk.y, base + sp - 1));
                if (c == sp - 1) stk = make_uint2(0u, 0u);
                sp--;
                if (e.y & 0xff000000u) ng = e;
                else { tg = e; ng = make_uint2(0u, 0u); }
                continue;
            }
            if (tg.y != 0u && instSp < 0) {
                // TLAS leaves: the first pending instance and its BLAS's root in one step, as the kernel takes them — through identity
                // instances only (the bundle is then the same in the BLAS's frame)
                if (!identityScene) break;
                const int off = 31 - __clz((int)tg.y);
                const uint2 rest = make_uint2(tg.x, tg.y & ~(1u << off));
                const uint32_t leaf = tg.x + (uint32_t)off;
                const NX_G InstTrav* rec = &S->instTrav[leaf];
                uint2 ng2, tg2;
                if (!group_child_trace(lb, (const NX_G uint4*)rec->root, invOct4, c, hitLo, hitHi, ng2, tg2)) break;
                if (rest.y) push(rest);
                if (ng.y & 0xff000000u) push(ng);
                instSp = sp;
                leafSlot = (int)leaf;
                ng = ng2;
                tg = tg2;
                steps++;
                nodes = leafNodes = rec->nodes;
                isect = rec->isect;
                instIdx = rec->instIdx;
                continue;
            }
            if (tg.y != 0u) {
                // the triangles of the pending leaf, in the loop's order, lane c classifying the c-th: a triangle every ray misses is
                // skipped; one every ray hits is consumed (at most one: its record goes into the state); once one is, a triangle that lies
                // behind its plane is skipped (the kernel's t < hitT fails for every ray) and any other one every ray hits ends the walk
                uint32_t pending = tg.y;
                for (int k = 0; k < c && pending != 0u; k++) pending &= ~(1u << (31 - __clz((int)pending)));
                int cls = kUndecided;
                double tLo = 0.0, tHi = 0.0;
                if (pending != 0u) {
                    const NX_G float4* r = isect + (size_t)(tg.x + (uint32_t)(31 - __clz((int)pending))) * (unsigned)kTriStride;
                    cls = classify_triangle(lb, r, tLo, tHi);
                    if (triLeaf >= 0) {  // (its bounding box behind the consumed triangle's plane)
                        const float4 r0 = r[0], r1 = r[1], r2 = r[2];
                        const double v0[3] = {(double)r0.x, (double)r0.y, (double)r0.z};
                        const double v1[3] = {v0[0] + (double)r1.x, v0[1] + (double)r1.y, v0[2] + (double)r1.z};
                        const double v2[3] = {v0[0] + (double)r2.x, v0[1] + (double)r2.y, v0[2] + (double)r2.z};
                        const double lo[3] = {fmin(v0[0], fmin(v1[0], v2[0])), fmin(v0[1], fmin(v1[1], v2[1])), fmin(v0[2], fmin(v1[2], v2[2]))};
                        const double hi[3] = {fmax(v0[0], fmax(v1[0], v2[0])), fmax(v0[1], fmax(v1[1], v2[1])), fmax(v0[2], fmax(v1[2], v2[2]))};
                        if (behind_hit_plane(lb, lo, hi)) cls = kMissAll;
                    }
                }
                bool stop = false;
                for (int k = 0; k < kGroup && tg.y != 0u; k++) {
                    int ck = __shfl(cls, base + k);
                    const double lk = __shfl(tLo, base + k), hk = __shfl(tHi, base + k);
                    const int off = 31 - __clz((int)tg.y);
                    if (ck == kHitAll && triLeaf >= 0) ck = kUndecided;
                    if (ck == kUndecided) { stop = true; break; }
                    tg.y &= ~(1u << off);
                    if (ck != kHitAll) {
                        skipped++;
                        continue;
                    }
                    const NX_G float4* r = isect + (size_t)(tg.x + (uint32_t)off) * (unsigned)kTriStride;
                    const float4 r0 = r[0], r1 = r[1], r2 = r[2];
                    triRec[0] = r0.x; triRec[1] = r0.y; triRec[2] = r0.z;
                    triRec[3] = r1.x; triRec[4] = r1.y; triRec[5] = r1.z;
                    triRec[6] = r2.x; triRec[7] = r2.y; triRec[8] = r2.z;
                    triWord = __float_as_uint(r0.w);
                    triLeaf = leafSlot;
                    triInst = instIdx;
                    hitLo = lk;  // (a ray's hit distance after the test: this one — it had none before)
                    hitHi = hk;
                    // its plane, for the boxes and triangles behind it: every ray's hit lies on it, within rounding, so whatever lies behind
                    // it by a thousandth of the hit distance is entered — if at all — behind the hit
                    const D3 q0{(double)r0.x, (double)r0.y, (double)r0.z};
                    D3 n = dcross(D3{(double)r1.x, (double)r1.y, (double)r1.z}, D3{(double)r2.x, (double)r2.y, (double)r2.z});
                    const double len = sqrt(ddot(n, n)) * (ddot(n, dsub(lb.org, q0)) > 0.0 ? -1.0 : 1.0);  // (pointing away from the apex)
                    lb.hitN = D3{n.x / len, n.y / len, n.z / len};
                    lb.hitC = ddot(lb.hitN, q0);
                    lb.hitGap = 1.0e-3 * hk + 1.0e-5 * (fabs(lb.org.x) + fabs(lb.org.y) + fabs(lb.org.z) + fabs(q0.x) + fabs(q0.y) + fabs(q0.z));
                    asm volatile("" ::: "memory");
                    break;  // (the rest of the leaf is classified again against the plane)
                }
                if (stop) break;
                continue;
            }
            // a node: the next child of the node group
            uint2 cur = ng;
            const int nodeOffset = 31 - __clz((int)cur.y);
            cur.y &= ~(1u << nodeOffset);
            const int slot = (nodeOffset - 24) ^ (int)(invOct4 & 7u);
            const int rel = __popc(cur.y & ~(0xffffffffu << slot));
            uint2 ng2, tg2;
            if (!group_child_trace(lb, nodes + (size_t)(cur.x + (uint32_t)rel) * (unsigned)kNodeStride, invOct4, c, hitLo, hitHi, ng2, tg2)) break;
            if (cur.y & 0xff000000u) push(cur);
            ng = ng2;
            tg = tg2;
            steps++;
        }
        return true;
    }();
    (void)walked;
    store();
}

// Eight lanes per run, eight runs per workgroup.  The table is the SLOT's own (DeviceState::entry / entryRuns of the slot on whose
// stream this launch is issued — a plain launch, no node of the pass graph): written here, read by the primary closest-hit launches
// of the slot's passes behind it in stream order, by nobody else.
__global__ void __launch_bounds__(64) entry_state_kernel(const DeviceState* __restrict__ S)
{
    const uint32_t run = (blockIdx.x * blockDim.x + threadIdx.x) / (unsigned)kGroup;
    if (run >= S->entryRuns || S->entry == nullptr) return;  // (the whole group: its lanes share the run)
    __shared__ Bundle bundles[64 / kGroup];
    walk_run(S, run, (int)(threadIdx.x & (unsigned)(kGroup - 1)), S->entry + run, bundles);
}

const void* entry_state_kernel_ptr() { return (const void*)entry_state_kernel; }

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_entry() { return layout_stamp(); }

}  // namespace nxd
