"""Hand-made BVH8 trees for the traversal tests: the host builders' trees keep a ray's stack at a handful of entries, so the
scratch half of the kernels' stack (entries kLdsDepth .. 31 of nx_traverse.h) and its 32-entry limit are reached with CHAINS instead.

A traversal pushes an entry when two or more inner children of one node are hit (or at a TLAS leaf with instances left over).  A
chain node has exactly two inner children: a "stub" — a node with one leaf slot — over one slab of z, and the rest of the chain over
the slabs behind it.  Which of the two a ray visits first is decided by the octant permutation: hit bit 24 + (slot ^ (7 - octant)),
highest bit first, the octant taken from the WORLD direction also inside an instance.  Slots 0 and 1 differ in bit 0 of that index,
which follows the sign of the direction's z alone.  With the stub in slot 0 a ray going down (-z) takes the rest first and leaves
the stub on its stack, level after level: D levels give a stack of exactly D - 1 entries, and the stub of level i is the entry at
stack position i.  The same ray going up visits the stub first and never holds more than one entry.  `deep=+1` swaps the slots and
with them the directions.

The node layout is include/nexus_pod.h's nx_bvh8_node (pod.NODE_DT); what the kernels require of a node array is
nxhip_scene.hip's wide_node_defect, and `check_nodes` below restates it."""
import ctypes as C
import math

import numpy as np

from nexus_amd import capi, pod
from tests import oracle_lib as O
from tests import scene_helpers as SH

CHAIN_P = (-1.0, -1.0, 0.0)   # frame of every chain BLAS node: x, y in [-1, 1] = q 0 .. 128 at 2^-6,
CHAIN_E = (121, 121, 120)     # z at 2^-7: one level is 4 steps = 1 / 32
COARSE_E = (121, 121, 122)    # z at 2^-5: one level is one step (towers of many chains in one frame)
LEVEL_DZ = 1.0 / 32.0


def _scale(e):
    return np.array([np.array([int(x) << 23], np.uint32).view(np.float32)[0] for x in e], np.float64)


def encode_node(p, e, slots, child_base=0, prim_base=0):
    """One 80-byte node.  p: grid origin (3 floats); e: biased exponents of the grid step per axis; slots: up to 8 entries,
    None (empty), ("inner", lo, hi) or ("leaf", offset, count, lo, hi) — boxes as floats, quantised outwards (floor / ceil) on the
    node's grid; offset / count: the leaf's primitives are prim_base + offset ... + count - 1 (count 1 .. 3).  The k-th inner slot in
    slot order is node child_base + k."""
    assert len(slots) <= 8
    n = np.zeros((), dtype=pod.NODE_DT)
    n["p"] = p
    n["e"] = e
    n["childBaseIdx"] = child_base
    n["triangleBaseIdx"] = prim_base
    p64, sc = np.asarray(n["p"], np.float64), _scale(e)
    imask = 0
    for s, slot in enumerate(slots):
        if slot is None:
            continue
        lo, hi = (np.asarray(b, np.float64) for b in slot[-2:])
        qlo, qhi = np.floor((lo - p64) / sc), np.ceil((hi - p64) / sc)
        assert np.all(qlo >= 0) and np.all(qhi <= 255) and np.all(qlo <= qhi), "box outside the node's grid: %r" % (slot,)
        for axis, name in enumerate("xyz"):
            n["qlo" + name][s] = int(qlo[axis])
            n["qhi" + name][s] = int(qhi[axis])
        if slot[0] == "inner":
            imask |= 1 << s
            n["meta"][s] = 0x20 | (24 + s)
        else:
            _kind, offset, count = slot[:3]
            assert 1 <= count <= 3 and 0 <= offset and offset + count <= 24
            n["meta"][s] = (((1 << count) - 1) << 5) | offset
    n["imask"] = imask
    return n


def check_nodes(nodes, prim_count):
    """what the device asks of a node array before it takes it (children in range and behind their parent, leaf ranges inside the
    primitive list, inner slots announced in imask)"""
    for i, n in enumerate(nodes):
        inner = bin(int(n["imask"])).count("1")
        prims = 0
        for s in range(8):
            m = int(n["meta"][s])
            if (m & 0x18) == 0x18 and (m >> 5):
                assert n["imask"] & (1 << s) and (m >> 5) == 1 and (m & 7) == s
            elif m >> 5:
                top = (m >> 5).bit_length()
                assert (m & 0x1F) + top <= 24
                prims = max(prims, (m & 0x1F) + top)
        assert not inner or (int(n["childBaseIdx"]) > i and int(n["childBaseIdx"]) + inner <= len(nodes))
        assert not prims or int(n["triangleBaseIdx"]) + prims <= prim_count


def chain_triangles(D, seed, per_level=1, first_level=0):
    """per_level triangles for each of D levels (per_level > 1: coincident copies — every hit then has a twin at exactly its
    distance).  Level i's lie inside the slab z in [(first_level + i) / 32, (first_level + i + 1) / 32], each with a position, size
    (edge 0.3 .. 0.8), orientation and tilt of its own, inside |x|, |y| < 0.95.  Triangle k belongs to level k // per_level."""
    rng = np.random.RandomState(seed)
    pos = np.zeros((D * per_level, 3, 3), np.float64)
    for i in range(D):
        c = rng.uniform(-0.45, 0.45, 2)
        r = rng.uniform(0.3, 0.8) / math.sqrt(3.0)
        th = rng.uniform(0.0, 2.0 * math.pi)
        for k in range(3):
            a = th + 2.0 * math.pi * k / 3.0
            pos[i * per_level:(i + 1) * per_level, k] = (c[0] + r * math.cos(a), c[1] + r * math.sin(a), (first_level + i + rng.uniform(0.2, 0.8)) * LEVEL_DZ)
    return pod.make_triangles(pos.astype(np.float32))


def chain_blas(D, seed, per_level=1, deep=-1, first_level=0, fine=True):
    """(nodes, triangles, triIdx) of a chain of D levels: 2 D - 1 nodes, D * per_level triangles.  Chain node i has the stub of level i
    (one leaf slot: that level's triangles) and the rest of the chain as its two inner children; the last chain node holds level D - 1
    as a leaf of its own.  deep = -1: the stub sits in slot 0, rays with direction z < 0 reach a stack of D - 1 and rays going up 1;
    deep = +1: the stub sits in slot 1 and it is the other way round.  Chain node 0 is node 0, the children of chain node i are nodes
    2 i + 1 and 2 i + 2 in slot order.  The chain starts at slab `first_level` of the frame; fine: the z grid has four steps per level
    (CHAIN_E; 63 levels fit), otherwise one (255 levels fit) — the levels are 1 / 32 apart either way."""
    e = CHAIN_E if fine else COARSE_E
    per = 4 if fine else 1
    assert D >= 1 and 1 <= per_level <= 3 and deep in (-1, 1) and per * (first_level + D) <= 255
    tris = chain_triangles(D, seed, per_level, first_level)

    def box(l0, l1):
        return ((-1.0, -1.0, (first_level + l0) * LEVEL_DZ), (1.0, 1.0, (first_level + l1) * LEVEL_DZ))

    def leaf_node(i):
        return encode_node(CHAIN_P, e, [("leaf", 0, per_level) + box(i, i + 1)], prim_base=i * per_level)

    out = [None] * (2 * D - 1)
    at = 0
    for i in range(D - 1):
        base = 2 * i + 1
        stub, rest = ("inner",) + box(i, i + 1), ("inner",) + box(i + 1, D)
        out[at] = encode_node(CHAIN_P, e, [stub, rest] if deep < 0 else [rest, stub], child_base=base)
        stub_at, at = (base, base + 1) if deep < 0 else (base + 1, base)
        out[stub_at] = leaf_node(i)
    out[at] = leaf_node(D - 1)
    nodes = np.array(out, dtype=pod.NODE_DT)
    check_nodes(nodes, len(tris))
    return nodes, tris, np.arange(len(tris), dtype=np.uint32)


def chain_tlas(instances, T):
    """(nodes, instIdx) of a TLAS chain of T levels over `instances` (pod.INST_DT, at least T of them): level i < T - 1 is a stub
    whose leaf slot holds instance i, the last chain node holds all remaining instances in leaf slots of up to three.  Boxes are the
    instances' world bounds, the rest-of-chain boxes their unions; one frame for all nodes.  A ray that goes down (-z) through all
    of them enters the last level's first instance with a stack of T - 1 entries — one more if the last node holds two or more —
    and the instance of level i with i."""
    instances = np.ascontiguousarray(instances, dtype=pod.INST_DT)
    n = len(instances)
    assert 1 <= T <= n and n - (T - 1) <= 24
    lo, hi = instances["boundsMin"].astype(np.float64), instances["boundsMax"].astype(np.float64)
    p = np.floor(lo.min(0) * 8.0) / 8.0 - 0.125
    ext = hi.max(0) - p
    e = [127 + int(math.ceil(math.log2(x / 255.0))) for x in ext * 1.01]
    rest_lo = np.minimum.accumulate(lo[::-1], 0)[::-1]  # union of instances i ..
    rest_hi = np.maximum.accumulate(hi[::-1], 0)[::-1]
    nodes = []
    for i in range(T - 1):
        nodes.append(encode_node(p, e, [("inner", lo[i], hi[i]), ("inner", rest_lo[i + 1], rest_hi[i + 1])], child_base=2 * i + 1))
        nodes.append(encode_node(p, e, [("leaf", 0, 1, lo[i], hi[i])], prim_base=i))
    slots = []
    for first in range(T - 1, n, 3):
        last = min(first + 3, n)
        slots.append(("leaf", first - (T - 1), last - first, lo[first:last].min(0), hi[first:last].max(0)))
    nodes.append(encode_node(p, e, slots, prim_base=T - 1))
    arr = np.array(nodes, dtype=pod.NODE_DT)
    check_nodes(arr, n)
    return arr, np.arange(n, dtype=np.uint32)


class CraftedScene(SH.BuiltScene):
    """A scene of crafted BLASes (as chain_blas returns them) and placements (blas, material, transform16), for the oracle and the
    device alike.  tlas_levels None: the product's TLAS builder; a number: chain_tlas of that many levels."""

    def __init__(self, blas, placements, tlas_levels=None, materials=None, lights=None, camera=None, settings=None):
        self.blas = [(np.ascontiguousarray(n, pod.NODE_DT), np.ascontiguousarray(t, pod.TRI_DT), np.ascontiguousarray(i, np.uint32)) for n, t, i in blas]
        self.meshes = [b[1] for b in self.blas]
        self.instances = np.array([capi.instance_init(m, mat, xf, self.blas[m][0][0]) for m, mat, xf in placements], dtype=pod.INST_DT)
        if tlas_levels is None:
            self.tlas_nodes, self.tlas_idx = capi.tlas_build(self.instances)
        else:
            self.tlas_nodes, self.tlas_idx = chain_tlas(self.instances, tlas_levels)
        self.materials = np.ascontiguousarray(materials if materials is not None else np.array([pod.make_material()], dtype=pod.MAT_DT), dtype=pod.MAT_DT)
        self.lights = np.ascontiguousarray(lights if lights is not None else np.zeros(0, pod.LIGHT_DT), dtype=pod.LIGHT_DT)
        self.camera = camera
        self.settings = settings if settings is not None else SH.workloads.make_settings()
        self.diffuse_maps, self.emissive_maps, self.hdr_map = [], [], None
        self.env_sampling = False

    def variant(self, **changed):
        """the same scene with some attributes replaced (a shallow copy)"""
        other = CraftedScene.__new__(CraftedScene)
        other.__dict__.update(self.__dict__)
        other.__dict__.update(changed)
        return other


def chain_scene(D, seed, per_level=1, deep=-1):
    """one chain BLAS under one identity instance, TLAS from the product's builder"""
    return CraftedScene([chain_blas(D, seed, per_level, deep)], [(0, 0, SH.IDENTITY)])


def without_levels(scene, first_level, per_level=1):
    """the scene with the triangles of BLAS 0's STUB levels >= first_level made zero-area (all three vertices in one point, still
    inside their slab: no ray hits them) — what is left of the chain for a ray whose pushes from stack position first_level on were
    dropped.  The last level is no stub (the last chain node's own leaf) and stays."""
    nodes, tris, idx = scene.blas[0]
    tris = tris.copy()
    D = len(tris) // per_level
    dead = slice(first_level * per_level, (D - 1) * per_level)
    tris["pos1"][dead] = tris["pos0"][dead]
    tris["pos2"][dead] = tris["pos0"][dead]
    return scene.variant(blas=[(nodes, tris, idx)] + list(scene.blas[1:]), meshes=[tris] + list(scene.meshes[1:]))


def world_triangle_points(scene, n, rng, favour_from=8):
    """n points inside triangles of the scene in world space (random instance, random triangle, random barycentrics).  Triangles of
    stub levels >= favour_from — the ones whose stack entry lives beyond the kernels' LDS part — are drawn at least three times as
    often as the others, and often enough to make up 60 % of the points."""
    out = np.zeros((n, 3), np.float64)
    which = rng.randint(0, len(scene.instances), n)
    for k, inst in enumerate(scene.instances):
        sel = np.flatnonzero(which == k)
        nodes, tris, _idx = scene.blas[int(inst["bvhIdx"])]
        level = np.arange(len(tris)) // (len(tris) // ((len(nodes) + 1) // 2))  # (2 D - 1 nodes, D levels, triangles in level order)
        far = (level >= favour_from) & (level < level.max())
        w = np.where(far, max(3.0, 1.5 * (~far).sum() / max(1, far.sum())), 1.0)  # (at least 60 % of the points where there are any)
        t = rng.choice(len(tris), size=len(sel), p=w / w.sum())
        a, b = rng.uniform(0, 1, len(sel)), rng.uniform(0, 1, len(sel))
        flip = a + b > 1
        a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
        p = (tris["pos0"][t].astype(np.float64) * (1 - a - b)[:, None] + tris["pos1"][t].astype(np.float64) * a[:, None]
             + tris["pos2"][t].astype(np.float64) * b[:, None])
        M = np.asarray(inst["transform"], np.float64).reshape(4, 4)
        out[sel] = p @ M[:3, :3].T + M[:3, 3]
    return out


def mixed_rays(scene, n, seed, shares=(0.5, 0.3, 0.2), slope=0.05, favour_from=8):
    """n rays for a crafted scene: `shares` of them from above going down (direction about (+-slope, +-slope, -1)), from below going up, and
    beside the scene (they miss the TLAS root) — shuffled, so that every wave holds all three kinds.  The first two are aimed at
    points inside triangles, most of them of stub levels >= favour_from (world_triangle_points)."""
    rng = np.random.RandomState(seed)
    z_lo = float(scene.instances["boundsMin"][:, 2].min()) - 1.0
    z_hi = float(scene.instances["boundsMax"][:, 2].max()) + 1.0
    x_side = float(scene.instances["boundsMax"][:, 0].max()) + 3.0
    n_down, n_up = int(n * shares[0]), int(n * shares[1])
    target = world_triangle_points(scene, n, rng, favour_from)
    d = np.zeros((n, 3), np.float64)
    d[:, :2] = rng.uniform(0.4 * slope, 1.6 * slope, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    d[:, 2] = -1.0
    d[n_down:n_down + n_up, 2] = 1.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    z0 = np.where(d[:, 2] < 0, z_hi, z_lo)
    o = target - d * ((target[:, 2] - z0) / d[:, 2])[:, None]
    o[n_down + n_up:, 0] += x_side + 2.0
    rays = np.zeros(n, dtype=pod.RAY_DT)
    rays["origin"], rays["direction"] = o.astype(np.float32), d.astype(np.float32)
    return rays[rng.permutation(n)]


def per_ray_stats(orc, rays, any_tmax=None):
    """the oracle's counts (tests.oracle_lib.TraceStats) of every single ray — closest hit, or any hit within any_tmax[i] —: a dict of
    arrays "maxStack", "nodes", "tris", "instances".  nodes + tris is the number of loop iterations the device's kernels spend on the ray
    (one record per iteration; an instance entry shares its iteration with the BLAS root)."""
    rays = np.ascontiguousarray(rays, dtype=pod.RAY_DT)
    L = O.lib()
    keys = ("maxStack", "nodes", "tris", "instances")
    out = {k: np.zeros(len(rays), np.int32) for k in keys}
    scene = C.byref(orc.c)
    base, step = rays.ctypes.data, rays.dtype.itemsize
    hit = np.zeros(1, dtype=pod.HIT_DT)
    occ = np.zeros(1, dtype=np.uint8)
    hit_p, occ_p = C.c_void_p(hit.ctypes.data), C.c_void_p(occ.ctypes.data)
    if any_tmax is not None:
        any_tmax = np.ascontiguousarray(any_tmax, dtype=np.float32)
        tbase = any_tmax.ctypes.data
    for i in range(len(rays)):
        st = O.TraceStats()
        if any_tmax is None:
            L.orc_trace_closest(scene, C.c_void_p(base + i * step), 1, hit_p, C.byref(st))
        else:
            L.orc_trace_any(scene, C.c_void_p(base + i * step), C.c_void_p(tbase + 4 * i), 1, occ_p, C.byref(st))
        for k in keys:
            out[k][i] = getattr(st, k)
    return out


def per_ray_stack(orc, rays, any_tmax=None):
    """the oracle's maxStack of every single ray: closest hit, or any hit within any_tmax[i]"""
    return per_ray_stats(orc, rays, any_tmax)["maxStack"]


def shadow_tmax(closest, seed):
    """any-hit limits for a batch with known closest hits, a third each: just short of the hit, just beyond it, and 10 (beyond the
    scene: no box is culled by the limit and the stack grows as for the closest hit); 10 for the rays that miss"""
    rng = np.random.RandomState(seed)
    factor = rng.choice([0.999, 1.001, 0.0], len(closest))
    return np.where((closest["hitDistance"] < 1e29) & (factor > 0.0), closest["hitDistance"] * factor, 10.0).astype(np.float32)


def tower_scene(T, depths, last=1, mixed=True, seed=1, deep=None, **scene_kw):
    """T - 1 + last instances of chain BLASes under a chain_tlas of T levels.  depths[i]: the levels of instance i's BLAS, bottom
    first; every BLAS occupies slabs of its own above the one before it in ONE frame, so that identity placements stack them along z.
    mixed False: every instance is the identity (the device's scene-wide flag is set); True: every second one is rotated about z, tilted
    by a few degrees, scaled and shifted instead.  deep[i]: +1 for a BLAS that is deep for rays going up.  scene_kw: CraftedScene's.
    material_of(i) in scene_kw: instance i's material."""
    assert len(depths) == T - 1 + last
    rng = np.random.RandomState(seed)
    material_of = scene_kw.pop("material_of", lambda i: 0)
    blas, placements, first = [], [], 0
    for i, D in enumerate(depths):
        blas.append(chain_blas(D, seed + 10 * i, deep=deep[i] if deep else -1, first_level=first, fine=False))
        first += D
        xf = SH.IDENTITY
        if mixed and i % 2 == 1:
            xf = capi.mat4_from_trs((rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(-0.01, 0.01)),
                                    (rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(0, 360)), (rng.uniform(0.85, 1.0), rng.uniform(0.85, 1.0), 1.0))
        placements.append((i, material_of(i), xf))
    return CraftedScene(blas, placements, tlas_levels=T, **scene_kw)


# ---- the cases of tests/test_gpu_deep_stack.py; tests/test_bvh_craft.py checks the same scenes and rays on the CPU

CHAIN_LEVELS = (8, 9, 10, 17, 32, 33)   # single chains of D levels: stack depth D - 1 = 7 (the last LDS entry), 8 (the first spilled one), ... 31, 32
LIMIT_LEVELS = (34, 40)                 # chains whose 33rd and later pushes the kernels drop
TOWERS = {"instSp 7": (8, 1, 26), "instSp 8": (8, 2, 25), "instSp 9": (10, 1, 24), "instSp 20": (21, 1, 13)}  # T, last, D of the top two BLASes
_cache = {}


def chain_case(D, per_level=1):
    """(scene, 20 000 mixed rays) of the single-chain case of D levels"""
    key = ("chain", D, per_level)
    if key not in _cache:
        scene = chain_scene(D, seed=100 + D, per_level=per_level)
        _cache[key] = (scene, mixed_rays(scene, 20000, seed=D))
    return _cache[key]


def limit_case(D):
    """(scene, 20 000 mixed rays) of a chain deeper than the kernels' stack; most rays are aimed at the levels whose pushes are dropped"""
    key = ("limit", D)
    if key not in _cache:
        scene = chain_scene(D, seed=100 + D)
        _cache[key] = (scene, mixed_rays(scene, 20000, seed=D, favour_from=32))
    return _cache[key]


def tower_case(name, mixed):
    """(scene, 12 000 mixed rays): a TLAS chain whose top instance is entered with `name`'s stack depth, over BLAS chains that take the
    rays that go down to 32 entries in the top instance and 31 in the one below; the lower levels hold chains of 6 levels"""
    key = ("tower", name, mixed)
    if key not in _cache:
        T, last, D = TOWERS[name]
        scene = tower_scene(T, [6] * (T + last - 3) + [D, D], last, mixed, seed=T + last)
        _cache[key] = (scene, mixed_rays(scene, 12000, seed=T, slope=0.01))
    return _cache[key]


def frame_scene(W, H, mixed, path_length=4):
    """A tower that renders: T = 10, seen from above (the primary rays go down: deep in the TLAS and in the BLASes), diffuse
    materials, the bottom instance emissive (the shadow rays go down as well), a background that lights what looks up.  Rays that
    bounce off a triangle go up, and up the TLAS chain and an ordinary chain BLAS are shallow whatever the instance's transform — the
    octant order follows the world direction — so every third BLAS has its stub in the other slot (deep = +1)."""
    T, D = 10, 24
    n = T
    depths = [8] * (n - 2) + [D, D]
    deep = [+1 if i % 3 == 1 else -1 for i in range(n - 2)] + [-1, -1]
    mats = np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(0.8, 0.8, 0.8), emissive=(1.0, 0.9, 0.8), intensity=30.0),
                     pod.make_material(pod.MAT_DIFFUSE, albedo=(0.75, 0.7, 0.65)), pod.make_material(pod.MAT_DIFFUSE, albedo=(0.3, 0.6, 0.8)),
                     pod.make_material(pod.MAT_DIFFUSE, albedo=(0.8, 0.4, 0.3))], dtype=pod.MAT_DT)
    z_top = sum(depths) * LEVEL_DZ
    cam = capi.camera_init((0.02, -0.03, z_top + 7.0), (0.0, 0.0, -1.0), 14.0, W, H, 5.0, 0.0)
    settings = SH.workloads.make_settings(use_mis=True, path_length=path_length, background=(0.7, 0.8, 1.0), background_intensity=0.6)
    scene = tower_scene(T, depths, 1, mixed, seed=77, deep=deep, materials=mats, camera=cam, settings=settings, material_of=lambda i: 0 if i == 0 else 1 + i % 3)
    scene.lights = SH.mesh_lights(scene.instances, scene.materials)
    return scene
