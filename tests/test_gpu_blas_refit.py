"""Deforming meshes on the device (nxhip_update_blas / nxhip_update_blas_device): new vertices for an existing BLAS — triangles,
intersection stream and nodes redone in HBM, then everything that embeds the BLAS's root (instance bounds, traversal records,
TLAS) before the next call that needs the scene.

The byte reference is the host's refit (nxh_bvh8_refit; tests/test_blas_refit.py pins it against the builder and against
geometry), BVHInstance::SetTransform's bounds and nxh_tlas_refit.  Hits are compared with the oracle walking that host-refitted
scene (bit for bit) and, on the clear rays, with float64 geometry built from the deformed triangles alone
(tests/geometry_reference.py, bars of tests/test_geometry_pins.py).  The meshes are the wavy grids of tests/deform_meshes.py; the
last deformation is 3.5 x the base amplitude, outside the old root box: a stale root copy, stale instance bounds or a stale TLAS
lose hits.  m = 100 has a level of 1 374 nodes (its own grid launch) above four narrow ones (one workgroup); m = 40 is narrow
throughout."""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen
from tests import deform_meshes as D
from tests import geometry_reference as G
from tests import oracle_lib as O
from tests import scene_helpers as SH
from tests.test_geometry_pins import BOUND, MAX_UNCLEAR, T_MIN

pytestmark = pytest.mark.gpu

PLACED = capi.mat4_from_trs((0.1, -0.2, 0.05), (20, 35, 10), (1.2, 0.8, 1.1))
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _one_mesh(m):
    """(scene with the base grid placed once, the host's answer after the largest deformation)"""
    def make():
        scene = SH.BuiltScene([D.base_grid(m)], [(0, 0, PLACED)])
        return scene, D.host_deformed(scene, {0: D.deformed_grid(m)})

    return _cached(("one", m), make)


def _levels(nodes):
    return np.bincount(D.node_depths(nodes)).tolist()


# ---- bytes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", D.SIZES)
def test_updated_nodes_equal_the_host_refit(gpu_ctx_factory, m):
    scene, after = _one_mesh(m)
    nodes, tris, idx = scene.blas[0]
    if m == 100:
        assert max(_levels(nodes)) > 1024 and sum(w <= 1024 for w in _levels(nodes)) >= 2, "both launch shapes"
    ctx = gpu_ctx_factory(64, 64)
    ctx.clear_blas()
    bid = ctx.upload_blas(nodes, tris, idx)
    for shape in range(len(D.SHAPES)):  # one after the other: each refit starts from the previous one's nodes
        moved = D.deformed_grid(m, shape)
        ctx.update_blas(bid, moved)
        got, got_idx = ctx.read_blas(bid, len(tris))
        assert np.array_equal(got_idx, idx)
        assert got.tobytes() == capi.bvh8_refit(nodes, idx, moved).tobytes(), "shape %d" % shape
    assert got.tobytes() == after.blas[0][0].tobytes()
    ctx.update_blas(bid, tris)  # ... and back: the builder's bytes
    assert ctx.read_blas(bid, len(tris))[0].tobytes() == nodes.tobytes()


@pytest.mark.parametrize("builder", [-1, 0, 16])  # NXHIP_BUILDER_SAH, radix tree, clustering
def test_device_built_trees_refit_to_the_host_bytes(gpu_ctx_factory, builder):
    m = 40
    tris, moved = D.base_grid(m), D.deformed_grid(m)
    ctx = gpu_ctx_factory(64, 64)
    ctx.clear_blas()
    ctx.set_device_builder(builder)
    bid = ctx.build_blas(tris)
    ctx.set_device_builder(-1)
    before, idx = ctx.read_blas(bid, len(tris))
    print("builder %d: %d nodes, levels %s, children before parents: %s" % (
        builder, len(before), _levels(before), bool(np.any(before["childBaseIdx"][before["imask"] != 0] <= np.flatnonzero(before["imask"] != 0)))))
    ctx.update_blas(bid, moved)
    got, got_idx = ctx.read_blas(bid, len(tris))
    assert np.array_equal(got_idx, idx)
    assert got.tobytes() == capi.bvh8_refit(before, idx, moved).tobytes()
    assert got.tobytes() != before.tobytes()


def test_one_mesh_of_a_batch_pool_is_refitted_and_its_neighbours_stay(gpu_ctx_factory):
    m = 40
    meshes = [scenegen.displaced_torus(32, 16, seed=2, major=0.5, minor=0.2), D.base_grid(m), scenegen.random_soup(500, seed=3, extent=0.5, size=0.1)]
    ctx = gpu_ctx_factory(64, 64)
    ctx.clear_blas()
    ctx.set_device_builder(-1)
    ids = ctx.build_blas_batch(meshes)
    before = ctx.read_blas_batch(ids[0], [len(t) for t in meshes])
    moved = D.deformed_grid(m)
    ctx.update_blas(ids[1], moved)
    after = ctx.read_blas_batch(ids[0], [len(t) for t in meshes])
    assert after[1][0].tobytes() == capi.bvh8_refit(before[1][0], before[1][1], moved).tobytes()
    assert after[1][0].tobytes() != before[1][0].tobytes()
    for k in (0, 2):
        assert after[k][0].tobytes() == before[k][0].tobytes() and np.array_equal(after[k][1], before[k][1]), "mesh %d of the pool" % k
    # the pooled triangles and streams too: the neighbours trace as before, the updated mesh like a fresh upload
    insts = np.array([capi.instance_init(k, 0, capi.mat4_from_trs((1.5 * (k - 1), 0, 0)), after[k][0][0]) for k in range(3)], dtype=pod.INST_DT)
    tlas = capi.tlas_build(insts)
    ctx.set_tlas(tlas[0], tlas[1], insts)
    ctx.set_materials(np.array([pod.make_material()], dtype=pod.MAT_DT))
    rays = D.rays_for(20000, 5, extent=2.0)
    want = O.OracleScene([(after[0][0], meshes[0], after[0][1]), (after[1][0], moved, after[1][1]), (after[2][0], meshes[2], after[2][1])], insts, tlas[0], tlas[1])
    assert SH.hit_records_equal(ctx.trace_batch(rays), want.trace_closest(rays))


# ---- hits ------------------------------------------------------------------------------------------------------------------------

def _conditioned(world, drawn, keep):
    """the first `keep` of the drawn rays whose float64 answer is a miss or a hit at T_MIN or beyond (the condition under which
    tests/test_geometry_pins.py measured its bounds), and those answers"""
    ref = world.closest(drawn)
    sel = np.flatnonzero(ref["t"] >= T_MIN)[:keep]
    assert len(sel) == keep
    return drawn[sel], {k: v[sel] for k, v in ref.items()}


def _world(m):
    """float64 geometry of the deformed grid under PLACED and 2 000 well-conditioned rays with their answers"""
    def make():
        world = G.World([D.deformed_grid(m)], [0], np.array([PLACED]))
        return (world,) + _conditioned(world, D.rays_for(3000, 41), 2000)

    return _cached(("world", m), make)


def _check_against_geometry(got, ref, what):
    clear = ~ref["unclear"]
    got_hit = got["hitDistance"] < pod.MISS_DISTANCE
    sel = clear & ref["hit"] & got_hit
    share = float(ref["unclear"].sum()) / max(1, int(ref["hit"].sum()))
    et = float(np.max(np.abs(got["hitDistance"][sel].astype(np.float64) - ref["t"][sel]) / ref["t"][sel]))
    print("%s: %d rays, %d hits, unclear %.4f of the hits; hit/miss differs on %d clear rays, triangle on %d; hitDistance %.3g relative (bound %.3g)" % (
        what, len(got), int(ref["hit"].sum()), share, int((got_hit != ref["hit"])[clear].sum()),
        int((got["triIdx"].astype(np.int64) != ref["tri"])[sel].sum()), et, BOUND["ordinary"]["t"]))
    assert share <= MAX_UNCLEAR
    assert ref["hit"].mean() > 0.2
    assert np.array_equal(got_hit[clear], ref["hit"][clear])
    assert np.array_equal(got["triIdx"][sel].astype(np.int64), ref["tri"][sel])
    assert et <= BOUND["ordinary"]["t"]


@pytest.mark.parametrize("thin", [False, True])
def test_hits_after_an_update_equal_the_oracle_and_geometry(gpu_ctx_factory, thin):
    m = 40
    scene, after = _one_mesh(m)
    ctx = gpu_ctx_factory(64, 64)
    scene.upload(ctx)
    if thin:
        ctx.debug_set_thin(lanes=64, iters=0, in_hooks=True)
    rays = D.rays_for(20000, 7)
    orc = after.oracle()
    want = _cached("want closest", lambda: orc.trace_closest(rays))
    before = ctx.trace_batch(rays)
    assert SH.hit_records_equal(before, _cached("base closest", lambda: scene.oracle().trace_closest(rays)))
    ctx.update_blas(0, after.blas[0][1])
    got = ctx.trace_batch(rays)
    assert SH.hit_records_equal(got, want)
    assert not SH.hit_records_equal(got, before)
    if thin:
        assert ctx.debug_thin_counts()[0] > 0, "no ray reached the thin kernel"
    rng = np.random.RandomState(9)
    hit = want["hitDistance"] < pod.MISS_DISTANCE
    tmax = (np.where(hit, want["hitDistance"], rng.uniform(1.0, 6.0, len(rays))) * rng.uniform(0.5, 1.5, len(rays))).astype(np.float32)
    occ = ctx.trace_shadow_batch(rays, tmax)
    want_occ = _cached("want any", lambda: orc.trace_any(rays, tmax))
    assert 0.05 < np.mean(want_occ) < 0.95
    assert np.array_equal(np.asarray(occ).astype(bool), np.asarray(want_occ).astype(bool))
    # float64 geometry from the deformed triangles alone
    _world_, grays, ref = _world(m)
    _check_against_geometry(ctx.trace_batch(grays), ref, "device after update_blas%s" % (", thin kernel" if thin else ""))
    if thin:
        ctx.debug_set_thin()


def test_update_blas_device_takes_a_torch_tensor(tmp_path):
    """in a process of its own (tests/_torch_update_worker.py: torch initialises the GPU first): the records written by a torch
    kernel on the context's stream, handed over by data_ptr() — the nodes and hits of the host form"""
    import os
    import subprocess
    import sys

    m = 40
    scene, after = _one_mesh(m)
    out = str(tmp_path / "torch_update.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tests", "_torch_update_worker.py"), out, str(m)] + [repr(float(x)) for x in PLACED]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    moved = after.blas[0][1]
    # base + (moved - base) in float32 need not give `moved` back to the bit: the reference is refitted to what the tensor held
    held = got["held"]
    assert np.abs(np.frombuffer(held.tobytes(), np.float32) - np.frombuffer(moved.tobytes(), np.float32)).max() < 1e-6
    want = D.host_deformed(scene, {0: held})
    assert got["nodes"].tobytes() == want.blas[0][0].tobytes()
    rays = D.rays_for(20000, 7)
    assert SH.hit_records_equal(got["hits"], want.oracle().trace_closest(rays))
    assert SH.hit_records_equal(got["before"], scene.oracle().trace_closest(D.rays_for(2000, 7)))


def test_bad_arguments_are_refused_and_change_nothing(gpu_ctx_factory):
    m = 7
    scene, after = _one_mesh(m)
    ctx = gpu_ctx_factory(64, 64)
    scene.upload(ctx)
    moved = after.blas[0][1]
    n = len(moved)
    L, INVALID = ctx.L, 1  # NXHIP_ERR_INVALID
    buf = np.ascontiguousarray(moved)
    vp = buf.ctypes.data
    assert L.nxhip_update_blas(ctx.h, 0, vp, n - 1) == INVALID           # wrong count
    assert L.nxhip_update_blas(ctx.h, 0, vp, n + 1) == INVALID
    assert L.nxhip_update_blas(ctx.h, 1, vp, n) == INVALID               # bad id
    assert L.nxhip_update_blas(ctx.h, -1, vp, n) == INVALID
    assert L.nxhip_update_blas(ctx.h, 0, None, n) == INVALID             # NULL
    assert L.nxhip_update_blas(None, 0, vp, n) == INVALID
    assert L.nxhip_update_blas_device(ctx.h, 0, None, n) == INVALID
    assert L.nxhip_update_blas_device(ctx.h, 0, vp, n - 1) == INVALID    # (refused before the pointer is looked at)
    assert L.nxhip_update_blas_device(ctx.h, 3, vp, n) == INVALID
    with pytest.raises(capi.NexusError):
        ctx.update_blas(0, moved[:-1])
    assert ctx.read_blas(0, n)[0].tobytes() == scene.blas[0][0].tobytes()
    rays = D.rays_for(4000, 11)
    assert SH.hit_records_equal(ctx.trace_batch(rays), scene.oracle().trace_closest(rays))


# ---- instances -------------------------------------------------------------------------------------------------------------------

N_INST = 7


def _instanced():
    """two BLASes — the m = 40 grid and a torus —, 7 rotated / scaled instances; the host's answer after BLAS 0 took shape k"""
    def make():
        rng = np.random.RandomState(23)
        meshes = [D.base_grid(40), scenegen.displaced_torus(32, 16, seed=5, major=0.5, minor=0.2)]
        placements = [(i % 2, 0, capi.mat4_from_trs(rng.uniform(-1.5, 1.5, 3), rng.uniform(0, 360, 3), rng.uniform(0.5, 1.5, 3))) for i in range(N_INST)]
        scene = SH.BuiltScene(meshes, placements)
        return scene, [D.host_deformed(scene, {0: D.deformed_grid(40, k)}) for k in range(len(D.SHAPES))]

    return _cached("instanced", make)


def test_host_tlas_follows_the_updated_blas_byte_for_byte(gpu_ctx_factory):
    scene, shapes = _instanced()
    after = shapes[-1]
    ctx = gpu_ctx_factory(64, 64)
    scene.upload(ctx)
    rays = D.rays_for(20000, 13, extent=2.5)
    before = ctx.trace_batch(rays)
    ctx.update_blas(0, after.blas[0][1])
    nodes, insts = ctx.read_tlas(len(scene.tlas_nodes), N_INST)
    assert insts.tobytes() == after.instances.tobytes()
    assert nodes.tobytes() == after.tlas_nodes.tobytes()
    assert nodes.tobytes() != np.ascontiguousarray(scene.tlas_nodes).tobytes(), "the deformation leaves the old bounds"
    assert ctx.read_blas(1, len(scene.meshes[1]))[0].tobytes() == scene.blas[1][0].tobytes()
    got = ctx.trace_batch(rays)
    assert SH.hit_records_equal(got, after.oracle().trace_closest(rays))
    assert not SH.hit_records_equal(got, before)
    # instances moved after the update derive their bounds from the new root
    ids = np.array([0, 3], np.uint32)
    xfs = np.array([capi.mat4_from_trs((0.4, 0.3, -0.2), (50, 10, 80), (0.9, 1.1, 1.3)), capi.mat4_from_trs((-0.8, 0.1, 0.6), (5, 200, 40), (1.4, 0.6, 1.0))], np.float32)
    ctx.set_instance_transforms(ids, xfs)
    moved = after.instances.copy()
    for i, xf in zip(ids, xfs):
        moved[i] = capi.instance_init(int(moved[i]["bvhIdx"]), int(moved[i]["materialId"]), xf, after.blas[int(moved[i]["bvhIdx"])][0][0])
    final = D.with_blas(after, after.blas, moved, (capi.tlas_refit(after.tlas_nodes, after.tlas_idx, moved), after.tlas_idx))
    nodes, insts = ctx.read_tlas(len(scene.tlas_nodes), N_INST)
    assert insts.tobytes() == moved.tobytes() and nodes.tobytes() == final.tlas_nodes.tobytes()
    assert SH.hit_records_equal(ctx.trace_batch(rays), final.oracle().trace_closest(rays))


def _check_tlas_structure(nodes, idx, instances, geometry):
    """tests/test_tlas_refit.py::_check_tlas_structure restated for geometry bounds: every instance exactly once, children behind
    their parent and consecutive, every leaf slot's dequantised box holds its instances' triangles (world space, float64)"""
    from tests.test_builder_parity import _decode_children

    assert sorted(idx.tolist()) == list(range(len(instances)))
    seen_nodes, seen = set(), set()
    stack = [0]
    while stack:
        ni = stack.pop()
        assert ni not in seen_nodes and ni < len(nodes)
        seen_nodes.add(ni)
        inner = []
        for s, kind, lo, hi, first, count in _decode_children(nodes[ni]):
            eps = 1e-5 * np.maximum(1.0, np.abs(hi))
            if kind == "inner":
                assert first > ni
                inner.append(first)
                stack.append(first)
            else:
                assert 1 <= count <= 3
                for k in range(first, first + count):
                    assert k not in seen
                    seen.add(k)
                    assert np.all(lo <= geometry[0][idx[k]] + eps) and np.all(hi >= geometry[1][idx[k]] - eps), (ni, s, k)
        assert inner == list(range(inner[0], inner[0] + len(inner))) if inner else True
    assert len(seen_nodes) == len(nodes) and len(seen) == len(instances)


def _geometry_bounds(meshes, instances):
    lo, hi = [], []
    for inst in instances:
        mesh = meshes[int(inst["bvhIdx"])]
        T = np.asarray(inst["transform"], np.float64).reshape(4, 4)
        w = np.concatenate([mesh["pos0"], mesh["pos1"], mesh["pos2"]]).astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        lo.append(w.min(0))
        hi.append(w.max(0))
    return np.array(lo), np.array(hi)


def test_device_built_tlas_follows_the_updated_blas(gpu_ctx_factory):
    scene, shapes = _instanced()
    after = shapes[-1]
    ctx = gpu_ctx_factory(64, 64)
    scene.upload(ctx)
    nodes, idx = ctx.rebuild_tlas(scene.instances)
    _check_tlas_structure(nodes, idx, scene.instances, _geometry_bounds(scene.meshes, scene.instances))
    stale_ok = True
    try:
        _check_tlas_structure(nodes, idx, after.instances, _geometry_bounds(after.meshes, after.instances))
    except AssertionError:
        stale_ok = False
    assert not stale_ok, "the deformation stays inside the old tree: the test shows nothing"
    ctx.update_blas(0, after.blas[0][1])
    refitted, insts = ctx.read_tlas(len(nodes), N_INST)
    assert insts.tobytes() == after.instances.tobytes()
    _check_tlas_structure(refitted, idx, after.instances, _geometry_bounds(after.meshes, after.instances))
    # hits = float64 geometry of the deformed scene
    xfs = np.array([np.asarray(i["transform"], np.float32).reshape(16) for i in scene.instances])
    world = G.World(after.meshes, [int(i["bvhIdx"]) for i in scene.instances], xfs)
    rays, ref = _conditioned(world, D.rays_for(1000, 17, extent=2.5), 900)
    got = ctx.trace_batch(rays)
    clear = ~ref["unclear"]
    got_hit = got["hitDistance"] < pod.MISS_DISTANCE
    sel = clear & ref["hit"] & got_hit
    assert ref["hit"].mean() > 0.2
    assert np.array_equal(got_hit[clear], ref["hit"][clear])
    assert np.array_equal(got["instanceIdx"][sel].astype(np.int64), ref["inst"][sel]) and np.array_equal(got["triIdx"][sel].astype(np.int64), ref["tri"][sel])
    et = float(np.max(np.abs(got["hitDistance"][sel].astype(np.float64) - ref["t"][sel]) / ref["t"][sel]))
    print("device TLAS after update_blas: hitDistance %.3g relative (bound %.3g)" % (et, BOUND["ordinary"]["t"]))
    assert et <= BOUND["ordinary"]["t"]
    # ... and bit for bit the oracle walking the tree the device holds
    held = D.with_blas(after, after.blas, after.instances, (refitted, idx))
    big = D.rays_for(20000, 13, extent=2.5)
    assert SH.hit_records_equal(ctx.trace_batch(big), held.oracle().trace_closest(big))


def test_three_updates_without_a_render_equal_one(gpu_ctx_factory):
    scene, shapes = _instanced()
    rays = D.rays_for(20000, 13, extent=2.5)
    three = gpu_ctx_factory(64, 64)
    scene.upload(three)
    for after in shapes:   # no render, ray batch or read-back in between: one deferred refresh serves all three
        three.update_blas(0, after.blas[0][1])
    got3 = three.trace_batch(rays)
    one = gpu_ctx_factory(64, 64)
    scene.upload(one)
    one.update_blas(0, shapes[-1].blas[0][1])
    got1 = one.trace_batch(rays)
    assert SH.hit_records_equal(got3, got1)
    assert SH.hit_records_equal(got3, shapes[-1].oracle().trace_closest(rays))
    for ctx in (three, one):
        nodes, insts = ctx.read_tlas(len(scene.tlas_nodes), N_INST)
        assert nodes.tobytes() == shapes[-1].tlas_nodes.tobytes() and insts.tobytes() == shapes[-1].instances.tobytes()
    # the refresh again (nothing pending) changes nothing
    assert SH.hit_records_equal(three.trace_batch(rays), got1)


# ---- frames ----------------------------------------------------------------------------------------------------------------------

W = H = 64


def _lit_room():
    """Cornell-sized: a floor, a back wall and a torus lit by the wavy grid (m = 7) hanging face down as the only light"""
    def make():
        meshes = [D.base_grid(7), scenegen.quad((-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2)), scenegen.quad((-2, 0, -2), (2, 0, -2), (2, 3, -2), (-2, 3, -2)),
                  scenegen.displaced_torus(24, 12, seed=3, major=0.45, minor=0.18)]
        mats = np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(0.8, 0.8, 0.8), emissive=(1.0, 0.95, 0.9), intensity=18.0),
                         pod.make_material(pod.MAT_DIFFUSE, albedo=(0.7, 0.7, 0.7)), pod.make_material(pod.MAT_DIFFUSE, albedo=(0.7, 0.3, 0.25)),
                         pod.make_material(pod.MAT_PLASTIC, albedo=(0.3, 0.5, 0.8), roughness=0.4, ior=1.5)], dtype=pod.MAT_DT)
        placements = [(0, 0, capi.mat4_from_trs((0.0, 2.4, 0.0), (180, 0, 0), (0.7, 1.5, 0.7))), (1, 1, SH.IDENTITY), (2, 2, SH.IDENTITY),
                      (3, 3, capi.mat4_from_trs((0.2, 0.5, -0.2), (25, 30, 0)))]
        cam = capi.camera_init((0.0, 1.2, 4.2), (0.0, -0.05, -1.0) / np.linalg.norm((0.0, -0.05, -1.0)), 45.0, W, H, 5.0, 0.0)
        sc = SH.BuiltScene(meshes, placements, materials=mats, camera=cam, settings=O.make_settings(use_mis=True, path_length=4))
        sc.lights = SH.mesh_lights(sc.instances, sc.materials)
        assert len(sc.lights) == 1
        return sc, D.host_deformed(sc, {0: D.deformed_grid(7)})

    return _cached("room", make)


def _passes(ctx, n):
    for _ in range(n):
        ctx.render_frame()
    ctx.accumulate()  # (asynchronous: nothing here waits for the device)


@pytest.mark.parametrize("entry,per_pass,in_flight", [(False, 1, 1), (True, 2, 2)])
def test_frames_after_an_update_equal_a_fresh_upload(gpu_ctx_factory, entry, per_pass, in_flight):
    """passes, the update, more passes with no sync in between, against a context that is handed the deformed triangles and the
    refitted nodes through nxhip_upload_blas at the same point; the frame number and the accumulation carry on"""
    scene, after = _lit_room()
    results = []
    for updated in (True, False):
        ctx = gpu_ctx_factory(W, H)
        scene.upload(ctx)
        ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
        ctx.set_entry_points(entry)
        ctx.set_frames_per_pass(per_pass)
        ctx.set_passes_in_flight(in_flight)
        ctx.reset_frame_number()
        _passes(ctx, 2)
        if updated:
            ctx.update_blas(0, after.blas[0][1])
        else:
            frame = ctx.frame_number()
            acc = ctx.read_accumulation()
            after.upload(ctx)
            ctx.write_accumulation(acc, frame)
        _passes(ctx, 2)
        assert ctx.frame_number() == 4 * per_pass
        results.append((ctx.read_radiance(), ctx.read_accumulation(), ctx.read_rgba8()))
        ctx.set_passes_in_flight(1)
    (rad_a, acc_a, px_a), (rad_b, acc_b, px_b) = results
    assert SH.frames_identical(rad_a, rad_b, "radiance of the last pass")
    assert np.array_equal(acc_a.view(np.uint32), acc_b.view(np.uint32))
    assert np.array_equal(px_a, px_b)
    assert float(np.mean(acc_a)) > 0.01, "the light does not reach the room"
    # the oracle agrees on the frames after the update (the emissive mesh is sampled by the NEE: it reads the new triangles)
    w = O.Wavefront(after.oracle(), W * H, None, pod.RNG_PIXEL_KEYED, pod.CONDUCTOR_REFERENCE)
    want = []
    for f in range(3 * per_pass + 1, 4 * per_pass + 1):
        w.render(f)
        want.append(w.radiance().copy())
    w.close()
    assert SH.frames_identical(rad_a, np.concatenate(want), "last pass against the oracle")
    # ... and they are not the old shape's
    w = O.Wavefront(scene.oracle(), W * H, None, pod.RNG_PIXEL_KEYED, pod.CONDUCTOR_REFERENCE)
    w.render(4 * per_pass)
    assert not np.array_equal(np.asarray(w.radiance(), np.float32).reshape(-1, 3), np.asarray(rad_a, np.float32).reshape(-1, 3)[-W * H:])
    w.close()
