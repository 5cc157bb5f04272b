"""Skinned meshes on the device (nxhip_set_blas_skin / nxhip_pose_blas, nexus_amd/csrc/device/nx_skin.hip): bind-pose triangles and a
joint palette become the BLAS's triangles and intersection stream in one pass, the node refit of nxhip_update_blas behind it.

Two yardsticks.  The posed triangles are held to float64 arithmetic over the same inputs by the bounds of include/nexus_hip.h
(tests/skin_cases.py check_posed: positions gamma_8 A, normals 2 gamma_16 ||t|| / ||v|| + 4 u).  Everything behind the triangles — the
intersection stream, the nodes, what follows the root, hits, frames, the light table — is held bit for bit to the path that existed
before: a second context given the read-back triangles through nxhip_update_blas."""
import os

import numpy as np
import pytest

from nexus_amd import animation, capi, loaders, pod, scenegen
from tests import bvh_audit as A
from tests import deform_meshes as D
from tests import oracle_lib as O
from tests import scene_helpers as SH
from tests import skin_cases as K

pytestmark = pytest.mark.gpu

INVALID = 1  # NXHIP_ERR_INVALID
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _mixed_ribbon():
    """65 triangles — one wave and one lane — every fifth without normals"""
    t = K.ribbon(65)
    for k in range(3):
        t["normal%d" % k][::5] = 0.0
    return t


def _fixture():
    return _cached("fixture", lambda: loaders.load_glb(os.path.join(SH.GOLDEN, "skinned_bar.glb"), skins=True))


def _fixture_bar():
    ls = _fixture()
    return ls.meshes[ls.skins[0]["mesh"]], ls.skins[0]["corners"]


# name -> (triangles, corners or None: tests/skin_cases.py two_joint_skin across `axis`, axis, how the BLAS gets to the device)
MESHES = {
    "one triangle": lambda: (K.ribbon(1), None, 1, "upload"),
    "one wave and a lane": lambda: (_mixed_ribbon(), None, 1, "upload"),
    "fixture bar": lambda: _fixture_bar() + (1, "build"),
    "grid 100": lambda: (D.base_grid(100), None, 0, "upload"),
    "middle of a batch pool": lambda: (D.base_grid(40), None, 0, "batch"),
}


def _extent(tris):
    p = K.corner_positions(tris)
    return float(np.max(p.max(0) - p.min(0)))


def _install(ctx, tris, how):
    """the BLAS on the device -> (id, nodes, index list)"""
    ctx.clear_blas()
    tris = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
    if how == "upload":
        nodes, idx = _cached(("host build", tris.tobytes()), lambda: capi.bvh8_build(tris, threads=2))
        return ctx.upload_blas(nodes, tris, idx), nodes, idx
    ctx.set_device_builder(-1)
    if how == "build":
        bid = ctx.build_blas(tris)
    else:
        bid = ctx.build_blas_batch([scenegen.displaced_torus(32, 16, seed=2, major=0.5, minor=0.2), tris, scenegen.random_soup(500, seed=3, extent=0.5, size=0.1)])[1]
    return (bid,) + ctx.read_blas(bid, len(tris))


def _case(name, joint_count=2):
    tris, corners, axis, how = MESHES[name]()
    tris = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
    if corners is None or joint_count != 2:
        corners = K.two_joint_skin(tris, axis, joint_count)
    return tris, corners, how


# ---- 1. posed triangles against float64 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(MESHES))
def test_posed_triangles_are_within_the_bounds_of_float64(gpu_ctx_factory, name):
    tris, corners, how = _case(name)
    stored = pod.normalise_skin_corners(corners, 2)
    ctx = gpu_ctx_factory(32, 32)
    bid, nodes0, idx0 = _install(ctx, tris, how)
    ctx.set_blas_skin(bid, corners, 2)
    ext = _extent(tris)
    palettes = [(kind, K.palette(kind, 2, ext, seed)) for kind, seed in (("ordinary", 1), ("ordinary", 2), ("mirror", 3), ("outward", 4))]
    if name == "fixture bar":
        palettes.append(("animation 0 at t = 0.5", animation.joint_palette(_fixture(), 0, 0, 0.5)))
    for kind, pal in palettes:
        ctx.pose_blas(bid, pal)
        got = ctx.read_blas_triangles(bid, len(tris))
        K.check_posed(got, tris, stored, pal, "%s, %s" % (name, kind))
        if kind == "mirror":
            assert np.all(np.linalg.det(pal.reshape(-1, 3, 4)[:, :, :3].astype(np.float64)) < 0)
        nodes, idx = ctx.read_blas(bid, len(tris))
        assert np.array_equal(idx, idx0)
        assert nodes.tobytes() == capi.bvh8_refit(nodes0, idx0, got).tobytes(), (name, kind)
        lo, hi = ctx.read_blas_bounds(bid)
        p = K.corner_positions(got)
        assert np.all(lo <= p.min(0)) and np.all(hi >= p.max(0)), (name, kind)
        assert np.array_equal(lo, nodes[0]["p"]) and np.array_equal(hi, nodes[0]["p"] + np.exp2(nodes[0]["e"].astype(np.float32) - 127) * np.float32(255.0))
        if kind == "outward":  # the stale-bounds trap of the refit tests: the pose leaves the old root box
            old_hi = nodes0[0]["p"] + np.exp2(nodes0[0]["e"].astype(np.float32) - 127) * np.float32(255.0)
            assert np.any(p.min(0) > old_hi), "the outward pose stays inside the old root box: the test shows nothing"


@pytest.mark.parametrize("joint_count", [1, 2, 1024, 1025])  # 1024: the last palette staged in the LDS, 1025: the first read from global memory
def test_joint_counts_on_both_sides_of_the_lds_limit(gpu_ctx_factory, joint_count):
    tris, corners, how = _case("one wave and a lane", joint_count)
    ctx = gpu_ctx_factory(32, 32)
    bid, _nodes, _idx = _install(ctx, tris, how)
    ctx.set_blas_skin(bid, corners, joint_count)
    pal = K.palette("ordinary", joint_count, _extent(tris), seed=7)
    ctx.pose_blas(bid, pal)
    got = ctx.read_blas_triangles(bid, len(tris))
    K.check_posed(got, tris, pod.normalise_skin_corners(corners, joint_count), pal, "%d joints" % joint_count)
    if joint_count >= 1024:  # the joints behind the second are present and unused: another palette for them changes nothing
        other = pal.copy()
        other[2:] = K.palette("mirror", joint_count - 2, 1.0, seed=9)
        ctx.pose_blas(bid, other)
        assert ctx.read_blas_triangles(bid, len(tris)).tobytes() == got.tobytes()


def test_one_hot_weights_and_identity_matrices_give_the_bind_pose_back_to_the_bit(gpu_ctx_factory):
    tris, _c, how = _case("grid 100")
    corners = K.two_joint_skin(tris, 0, 2, one_hot=True)
    ctx = gpu_ctx_factory(32, 32)
    bid, nodes0, idx0 = _install(ctx, tris, how)
    ctx.set_blas_skin(bid, corners, 2)
    ctx.pose_blas(bid, K.palette("ordinary", 2, 1.0, seed=11))
    assert ctx.read_blas(bid, len(tris))[0].tobytes() != nodes0.tobytes()
    ctx.pose_blas(bid, K.palette("identity", 2, 1.0))
    got = ctx.read_blas_triangles(bid, len(tris))
    for k in range(3):
        assert got["pos%d" % k].tobytes() == tris["pos%d" % k].tobytes()
        assert got["texCoord%d" % k].tobytes() == tris["texCoord%d" % k].tobytes()
    assert ctx.read_blas(bid, len(tris))[0].tobytes() == nodes0.tobytes(), "the builder's node bytes"


# ---- 2. and 5. the fused pass equals update_blas of the same triangles, bit for bit -----------------------------------------------------

W = H = 64


def _room(power):
    """tests/test_gpu_blas_refit.py's lit room: a floor, a back wall and a torus lit by the wavy grid (m = 7) hanging face down as the
    only light — here the grid is the skinned mesh"""
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
        if power:
            sc.light_sampling = pod.LIGHTS_POWER
        return sc

    return _cached(("room", power), make)


# a pose that stretches the emitter: joint 1 scaled and pushed outward
STRETCH = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], [1.6, 0.1, 0, 0.5, -0.1, 1.3, 0, 0.05, 0, 0, 1.4, 0.2]], np.float32)


def _passes(ctx, n):
    for _ in range(n):
        ctx.render_frame()
    ctx.accumulate()


def _fused_and_existing(gpu_ctx_factory, scene, compact, entry, in_flight):
    """context A poses; context B is handed A's triangles through nxhip_update_blas at the same point -> what each then holds"""
    corners = K.two_joint_skin(scene.meshes[0], 0, 2)
    rays = D.rays_for(20000, 7, extent=2.5)
    rng = np.random.RandomState(9)
    tmax = rng.uniform(0.5, 6.0, len(rays)).astype(np.float32)
    out, posed = [], None
    for fused in (True, False):
        ctx = gpu_ctx_factory(W, H)
        scene.upload(ctx)
        ctx.set_modes(pod.RNG_PIXEL_KEYED, compact, pod.CONDUCTOR_REFERENCE)
        ctx.set_entry_points(entry)
        ctx.set_passes_in_flight(in_flight)
        ctx.reset_frame_number()
        if fused:
            ctx.set_blas_skin(0, corners, 2)
        _passes(ctx, 2)
        if fused:
            ctx.pose_blas(0, STRETCH)  # (between passes, nothing waited for)
        else:
            ctx.update_blas(0, posed)
        _passes(ctx, 2)
        held = dict(radiance=ctx.read_radiance(), accumulation=ctx.read_accumulation(), rgba8=ctx.read_rgba8(), frame=ctx.frame_number())
        ctx.set_passes_in_flight(1)
        if fused:
            posed = ctx.read_blas_triangles(0, len(scene.meshes[0]))
        held["nodes"], held["idx"] = ctx.read_blas(0, len(scene.meshes[0]))
        held["tlas"], held["instances"] = ctx.read_tlas(len(scene.tlas_nodes), len(scene.instances))
        held["hits"], held["occluded"] = ctx.trace_batch(rays), ctx.trace_shadow_batch(rays, tmax)
        if scene.light_sampling == pod.LIGHTS_POWER:
            held["light table"] = ctx.read_light_table(len(scene.lights))
        out.append(held)
    return out[0], out[1], posed


def _same(a, b):
    assert a["nodes"].tobytes() == b["nodes"].tobytes() and np.array_equal(a["idx"], b["idx"])
    assert a["tlas"].tobytes() == b["tlas"].tobytes() and a["instances"].tobytes() == b["instances"].tobytes()
    assert SH.hit_records_equal(a["hits"], b["hits"])
    assert np.array_equal(a["occluded"], b["occluded"]) and 0.02 < np.mean(a["occluded"]) < 0.98
    assert a["frame"] == b["frame"] == 4
    assert SH.frames_identical(a["radiance"], b["radiance"], "radiance of the last pass")
    assert np.array_equal(a["accumulation"].view(np.uint32), b["accumulation"].view(np.uint32))
    assert np.array_equal(a["rgba8"], b["rgba8"])
    assert float(np.mean(a["accumulation"])) > 0.01, "the light does not reach the room"


@pytest.mark.parametrize("compact,entry,in_flight", [(pod.COMPACT_FAST, False, 1), (pod.COMPACT_ORDERED, False, 1), (pod.COMPACT_FAST, True, 1), (pod.COMPACT_FAST, True, 2)])
def test_the_fused_pass_equals_update_blas_of_its_triangles(gpu_ctx_factory, compact, entry, in_flight):
    scene = _room(False)
    a, b, posed = _fused_and_existing(gpu_ctx_factory, scene, compact, entry, in_flight)
    _same(a, b)
    assert a["idx"].tobytes() == np.ascontiguousarray(scene.blas[0][2]).tobytes(), "the index list is unchanged"
    assert a["nodes"].tobytes() != np.ascontiguousarray(scene.blas[0][0]).tobytes()
    # ... and both are the host's answer for those triangles
    want = D.host_deformed(scene, {0: posed})
    assert a["nodes"].tobytes() == want.blas[0][0].tobytes() and a["tlas"].tobytes() == want.tlas_nodes.tobytes()
    assert a["instances"].tobytes() == want.instances.tobytes()


def test_a_posed_emitter_rebuilds_the_light_table(gpu_ctx_factory):
    scene = _room(True)
    a, b, posed = _fused_and_existing(gpu_ctx_factory, scene, pod.COMPACT_FAST, False, 1)
    _same(a, b)
    for x, y in zip(a["light table"], b["light table"]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    # the stretch changed the table: a context that never posed holds another one
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    rest = ctx.read_light_table(len(scene.lights))
    assert np.asarray(rest[0]).tobytes() != np.asarray(a["light table"][0]).tobytes()


# ---- 3. exact audit ------------------------------------------------------------------------------------------------------------------

def test_posed_blas_and_the_tlas_behind_it_pass_the_exact_audit(gpu_ctx_factory):
    rng = np.random.RandomState(23)
    meshes = [D.base_grid(40), scenegen.displaced_torus(32, 16, seed=5, major=0.5, minor=0.2)]
    placements = [(i % 2, 0, capi.mat4_from_trs(rng.uniform(-1.5, 1.5, 3), rng.uniform(0, 360, 3), rng.uniform(0.5, 1.5, 3))) for i in range(7)]
    scene = _cached("audit scene", lambda: SH.BuiltScene(meshes, placements))
    ctx = gpu_ctx_factory(32, 32)
    scene.upload(ctx)
    cam = capi.camera_init((0.0, 1.0, 6.0), (0.0, 0.0, -1.0), 45.0, 32, 32, 5.0, 0.0)
    ctx.set_camera(cam)
    corners = K.two_joint_skin(scene.meshes[0], 0, 2)
    ctx.set_blas_skin(0, corners, 2)
    for kind, seed in (("ordinary", 1), ("mirror", 3), ("outward", 4)):
        ctx.pose_blas(0, K.palette(kind, 2, 2.0, seed))
        posed = ctx.read_blas_triangles(0, len(scene.meshes[0]))
        nodes, idx = ctx.read_blas(0, len(posed))
        rep = A.audit(nodes, idx, *A.triangle_boxes(posed))
        print(rep.line("posed BLAS, %s" % kind))
        ctx.render_frame()  # the deferred refresh: instance bounds, traversal records, the TLAS
        tn, insts = ctx.read_tlas(len(scene.tlas_nodes), len(scene.instances))
        rep = A.audit(tn, scene.tlas_idx, *A.instance_boxes(insts), tlas=True)
        print(rep.line("TLAS after the next render, %s" % kind))
        want = D.host_deformed(scene, {0: posed})
        assert insts.tobytes() == want.instances.tobytes() and tn.tobytes() == want.tlas_nodes.tobytes()


# ---- 4. poses do not accumulate ---------------------------------------------------------------------------------------------------------

def test_poses_do_not_accumulate(gpu_ctx_factory):
    tris, corners, how = _case("one wave and a lane")
    stored = pod.normalise_skin_corners(corners, 2)
    ext = _extent(tris)
    p1, p2, rest = K.palette("ordinary", 2, ext, 1), K.palette("mirror", 2, ext, 3), K.palette("identity", 2, ext)
    both = gpu_ctx_factory(32, 32)
    bid, nodes0, idx0 = _install(both, tris, how)
    both.set_blas_skin(bid, corners, 2)
    both.pose_blas(bid, p1)
    both.pose_blas(bid, p2)
    fresh = gpu_ctx_factory(32, 32)
    fid, _n, _i = _install(fresh, tris, how)
    fresh.set_blas_skin(fid, corners, 2)
    fresh.pose_blas(fid, p2)
    assert both.read_blas_triangles(bid, len(tris)).tobytes() == fresh.read_blas_triangles(fid, len(tris)).tobytes()
    assert both.read_blas(bid, len(tris))[0].tobytes() == fresh.read_blas(fid, len(tris))[0].tobytes()
    both.pose_blas(bid, rest)
    back = both.read_blas_triangles(bid, len(tris))
    K.check_posed(back, tris, stored, rest, "rest pose after two poses")
    # a skin set on a posed BLAS binds THAT shape: the bind copy is the triangles as they were when the skin was set
    fresh.set_blas_skin(fid, corners, 2)
    held = fresh.read_blas_triangles(fid, len(tris))
    fresh.pose_blas(fid, p1)
    K.check_posed(fresh.read_blas_triangles(fid, len(tris)), held, stored, p1, "a skin set on the posed shape")


# ---- 6. validation ---------------------------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_triangles_and_nodes_as_they_were(gpu_ctx_factory):
    tris, corners, how = _case("one wave and a lane")
    n = len(tris)
    ctx = gpu_ctx_factory(32, 32)
    bid, _nodes, _idx = _install(ctx, tris, how)
    L = ctx.L
    pal = K.palette("ordinary", 2, 1.0, 1)
    good = np.ascontiguousarray(corners)

    def state():
        return ctx.read_blas_triangles(bid, n).tobytes(), ctx.read_blas(bid, n)[0].tobytes()

    def refused(rc, what):
        assert rc == INVALID, what
        assert L.nxhip_last_error(), what

    def skin(c, count=None, joints=2, blas=None):
        c = np.ascontiguousarray(c, dtype=pod.SKIN_CORNER_DT)
        return L.nxhip_set_blas_skin(ctx.h, bid if blas is None else blas, c.ctypes.data, len(c) if count is None else count, joints)

    def pose(p, joints=2, blas=None):
        p = np.ascontiguousarray(p, dtype=np.float32)
        return L.nxhip_pose_blas(ctx.h, bid if blas is None else blas, p.ctypes.data, joints)

    def bad(field, corner, slot, value):
        c = good.copy()
        c[field][corner, slot] = value
        return c

    for with_skin in (False, True):
        if with_skin:
            ctx.set_blas_skin(bid, corners, 2)
            ctx.pose_blas(bid, pal)
        before = state()
        refused(skin(good, blas=bid + 1), "bad id")
        refused(skin(good, blas=-1), "bad id")
        refused(skin(good, count=3 * n - 3), "wrong count")
        refused(skin(good[:-3]), "wrong count")
        refused(skin(good, joints=0), "no joints")
        refused(skin(good, joints=65537), "too many joints")
        refused(skin(good, joints=1), "a joint index at the joint count, under a non-zero weight")
        refused(skin(bad("weight", 4, 1, np.nan)), "NaN weight")
        refused(skin(bad("weight", 4, 1, np.inf)), "infinite weight")
        refused(skin(bad("weight", 4, 1, -0.25)), "negative weight")
        zero = good.copy()
        zero["weight"][7] = 0.0
        refused(skin(zero), "weights that sum to 0")
        if with_skin:
            refused(pose(pal, blas=bid + 1), "bad id")
            refused(pose(pal, joints=3), "another joint count")
            refused(L.nxhip_pose_blas(ctx.h, bid, None, 2), "NULL")
            for value in (np.nan, np.inf, -np.inf):
                p = pal.copy()
                p[1, 7] = value
                refused(pose(p), "a matrix entry that is not finite")
        else:
            refused(pose(pal), "no skin")
        refused(L.nxhip_read_blas_triangles(ctx.h, bid, np.zeros(n, pod.TRI_DT).ctypes.data, n - 1), "destination too small")
        refused(L.nxhip_read_blas_bounds(ctx.h, bid + 1, np.zeros(3, np.float32).ctypes.data, np.zeros(3, np.float32).ctypes.data), "bad id")
        assert state() == before
    # the previous skin is still in place: the same pose gives the same triangles
    posed = ctx.read_blas_triangles(bid, n)
    ctx.pose_blas(bid, K.palette("identity", 2, 1.0))
    ctx.pose_blas(bid, pal)
    assert ctx.read_blas_triangles(bid, n).tobytes() == posed.tobytes()
    # an unused slot may name a joint the skin does not have
    ok = good.copy()
    ok["joint"][ok["weight"] == 0] = 999
    ctx.set_blas_skin(bid, None, 0)
    ctx.update_blas(bid, tris)
    ctx.set_blas_skin(bid, ok, 2)
    ctx.pose_blas(bid, pal)
    assert ctx.read_blas_triangles(bid, n).tobytes() == posed.tobytes()


def test_removing_the_skin_leaves_a_context_that_never_had_one(gpu_ctx_factory):
    scene = _room(False)
    corners = K.two_joint_skin(scene.meshes[0], 0, 2)
    frames = []
    for skinned in (True, False):
        ctx = gpu_ctx_factory(W, H)
        scene.upload(ctx)
        ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
        ctx.reset_frame_number()
        if skinned:
            ctx.set_blas_skin(0, corners, 2)
            ctx.set_blas_skin(0, None, 0)
            with pytest.raises(capi.NexusError):
                ctx.pose_blas(0, STRETCH)
        _passes(ctx, 2)
        frames.append((ctx.read_radiance(), ctx.read_rgba8(), ctx.read_blas(0, len(scene.meshes[0]))[0].tobytes()))
    assert SH.frames_identical(frames[0][0], frames[1][0], "frames")
    assert np.array_equal(frames[0][1], frames[1][1]) and frames[0][2] == frames[1][2]


def test_update_blas_on_a_skinned_blas_leaves_the_bind_copy_alone(gpu_ctx_factory):
    tris, corners, how = _case("one wave and a lane")
    ctx = gpu_ctx_factory(32, 32)
    bid, _nodes, _idx = _install(ctx, tris, how)
    ctx.set_blas_skin(bid, corners, 2)
    pal = K.palette("ordinary", 2, _extent(tris), 1)
    ctx.pose_blas(bid, pal)
    posed = ctx.read_blas_triangles(bid, len(tris))
    moved = tris.copy()
    for k in range(3):
        moved["pos%d" % k] += np.float32(0.37)
    ctx.update_blas(bid, moved)
    assert ctx.read_blas_triangles(bid, len(tris)).tobytes() == moved.tobytes()
    ctx.pose_blas(bid, pal)
    assert ctx.read_blas_triangles(bid, len(tris)).tobytes() == posed.tobytes()
