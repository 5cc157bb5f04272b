"""Morph targets on the device (nxhip_set_blas_morph / nxhip_pose_blas_morph, nexus_amd/csrc/device/nx_skin.hip): bind triangles, the
active targets' deltas and — on a skinned BLAS — a joint palette become the BLAS's triangles and intersection stream in one pass, the node
refit of nxhip_update_blas behind it.

The yardsticks are those of tests/test_gpu_pose_blas.py, whose helpers this file uses.  The triangles are held to float64 arithmetic over
the same inputs by the derived bounds of tests/morph_cases.py (stated in include/nexus_hip.h as well); everything behind the triangles is
held bit for bit to the path that existed before: a second context given the read-back triangles through nxhip_update_blas."""
import os

import numpy as np
import pytest

from nexus_amd import animation, capi, loaders, pod, scenegen
from tests import bvh_audit as A
from tests import deform_meshes as D
from tests import morph_cases as M
from tests import scene_helpers as SH
from tests import skin_cases as K
from tests import test_gpu_pose_blas as PB  # (its helpers: _install, _room, _passes, _same — no test of it is named here)

pytestmark = pytest.mark.gpu

INVALID = 1  # NXHIP_ERR_INVALID
_cached, _install, _extent = PB._cached, PB._install, PB._extent


def _fixture():
    return _cached("morph fixture", lambda: loaders.load_glb(os.path.join(SH.GOLDEN, "morph_bar.glb"), skins=True, morphs=True))


def _fixture_bar():
    ls = _fixture()
    return ls.meshes[ls.morphs[0]["mesh"]]


# name -> (triangles, how the BLAS gets to the device)
MESHES = {
    "one triangle": lambda: (K.ribbon(1), "upload"),
    "one wave and a lane": lambda: (PB._mixed_ribbon(), "upload"),
    "fixture bar": lambda: (_fixture_bar(), "build"),
    "grid 100": lambda: (D.base_grid(100), "upload"),
    "middle of a batch pool": lambda: (D.base_grid(40), "batch"),
}

# T = 3, target 1 carries the mesh out of its box (morph_cases.deltas outward=1) and has no NORMAL
WEIGHT_SETS = [("one active of three", [0.0, 1.0, 0.0]), ("all three", [0.5, 0.25, 0.75]), ("negative and above 1", [-0.5, 0.0, 1.5])]


def _case(name):
    tris, how = MESHES[name]()
    tris = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
    return tris, M.deltas(tris, 3, outward=1), how


def _root_hi(nodes):
    return nodes[0]["p"] + np.exp2(nodes[0]["e"].astype(np.float32) - 127) * np.float32(255.0)


def _check_behind(ctx, bid, got, nodes0, idx0, what):
    """what follows the triangles: the index list, the refitted nodes, the bounds"""
    nodes, idx = ctx.read_blas(bid, len(got))
    assert np.array_equal(idx, idx0), what
    assert nodes.tobytes() == capi.bvh8_refit(nodes0, idx0, got).tobytes(), what
    lo, hi = ctx.read_blas_bounds(bid)
    p = K.corner_positions(got)
    assert np.all(lo <= p.min(0)) and np.all(hi >= p.max(0)), what
    assert np.array_equal(lo, nodes[0]["p"]) and np.array_equal(hi, _root_hi(nodes)), what
    return p


# ---- 1. morph only, against float64 -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(MESHES))
def test_morphed_triangles_are_within_the_bounds_of_float64(gpu_ctx_factory, name):
    tris, d, how = _case(name)
    ctx = gpu_ctx_factory(32, 32)
    bid, nodes0, idx0 = _install(ctx, tris, how)
    runs = [(d, np.array(w, np.float32), what) for what, w in WEIGHT_SETS] + [(d[:1], np.array([0.7], np.float32), "T = 1")]
    if name == "fixture bar":  # the file's own targets: the defaults it carries, and all three
        m = _fixture().morphs[0]
        runs += [(m["deltas"], m["weights"], "the file's targets, its default weights"), (m["deltas"], np.array([0.6, -0.3, 1.0], np.float32), "the file's targets, all three")]
    held = None
    for dd, w, what in runs:
        if dd is not held:
            ctx.set_blas_morph(bid, None)
            ctx.update_blas(bid, tris)
            ctx.set_blas_morph(bid, dd)
            held = dd
        ctx.pose_blas_morph(bid, w)
        got = ctx.read_blas_triangles(bid, len(tris))
        M.check_morphed(got, tris, dd, w, "%s, %s" % (name, what))
        p = _check_behind(ctx, bid, got, nodes0, idx0, (name, what))
        if what == "one active of three":  # the stale-bounds trap of the refit tests: the pose leaves the old root box
            assert np.any(p.min(0) > _root_hi(nodes0)), "the outward target stays inside the old root box: the test shows nothing"


def _ribbon_1024():
    """the 65-triangle ribbon under 1024 targets, of which the first and the last are the only ones a test makes active"""
    tris = np.ascontiguousarray(PB._mixed_ribbon(), dtype=pod.TRI_DT)
    two = M.deltas(tris, 2, seed=17)
    d = np.zeros((1024, two.shape[1]), dtype=pod.MORPH_CORNER_DT)
    d[1:1023] = M.deltas(tris, 1, seed=19)[0]  # (what a kernel that visited an inactive target would add)
    d[0], d[1023] = two[0], two[1]
    w = np.zeros(1024, np.float32)
    w[0], w[1023] = 0.8, -0.45
    return tris, d, w, two


def test_1024_targets_with_the_first_and_the_last_active(gpu_ctx_factory):
    tris, d, w, _two = _ribbon_1024()
    ctx = gpu_ctx_factory(32, 32)
    bid, nodes0, idx0 = _install(ctx, tris, "upload")
    ctx.set_blas_morph(bid, d)
    ctx.pose_blas_morph(bid, w)
    got = ctx.read_blas_triangles(bid, len(tris))
    M.check_morphed(got, tris, d, w, "T = 1024, targets 0 and 1023")
    _check_behind(ctx, bid, got, nodes0, idx0, "T = 1024")


# ---- 2. no active target ----------------------------------------------------------------------------------------------------------------

def test_no_active_target_gives_the_bind_copy_or_the_plain_pose_to_the_bit(gpu_ctx_factory):
    tris, d, how = _case("one wave and a lane")
    n = len(tris)
    ctx = gpu_ctx_factory(32, 32)
    bid, nodes0, idx0 = _install(ctx, tris, how)
    ctx.set_blas_morph(bid, d)
    ctx.pose_blas_morph(bid, [0.5, 0.25, 0.75])
    assert ctx.read_blas_triangles(bid, n).tobytes() != tris.tobytes()
    ctx.pose_blas_morph(bid, [0.0, -0.0, 0.0])
    assert ctx.read_blas_triangles(bid, n).tobytes() == tris.tobytes(), "unskinned, no active target: the bind copy"
    assert ctx.read_blas(bid, n)[0].tobytes() == nodes0.tobytes(), "the builder's node bytes"
    # skinned: nxhip_pose_blas's triangles and nodes, from a context that has no morph
    corners = K.two_joint_skin(tris, 1, 2)
    pal = K.palette("ordinary", 2, _extent(tris), 1)
    ctx.set_blas_skin(bid, corners, 2)
    ctx.pose_blas_morph(bid, [0.5, 0.25, 0.75], pal)
    ctx.pose_blas_morph(bid, np.zeros(3, np.float32), pal)
    plain = gpu_ctx_factory(32, 32)
    pid, _n, _i = _install(plain, tris, how)
    plain.set_blas_skin(pid, corners, 2)
    plain.pose_blas(pid, pal)
    assert ctx.read_blas_triangles(bid, n).tobytes() == plain.read_blas_triangles(pid, n).tobytes()
    assert ctx.read_blas(bid, n)[0].tobytes() == plain.read_blas(pid, n)[0].tobytes()
    assert plain.read_blas_triangles(pid, n).tobytes() != tris.tobytes()


# ---- 3. compaction ----------------------------------------------------------------------------------------------------------------------

def test_two_active_of_1024_equal_a_two_target_morph_to_the_bit(gpu_ctx_factory):
    tris, d, w, two = _ribbon_1024()
    n = len(tris)
    wide = gpu_ctx_factory(32, 32)
    bid, _nodes, _idx = _install(wide, tris, "upload")
    wide.set_blas_morph(bid, d)
    wide.pose_blas_morph(bid, w)
    narrow = gpu_ctx_factory(32, 32)
    nid, _nodes, _idx = _install(narrow, tris, "upload")
    narrow.set_blas_morph(nid, two)
    narrow.pose_blas_morph(nid, [w[0], w[1023]])
    assert wide.read_blas_triangles(bid, n).tobytes() == narrow.read_blas_triangles(nid, n).tobytes()
    assert wide.read_blas(bid, n)[0].tobytes() == narrow.read_blas(nid, n)[0].tobytes()
    assert wide.read_blas_triangles(bid, n).tobytes() != tris.tobytes()


# ---- 4. morph + skin, against float64 ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("joint_count", [2, 1025])  # 1025: the first palette read from global memory
@pytest.mark.parametrize("kind,seed", [("ordinary", 1), ("mirror", 3)])
def test_morph_then_skin_is_within_the_bounds_of_float64(gpu_ctx_factory, kind, seed, joint_count):
    tris, d, how = _case("one wave and a lane")
    corners = K.two_joint_skin(tris, 1, joint_count)
    ctx = gpu_ctx_factory(32, 32)
    bid, nodes0, idx0 = _install(ctx, tris, how)
    ctx.set_blas_skin(bid, corners, joint_count)
    ctx.set_blas_morph(bid, d)
    pal = K.palette(kind, joint_count, _extent(tris), seed)
    w = np.array([0.6, 0.0, -0.4], np.float32)  # two active targets
    ctx.pose_blas_morph(bid, w, pal)
    got = ctx.read_blas_triangles(bid, len(tris))
    M.check_morphed_and_posed(got, tris, d, w, pod.normalise_skin_corners(corners, joint_count), pal, "%s, %d joints" % (kind, joint_count))
    _check_behind(ctx, bid, got, nodes0, idx0, (kind, joint_count))


def test_the_fixture_bar_morphed_and_posed_at_half_a_second(gpu_ctx_factory):
    ls = _fixture()
    morph, skin = ls.morphs[0], ls.skins[0]
    assert morph["mesh"] == skin["mesh"]
    tris = np.ascontiguousarray(ls.meshes[morph["mesh"]], dtype=pod.TRI_DT)
    w = animation.morph_weights(ls, 0, 2, 0.5)
    pal = animation.joint_palette(ls, 0, 0, 0.5)
    assert np.count_nonzero(w) >= 2 and w.dtype == np.float32
    ctx = gpu_ctx_factory(32, 32)
    bid, nodes0, idx0 = _install(ctx, tris, "build")
    ctx.set_blas_morph(bid, morph["deltas"])
    ctx.set_blas_skin(bid, skin["corners"], len(skin["joints"]))
    ctx.pose_blas_morph(bid, w, pal)
    got = ctx.read_blas_triangles(bid, len(tris))
    M.check_morphed_and_posed(got, tris, morph["deltas"], w, pod.normalise_skin_corners(skin["corners"], len(skin["joints"])), pal, "fixture bar at t = 0.5")
    _check_behind(ctx, bid, got, nodes0, idx0, "fixture bar")


# ---- 5. the fused pass equals update_blas of the same triangles, bit for bit ------------------------------------------------------------

W, H = PB.W, PB.H
ROOM_WEIGHTS = np.array([0.8, 0.0, -0.6], np.float32)


def _fused_and_existing(gpu_ctx_factory, scene, compact, entry, in_flight):
    """test_gpu_pose_blas._fused_and_existing with the morph in the skin's place: context A poses by weights; context B is handed A's
    triangles through nxhip_update_blas at the same point -> what each then holds"""
    d = M.deltas(scene.meshes[0], 3, seed=5, plain=(1,))
    rays = D.rays_for(20000, 7, extent=2.5)
    tmax = np.random.RandomState(9).uniform(0.5, 6.0, len(rays)).astype(np.float32)
    out, posed = [], None
    for fused in (True, False):
        ctx = gpu_ctx_factory(W, H)
        scene.upload(ctx)
        ctx.set_modes(pod.RNG_PIXEL_KEYED, compact, pod.CONDUCTOR_REFERENCE)
        ctx.set_entry_points(entry)
        ctx.set_passes_in_flight(in_flight)
        ctx.reset_frame_number()
        if fused:
            ctx.set_blas_morph(0, d)
        PB._passes(ctx, 2)
        if fused:
            ctx.pose_blas_morph(0, ROOM_WEIGHTS)  # (between passes, nothing waited for)
        else:
            ctx.update_blas(0, posed)
        PB._passes(ctx, 2)
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


@pytest.mark.parametrize("compact,entry,in_flight", [(pod.COMPACT_FAST, True, 2), (pod.COMPACT_ORDERED, False, 1)])
def test_the_fused_pass_equals_update_blas_of_its_triangles(gpu_ctx_factory, compact, entry, in_flight):
    scene = PB._room(False)
    a, b, posed = _fused_and_existing(gpu_ctx_factory, scene, compact, entry, in_flight)
    PB._same(a, b)
    assert a["idx"].tobytes() == np.ascontiguousarray(scene.blas[0][2]).tobytes(), "the index list is unchanged"
    assert a["nodes"].tobytes() != np.ascontiguousarray(scene.blas[0][0]).tobytes()
    want = D.host_deformed(scene, {0: posed})
    assert a["nodes"].tobytes() == want.blas[0][0].tobytes() and a["tlas"].tobytes() == want.tlas_nodes.tobytes()
    assert a["instances"].tobytes() == want.instances.tobytes()


def test_a_morphed_emitter_rebuilds_the_light_table(gpu_ctx_factory):
    scene = PB._room(True)
    a, b, _posed = _fused_and_existing(gpu_ctx_factory, scene, pod.COMPACT_FAST, False, 1)
    PB._same(a, b)
    for x, y in zip(a["light table"], b["light table"]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    rest = ctx.read_light_table(len(scene.lights))
    assert np.asarray(rest[0]).tobytes() != np.asarray(a["light table"][0]).tobytes()


def test_morphed_blas_and_the_tlas_behind_it_pass_the_exact_audit(gpu_ctx_factory):
    rng = np.random.RandomState(23)
    meshes = [D.base_grid(40), scenegen.displaced_torus(32, 16, seed=5, major=0.5, minor=0.2)]
    placements = [(i % 2, 0, capi.mat4_from_trs(rng.uniform(-1.5, 1.5, 3), rng.uniform(0, 360, 3), rng.uniform(0.5, 1.5, 3))) for i in range(7)]
    scene = _cached("audit scene", lambda: SH.BuiltScene(meshes, placements))
    ctx = gpu_ctx_factory(32, 32)
    scene.upload(ctx)
    ctx.set_camera(capi.camera_init((0.0, 1.0, 6.0), (0.0, 0.0, -1.0), 45.0, 32, 32, 5.0, 0.0))
    ctx.set_blas_morph(0, M.deltas(scene.meshes[0], 3, outward=1))
    ctx.pose_blas_morph(0, [0.4, 1.0, -0.7])
    posed = ctx.read_blas_triangles(0, len(scene.meshes[0]))
    nodes, idx = ctx.read_blas(0, len(posed))
    print(A.audit(nodes, idx, *A.triangle_boxes(posed)).line("morphed BLAS"))
    ctx.render_frame()  # the deferred refresh: instance bounds, traversal records, the TLAS
    tn, insts = ctx.read_tlas(len(scene.tlas_nodes), len(scene.instances))
    print(A.audit(tn, scene.tlas_idx, *A.instance_boxes(insts), tlas=True).line("TLAS after the next render"))
    want = D.host_deformed(scene, {0: posed})
    assert insts.tobytes() == want.instances.tobytes() and tn.tobytes() == want.tlas_nodes.tobytes()


# ---- 6. state rules ---------------------------------------------------------------------------------------------------------------------

def test_poses_do_not_accumulate_and_weights_do_not_persist(gpu_ctx_factory):
    tris, d, how = _case("one wave and a lane")
    n = len(tris)
    corners = K.two_joint_skin(tris, 1, 2)
    pal = K.palette("ordinary", 2, _extent(tris), 1)
    w1, w2 = [0.5, 0.25, 0.75], [-0.5, 0.0, 1.5]
    both = gpu_ctx_factory(32, 32)
    bid, _nodes, _idx = _install(both, tris, how)
    both.set_blas_morph(bid, d)
    both.pose_blas_morph(bid, w1)
    both.pose_blas_morph(bid, w2)
    fresh = gpu_ctx_factory(32, 32)
    fid, _nodes, _idx = _install(fresh, tris, how)
    fresh.set_blas_morph(fid, d)
    fresh.pose_blas_morph(fid, w2)
    assert both.read_blas_triangles(bid, n).tobytes() == fresh.read_blas_triangles(fid, n).tobytes()
    assert both.read_blas(bid, n)[0].tobytes() == fresh.read_blas(fid, n)[0].tobytes()
    # weights do not persist: the plain pose after a morphed one is the plain pose of a context that never morphed
    both.set_blas_skin(bid, corners, 2)
    both.pose_blas_morph(bid, w1, pal)
    morphed = both.read_blas_triangles(bid, n).tobytes()
    both.pose_blas(bid, pal)
    fresh.set_blas_morph(fid, None)
    fresh.update_blas(fid, tris)
    fresh.set_blas_skin(fid, corners, 2)
    fresh.pose_blas(fid, pal)
    assert both.read_blas_triangles(bid, n).tobytes() == fresh.read_blas_triangles(fid, n).tobytes() != morphed


def test_skin_and_morph_share_one_bind_copy_in_either_order(gpu_ctx_factory):
    tris, d, how = _case("one wave and a lane")
    n = len(tris)
    corners = K.two_joint_skin(tris, 1, 2)
    stored = pod.normalise_skin_corners(corners, 2)
    pal = K.palette("ordinary", 2, _extent(tris), 1)
    w = np.array([0.6, 0.0, -0.4], np.float32)
    a = gpu_ctx_factory(32, 32)
    aid, _nodes, _idx = _install(a, tris, how)
    a.set_blas_skin(aid, corners, 2)
    a.pose_blas(aid, pal)  # (the second to be set must NOT bind this posed shape)
    a.set_blas_morph(aid, d)
    a.pose_blas_morph(aid, w, pal)
    b = gpu_ctx_factory(32, 32)
    bid, _nodes, _idx = _install(b, tris, how)
    b.set_blas_morph(bid, d)
    b.pose_blas_morph(bid, [0.3, 0.3, 0.3])
    b.set_blas_skin(bid, corners, 2)
    b.pose_blas_morph(bid, w, pal)
    both = a.read_blas_triangles(aid, n)
    assert both.tobytes() == b.read_blas_triangles(bid, n).tobytes()
    M.check_morphed_and_posed(both, tris, d, w, stored, pal, "skin then morph")
    # removing either one leaves the other working from the same bind copy
    a.set_blas_morph(aid, None)
    with pytest.raises(capi.NexusError):
        a.pose_blas_morph(aid, w, pal)
    a.pose_blas(aid, pal)
    K.check_posed(a.read_blas_triangles(aid, n), tris, stored, pal, "the skin after the morph went")
    b.set_blas_skin(bid, None, 0)
    with pytest.raises(capi.NexusError):
        b.pose_blas(bid, pal)
    b.pose_blas_morph(bid, w)
    M.check_morphed(b.read_blas_triangles(bid, n), tris, d, w, "the morph after the skin went")


def test_removing_both_leaves_a_context_that_never_had_either(gpu_ctx_factory):
    scene = PB._room(False)
    corners = K.two_joint_skin(scene.meshes[0], 0, 2)
    d = M.deltas(scene.meshes[0], 3, seed=5)
    frames = []
    for had in (True, False):
        ctx = gpu_ctx_factory(W, H)
        scene.upload(ctx)
        ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
        ctx.reset_frame_number()
        if had:
            ctx.set_blas_morph(0, d)
            ctx.set_blas_skin(0, corners, 2)
            ctx.set_blas_skin(0, None, 0)
            ctx.set_blas_morph(0, None)
            with pytest.raises(capi.NexusError):
                ctx.pose_blas_morph(0, ROOM_WEIGHTS)
            with pytest.raises(capi.NexusError):
                ctx.pose_blas(0, PB.STRETCH)
        PB._passes(ctx, 2)
        frames.append((ctx.read_radiance(), ctx.read_rgba8(), ctx.read_blas(0, len(scene.meshes[0]))[0].tobytes()))
    assert SH.frames_identical(frames[0][0], frames[1][0], "frames")
    assert np.array_equal(frames[0][1], frames[1][1]) and frames[0][2] == frames[1][2]


def test_update_blas_on_a_morphed_blas_leaves_the_bind_copy_alone(gpu_ctx_factory):
    tris, d, how = _case("one wave and a lane")
    n = len(tris)
    ctx = gpu_ctx_factory(32, 32)
    bid, _nodes, _idx = _install(ctx, tris, how)
    ctx.set_blas_morph(bid, d)
    w = [0.5, 0.25, 0.75]
    ctx.pose_blas_morph(bid, w)
    posed = ctx.read_blas_triangles(bid, n)
    moved = tris.copy()
    for k in range(3):
        moved["pos%d" % k] += np.float32(0.37)
    ctx.update_blas(bid, moved)
    assert ctx.read_blas_triangles(bid, n).tobytes() == moved.tobytes()
    ctx.pose_blas_morph(bid, w)
    assert ctx.read_blas_triangles(bid, n).tobytes() == posed.tobytes()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_triangles_and_nodes_as_they_were(gpu_ctx_factory):
    tris, d, how = _case("one wave and a lane")
    n = len(tris)
    ctx = gpu_ctx_factory(32, 32)
    bid, _nodes, _idx = _install(ctx, tris, how)
    L = ctx.L
    good = np.ascontiguousarray(d)
    weights = np.array([0.5, 0.25, 0.75], np.float32)
    pal = K.palette("ordinary", 2, 1.0, 1)

    def state():
        return ctx.read_blas_triangles(bid, n).tobytes(), ctx.read_blas(bid, n)[0].tobytes()

    def refused(rc, what):
        assert rc == INVALID, what
        assert L.nxhip_last_error(), what

    def morph(dd, corners=None, targets=None, blas=None):
        dd = np.ascontiguousarray(dd, dtype=pod.MORPH_CORNER_DT)
        return L.nxhip_set_blas_morph(ctx.h, bid if blas is None else blas, dd.ctypes.data, dd.shape[1] if corners is None else corners,
                                      dd.shape[0] if targets is None else targets)

    def pose(w, p=None, joints=None, blas=None):
        w = np.ascontiguousarray(w, dtype=np.float32)
        p = None if p is None else np.ascontiguousarray(p, dtype=np.float32)
        return L.nxhip_pose_blas_morph(ctx.h, bid if blas is None else blas, w.ctypes.data, len(w), None if p is None else p.ctypes.data,
                                       (0 if p is None else len(p)) if joints is None else joints)

    def bad(field, target, corner, axis, value):
        c = good.copy()
        c[field][target, corner, axis] = value
        return c

    for stage in ("nothing", "morph", "morph and skin"):
        if stage == "morph":
            ctx.set_blas_morph(bid, good)
            ctx.pose_blas_morph(bid, weights)
        if stage == "morph and skin":
            ctx.set_blas_skin(bid, K.two_joint_skin(tris, 1, 2), 2)
            ctx.pose_blas_morph(bid, weights, pal)
        before = state()
        refused(morph(good, blas=bid + 1), "bad id")
        refused(morph(good, blas=-1), "bad id")
        refused(morph(good, corners=3 * n - 3), "wrong corner count")
        refused(morph(good[:, :-3]), "wrong corner count")
        refused(morph(good, targets=0), "0 targets")
        refused(morph(np.zeros((1025, 3 * n), pod.MORPH_CORNER_DT)), "1025 targets")
        refused(morph(bad("dPosition", 1, 4, 2, np.nan)), "NaN delta")
        refused(morph(bad("dNormal", 2, 3 * n - 1, 0, np.inf)), "infinite delta")
        refused(morph(bad("dPosition", 0, 0, 0, -np.inf)), "infinite delta")
        if stage == "nothing":
            refused(pose(weights), "a pose without a morph")
        else:
            skinned = stage == "morph and skin"
            p = pal if skinned else None
            refused(pose(weights, p, blas=bid + 1), "bad id")
            refused(pose(weights[:2], p), "another target count")
            refused(pose(np.zeros(4, np.float32), p), "another target count")
            refused(L.nxhip_pose_blas_morph(ctx.h, bid, None, 3, None if p is None else p.ctypes.data, 2 if skinned else 0), "NULL weights")
            for value in (np.nan, np.inf):
                w = weights.copy()
                w[1] = value
                refused(pose(w, p), "a weight that is not finite")
            if skinned:
                refused(pose(weights), "no palette on a skinned BLAS")
                refused(pose(weights, K.palette("ordinary", 3, 1.0, 1)), "another joint count")
                q = pal.copy()
                q[1, 7] = np.nan
                refused(pose(weights, q), "a matrix entry that is not finite")
            else:
                refused(pose(weights, pal), "a palette on an unskinned BLAS")
                refused(pose(weights, None, joints=2), "a joint count on an unskinned BLAS")
        assert state() == before, stage
    # the previous morph and skin are still in place: the same pose gives the same triangles
    posed = ctx.read_blas_triangles(bid, n)
    ctx.pose_blas_morph(bid, np.zeros(3, np.float32), pal)
    ctx.pose_blas_morph(bid, weights, pal)
    assert ctx.read_blas_triangles(bid, n).tobytes() == posed.tobytes()
