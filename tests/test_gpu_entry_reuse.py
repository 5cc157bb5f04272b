"""Entry states outlive the pass (nxhip_render.hip walk_entry_states): a slot's table is walked by a plain launch in front of the pass
that finds it stale and read by every later pass of the slot, until a call changes something the walk reads (nx_context.h
entryGeneration).  nxhip_debug_entry_walks counts the launches, so "reused" and "recomputed" can be told apart.

The comparison context is a second context with entry points off: hit records are bit-equal either way by design, so a stale table
shows up as differing radiance.  Every comparison is bit for bit."""
import numpy as np
import pytest

from nexus_amd import capi, multigpu, pod, scenegen, workloads
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

W = H = 96
FAST = (pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
_SCENES = {}


def _cornell():
    if "cornell" not in _SCENES:
        _SCENES["cornell"] = SH.cornell_scene(W, H, path_length=4)
    return _SCENES["cornell"]


def _torus(nu=96, nv=48):
    """identity instances: the walk goes on through the torus's BLAS, down to its triangles"""
    if "torus" not in _SCENES:
        _SCENES["torus"] = workloads.config2(64, 32, nu, nv, 4, cls=SH.BuiltScene)
    return _SCENES["torus"]


def _ctx(factory, scene, entry, in_flight=1, modes=FAST, per_pass=2):
    w, h = int(scene.camera["resolution"][0]), int(scene.camera["resolution"][1])
    ctx = factory(w, h)
    scene.upload(ctx)
    ctx.set_modes(*modes)
    ctx.set_pixel_order(pod.ORDER_TILES)  # (a run of 64 paths is an 8 x 8 pixel tile, as in the benchmark: most runs start below the root)
    ctx.set_frames_per_pass(per_pass)
    ctx.set_passes_in_flight(in_flight)
    ctx.set_entry_points(entry)
    return ctx


def _passes(ctx, n):
    """n passes from frame 0: every pass's radiance and the accumulation after the last, as bits"""
    ctx.reset_frame_number()
    out = []
    for _ in range(n):
        ctx.render_frame()
        ctx.accumulate()
        out.append(ctx.read_radiance().view(np.uint32).copy())
    return out, ctx.read_accumulation().view(np.uint32).copy()


def _same(a, b):
    return len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])


def _invalidation(factory, scene, change, in_flight, states_change=True):
    """render, change, render: one walk per slot that rendered, before and after; the frames after the change equal those of a fresh
    context without entry points that was given the same change"""
    on = _ctx(factory, scene, True, in_flight)
    before = _passes(on, in_flight)  # every slot renders once
    assert on.debug_entry_walks() == in_flight
    s0 = on.read_entry_states()
    change(on)
    got = _passes(on, in_flight)
    assert on.debug_entry_walks() == 2 * in_flight, "exactly one more walk per slot that rendered"
    s1 = on.read_entry_states()
    again = _passes(on, in_flight)
    assert on.debug_entry_walks() == 2 * in_flight and _same(again, got), "and none after that"
    off = _ctx(factory, scene, False, in_flight)
    change(off)
    want = _passes(off, in_flight)
    assert off.debug_entry_walks() == 0
    assert _same(got, want), "a stale entry table (or a wrong one) renders another image"
    if states_change:  # (the change does reach the walk: the old table would have been the wrong one)
        assert s0.shape != s1.shape or not np.array_equal(s0, s1)
    print("runs that start below the root: %.2f before, %.2f after the change" % ((s0[:, 19] >= 1).mean(), (s1[:, 19] >= 1).mean()))
    assert (s0[:, 19] >= 1).any() and (s1[:, 19] >= 1).any(), "some runs start below the root: the table matters to the image"
    on.close()
    off.close()
    return before, got


@pytest.mark.parametrize("in_flight", [1, 3])
def test_four_passes_with_nothing_changed_walk_once_per_slot(gpu_ctx_factory, in_flight):
    for scene in (_cornell(), _torus()):
        on, off = _ctx(gpu_ctx_factory, scene, True, in_flight), _ctx(gpu_ctx_factory, scene, False, in_flight)
        got, want = _passes(on, 4), _passes(off, 4)
        assert on.debug_entry_walks() == min(4, in_flight) and off.debug_entry_walks() == 0
        assert _same(got, want)
        assert (on.read_entry_states()[:, 19] >= 1).any()
        # ... and four more, from frame 0 again (the frame number is not an input)
        assert _same(_passes(on, 4), want) and on.debug_entry_walks() == min(4, in_flight)
        on.close()
        off.close()


@pytest.mark.parametrize("in_flight", [1, 2])
def test_a_moved_camera_walks_again(gpu_ctx_factory, in_flight):
    fwd = np.array((-0.45, -0.1, -1.0))
    cam = capi.camera_init((1.1, 1.5, 3.4), fwd / np.linalg.norm(fwd), 40.0, W, H, 5.0, 0.0)
    before, after = _invalidation(gpu_ctx_factory, _cornell(), lambda ctx: ctx.set_camera(cam), in_flight)
    assert not np.array_equal(before[1], after[1])
    # (the same camera again is no change: nxhip_set_camera compares)
    on = _ctx(gpu_ctx_factory, _cornell(), True)
    _passes(on, 1)
    on.set_camera(_cornell().camera)
    _passes(on, 1)
    assert on.debug_entry_walks() == 1
    on.close()


def test_a_resize_walks_again(gpu_ctx_factory):
    def change(ctx):
        ctx.resize(80, 56)
        ctx.set_camera(capi.camera_init((0.0, 1.0, 3.9), (0.0, 0.0, -1.0), 40.0, 80, 56, 5.0, 0.0))

    _invalidation(gpu_ctx_factory, _cornell(), change, 1)
    _invalidation(gpu_ctx_factory, _cornell(), change, 2)


def test_a_tile_split_pixel_map_walks_again(gpu_ctx_factory):
    pm = multigpu.tiled_order(multigpu.tile_pixel_map(W, H, 1, 2, 8), W)  # rank 1 of 2
    _invalidation(gpu_ctx_factory, _cornell(), lambda ctx: ctx.set_pixel_map(pm), 1)
    _invalidation(gpu_ctx_factory, _cornell(), lambda ctx: ctx.set_pixel_map(pm), 2)


def test_the_pixel_order_walks_again_both_ways(gpu_ctx_factory):
    scene = _cornell()
    on, off = _ctx(gpu_ctx_factory, scene, True), _ctx(gpu_ctx_factory, scene, False)
    walks = 0
    for order in (pod.ORDER_ROWS, pod.ORDER_TILES, pod.ORDER_ROWS, pod.ORDER_TILES):
        for ctx in (on, off):
            ctx.set_pixel_order(order)
        got, want = _passes(on, 2), _passes(off, 2)
        walks += 1
        assert on.debug_entry_walks() == walks and _same(got, want), order
    on.close()
    off.close()


@pytest.mark.parametrize("in_flight", [1, 2])
def test_entry_points_off_then_on_walk_again(gpu_ctx_factory, in_flight):
    scene = _cornell()
    on, off = _ctx(gpu_ctx_factory, scene, True, in_flight), _ctx(gpu_ctx_factory, scene, False, in_flight)
    want = _passes(off, in_flight)
    assert _same(_passes(on, in_flight), want) and on.debug_entry_walks() == in_flight
    on.set_entry_points(False)
    assert _same(_passes(on, in_flight), want) and on.debug_entry_walks() == in_flight and len(on.read_entry_states()) == 0
    on.set_entry_points(True)
    assert _same(_passes(on, in_flight), want) and on.debug_entry_walks() == 2 * in_flight
    assert (on.read_entry_states()[:, 19] >= 1).any()
    on.close()
    off.close()


@pytest.mark.parametrize("which", ["cornell", "torus"])
def test_a_rebuilt_tlas_with_a_moved_instance_walks_again(gpu_ctx_factory, which):
    scene = _cornell() if which == "cornell" else _torus()
    insts = scene.instances.copy()
    k = 0 if which == "torus" else len(insts) - 1
    xf = insts[k]["transform"].copy()
    xf[[3, 7, 11]] += np.array((0.35, 0.2, -0.3), np.float32)  # (row-major: the translation column)
    b = int(insts[k]["bvhIdx"])
    insts[k] = capi.instance_init(b, int(insts[k]["materialId"]), xf, scene.blas[b][0][0])
    for in_flight in (1, 2):
        before, after = _invalidation(gpu_ctx_factory, scene, lambda ctx: ctx.rebuild_tlas(insts), in_flight)
        assert not np.array_equal(before[1], after[1])


def test_instance_transforms_set_on_the_device_walk_again(gpu_ctx_factory):
    scene = _torus()
    xf = capi.mat4_from_trs((0.3, 0.25, -0.2), (0, 0, 0), (1, 1, 1))
    _invalidation(gpu_ctx_factory, scene, lambda ctx: ctx.set_instance_transforms(np.array([0], np.uint32), xf.reshape(1, 16)), 1)


def test_an_updated_blas_walks_again_behind_its_deferred_refresh(gpu_ctx_factory):
    scene = _torus()
    base = scene.blas[0][1]
    moved = scenegen.displaced_torus(96, 48, seed=7, major=1.0, minor=0.52, amp=0.12, center=(0.0, 0.66, 0.0))  # same topology, other vertices
    assert len(moved) == len(base)
    for in_flight in (1, 2):
        before, after = _invalidation(gpu_ctx_factory, scene, lambda ctx: ctx.update_blas(0, moved), in_flight)
        assert not np.array_equal(before[1], after[1])


def test_a_material_type_walks_again(gpu_ctx_factory):
    """An entry state carries the instance index WITH its material code (InstTrav::instIdx), which the SCAN pipeline's hit records hand to
    the material launch: a table from before nxhip_set_materials would send the hits of a consumed triangle to the old type's code."""
    scene = _torus()
    mats = scene.materials.copy()
    mats["type"][1] = pod.MAT_PLASTIC  # the floor
    _invalidation(gpu_ctx_factory, scene, lambda ctx: ctx.set_materials(mats), 1, states_change=False)  # (only the states inside the floor's instance change)


def test_an_adaptive_active_set_update_walks_again(gpu_ctx_factory):
    """The table is indexed by the runs of the ACTIVE set: after blocks are culled, run k is another tile of the image."""
    scene = _cornell()
    ctxs = [_ctx(gpu_ctx_factory, scene, entry) for entry in (True, False)]
    threshold = None
    for ctx in ctxs:
        ctx.reset_frame_number()
        ctx.set_adaptive(threshold=0.0, lum_floor=0.01, min_samples=4, cull=1)
        for _ in range(2):
            ctx.render_frame()
            ctx.accumulate()
        ctx.adaptive_update()
        if threshold is None:
            bmax, _ = ctx.read_block_noise()
            threshold = float(np.median(bmax[bmax > 0]))
        ctx.set_adaptive(threshold=threshold, lum_floor=0.01, min_samples=4, cull=1)
    on, off = ctxs
    on.render_frame()  # (whatever the first update did to the set: the table is current from here on)
    on.accumulate()
    off.render_frame()
    off.accumulate()
    walks = on.debug_entry_walks()
    active = [ctx.adaptive_update()[0] for ctx in ctxs]
    assert active[0] == active[1] and 0 < active[0] < W * H, "some blocks culled, some alive"
    for _ in range(2):
        for ctx in ctxs:
            ctx.render_frame()
            ctx.accumulate()
    assert on.debug_entry_walks() == walks + 1 and off.debug_entry_walks() == 0
    assert np.array_equal(on.read_sample_counts(), off.read_sample_counts())
    assert np.array_equal(on.read_accumulation().view(np.uint32), off.read_accumulation().view(np.uint32))
    for ctx in ctxs:
        ctx.close()


def test_pass_size_and_modes_are_not_inputs(gpu_ctx_factory):
    scene = _cornell()
    on, off = _ctx(gpu_ctx_factory, scene, True), _ctx(gpu_ctx_factory, scene, False)
    assert _same(_passes(on, 1), _passes(off, 1)) and on.debug_entry_walks() == 1
    steps = [("frames per pass", lambda c: c.set_frames_per_pass(3)),
             ("frames per pass", lambda c: c.set_frames_per_pass(1)),
             # (the compaction first: slot-keyed random numbers give a reproducible image only with the ordered compaction's slots)
             ("compaction mode", lambda c: c.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_ORDERED, pod.CONDUCTOR_REFERENCE)),
             ("RNG mode", lambda c: c.set_modes(pod.RNG_REFERENCE_SLOT, pod.COMPACT_ORDERED, pod.CONDUCTOR_REFERENCE)),
             ("conductor mode", lambda c: c.set_modes(pod.RNG_REFERENCE_SLOT, pod.COMPACT_ORDERED, pod.CONDUCTOR_EXTENDED)),
             ("all three modes back", lambda c: c.set_modes(*FAST)),
             ("light sampling", lambda c: c.set_light_sampling(pod.LIGHTS_POWER)),
             ("tail bounce", lambda c: c.set_tail_bounce(2))]
    for what, step in steps:
        step(on)
        step(off)
        assert _same(_passes(on, 2), _passes(off, 2)), what
        assert on.debug_entry_walks() == 1, what
    on.close()
    off.close()
