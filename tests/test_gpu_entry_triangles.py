"""Entry states that walk past the first triangles (nx_entry.hip): a triangle every ray of a run misses is skipped, one every ray
hits is consumed — its record travels in the entry state and every ray computes its own hit for it at install — and the run's
hit-distance interval bounds the boxes behind it.  The bar: every frame equals the frame without entry points bit for bit."""
import numpy as np
import pytest

from nexus_amd import capi, multigpu, pod, scenegen, workloads
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

# columns of Context.read_entry_states()
STEPS, LEAF_TG, TRI_LEAF, SKIPPED, INST_WORD = 19, 15, 31, 35, 37
INST_INDEX = (1 << 29) - 1  # the instance index in an instance word (the material type rides above it)


def _frames(ctx, n, per_pass=1, in_flight=1):
    ctx.set_frames_per_pass(per_pass)
    ctx.set_passes_in_flight(in_flight)
    ctx.reset_frame_number()
    out = []
    for _ in range(n // per_pass):
        ctx.render_frame()
        ctx.accumulate()
        out.append(ctx.read_radiance())
    return out, ctx.read_accumulation()


def _box(lo, hi):
    """the six faces of an axis-aligned box, twelve triangles"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    faces = [((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)), ((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)),
             ((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)), ((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)),
             ((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)), ((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1))]
    return np.concatenate([scenegen.quad(*f) for f in faces])


def _scene(W, H, eye, fwd, torus_xform=workloads.IDENTITY, hfov=60.0, torus=None):
    if torus is None:
        torus = scenegen.displaced_torus(96, 48, seed=3, major=1.0, minor=0.45, amp=0.05, center=(0.0, 0.5, 0.0))
    floor = scenegen.quad((-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6))
    light = scenegen.quad((-1.2, 4.0, -1.2), (1.2, 4.0, -1.2), (1.2, 4.0, 1.2), (-1.2, 4.0, 1.2))
    mats = np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(0.6, 0.5, 0.4)), pod.make_material(pod.MAT_DIFFUSE, albedo=(0.7, 0.7, 0.7)),
                     pod.make_material(pod.MAT_DIFFUSE, albedo=(0.8, 0.8, 0.8), emissive=(1.0, 1.0, 1.0), intensity=20.0)], dtype=pod.MAT_DT)
    f = np.asarray(fwd, np.float64)
    cam = capi.camera_init(eye, f / np.linalg.norm(f), hfov, W, H, 5.0, 0.0)
    scene = SH.BuiltScene([torus, floor, light], [(0, 0, torus_xform), (1, 1, workloads.IDENTITY), (2, 2, workloads.IDENTITY)], materials=mats, camera=cam,
                          settings=workloads.make_settings(use_mis=True, path_length=3, background=(0.2, 0.3, 0.4), background_intensity=1.0))
    scene.lights = SH.mesh_lights(scene.instances, scene.materials)
    return scene


def _on_off(ctx_factory, scene, W, H, n=2, per_pass=1, in_flight=1):
    """frames without and with entry points (bit-equal) and the entry states of the last pass"""
    ctx = ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.set_pixel_map(multigpu.tiled_order(np.arange(W * H, dtype=np.uint32), W))
    base, base_acc = _frames(ctx, n)
    ctx.set_entry_points(True)
    got, got_acc = _frames(ctx, n, per_pass, in_flight)
    states = ctx.read_entry_states()
    if per_pass == 1:
        for k in range(n):
            assert np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)), "frame %d" % k
    assert np.array_equal(got_acc.view(np.uint32), base_acc.view(np.uint32))
    return states


def test_runs_consume_and_skip_the_floor_triangles(gpu_ctx_factory):
    """The view of configs[1]: runs on the floor consume the floor triangle they all hit and skip the one they all miss, then walk on."""
    W, H = 256, 144
    states = _on_off(gpu_ctx_factory, _scene(W, H, (0.0, 3.3, 4.9), (0.0, -2.95, -4.9)), W, H)
    consumed = states[:, TRI_LEAF] >= 0
    skipped = states[:, SKIPPED] > 0
    print("runs: %.2f consumed a triangle, %.2f skipped one, %.2f walked 3 steps or more"
          % (consumed.mean(), skipped.mean(), (states[:, STEPS] >= 3).mean()))
    assert consumed.mean() > 0.2 and skipped.mean() > 0.2
    lo = states[consumed, 38].view(np.float32)
    hi = states[consumed, 39].view(np.float32)
    assert np.all(lo > 0.0) and np.all(lo <= hi) and np.all(states[~consumed, 39].view(np.float32) == np.float32(1e30))


def test_a_grazing_floor_ends_the_walk_undecided(gpu_ctx_factory):
    """A camera just above the floor looking along it: near the horizon the floor is neither hit nor missed by every ray of a run, and
    those runs must stop in front of its triangles (pending leaf bits in the state)."""
    W, H = 192, 128
    states = _on_off(gpu_ctx_factory, _scene(W, H, (0.0, 0.002, 5.5), (0.0, -0.05, -1.0)), W, H)
    stopped_at_triangles = (states[:, LEAF_TG] != 0) & (states[:, STEPS] >= 1)
    on_floor = stopped_at_triangles & ((states[:, INST_WORD] & INST_INDEX) == 1)
    print("runs stopped in front of an undecided triangle: %.2f, of the floor: %.2f" % (stopped_at_triangles.mean(), on_floor.mean()))
    # (those runs stopped at a floor triangle they could not decide, and consumed none: the same walk consumes and skips the floor's
    #  triangles where the view is not grazing — the first test)
    assert on_floor.any() and np.all(states[on_floor, TRI_LEAF] == -1)


@pytest.mark.parametrize("box", [((0.2, -0.3, 0.2), (0.8, 0.9, 0.8)), ((0.2, -0.02, 0.2), (0.8, 0.9, 0.8))])
def test_an_instance_that_pierces_the_floor(gpu_ctx_factory, box):
    """A box that goes through the floor, the camera aimed at its contact corner with a narrow view (runs 2-4 cm across straddle the
    corner): runs that consume the floor triangle must not take the box's instance or its nodes for missed — parts of it lie in
    front of the floor for some of their rays."""
    W, H = 256, 144
    corner = np.array((box[1][0], 0.0, box[1][2]))
    eye = corner + (1.2, 1.4, 2.6)
    scene = _scene(W, H, tuple(eye), tuple(corner - eye), hfov=8.0, torus=_box(*box))
    states = _on_off(gpu_ctx_factory, scene, W, H)
    print("runs: %.2f consumed a triangle, %.2f walked 3 steps or more" % ((states[:, TRI_LEAF] >= 0).mean(), (states[:, STEPS] >= 3).mean()))
    assert (states[:, TRI_LEAF] >= 0).any()


def test_rotated_instances_stop_the_walk_in_front(gpu_ctx_factory):
    """A rotated torus: the scene is no longer one of identity instances, so the walk never enters an instance (no triangle
    consumed), and the frames stay the same."""
    W, H = 192, 128
    a = np.radians(30.0)
    rot = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]], np.float32).reshape(16)
    states = _on_off(gpu_ctx_factory, _scene(W, H, (0.0, 3.3, 4.9), (0.0, -2.95, -4.9), torus_xform=rot), W, H)
    assert np.all(states[:, TRI_LEAF] == -1) and np.all(states[:, 17] == -1)


def test_two_passes_in_flight(gpu_ctx_factory):
    """Two passes in flight, each with its own entry table holding consumed triangles: the accumulated image is unchanged."""
    W, H = 256, 144
    states = _on_off(gpu_ctx_factory, _scene(W, H, (0.0, 3.3, 4.9), (0.0, -2.95, -4.9)), W, H, n=8, per_pass=2, in_flight=2)
    assert (states[:, TRI_LEAF] >= 0).any()


def test_configs1_runs_walk_deeper(gpu_ctx_factory):
    """configs[1] as bench.py renders it (1920 x 1080, 8 x 8 tiles): at least half of the runs get three node steps or more (entry
    states that end at the first triangles: two steps for 97.5 % of them)."""
    W, H = 1920, 1080
    scene = workloads.config2(W, H, cls=SH.BuiltScene)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    ctx.set_pixel_map(multigpu.tiled_order(np.arange(W * H, dtype=np.uint32), W))
    ctx.set_entry_points(True)
    ctx.set_frames_per_pass(1)
    ctx.reset_frame_number()
    ctx.render_frame()
    states = ctx.read_entry_states()
    deep = float((states[:, STEPS] >= 3).mean())
    print("configs[1]: %.3f of the runs walk 3 steps or more, %.3f consume a triangle" % (deep, (states[:, TRI_LEAF] >= 0).mean()))
    assert deep >= 0.5
