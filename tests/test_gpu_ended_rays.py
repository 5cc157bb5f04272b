"""Continuation rays the Russian roulette has already ended (nx_wavefront.h shade_scan_type, kShadeDropEnded): under the SCAN
pipeline with pixel-keyed random numbers and no miss type in the pass (no environment map, black background) the material launch
does not queue a continuation ray whose roulette draw it has just lost — nothing could read what such a ray hits.  The bar: every
frame, accumulation, RGBA8 image and queue size stays the oracle's (which queues and traces those rays), the drop is off wherever a
miss can contribute or the draw is keyed by the slot, and a change of background rebuilds the pass."""
import os

import numpy as np
import pytest

from nexus_amd import capi, pod, workloads
from tests import oracle_lib as O
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

FAST = (pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)


def _floor_and_mesh(W, H, path_length=6, background_intensity=0.0):
    scene = workloads.config2(W, H, 128, 64, path_length, cls=SH.BuiltScene)
    scene.settings = O.make_settings(use_mis=True, path_length=path_length, background=(1, 1, 1), background_intensity=background_intensity)
    return scene


def _ended(ctx, path_length):
    """ended rays per bounce slot 0 .. path_length (the device's count of what it did not queue, last pass)"""
    return [ctx.debug_ended_rays_of_pass(b) for b in range(path_length + 1)]


def _oracle_passes(scene, n, passes, per_pass, modes=FAST, pixel_map=None):
    """The oracle's frames 1 .. passes * per_pass; returns the radiance slices and summed queue sizes of the LAST pass, the
    accumulation and the RGBA8 image after it."""
    w = O.Wavefront(scene.oracle(), n, pixel_map, modes[0], modes[2])
    rad, q = [], None
    for f in range(1, passes * per_pass + 1):
        w.render(f, threads=8)
        w.accumulate(f)
        if f > (passes - 1) * per_pass:
            rad.append(w.radiance().copy())
            qs = w.queue_sizes()
            q = qs if q is None else {k: q[k] + qs[k] for k in qs}
    out = np.concatenate(rad), q, w.accumulation().copy(), w.rgba8().copy()
    w.close()
    return out


def _device_passes(ctx, passes):
    ctx.reset_frame_number()
    for _ in range(passes):
        ctx.render_frame()
        ctx.accumulate()
    return ctx.read_radiance(), ctx.read_queue_sizes(), ctx.read_accumulation(), ctx.read_rgba8()


def _same(got, want, what):
    assert SH.frames_identical(got[0], want[0], what), what
    assert SH.queue_sizes_identical(got[1], want[1]), what  # (all words of every queue)
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), what + ": accumulation"
    assert np.array_equal(got[3], want[3]), what + ": RGBA8"


def test_black_background_equals_the_oracle_and_rays_are_dropped(gpu_ctx_factory):
    """(a) floor + mesh, black background, several frames per pass, two passes in flight"""
    W, H, L, PER, PASSES = 192, 108, 6, 3, 3
    scene = _floor_and_mesh(W, H, L)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(*FAST)
    ctx.set_tail_bounce(0)  # (the queue sizes of every bounce are compared)
    ctx.set_frames_per_pass(PER)
    ctx.set_passes_in_flight(2)
    got = _device_passes(ctx, PASSES)
    want = _oracle_passes(scene, W * H, PASSES, PER)
    ended = _ended(ctx, L)
    reported = [int(x) for x in got[1]["traceSize"][:L + 1]]
    print("ended rays per bounce %s of reported trace sizes %s" % (ended, reported))
    _same(got, want, "floor and mesh, black background")
    assert ended[0] == 0 and ended[L] == 0, "primary rays and the last bounce queue nothing to drop"
    assert all(0 <= e <= r for e, r in zip(ended, reported))
    assert 0 < sum(ended) < sum(reported[1:]), "the drop did run, and did not take every ray"
    assert ended[1] > 0.1 * reported[1], "a 0.7 floor in half the view ends a good share of the first continuation rays"
    ctx.set_passes_in_flight(1)


def test_every_material_type_and_pass_through_with_a_black_background(gpu_ctx_factory):
    """(a') the material zoo without its map and with a black background: all four types, opacity / alpha pass-through
    continuations (whose draw uses the throughput the path arrived with), emissive hits under MIS; then with the tail kernel behind it"""
    W, H, L = 96, 64, 5
    scene = SH.material_zoo_scene(W, H, path_length=L, hdr=False)
    scene.settings = O.make_settings(use_mis=True, path_length=L, background=(0.6, 0.7, 0.9), background_intensity=0.0)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(*FAST)
    ctx.set_tail_bounce(0)
    got = _device_passes(ctx, 3)
    want = _oracle_passes(scene, W * H, 3, 1)
    ended = _ended(ctx, L)
    print("material zoo, black background: ended rays per bounce %s of %s" % (ended, got[1]["traceSize"][:L + 1].tolist()))
    _same(got, want, "material zoo, black background")
    assert sum(ended) > 0
    # ... and with the tail kernel taking the late bounces (it reports no queue sizes: frames only)
    ctx.set_tail_bounce(3)
    tail = _device_passes(ctx, 3)
    assert SH.frames_identical(tail[0], want[0], "material zoo, black background, tail kernel from bounce 3")
    assert np.array_equal(tail[2].view(np.uint32), want[2].view(np.uint32))


def test_stale_queue_contents_do_not_show(gpu_ctx_factory):
    """(b) view A, another view B, then A again from frame 1 in the same context: the slots the shorter queues no longer write
    hold records of earlier passes — the second A equals the first bit for bit"""
    W, H, L = 192, 108, 6
    scene = _floor_and_mesh(W, H, L)
    cam_a = scene.camera
    cam_b = workloads._look((2.5, 1.2, 3.0), (0.0, 0.5, 0.0), 35.0, W, H)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(*FAST)
    ctx.set_tail_bounce(0)
    ctx.set_frames_per_pass(2)
    first = _device_passes(ctx, 2)
    ctx.set_camera(cam_b)
    other = _device_passes(ctx, 2)
    assert not np.array_equal(other[0], first[0])
    ctx.set_camera(cam_a)
    again = _device_passes(ctx, 2)
    _same(again, first, "view A after view B")
    assert sum(_ended(ctx, L)) > 0


def test_a_background_that_is_not_black_keeps_every_ray(gpu_ctx_factory):
    """(c) a miss can contribute: the drop is off — a faint flat background, and the material zoo under its environment map"""
    W, H, L = 160, 90, 6
    scene = _floor_and_mesh(W, H, L, background_intensity=1.0e-3)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(*FAST)
    ctx.set_tail_bounce(0)
    ctx.set_frames_per_pass(2)
    got = _device_passes(ctx, 2)
    want = _oracle_passes(scene, W * H, 2, 2)
    _same(got, want, "faint background")
    assert _ended(ctx, L) == [0] * (L + 1)

    W, H, L = 96, 64, 5
    zoo = SH.material_zoo_scene(W, H, path_length=L)
    ctx = gpu_ctx_factory(W, H)
    zoo.upload(ctx)
    ctx.set_modes(*FAST)
    ctx.set_tail_bounce(0)
    got = _device_passes(ctx, 3)
    want = _oracle_passes(zoo, W * H, 3, 1)
    _same(got, want, "material zoo under its environment map")
    assert _ended(ctx, L) == [0] * (L + 1)


SLOT_KEYED_GOLDEN = os.path.join(SH.GOLDEN, "ended_rays_slot_keyed_scan.bin")


def slot_keyed_scan_frames(ctx):
    """(d)'s calls: the Cornell box (one material type in the pass) at 32 x 16, slot-keyed random numbers, SCAN pipeline, six
    one-frame passes.  Slot-keyed numbers under racing compaction follow the order in which waves and workgroups reach their
    atomics, so the mode is reproducible only where that order is fixed: 512 paths are 64 per queue region — one workgroup per
    region, and in it one wave that finds and numbers every item.  Returns the frames (float32 [6][512][3]) and the last pass's
    queue sizes."""
    W, H = 32, 16
    scene = SH.cornell_scene(W, H, path_length=5)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_REFERENCE_SLOT, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.set_tail_bounce(0)
    ctx.reset_frame_number()
    frames = []
    for _ in range(6):
        ctx.render_frame()
        ctx.accumulate()
        frames.append(ctx.read_radiance())
    return np.stack(frames).astype(np.float32), ctx.read_queue_sizes()


def test_slot_keyed_numbers_keep_todays_behaviour(gpu_ctx_factory):
    """(d) slot-keyed random numbers under the SCAN pipeline: the draw is keyed by the slot the ray goes to, so nothing is
    dropped, and the frames are the ones the library rendered before this change (tests/golden/ended_rays_slot_keyed_scan.bin:
    the parent commit's output of slot_keyed_scan_frames, float32 radiance then int32 traceSize / traceShadowSize / diffuseSize [6])"""
    ctx = gpu_ctx_factory(32, 16)
    frames, q = slot_keyed_scan_frames(ctx)
    assert _ended(ctx, 5) == [0] * 6
    raw = np.fromfile(SLOT_KEYED_GOLDEN, dtype=np.uint32)
    n = frames.size
    assert raw.size == n + 18
    same = frames.view(np.uint32).reshape(-1) == raw[:n]
    print("slot-keyed SCAN frames: %d of %d words equal the parent's" % (int(same.sum()), n))
    assert same.all()
    sizes = np.concatenate([np.asarray(q[k][:6], np.int32) for k in ("traceSize", "traceShadowSize", "diffuseSize")])
    print("queue sizes %s, the parent's %s" % (sizes.tolist(), raw[n:].view(np.int32).tolist()))
    assert np.array_equal(sizes.view(np.uint32), raw[n:])


def test_switching_the_background_rebuilds_the_pass(gpu_ctx_factory):
    """(e) black -> not black -> black between passes of one context: each equals the oracle's, and the drop follows the shape"""
    W, H, L = 160, 90, 6
    ctx = gpu_ctx_factory(W, H)
    scene = _floor_and_mesh(W, H, L)
    scene.upload(ctx)
    ctx.set_modes(*FAST)
    ctx.set_tail_bounce(0)
    for k, intensity in enumerate((0.0, 2.0e-3, 0.0)):
        scene.settings = O.make_settings(use_mis=True, path_length=L, background=(1, 1, 1), background_intensity=intensity)
        ctx.set_render_settings(scene.settings)
        got = _device_passes(ctx, 2)
        want = _oracle_passes(scene, W * H, 2, 1)
        _same(got, want, "background intensity %g (step %d)" % (intensity, k))
        ended = sum(_ended(ctx, L))
        assert (ended > 0) == (intensity == 0.0), (intensity, ended)
    # ... and a change of the random-number mode alone: slot-keyed numbers keep every ray, pixel-keyed ones drop again
    ctx.set_modes(pod.RNG_REFERENCE_SLOT, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    _device_passes(ctx, 1)
    assert sum(_ended(ctx, L)) == 0
    ctx.set_modes(*FAST)
    got = _device_passes(ctx, 2)
    _same(got, want, "pixel-keyed numbers again")
    assert sum(_ended(ctx, L)) > 0
