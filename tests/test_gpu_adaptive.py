"""Adaptive sampling on the device: nxhip_set_adaptive / adaptive_update / render_adaptive and the read-backs (include/nexus_hip.h).

Reference: a SECOND, plain context on the same scene that renders frame by frame — with pixel-keyed random numbers a path's radiance is a
function of (global pixel, frame) only, and the plain device path is pinned against the oracle elsewhere — together with the numpy
restatement of the bookkeeping (tests/adaptive_reference.py, checked on synthetic data by tests/test_adaptive_reference.py).  Everything
is compared bit for bit; no tolerance appears in this file.
"""
import ctypes as C

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import adaptive_reference as A
from tests import feature_scenes as FS
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

MAX_FRAMES, INTERVAL, MIN_SAMPLES, LUM_FLOOR = 48, 4, 8, 0.01


def _zoo():
    zoo = SH.material_zoo_scene(96, 64)
    zoo.camera["lensRadius"] = 0.0
    return zoo


def _small_cornell():
    sc = SH.cornell_scene(40, 30, path_length=4)
    return sc


SCENES = {
    "cornell": (lambda: SH.cornell_scene(64, 64, path_length=4), 64, 64),  # 64 blocks
    "zoo": (_zoo, 96, 64),                                                 # 96 blocks
    "partial": (_small_cornell, 40, 30),                                   # 18 blocks and one of 48 pixels
    "all features": (lambda: FS.all_features_scene(64, 48), 64, 48),       # 48 blocks; every shading feature on (tests/feature_scenes.py)
}


def _ctx(factory, sc, W, H, compact=pod.COMPACT_FAST, order=pod.ORDER_ROWS, entry=False, per_pass=1, in_flight=1, aov=False):
    ctx = factory(W, H)
    sc.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, compact, pod.CONDUCTOR_EXTENDED)
    ctx.reset_frame_number()
    if order != pod.ORDER_ROWS:
        ctx.set_pixel_order(order)
    if entry:
        ctx.set_entry_points(True)
    ctx.set_frames_per_pass(per_pass)
    ctx.set_passes_in_flight(in_flight)
    if aov:
        ctx.set_aov(True)
    return ctx


_REFERENCE = {}


def _reference(factory, name):
    """The plain context's record of `name`, made once: per-frame radiance (and feature buffers), accumulation and RGBA8 after 12 frames and
    after all of them.  Row order."""
    if name not in _REFERENCE:
        make, W, H = SCENES[name]
        sc = make()
        ctx = _ctx(factory, sc, W, H, aov=True)
        rec = dict(scene=sc, W=W, H=H, radiance=[], aov=[], acc={}, rgba8={})
        for f in range(1, MAX_FRAMES + 1):
            ctx.render_frame()
            rec["radiance"].append(ctx.read_radiance())
            ctx.accumulate()
            rec["aov"].append(ctx.read_aov_frame())
            if f in (12, MAX_FRAMES):
                rec["acc"][f], rec["rgba8"][f] = ctx.read_accumulation(), ctx.read_rgba8()
        ctx.close()
        _REFERENCE[name] = rec
    return _REFERENCE[name]


def _threshold(rec):
    """the median over blocks of the block's largest e after MIN_SAMPLES frames of the reference data"""
    sim = A.Simulator(len(rec["radiance"][0]), 0.0, LUM_FLOOR, MIN_SAMPLES, cull=False)
    for f in range(MIN_SAMPLES):
        sim.fold(rec["radiance"][f])
    sim.update()
    return float(np.median(sim.block_max))


def _simulated(rec, cull=True, extras=False):
    thr = _threshold(rec)
    sim, hist = A.run(rec["radiance"], thr, LUM_FLOOR, MIN_SAMPLES, cull, INTERVAL, MAX_FRAMES, extras=rec["aov"] if extras else None)
    blocks = sim.blocks
    first = hist[MIN_SAMPLES // INTERVAL - 1]  # the first decision at which a pixel can have settled
    share = 1.0 - first["active_blocks"] / blocks
    print("threshold %.6g: blocks alive after each decision %s of %d; culled at the first decision %.3f" % (thr, [h["active_blocks"] for h in hist], blocks, share))
    assert 0.10 <= share <= 0.90, "the scene does not exercise the decision: choose another one"
    assert hist[MIN_SAMPLES // INTERVAL + 1]["active_blocks"] >= 1, "nothing left to render two decisions later"
    return thr, sim, hist


def _rows(ctx_order, W, H, *arrays):
    """arrays in the context's base order -> row order"""
    if ctx_order == pod.ORDER_ROWS:
        return arrays
    pm = capi.tile_pixel_map(W, H, 1, 0, 1, tiled=True)
    out = []
    for a in arrays:
        r = np.zeros_like(a)
        r[pm] = a
        out.append(r)
    return out


def _estimate_only(factory, rec, frames=12, **how):
    in_flight, per_pass, order = how.get("in_flight", 1), how.get("per_pass", 1), how.get("order", pod.ORDER_ROWS)
    ctx = _ctx(factory, rec["scene"], rec["W"], rec["H"], **how)
    ctx.set_adaptive(threshold=0.0, lum_floor=LUM_FLOOR, min_samples=MIN_SAMPLES, cull=0)
    radiance = []
    for _ in range(frames // per_pass // in_flight):
        for _ in range(in_flight):
            ctx.render_frame()
            if in_flight == 1:
                radiance.append(ctx.read_radiance())
        ctx.accumulate()
    decided = ctx.adaptive_update()
    assert ctx.frame_number() == frames
    assert ctx.active_count() == ctx.local_count, "estimate only: nothing is ever deactivated"
    out = _rows(order, rec["W"], rec["H"], ctx.read_sample_counts(), ctx.read_noise_stats(), ctx.read_accumulation(), ctx.read_rgba8())
    ctx.close()
    return list(out) + [radiance, decided]


def _numpy_stats(rec, frames):
    sim = A.Simulator(len(rec["radiance"][0]), 0.0, LUM_FLOOR, MIN_SAMPLES, cull=False)
    for f in range(frames):
        sim.fold(rec["radiance"][f])
    return sim


@pytest.mark.parametrize("name", ["cornell", "partial"])
def test_estimate_only_leaves_the_image_alone_and_gives_the_numpy_statistics(gpu_ctx_factory, name):
    rec = _reference(gpu_ctx_factory, name)
    count, stats, acc, rgba8, radiance, decided = _estimate_only(gpu_ctx_factory, rec)
    for f, r in enumerate(radiance):
        assert A.same_bits(r, rec["radiance"][f]), "radiance of frame %d" % (f + 1)
    assert A.same_bits(acc, rec["acc"][12]) and np.array_equal(rgba8, rec["rgba8"][12])
    assert np.all(count == 12)
    sim = _numpy_stats(rec, 12)
    assert A.same_bits(stats[:, 0], sim.mean) and A.same_bits(stats[:, 1], sim.m2)
    assert A.same_bits(acc, sim.acc)
    assert decided == sim.update(), "threshold 0: a block settles only if none of its pixels shows any variance"
    assert np.all(stats[:, 1] >= 0) and stats[:, 1].max() > 0
    variants = {
        "3 frames per pass": dict(per_pass=3),
        "3 passes in flight": dict(in_flight=3),
        "tile order": dict(order=pod.ORDER_TILES),
        "tile order + entry points": dict(order=pod.ORDER_TILES, entry=True),
        "ordered compaction": dict(compact=pod.COMPACT_ORDERED),
    }
    if name == "partial":
        variants = {k: variants[k] for k in ("3 frames per pass", "tile order + entry points")}
    for what, how in variants.items():
        c2, s2, a2, p2, _, d2 = _estimate_only(gpu_ctx_factory, rec, **how)
        assert np.array_equal(c2, count), what
        if "tile" not in what:  # (tiles are other blocks)
            assert d2 == decided, what
        assert A.same_bits(s2, stats), what
        assert A.same_bits(a2, acc) and np.array_equal(p2, rgba8), what


def _hand_driven(ctx, rec, hist, check=True):
    """{INTERVAL x (render_frame, accumulate), adaptive_update} until the simulator stops; after every update the device's state against
    the simulator's.  Returns per decision (counts, accumulation, rgba8)."""
    snaps, frame = [], 0
    active = np.arange(ctx.local_count)
    for k, want in enumerate(hist):
        for _ in range(want["frames_issued"] - frame):
            ctx.render_frame()
            if check:
                r = ctx.read_radiance()
                assert r.shape[0] == len(active)
                assert A.same_bits(r, rec["radiance"][frame][active]), "radiance of frame %d at the active pixels" % (frame + 1)
            ctx.accumulate()
            frame += 1
        pixels, blocks = ctx.adaptive_update()
        assert ctx.frame_number() == frame
        active = ctx.read_active_map()
        bmax, flags = ctx.read_block_noise()
        count, stats, acc, rgba8 = ctx.read_sample_counts(), ctx.read_noise_stats(), ctx.read_accumulation(), ctx.read_rgba8()
        if check:
            what = "decision %d (frame %d)" % (k, frame)
            assert (pixels, blocks) == (want["active_pixels"], want["active_blocks"]), what
            assert np.array_equal(flags.astype(bool), want["flags"]), what
            assert np.array_equal(active, want["active"]), what
            assert np.array_equal(count, want["count"]), what
            assert A.same_bits(stats, want["stats"]), what
            assert A.same_bits(acc, want["acc"]), what
            assert A.same_bits(bmax, want["block_max"]), what
        snaps.append((count, acc, rgba8, flags.astype(bool)))
    return snaps


def _adaptive_ctx(factory, rec, thr, cull=1, **how):
    ctx = _ctx(factory, rec["scene"], rec["W"], rec["H"], **how)
    ctx.set_adaptive(threshold=thr, lum_floor=LUM_FLOOR, min_samples=MIN_SAMPLES, cull=cull)
    return ctx


@pytest.mark.parametrize("name", ["cornell", "zoo", "partial", "all features"])
def test_decisions_active_set_and_statistics_follow_the_simulator(gpu_ctx_factory, name):
    rec = _reference(gpu_ctx_factory, name)
    thr, sim, hist = _simulated(rec)
    ctx = _adaptive_ctx(gpu_ctx_factory, rec, thr)
    snaps = _hand_driven(ctx, rec, hist)
    assert len(snaps) == len(hist)
    if name == "partial" and hist[-1]["flags"][-1]:
        assert hist[-1]["active_pixels"] % 64 == 48, "the partial block is alive and counted with its 48 pixels"
    ctx.close()


def test_culling_in_tile_order_with_entry_points(gpu_ctx_factory):
    """Blocks are 8 x 8 pixel tiles and entry-state runs: a pass over the surviving tiles walks its runs' entry states from the active map."""
    rows = _reference(gpu_ctx_factory, "cornell")
    pm = capi.tile_pixel_map(rows["W"], rows["H"], 1, 0, 1, tiled=True)
    rec = dict(rows, radiance=[r[pm] for r in rows["radiance"]])  # the same record in the tile order's base order
    thr, sim, hist = _simulated(rec)
    ctx = _adaptive_ctx(gpu_ctx_factory, rec, thr, order=pod.ORDER_TILES, entry=True)
    _hand_driven(ctx, rec, hist)
    ctx.close()


def test_culled_blocks_are_not_touched_again(gpu_ctx_factory):
    rec = _reference(gpu_ctx_factory, "cornell")
    thr, sim, hist = _simulated(rec)
    ctx = _adaptive_ctx(gpu_ctx_factory, rec, thr, in_flight=2)
    snaps = _hand_driven(ctx, rec, hist, check=False)
    final_count, final_acc, final_rgba8, _ = snaps[-1]
    seen = 0
    for k, (count, acc, rgba8, flags) in enumerate(snaps[:-1]):
        culled = ~np.repeat(flags, 64)[:len(count)]
        seen = max(seen, int(culled.sum()))
        assert np.array_equal(final_count[culled], count[culled]), "decision %d" % k
        assert A.same_bits(final_acc[culled], acc[culled]) and np.array_equal(final_rgba8[culled], rgba8[culled]), "decision %d" % k
        assert np.all(count[culled] == hist[k]["count"][culled])
    assert seen >= 64
    # ... and with two passes in flight the run is the simulator's as well
    assert np.array_equal(final_count, hist[-1]["count"]) and A.same_bits(final_acc, hist[-1]["acc"])
    ctx.close()


def test_render_adaptive_is_the_hand_driven_loop(gpu_ctx_factory):
    rec = _reference(gpu_ctx_factory, "cornell")
    thr, sim, hist = _simulated(rec)
    ctx = _adaptive_ctx(gpu_ctx_factory, rec, thr)
    frames, pixels = ctx.render_adaptive(MAX_FRAMES, INTERVAL)
    assert (frames, pixels) == (hist[-1]["frames_issued"], hist[-1]["active_pixels"])
    assert np.array_equal(ctx.read_sample_counts(), hist[-1]["count"])
    assert A.same_bits(ctx.read_accumulation(), hist[-1]["acc"]) and A.same_bits(ctx.read_noise_stats(), hist[-1]["stats"])
    assert np.array_equal(ctx.read_active_map(), hist[-1]["active"])
    assert frames == ctx.frame_number()
    assert hist[-1]["active_pixels"] * 2 <= ctx.local_count, "the last intervals packed at least two frames into a pass"
    # estimate only: the same stop rule, every pixel sampled in every frame
    _, hist0 = A.run(rec["radiance"], thr, LUM_FLOOR, MIN_SAMPLES, False, INTERVAL, MAX_FRAMES)
    ctx0 = _adaptive_ctx(gpu_ctx_factory, rec, thr, cull=0)
    frames0, pixels0 = ctx0.render_adaptive(MAX_FRAMES, INTERVAL)
    assert (frames0, pixels0) == (hist0[-1]["frames_issued"], hist0[-1]["active_pixels"])
    assert np.all(ctx0.read_sample_counts() == frames0) and A.same_bits(ctx0.read_accumulation(), hist0[-1]["acc"])
    assert np.array_equal(ctx0.read_block_noise()[1].astype(bool), hist0[-1]["flags"])
    ctx0.close()
    # convergence: a threshold every finite error meets settles every block at the floor; a second call returns at once
    ctx.reset_frame_number()
    ctx.set_adaptive(threshold=3e38, lum_floor=LUM_FLOOR, min_samples=MIN_SAMPLES, cull=1)
    assert ctx.render_adaptive(MAX_FRAMES, INTERVAL) == (MIN_SAMPLES, 0)
    assert np.all(ctx.read_sample_counts() == MIN_SAMPLES) and ctx.frame_number() == MIN_SAMPLES
    assert ctx.render_adaptive(MAX_FRAMES, INTERVAL) == (0, 0) and ctx.frame_number() == MIN_SAMPLES
    ctx.close()


def test_feature_buffers_cover_the_same_samples_and_feed_the_denoiser(gpu_ctx_factory):
    rec = _reference(gpu_ctx_factory, "zoo")
    thr, sim, hist = _simulated(rec, extras=True)
    ctx = _adaptive_ctx(gpu_ctx_factory, rec, thr, aov=True)
    frames, _ = ctx.render_adaptive(MAX_FRAMES, INTERVAL)
    assert frames == hist[-1]["frames_issued"] and np.array_equal(ctx.read_sample_counts(), hist[-1]["count"])
    assert len(np.unique(hist[-1]["count"])) >= 2, "some pixels stopped earlier than others"
    albedo, normal_depth = ctx.read_aov()
    assert A.same_bits(albedo, hist[-1]["extra"][0]) and A.same_bits(normal_depth, hist[-1]["extra"][1])
    acc = ctx.read_accumulation()
    assert A.same_bits(acc, hist[-1]["acc"])
    ctx.denoise()
    got, got8 = ctx.read_denoised(), ctx.read_denoised_rgba8()
    plain = _ctx(gpu_ctx_factory, rec["scene"], rec["W"], rec["H"], aov=True)
    plain.write_accumulation(acc, frames)
    plain.write_aov(albedo, normal_depth)
    plain.denoise()
    assert A.same_bits(plain.read_denoised(), got) and np.array_equal(plain.read_denoised_rgba8(), got8)
    assert not A.same_bits(got, acc), "the filter did something"
    plain.close()
    ctx.close()


def _refused(fn, match):
    with pytest.raises(capi.NexusError, match=match):
        fn()


def test_refusals_and_resets(gpu_ctx_factory):
    rec = _reference(gpu_ctx_factory, "cornell")
    sc, W, H = rec["scene"], rec["W"], rec["H"]
    n = W * H
    d = capi.adaptive_defaults()
    assert (float(d["threshold"][0]), float(d["lumFloor"][0]), int(d["minSamples"][0]), int(d["cull"][0])) == (np.float32(0.05), np.float32(0.01), 16, 1)
    ctx = _ctx(gpu_ctx_factory, sc, W, H, aov=True)
    # off: the read-backs and the update say so
    for fn in (ctx.adaptive_update, ctx.read_sample_counts, ctx.read_noise_stats, ctx.read_block_noise, ctx.read_active_map, lambda: ctx.render_adaptive(4, 2)):
        _refused(fn, "adaptive sampling is off")
    # slot-keyed random numbers
    ctx.set_modes(pod.RNG_REFERENCE_SLOT, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    _refused(ctx.set_adaptive, "NX_RNG_PIXEL_KEYED")
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    _refused(lambda: ctx.set_adaptive(threshold=-1.0), "threshold")
    _refused(lambda: ctx.set_adaptive(lum_floor=0.0), "lumFloor")
    # after frames were accumulated
    ctx.render_frame()
    ctx.accumulate()
    _refused(ctx.set_adaptive, "reset the frame number")
    assert ctx.frame_number() == 1 and not ctx.adaptive
    ctx.reset_frame_number()
    ctx.set_adaptive(threshold=3e38, lum_floor=LUM_FLOOR, min_samples=2, cull=1)
    _refused(lambda: ctx.set_modes(pod.RNG_REFERENCE_SLOT, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED), "adaptive sampling is on")
    _refused(lambda: ctx.write_accumulation(np.zeros((n, 3), np.float32), 3), "adaptive sampling is on")
    _refused(lambda: ctx.write_aov(np.zeros((n, 4), np.float32), None), "adaptive sampling is on")
    lib = capi.lib()
    assert lib.nxhip_mgpu_attach(ctx.h, C.c_void_p(1), 2, 0, 8) == 1 and b"adaptive sampling is on" in lib.nxhip_last_error()
    assert lib.nxhip_render_adaptive(ctx.h, 4, 0, None, None) == 1 and b"interval" in lib.nxhip_last_error()
    assert ctx.frame_number() == 0 and np.all(ctx.read_sample_counts() == 0), "nothing was launched behind the refused calls"
    # accumulate with nothing pending: no sample is counted twice
    ctx.render_frame()
    ctx.accumulate()
    ctx.accumulate()
    assert np.all(ctx.read_sample_counts() == 1)
    assert A.same_bits(ctx.read_accumulation(), rec["radiance"][0])
    ctx.render_frame()
    assert ctx.adaptive_update() == (0, 0), "the update folds the pending pass; with this threshold every block settles at two samples"
    assert ctx.active_count() == 0 and len(ctx.read_active_map()) == 0
    # no active block: nothing is rendered, the frame number stays
    acc = ctx.read_accumulation()
    ctx.render_frame()
    ctx.accumulate()
    ctx.render(3)
    assert ctx.frame_number() == 2 and np.all(ctx.read_sample_counts() == 2) and A.same_bits(ctx.read_accumulation(), acc)
    assert ctx.read_radiance().shape == (n, 3), "the last pass that was rendered"
    assert not ctx.read_block_noise()[1].any()
    # every way of starting over: counts 0, every block active, and the image is the plain one again
    def started_over(count):
        assert ctx.frame_number() == 0
        assert ctx.local_count == count and np.all(ctx.read_sample_counts() == 0) and np.all(ctx.read_noise_stats() == 0)
        bmax, flags = ctx.read_block_noise()
        assert len(flags) == (count + 63) // 64 and flags.all() and np.all(bmax == 0)
        assert np.array_equal(ctx.read_active_map(), np.arange(count))

    ctx.reset_frame_number()
    started_over(n)
    ctx.render_frame()
    ctx.accumulate()
    assert A.same_bits(ctx.read_accumulation(), rec["radiance"][0]) and np.all(ctx.read_sample_counts() == 1)
    ctx.set_pixel_order(pod.ORDER_TILES)
    started_over(n)
    ctx.render_frame()
    assert ctx.adaptive_update() == (n, n // 64)
    ctx.set_pixel_map(np.arange(100, 100 + 150, dtype=np.uint32))
    started_over(150)
    ctx.render_frame()
    assert ctx.read_radiance().shape == (150, 3) and A.same_bits(ctx.read_radiance(), rec["radiance"][0][100:250])
    assert ctx.adaptive_update() == (150, 3)
    ctx.resize(40, 30)
    started_over(1200)
    # off again: the base set, the plain accumulate
    ctx.resize(W, H)
    ctx.set_pixel_order(pod.ORDER_ROWS)
    sc.upload(ctx)
    ctx.set_adaptive(on=False)
    _refused(ctx.read_sample_counts, "adaptive sampling is off")
    ctx.reset_frame_number()
    for f in range(2):
        ctx.render_frame()
        ctx.accumulate()
    sim = _numpy_stats(rec, 2)
    assert A.same_bits(ctx.read_accumulation(), sim.acc)
    ctx.close()


def test_facade_render_adaptive_is_the_c_abi_loop(tmp_path):
    """nexus::Renderer::SetAdaptive / RenderAdaptive / SaveSampleCountEXR through their C views, on the Cornell .glb"""
    import os

    from nexus_amd import imageio
    from tests import oracle_lib as O

    W, H, max_frames, interval = 96, 64, 32, 4

    def scene():
        sc = capi.Scene(W, H)
        sc.load_file(SH.GOLDEN + os.sep, "cornell_box.glb")
        sc.set_camera((0.0, 1.0, 3.9), (0.0, 0.0, -1.0), 40.0, 5.0, 0.0)
        sc.set_render_settings(O.make_settings(use_mis=True, path_length=3))
        return sc

    params = capi.adaptive_defaults()
    params["threshold"], params["minSamples"] = 0.25, 8
    # the C-ABI loop, on the device context of a renderer that has the scene on the device
    sc1 = scene()
    r1 = capi.Renderer(W, H, sc1)
    r1.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    r1.render(sc1, 0.0)
    ctx = r1.device_context()
    ctx.reset_frame_number()
    ctx.set_adaptive(threshold=0.25, min_samples=8)
    frames, blocks, alive = 0, 1, []
    while blocks and frames < max_frames:
        for _ in range(interval):
            ctx.render_frame()
            ctx.accumulate()
        frames += interval
        _, blocks = ctx.adaptive_update()
        alive.append(blocks)
    want_counts, want_rgba8, want_acc = ctx.read_sample_counts(), ctx.read_rgba8(), ctx.read_accumulation()
    print("C-ABI loop: %d frames, blocks alive %s, samples per pixel %d .. %d" % (frames, alive, want_counts.min(), want_counts.max()))
    # the facade
    sc2 = scene()
    r2 = capi.Renderer(W, H, sc2)
    r2.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    r2.set_adaptive(params)
    assert r2.render_adaptive(sc2, max_frames, interval) == frames and r2.frame_number() == frames
    assert np.array_equal(r2.read_pixels(), want_rgba8)
    assert A.same_bits(r2.read_accumulation(), want_acc)
    r2.save_sample_count_exr(str(tmp_path / "n.exr"))
    img, w, h = imageio.read_exr(str(tmp_path / "n.exr"))
    assert (w, h) == (W, H) and np.array_equal(img[::-1].reshape(-1, 3), np.repeat(want_counts.astype(np.float32)[:, None], 3, axis=1))
    r2.set_adaptive(None)
    with pytest.raises(capi.NexusError, match="adaptive sampling"):
        r2.save_sample_count_exr(str(tmp_path / "no.exr"))
    r1.close()
    r2.close()
