"""Feature buffers (AOVs) on the device: nxhip_set_aov / read_aov / read_aov_frame / write_aov (include/nexus_hip.h).

Reference: the primary ray restated in numpy and traced by the CPU oracle (tests/aov_reference.py; pinned against the oracle's own
wavefront by tests/test_aov.py).  Albedo, coverage and depth must equal it bit for bit.  The shading normal is recomputed in float64 from
the oracle's hit record; its tolerance is 8 x the largest deviation of a float32 numpy evaluation of the same expression from the
float64 one on those hits (a handful of roundings; the factor covers another legal placement of the fused operations).
"""
import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import aov_reference as R
from tests import oracle_lib as O
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu


def _pinhole_zoo(textures, hdr=False):
    zoo = SH.material_zoo_scene(96, 64, hdr=hdr, textures=textures)
    zoo.camera["lensRadius"] = 0.0
    return zoo


def _instanced():
    sc = SH.instanced_scene()
    sc.camera = capi.camera_init((0.0, 0.5, 6.0), (0.0, -0.05, -1.0), 55.0, 128, 96, 5.0, 0.0)
    sc.settings = O.make_settings(use_mis=False, path_length=2)  # (the scene has no lights)
    return sc


def _ctx(factory, sc, W, H, rng=pod.RNG_PIXEL_KEYED, compact=pod.COMPACT_FAST, conductor=pod.CONDUCTOR_EXTENDED, aov=True):
    ctx = factory(W, H)
    sc.upload(ctx)
    ctx.set_modes(rng, compact, conductor)
    ctx.reset_frame_number()
    if aov:
        ctx.set_aov(True)
    return ctx


SCENES = {
    "cornell": (lambda: SH.cornell_scene(160, 160, path_length=4), 160, 160),
    "zoo": (lambda: _pinhole_zoo(False), 96, 64),
    "zoo_textured": (lambda: _pinhole_zoo(True, hdr=True), 96, 64),
    "instanced": (_instanced, 128, 96),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_frame_aovs_equal_the_restatement(gpu_ctx_factory, name):
    make, W, H = SCENES[name]
    sc = make()
    ctx = _ctx(gpu_ctx_factory, sc, W, H)
    for frame in (1, 2):
        ctx.render_frame()
        ctx.accumulate()
        albedo, nd = ctx.read_aov_frame()
        want_albedo, want_depth, hits, rays = R.primary_features(sc, W, H, frame)
        hit = hits["hitDistance"] < pod.MISS_DISTANCE
        same_a = np.all(albedo.view(np.uint32) == want_albedo.view(np.uint32), axis=1)
        same_z = nd[:, 3].view(np.uint32) == want_depth.view(np.uint32)
        n64, _ = R.shading_normals(sc, hits, rays, np.float64)
        n32, _ = R.shading_normals(sc, hits, rays, np.float32)
        tol = 8.0 * float(np.max(np.abs(n32.astype(np.float64) - n64)))
        err = float(np.max(np.abs(nd[:, 0:3].astype(np.float64) - n64)))
        print("%s frame %d: albedo+coverage %d of %d equal bits, depth %d of %d; hit share %.3f; normal: largest deviation %.3g, tolerance %.3g (8 x float32's own)" % (
            name, frame, same_a.sum(), len(same_a), same_z.sum(), len(same_z), hit.mean(), err, tol))
        assert same_a.all() and same_z.all()
        assert 0.0 < tol < 1e-5 and err <= tol
        assert 0.02 < hit.mean() < 0.98
    # one frame accumulated after the other: the running mean of accumulate_kernel
    acc_a, acc_n = ctx.read_aov()
    assert R.same_bits(acc_n[:, 3], R.running_mean32([R.primary_features(sc, W, H, f)[1] for f in (1, 2)]))
    assert R.same_bits(acc_a, R.running_mean32([R.primary_features(sc, W, H, f)[0] for f in (1, 2)]))


def _accumulated(factory, sc, W, H, frames=6, per_pass=1, in_flight=1, compact=pod.COMPACT_FAST, order=pod.ORDER_ROWS, entry=False, collect=False):
    ctx = _ctx(factory, sc, W, H, compact=compact, aov=False)
    if order != pod.ORDER_ROWS:
        ctx.set_pixel_order(order)
    if entry:
        ctx.set_entry_points(True)
    ctx.set_frames_per_pass(per_pass)
    ctx.set_passes_in_flight(in_flight)
    ctx.set_aov(True)
    per_frame = []
    if in_flight > 1:  # as many passes as there are slots, then one accumulate for all of them
        for _ in range(frames // per_pass // in_flight):
            for _ in range(in_flight):
                ctx.render_frame()
            ctx.accumulate()
    else:
        for _ in range(frames // per_pass):
            ctx.render_frame()
            ctx.accumulate()
            if collect:
                per_frame.append(ctx.read_aov_frame())
    a, n = ctx.read_aov()
    colour = ctx.read_accumulation()
    if order == pod.ORDER_TILES:  # back to rows
        pm = capi.tile_pixel_map(W, H, 1, 0, 1, tiled=True)
        rows = [np.zeros_like(x) for x in (a, n, colour)]
        for dst, src in zip(rows, (a, n, colour)):
            dst[pm] = src
        a, n, colour = rows
    ctx.close()
    return a, n, colour, per_frame


@pytest.mark.parametrize("name", ["cornell", "zoo_textured"])
def test_accumulated_aovs_do_not_depend_on_how_the_frames_were_rendered(gpu_ctx_factory, name):
    make, W, H = SCENES[name]
    sc = make()
    a0, n0, c0, per_frame = _accumulated(gpu_ctx_factory, sc, W, H, collect=True)
    # the running mean of the per-frame values in accumulate_kernel's order, formed in numpy float32
    assert R.same_bits(a0, R.running_mean32([f[0] for f in per_frame]))
    assert R.same_bits(n0, R.running_mean32([f[1] for f in per_frame]))
    variants = {
        "3 frames per pass": dict(per_pass=3),
        "3 passes in flight": dict(in_flight=3),
        "classic pipeline": dict(compact=pod.COMPACT_ORDERED),
        "tile order": dict(order=pod.ORDER_TILES),
        "entry points": dict(entry=True, order=pod.ORDER_TILES),
    }
    for what, kw in variants.items():
        a, n, c, _ = _accumulated(gpu_ctx_factory, sc, W, H, **kw)
        print("%s, %s: albedo %s, normal+depth %s, colour %s" % (name, what, R.same_bits(a, a0), R.same_bits(n, n0), R.same_bits(c, c0)))
        assert R.same_bits(a, a0) and R.same_bits(n, n0), what
        assert R.same_bits(c, c0), what


@pytest.mark.parametrize("name", ["cornell", "zoo_textured"])
@pytest.mark.parametrize("compact", [pod.COMPACT_FAST, pod.COMPACT_ORDERED])
def test_nothing_else_moves(gpu_ctx_factory, name, compact):
    """With the feature buffers on, radiance, accumulation, RGBA8 and every queue size are those of the same context without them."""
    make, W, H = SCENES[name]
    sc = make()
    got = []
    for aov in (False, True):
        ctx = _ctx(gpu_ctx_factory, sc, W, H, compact=compact, aov=aov)
        frames = []
        for _ in range(3):
            ctx.render_frame()
            ctx.accumulate()
            frames.append((ctx.read_radiance(), ctx.read_queue_sizes()))
        got.append((frames, ctx.read_accumulation(), ctx.read_rgba8()))
        ctx.close()
    (f0, acc0, px0), (f1, acc1, px1) = got
    for (r0, q0), (r1, q1) in zip(f0, f1):
        assert R.same_bits(r0, r1)
        assert SH.queue_sizes_identical(q1, q0)
    assert R.same_bits(acc0, acc1) and np.array_equal(px0, px1)


def test_lens_camera_albedo_is_the_radiance_of_the_emission_twin(gpu_ctx_factory):
    """Lens radius > 0 (the zoo's own camera): albedo and coverage equal the radiance the device itself
    renders for the pathLength-1 twin whose emission is the albedo (at bounce 1 no MIS weight applies: the radiance IS the emission)."""
    W, H = 96, 64
    sc = SH.material_zoo_scene(W, H, hdr=False, textures=True)
    assert float(sc.camera["lensRadius"]) > 0.0
    sc.settings["backgroundIntensity"] = 0.0
    ctx = _ctx(gpu_ctx_factory, sc, W, H)
    twin = SH.material_zoo_scene(W, H, hdr=False, textures=True)
    twin.materials["emissive"] = R.material_albedo(twin.materials)
    twin.materials["intensity"] = 1.0
    twin.materials["emissiveMapId"] = np.where(twin.materials["diffuseMapId"] >= 0, 0, -1)
    twin.emissive_maps = [twin.diffuse_maps[0]]  # the diffuse image again, as the emissive map
    twin.settings["pathLength"] = 1
    twin.settings["backgroundIntensity"] = 0.0
    tctx = _ctx(gpu_ctx_factory, twin, W, H, aov=False)
    for frame in (1, 2, 3):
        ctx.render_frame()
        ctx.accumulate()
        tctx.render_frame()
        tctx.accumulate()
        albedo, nd = ctx.read_aov_frame()
        rad = tctx.read_radiance()
        same = np.all(albedo[:, 0:3].view(np.uint32) == rad.view(np.uint32), axis=1)
        print("lens camera frame %d: %d of %d pixels equal bits, coverage %.3f" % (frame, same.sum(), len(same), albedo[:, 3].mean()))
        assert same.all()
        assert np.array_equal(albedo[:, 3] == 1.0, nd[:, 3] > 0.0) and set(np.unique(albedo[:, 3])) <= {0.0, 1.0}
        # ... and, since the restatement has the lens path (held to the float64 camera by tests/test_camera_reference.py): the oracle's hit of
        # the restated lens ray, bit for bit
        want_albedo, want_depth, _, _ = R.primary_features(sc, W, H, frame)
        same_a = np.all(albedo.view(np.uint32) == want_albedo.view(np.uint32), axis=1)
        same_z = nd[:, 3].view(np.uint32) == want_depth.view(np.uint32)
        print("lens camera frame %d against the restated lens rays: albedo+coverage %d of %d equal bits, depth %d of %d" % (frame, same_a.sum(), len(same_a), same_z.sum(), len(same_z)))
        assert same_a.all() and same_z.all()


def test_write_read_round_trip_and_statuses(gpu_ctx_factory):
    W, H = 64, 48
    sc = SH.cornell_scene(W, H, path_length=3)
    ctx = _ctx(gpu_ctx_factory, sc, W, H, aov=False)
    with pytest.raises(capi.NexusError, match="feature buffers are off"):
        ctx.read_aov()
    with pytest.raises(capi.NexusError, match="feature buffers are off"):
        ctx.denoise()
    ctx.render(2)
    with pytest.raises(capi.NexusError, match="reset the frame number first"):
        ctx.set_aov(True)
    ctx.reset_frame_number()
    ctx.set_aov(True)
    with pytest.raises(capi.NexusError, match="no pass has been rendered"):
        ctx.read_aov_frame()
    rng = np.random.RandomState(5)
    a = rng.uniform(0, 1, (W * H, 4)).astype(np.float32)
    n = rng.uniform(-1, 1, (W * H, 4)).astype(np.float32)
    ctx.write_aov(a, n)
    ra, rn = ctx.read_aov()
    assert R.same_bits(ra, a) and R.same_bits(rn, n)
    ctx.write_aov(None, a)  # one of the two
    ra, rn = ctx.read_aov()
    assert R.same_bits(ra, a) and R.same_bits(rn, a)
    # a resumed accumulation continues bit for bit: colour AND features
    ctx.reset_frame_number()
    ctx.render(3)
    acc, (fa, fn) = ctx.read_accumulation(), ctx.read_aov()
    ctx.render(2)
    want = ctx.read_accumulation(), ctx.read_aov()
    ctx.write_accumulation(acc, 3)
    ctx.write_aov(fa, fn)
    ctx.render(2)
    assert R.same_bits(ctx.read_accumulation(), want[0])
    assert R.same_bits(ctx.read_aov()[0], want[1][0]) and R.same_bits(ctx.read_aov()[1], want[1][1])
    # survives a resize and a released queue set; off and on again
    ctx.release_queues()
    ctx.render(1)
    ctx.resize(32, 24)
    ctx.set_camera(capi.camera_init((0.0, 1.0, 3.9), (0.0, 0.0, -1.0), 40.0, 32, 24, 5.0, 0.0))
    ctx.render(2)
    assert ctx.read_aov()[0].shape == (32 * 24, 4) and ctx.read_aov()[0][:, 3].max() == 1.0
    ctx.set_aov(False)
    ctx.render(1)
    ctx.reset_frame_number()
    ctx.set_aov(True)
    ctx.render(1)
    assert ctx.read_aov_frame()[0][:, 3].max() == 1.0


def test_tile_split_context_refuses_denoise(gpu_ctx_factory):
    W, H = 64, 64
    sc = SH.cornell_scene(W, H, path_length=3)
    ctx = _ctx(gpu_ctx_factory, sc, W, H)
    ctx.set_pixel_map(capi.tile_pixel_map(W, H, 2, 0, 8, tiled=True))
    ctx.render(2)
    assert ctx.read_aov()[0].shape == (W * H // 2, 4)
    with pytest.raises(capi.NexusError, match="full frame"):
        ctx.denoise()
    doubled = np.arange(W * H, dtype=np.uint32)
    doubled[1] = 0  # as many pixels as the frame, but not each of them once
    ctx.set_pixel_map(doubled)
    ctx.render(1)
    with pytest.raises(capi.NexusError, match="full frame"):
        ctx.denoise()
    ctx.set_pixel_order(pod.ORDER_TILES)
    ctx.render(1)
    ctx.denoise()
    assert ctx.read_denoised().shape == (W * H, 3)
