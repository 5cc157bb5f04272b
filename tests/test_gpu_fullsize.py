"""GPU parity at BASELINE.json's full sizes (configs[1], [3], [4]): the oracle cannot render whole frames of these in
seconds, so it renders a seeded subset of the pixels (pixel-keyed RNG makes a pixel's path independent of the other
pixels) and traces seeded ray batches; on top of that come size-independent properties: closest-hit / any-hit
consistency, brute force on a handful of rays, bitwise reproducibility."""
import numpy as np
import pytest

from nexus_amd import pod, scenegen
from tests import config_scenes as CS
from tests import oracle_lib as O
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu


def _subset(width, height, n, seed):
    return np.sort(np.random.RandomState(seed).choice(width * height, n, replace=False)).astype(np.uint32)


def _camera_like_rays(scene, n, seed, extent, radius):
    a = scenegen.random_rays(n // 2, seed=seed, radius=radius, target_extent=extent)
    b = scenegen.interior_rays(n - n // 2, seed=seed + 1, extent=extent)
    return np.concatenate([a, b])


def _check_trace_level(ctx, scene, rays, brute=48):
    orc = scene.oracle()
    got = ctx.trace_batch(rays)
    want = orc.trace_closest(rays, threads=8)
    hit = want["hitDistance"] < 1e29
    assert hit.mean() > 0.05, "the ray batch must hit the scene"
    assert SH.hit_records_equal(got, want), "GPU hit records differ from the oracle's"
    # closest hit <-> any hit: occluded just beyond the closest hit, free just short of it
    rng = np.random.RandomState(5)
    side = rng.choice([0.999, 1.001], len(rays))
    tmax = np.where(hit, want["hitDistance"] * side, 50.0).astype(np.float32)
    occ = ctx.trace_shadow_batch(rays, tmax)
    assert np.array_equal(occ[hit], (side[hit] > 1.0)), "any-hit disagrees with the closest hit distance"
    assert not occ[~hit].any()
    # ground truth without any BVH on a few rays
    sub = np.flatnonzero(hit)[:brute]
    bf = orc.brute_closest(rays[sub])
    assert np.array_equal(got["hitDistance"][sub].view(np.uint32), bf["hitDistance"].view(np.uint32))


def _check_frames(ctx, scene, width, height, n_pixels, frames):
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    pm = _subset(width, height, n_pixels, seed=17)
    w = O.Wavefront(scene.oracle(), len(pm), pm, pod.RNG_PIXEL_KEYED, pod.CONDUCTOR_EXTENDED)
    ctx.reset_frame_number()
    first = None
    for f in range(1, frames + 1):
        ctx.render_frame()
        ctx.accumulate()
        rad = ctx.read_radiance()
        assert np.isfinite(rad).all()
        if first is None:
            first = rad
        w.render(f, threads=8)
        w.accumulate(f)
        want = w.radiance()
        assert want.max() > 0.0, "the pixel subset must see light"
        # bit for bit (round 4; until round 3: ">= 97-99 % of the subset within 1e-3", with the measured figure printed nowhere)
        assert SH.frames_identical(rad[pm], want, "%d x %d frame %d, %d seeded pixels" % (width, height, f, n_pixels))
    acc = ctx.read_accumulation()
    assert SH.frames_identical(acc[pm], w.accumulation(), "accumulation")
    assert np.array_equal(ctx.read_rgba8()[pm], w.rgba8())
    q = ctx.read_queue_sizes()
    assert q["traceSize"][0] == width * height
    # idempotence: the same frames again, bit for bit
    ctx.reset_frame_number()
    ctx.render_frame()
    assert np.array_equal(ctx.read_radiance().view(np.uint32), first.view(np.uint32))
    return w


def test_config2_one_million_triangles_1080p(gpu_ctx_factory):
    W, H = 1920, 1080
    scene = CS.config2(W, H)
    assert sum(len(b[1]) for b in scene.blas) == 1048576 + 4
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    _check_trace_level(ctx, scene, _camera_like_rays(scene, 200000, 3, extent=1.6, radius=6.0))
    _check_frames(ctx, scene, W, H, n_pixels=16384, frames=2)


def test_config2_reference_semantics_on_the_whole_chip(gpu_ctx_factory):
    """configs[1] with the reference's own semantics — random numbers keyed by queue slot, slots in serial order, no conductor
    kernel (PathTracer.cu:143, 326, 475-478; Random.cuh:79-82) — at full size: 2 M paths are some 8 000 tiles of the
    grid-wide ordered compaction (tickets + decoupled look-back, nx_wavefront.h), every one of whose slots decides which
    random numbers a path draws next.  The oracle renders the whole frame serially; radiance and every queue size of every
    bounce must be equal."""
    W, H = 1920, 1080
    scene = CS.config2(W, H)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_REFERENCE_SLOT, pod.COMPACT_ORDERED, pod.CONDUCTOR_REFERENCE)
    ctx.set_tail_bounce(0)
    w = O.Wavefront(scene.oracle(), W * H, None, pod.RNG_REFERENCE_SLOT, pod.CONDUCTOR_REFERENCE)
    ctx.reset_frame_number()
    for f in (1, 2):
        ctx.render_frame()
        ctx.accumulate()
        w.render(f, threads=8)
        w.accumulate(f)
        assert SH.frames_identical(ctx.read_radiance(), w.radiance(), "reference semantics, 1080p frame %d" % f)
        assert SH.queue_sizes_identical(ctx.read_queue_sizes(), w.queue_sizes(), int(scene.settings["pathLength"]) + 2)
    assert np.array_equal(ctx.read_rgba8(), w.rgba8())
    # extended conductor, still slot-keyed and ordered: the material kernels now chain through four queues' worth of slots
    ctx.set_modes(pod.RNG_REFERENCE_SLOT, pod.COMPACT_ORDERED, pod.CONDUCTOR_EXTENDED)
    ctx.set_tail_bounce(0)
    w = O.Wavefront(scene.oracle(), W * H, None, pod.RNG_REFERENCE_SLOT, pod.CONDUCTOR_EXTENDED)
    ctx.reset_frame_number()
    ctx.render_frame()
    w.render(1, threads=8)
    assert SH.frames_identical(ctx.read_radiance(), w.radiance(), "slot-keyed, ordered, extended conductor, 1080p")
    assert SH.queue_sizes_identical(ctx.read_queue_sizes(), w.queue_sizes(), int(scene.settings["pathLength"]) + 2)


def test_config4_thousand_instances_dielectric_environment(gpu_ctx_factory):
    W, H = 1920, 1080
    scene = CS.config4(W, H)
    assert len(scene.instances) == 1000 and len(scene.blas[0][1]) == 100000
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    _check_trace_level(ctx, scene, _camera_like_rays(scene, 100000, 7, extent=8.0, radius=25.0), brute=8)
    _check_frames(ctx, scene, W, H, n_pixels=8192, frames=2)


def test_config5_ten_million_triangles_4k_path16(gpu_ctx_factory):
    W, H = 3840, 2160
    scene = CS.config5(W, H)
    assert sum(len(b[1]) for b in scene.blas) > 9_900_000
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    _check_trace_level(ctx, scene, _camera_like_rays(scene, 100000, 9, extent=5.0, radius=12.0), brute=4)
    w = _check_frames(ctx, scene, W, H, n_pixels=8192, frames=1)
    # every material queue is exercised at this size
    q = ctx.read_queue_sizes()
    for k in ("diffuseSize", "plasticSize", "dielectricSize", "conductorSize"):
        assert q[k][1] > 0, k
    assert q["traceShadowSize"][1] > 0


def test_config1_gpu_bvh8_against_the_cpu_bvh2_path(gpu_ctx_factory):
    """BASELINE.json configs[0] names a "CPU BVH2 intersect reference path": the Cornell box flattened to 32 world-space
    triangles, a binary BVH2 over them and the two-child ordered descent (the oracle's restatement of the algorithm in
    the reference's un-included Cuda/BVH/BVH2Traversal.cuh:7-52), against the GPU's TLAS + BVH8 traversal of the instanced
    scene, for every primary ray of the 512 x 512 view.  Different arithmetic (world-space triangles vs instance-space
    rays), so distances agree to 1e-5 relative, hit / miss exactly away from silhouettes."""
    import ctypes as C

    W = H = 512
    scene = SH.cornell_scene(W, H, path_length=4)
    # world-space copy of every instance's triangles
    world = []
    for inst in scene.instances:
        tris = scene.blas[int(inst["bvhIdx"])][1].copy()
        M = inst["transform"].reshape(4, 4).astype(np.float64)
        for k in ("pos0", "pos1", "pos2"):
            p = tris[k].astype(np.float64)
            tris[k] = (p @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
        world.append(tris)
    world = np.concatenate(world)
    assert len(world) == 32
    # the camera's pixel-centre rays (no lens, no jitter)
    cam = scene.camera
    jj, ii = np.mgrid[0:H, 0:W]
    x = ((ii + 0.5) / W).reshape(-1, 1)
    y = ((jj + 0.5) / H).reshape(-1, 1)
    target = cam["lowerLeftCorner"].astype(np.float64) + cam["viewportX"].astype(np.float64) * x + cam["viewportY"].astype(np.float64) * y
    d = target - cam["position"].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(W * H, dtype=pod.RAY_DT)
    rays["origin"] = cam["position"]
    rays["direction"] = d.astype(np.float32)

    b = O._Bvh2()
    assert O.lib().orc_bvh2_build(O._ptr(world), len(world), C.byref(b)) == 0
    want = np.zeros(len(rays), dtype=pod.HIT_DT)
    O.lib().orc_bvh2_trace_closest(C.byref(b), O._ptr(world), O._ptr(rays), len(rays), O._ptr(want))
    O.lib().orc_bvh2_free(C.byref(b))

    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    got = ctx.trace_batch(rays)
    hit_g, hit_w = got["hitDistance"] < 1e29, want["hitDistance"] < 1e29
    assert hit_w.mean() > 0.85
    assert (hit_g == hit_w).mean() > 0.9995  # silhouette pixels may fall either side
    both = hit_g & hit_w
    rel = np.abs(got["hitDistance"][both] - want["hitDistance"][both]) / want["hitDistance"][both]
    assert np.quantile(rel, 0.999) < 1e-5 and (rel < 1e-3).mean() > 0.9995
