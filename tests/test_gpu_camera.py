"""The primary rays of the device against the float64 camera of tests/camera_reference.py, read back with nxhip_debug_read_primary_rays.

Every clear path's origin and direction lies within the derived bound (C = 44, C0 = 7.5, C' = 17: the derivation is in
tests/camera_reference.py) of the ray the camera's definition gives for its global pixel and frame; the path number in direction.w is the
path's; a pinhole's origin is the position bit for bit; at most 1e-4 of the paths are `unclear` (seen: 0 of the 335 509 paths of the table
and the lens statistics).  The table's cameras run at the sizes it pairs them with, frames 1, 2 and 47, one and three frames per pass, in
both pipelines; then pixel orders, a tile-split rank, entry points, the two RNG modes, a resize and the facade.  The thin-lens invariants
use the device's rays alone; the depth-of-field pins use no hook at all, only the coverage of the feature buffers (N = 1024 frames of
48 x 16, fixed on the CPU by tests/test_camera_reference.py::test_depth_of_field_simulation_fixes_the_frame_count)."""
import ctypes as C

import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen, workloads
from tests import camera_reference as CR
from tests import scene_helpers as SH
from tests import test_camera_reference as T

pytestmark = pytest.mark.gpu

ORDER_ROWS, ORDER_TILES = 0, 1


def _scene(cam, quad=None):
    """one quad (a floor under the table's cameras unless given), pathLength 1"""
    quad = quad if quad is not None else scenegen.quad((-30, 0, -30), (30, 0, -30), (30, 0, 30), (-30, 0, 30))
    return SH.BuiltScene([quad], [(0, 0, workloads.IDENTITY)], camera=capi.camera_init(*cam.args()), settings=workloads.make_settings(path_length=1))


def _ctx(factory, cam, rng=pod.RNG_PIXEL_KEYED, compact=pod.COMPACT_FAST, quad=None):
    ctx = factory(cam.W, cam.H)
    _scene(cam, quad).upload(ctx)
    ctx.set_modes(rng, compact, pod.CONDUCTOR_REFERENCE)
    return ctx


def _use(ctx, cam):
    """another camera (and size) on the same context"""
    if (ctx.width, ctx.height) != (cam.W, cam.H):
        ctx.resize(cam.W, cam.H)
    ctx.set_camera(capi.camera_init(*cam.args()))


def _pass(ctx, last_frame, frames=1):
    """render frames last_frame - frames + 1 .. last_frame as one pass and read its primary rays: (origin, direction, index, frame per path)"""
    ctx.set_frames_per_pass(frames)
    ctx.set_frame_number(last_frame - frames)
    ctx.render_frame()
    o, d, idx = ctx.debug_read_primary_rays()
    assert len(idx) == ctx.local_count * frames
    assert np.array_equal(idx, np.arange(len(idx), dtype=np.uint32)), "direction.w is the path's number"
    return o, d, np.repeat(np.arange(last_frame - frames + 1, last_frame + 1), ctx.local_count)


def _check(ctx, cam, quirk, last_frame, frames=1, pixels=None):
    """the per-ray check of one pass; pixels: the global pixel of every local pixel (default: rows)"""
    o, d, frame = _pass(ctx, last_frame, frames)
    g = np.arange(cam.W * cam.H) if pixels is None else np.asarray(pixels, np.int64)
    rays = CR.primary_rays(cam, frame, np.tile(g, frames), quirk=quirk)
    seen = CR.check_rays(cam, rays, o, d, quirk)
    print("%-24s frames %d..%d: %s" % (cam.name, last_frame - frames + 1, last_frame, seen))
    return o, d, rays


@pytest.mark.parametrize("compact", [pod.COMPACT_FAST, pod.COMPACT_ORDERED], ids=["scan", "classic"])
def test_rays_of_every_camera_are_the_float64_cameras(gpu_ctx_factory, compact):
    """the table: every camera at its sizes, frames 1, 2 and 47 one per pass, and 45..47 as one pass of three (path_id's slice)"""
    ctx = None
    for cam, quirk in CR.cameras():
        if ctx is None:
            ctx = _ctx(gpu_ctx_factory, cam, compact=compact)
        _use(ctx, cam)
        for frame in CR.FRAMES:
            _check(ctx, cam, quirk, frame)
        _check(ctx, cam, quirk, 47, frames=3)


def test_pitched_cameras_miss_the_definition_by_the_cosine(gpu_ctx_factory):
    """the quirk on the device's rays: held to the model with quirk=True above; against the camera of the definition they are refused, and
    the lens offsets are cos 35 degrees of the definition's"""
    cam, quirk = CR.camera("pitched_up", 33, 17)
    ctx = _ctx(gpu_ctx_factory, cam)
    o, d, _ = _check(ctx, cam, True, 1)
    ideal = CR.primary_rays(cam, 1, quirk=False)
    assert CR.rejects(cam, ideal, o, d, False)
    c = np.cos(np.radians(35.0))
    assert np.max(np.abs((o - cam.position) - c * ideal.offset)) < 1e-6 * cam.lens_radius() + CR.bounds(cam, ideal)[1]


def test_pixel_orders_and_a_tile_split_rank(gpu_ctx_factory):
    """the global pixel of path k: rows, 8 x 8 tiles (also where the image is no multiple of a tile), rank 1 of a two-rank tile split"""
    for name, W, H in (("level_lens", 64, 64), ("level_lens", 33, 17)):
        cam, quirk = CR.camera(name, W, H)
        ctx = _ctx(gpu_ctx_factory, cam)
        ctx.set_pixel_order(ORDER_TILES)
        _check(ctx, cam, quirk, 2, pixels=T.tiles_order(W, H))
        _check(ctx, cam, quirk, 47, frames=3, pixels=T.tiles_order(W, H))
        ctx.set_pixel_order(ORDER_ROWS)
        _check(ctx, cam, quirk, 2)
    cam, quirk = CR.camera("level_lens", 64, 64)
    ctx = _ctx(gpu_ctx_factory, cam)
    for tiled in (True, False):
        pm = capi.tile_pixel_map(64, 64, 2, 1, 8, tiled=tiled)
        assert len(pm) == 64 * 32 and pm.min() == 8 * 64  # (rows 8..15 are the rank's first)
        ctx.set_pixel_map(pm)
        _check(ctx, cam, quirk, 2, pixels=pm)
        _check(ctx, cam, quirk, 47, frames=3, pixels=pm)


def test_entry_points_leave_the_rays_alone(gpu_ctx_factory):
    """the entry bits live in origin.w: x, y, z of every ray are what they are without entry points, bit for bit, and the model's"""
    cam, quirk = CR.camera("level", 64, 64)
    ctx = _ctx(gpu_ctx_factory, cam)
    ctx.set_pixel_order(ORDER_TILES)
    o0, d0, _ = _check(ctx, cam, quirk, 2, pixels=T.tiles_order(64, 64))
    ctx.set_entry_points(True)
    o1, d1, _ = _check(ctx, cam, quirk, 2, pixels=T.tiles_order(64, 64))
    assert ctx.debug_entry_walks() >= 1
    assert np.array_equal(o0.view(np.uint32), o1.view(np.uint32)) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))


def test_the_primary_sample_is_pixel_keyed_in_both_rng_modes(gpu_ctx_factory):
    cam, quirk = CR.camera("level_lens", 33, 17)
    got = []
    for rng in (pod.RNG_REFERENCE_SLOT, pod.RNG_PIXEL_KEYED):
        ctx = _ctx(gpu_ctx_factory, cam, rng=rng)
        o, d, _ = _check(ctx, cam, quirk, 47, frames=3)
        got.append((o, d))
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32)) and np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))


def test_after_a_resize_to_another_aspect(gpu_ctx_factory):
    cam, quirk = CR.camera("yawed", 33, 17)
    ctx = _ctx(gpu_ctx_factory, cam)
    _check(ctx, cam, quirk, 1)
    tall = cam.resized(17, 40)
    ctx.resize(17, 40)
    assert ctx.frame_number() == 0
    ctx.set_camera(capi.camera_init(*tall.args()))
    _check(ctx, tall, quirk, 1)


def test_through_the_facade(gpu_ctx_factory):
    """Scene::SetCamera -> nxs_* -> PathTracer::Render: the rays of frame 1 are the float64 camera's"""
    cam, quirk = CR.camera("yawed", 33, 17)
    sc = capi.Scene(cam.W, cam.H)
    mat = sc.add_material(pod.make_material())
    mesh = sc.add_mesh(scenegen.quad((-30, 0, -30), (30, 0, -30), (30, 0, 30), (-30, 0, 30)), mat)
    sc.create_instance(mesh, mat)
    sc.set_camera(cam.position, cam.forward, cam.hfov, cam.focus, cam.defocus)
    sc.set_render_settings(workloads.make_settings(path_length=1))
    sc.update()
    pt = capi.PathTracer(cam.W, cam.H)
    try:
        pt.update_device_scene(sc)
        pt.render(sc)
        assert pt.frame_number() == 1
        ctx = capi.Context.__new__(capi.Context)  # (the path tracer's own context, not owned: as Renderer.device_context wraps its one)
        ctx.L = capi.lib()
        ctx.h = C.c_void_p(ctx.L.nxs_pathtracer_device_context(pt.h))
        ctx.close = lambda: None
        o, d, idx = ctx.debug_read_primary_rays()
        assert np.array_equal(idx, np.arange(cam.W * cam.H, dtype=np.uint32))
        print(CR.check_rays(cam, CR.primary_rays(cam, 1, quirk=quirk), o, d, quirk))
    finally:
        pt.close()
        sc.close()


# ---- thin-lens invariants, on the device's rays alone -------------------------------------------------------------------

def _landing(cam, o, d):
    """where the ray meets the focal plane, in the rectangle's own coordinates (0..W, 0..H): needs position, forward, the focus distance
    and the focal-plane rectangle — not the lens, not the random numbers"""
    o, d = o.astype(np.float64), d.astype(np.float64)
    t = (cam.focus - (o - cam.position) @ cam.forward) / (d @ cam.forward)
    rel = o + d * t[:, None] - (cam.position + cam.focus * cam.forward)
    right, up = cam.basis()
    a = cam.half_width()
    return (rel @ right / a + 1.0) * 0.5 * cam.W, (rel @ up / (a * cam.H / cam.W) + 1.0) * 0.5 * cam.H


def test_thin_lens_invariants(gpu_ctx_factory):
    lens, _ = CR.camera("yawed", 33, 17)
    pin = CR.Camera(lens.position, lens.forward, lens.hfov, 33, 17, lens.focus, 0.0, name="yawed pinhole")
    ctx = _ctx(gpu_ctx_factory, lens)
    ol, dl, frame = _pass(ctx, 47, frames=3)
    ctx.set_camera(capi.camera_init(*pin.args()))
    op, dp, _ = _pass(ctx, 47, frames=3)
    R = lens.lens_radius()
    off = ol.astype(np.float64) - lens.position
    tol = CR.bounds(lens, CR.primary_rays(lens, frame, np.tile(np.arange(33 * 17), 3)))[1]
    assert np.max(np.abs(off @ lens.forward)) <= 2.0 * tol, "the lens point lies in the plane through the position, across forward"
    assert np.max(np.linalg.norm(off, axis=1)) < R + 2.0 * tol and np.max(np.linalg.norm(off, axis=1)) > 0.9 * R
    xl, yl = _landing(lens, ol, dl)
    xp, yp = _landing(pin, op, dp)
    g = np.tile(np.arange(33 * 17), 3)
    cell = 1e-3  # (of a pixel: what test_bounds_meet_their_conditions holds the bound under)
    assert np.all((xl > g % 33 - cell) & (xl < g % 33 + 1 + cell) & (yl > g // 33 - cell) & (yl < g // 33 + 1 + cell)), "the focal point lies in the pixel's cell"
    assert max(np.max(np.abs(xl - xp)), np.max(np.abs(yl - yp))) < 2.0 * cell, "the jitter is drawn before the disk: the pinhole's focal point"


def test_lens_points_are_uniform_over_the_disk(gpu_ctx_factory):
    """64 frames of 64 x 64: chi-square over 8 rings x 16 sectors of equal area, 127 degrees of freedom, bar 127 + 4.5 sqrt(254) = 198.7
    (the model's own draws: 114.8, tests/test_camera_reference.py)"""
    cam, _ = CR.camera("level_lens", 64, 64)
    ctx = _ctx(gpu_ctx_factory, cam)
    o, d, frame = _pass(ctx, T.LENS_FRAMES, frames=T.LENS_FRAMES)
    right, up = cam.basis()
    off = (o.astype(np.float64) - cam.position) / cam.lens_radius()
    p = np.stack([off @ right, off @ up], 1)
    chi2 = T.disk_chi2(p)
    print("device: chi2 %.1f over %d lens points, %d degrees of freedom, bar %.1f" % (chi2, len(p), T.CHI2_DOF, T.CHI2_BAR))
    assert len(p) == 64 * 64 * 64 and chi2 < T.CHI2_BAR
    _, rays = T.lens_statistics_rays()
    assert np.max(np.abs(p - rays.lens)[~rays.unclear]) < 2.0 * CR.bounds(cam, rays)[1] / cam.lens_radius(), "and they are the model's points"


# ---- depth of field as transport: coverage of a half plane, feature buffers only -----------------------------------------

def _half_plane(d):
    e = T.DOF["edge_per_distance"] * d
    return scenegen.quad((e, -20.0, -d), (e + 40.0, -20.0, -d), (e + 40.0, 20.0, -d), (e, 20.0, -d))


def _coverage(factory, d, defocus, frames):
    cam = T.dof_camera(defocus)
    ctx = _ctx(factory, cam, quad=_half_plane(d))
    ctx.reset_frame_number()
    ctx.set_aov(True)
    per_pass = 64
    ctx.set_frames_per_pass(per_pass)
    out = []
    for _ in range(frames // per_pass):
        ctx.render_frame()
        ctx.accumulate()
        out.append(ctx.read_aov_frame()[0][:, 3].reshape(per_pass, cam.H, cam.W))
    cov = np.concatenate(out).astype(np.float64)
    assert set(np.unique(cov)) <= {0.0, 1.0}
    return cov


@pytest.mark.parametrize("d", [8.0, 2.0])
def test_blur_of_an_edge_off_the_focal_plane(gpu_ctx_factory, d):
    """d = 2 focus and d = focus / 2: the per-column coverage over N = 1024 frames of 48 x 16 against the float64 quadrature of P(hit) (the
    jitter over the cell in closed form, the uniform disk on a 600 x 600 midpoint grid; blur circle 2 R |d - focus| / focus: 5.8 and 11.5
    pixels).  Bar: |z| < 4.5 and mean z^2 < 1.6 over the columns with n p (1 - p) >= 25; the same data refuse a lens radius x 1.10 and a
    disk uniform in radius.  Simulated with the model's own rays (tests/test_camera_reference.py): d = 8: max |z| 1.22, mean z^2 0.52,
    controls max |z| 12.1 and 26.5; d = 2: max |z| 1.94, mean z^2 1.25, controls 16.4 and 29.6."""
    cov = _coverage(gpu_ctx_factory, d, None, T.DOF["frames"])
    T.dof_check(cov, d, "device")
    model, _ = T.dof_model_coverage(d)
    print("d = %g: %d of %d samples differ from the model's own rays" % (d, int((model != cov).sum()), cov.size))


def test_an_edge_in_the_focal_plane_is_as_sharp_as_the_pinholes(gpu_ctx_factory):
    """d = focus: the lens changes nothing — per frame and pixel the coverage is the pinhole's, except where the focal point lies within
    a thousandth of a pixel of the edge (the bound on a ray's direction, test_bounds_meet_their_conditions)"""
    d, frames = T.DOF["focus"], 64
    lens = _coverage(gpu_ctx_factory, d, None, frames)
    pin = _coverage(gpu_ctx_factory, d, 0.0, frames)
    _, rays = T.dof_model_coverage(d, frames=frames)
    cam = T.dof_camera()
    margin = 1e-3 * 2.0 * cam.half_width() / cam.W
    far = (np.abs(rays.focal[:, 0] - T.DOF["edge_per_distance"] * d) > margin).reshape(lens.shape)
    print("d = focus: %d of %d samples within the margin, coverage %.3f" % (int((~far).sum()), far.size, lens.mean()))
    assert far.mean() > 0.99 and np.array_equal(lens[far], pin[far]) and 0.3 < lens.mean() < 0.6


# ---- what the hook refuses -------------------------------------------------------------------------------------------------

def test_hook_refuses_what_it_cannot_answer(gpu_ctx_factory):
    cam, _ = CR.camera("level", 33, 17)
    ctx = gpu_ctx_factory(33, 17)
    with pytest.raises(capi.NexusError, match="no pass has been rendered"):
        ctx.debug_read_primary_rays()
    sc = _scene(cam)
    sc.settings["pathLength"] = 2
    sc.upload(ctx)
    ctx.render_frame()
    with pytest.raises(capi.NexusError, match="pathLength == 1"):
        ctx.debug_read_primary_rays()
    ctx.set_render_settings(workloads.make_settings(path_length=1))
    ctx.render_frame()
    with pytest.raises(capi.NexusError, match="capacity too small"):
        ctx.debug_read_primary_rays(capacity=33 * 17 - 1)
    n = C.c_uint32(0)
    assert ctx.L.nxhip_debug_read_primary_rays(ctx.h, None, None, None, 0, C.byref(n)) != 0 and n.value == 33 * 17  # (the count comes back with the refusal)
    assert ctx.L.nxhip_debug_read_primary_rays(ctx.h, None, None, None, 0, None) != 0 and b"null count" in ctx.L.nxhip_last_error()
    assert ctx.L.nxhip_debug_read_primary_rays(None, None, None, None, 0, C.byref(n)) != 0
    o, d, idx = ctx.debug_read_primary_rays(capacity=33 * 17 + 5)  # (more room than paths is fine)
    assert len(idx) == 33 * 17
    ctx.set_passes_in_flight(2)  # (refused from the setting alone: which slot the next pass goes to is then the context's business)
    with pytest.raises(capi.NexusError, match="one pass in flight"):
        ctx.debug_read_primary_rays()
    ctx.set_passes_in_flight(1)
    assert len(ctx.debug_read_primary_rays()[2]) == 33 * 17
    ctx.release_queues()
    with pytest.raises(capi.NexusError, match="queues of the last pass are gone"):
        ctx.debug_read_primary_rays()
    ctx.render_frame()
    assert len(ctx.debug_read_primary_rays()[2]) == 33 * 17
