"""The camera against its definition, on the CPU: tests/camera_reference.py (float64, written from the parameters) holds

  * the nx_camera struct that Camera::ToDevice (capi.camera_init) and the oracle's orc_camera_init form, field by field;
  * the binary32 restatement of generate_kernel in tests/aov_reference.py, pinhole and thin lens — the rays every test of the feature
    buffers and tests/test_geometry_pins.py start from;
  * itself: the ray checker must refuse each of nine wrong cameras, and the bounds must be small against a pixel.

It also fixes, by simulation with the model's own rays, the frame count of the depth-of-field pin of tests/test_gpu_camera.py.

Numbers (the derivation is in tests/camera_reference.py): C = 44, C0 = 7.5 for the direction, C' = 17 for the origin.  Largest share of a
bound used by the restated rays: direction 0.046, origin 0.034 (the device's rays: the same).  `unclear` paths among the 335 509 of the
table and the lens statistics: 0.  Depth-of-field pin: N = 1024 frames of 48 x 16 — see test_depth_of_field_simulation_fixes_the_frame_count."""
import numpy as np
import pytest

from nexus_amd import capi
from tests import aov_reference as A
from tests import camera_reference as CR
from tests import oracle_lib as O
from tests.test_physics_pins import _assert_agree, _z

FIELDS = ("position", "right", "up", "viewportX", "viewportY", "lowerLeftCorner", "lensRadius", "resolution")
ALL = CR.cameras()
IDS = [c.name.replace(" ", "-") for c, _ in ALL]


def _check_struct(cam, quirk, struct, who):
    want, bound = cam.struct(quirk), cam.struct_bounds(quirk)
    for f in FIELDS:
        got = np.asarray(struct[f], np.float64).reshape(-1)
        err = np.max(np.abs(got - np.asarray(want[f], np.float64).reshape(-1)))
        assert err <= bound[f], "%s, %s: %s is %.3g off, bound %.3g" % (who, cam.name, f, err, bound[f])


@pytest.mark.parametrize("maker", [capi.camera_init, O.camera_init], ids=["product", "oracle"])
def test_camera_struct_is_the_float64_camera(maker):
    """every camera of the table, every field, within the host part of the bound (pitched cameras with the quirk: section below)"""
    for cam, quirk in ALL:
        _check_struct(cam, quirk, maker(*cam.args()), maker.__module__)
    # resolution and position are exact; a struct from the wrong angle is refused
    cam, quirk = CR.camera("level_lens", 33, 17)
    with pytest.raises(AssertionError, match="lensRadius"):
        _check_struct(cam, quirk, maker(cam.position, cam.forward, cam.hfov, 33, 17, cam.focus, 2.0 * cam.defocus), "control")
    with pytest.raises(AssertionError, match="viewportY"):
        _check_struct(cam, quirk, maker(cam.position, cam.forward, cam.hfov, 17, 33, cam.focus, cam.defocus), "control")


def test_bounds_meet_their_conditions():
    """A bound wider than a pixel could hide a half-pixel shift or a flipped axis: on every camera but `far` the direction bound is under a
    thousandth of the pixel's angular width, on every pixel."""
    for cam, quirk in ALL:
        rays = CR.primary_rays(cam, 1, quirk=quirk)
        bd, bo = CR.bounds(cam, rays, quirk)
        ratio = float(np.max(bd / CR.pixel_angle(cam, quirk)))
        print("%-24s direction bound %.2e rad = %.2e pixel, origin bound %.2e" % (cam.name, bd.max(), ratio, bo))
        if not cam.name.startswith("far"):
            assert ratio < 1e-3, cam.name
    far, _ = CR.camera("far", 33, 17)
    assert np.max(CR.bounds(far, CR.primary_rays(far, 1))[0] / CR.pixel_angle(far)) > 1.0  # (the camera `far` is there for: cancellation larger than a pixel)


def _restated(cam, frame):
    r = A.primary_rays(capi.camera_init(*cam.args()), cam.W, cam.H, frame)
    return r["origin"], r["direction"]


@pytest.mark.parametrize("cam,quirk", ALL, ids=IDS)
def test_restated_rays_are_the_float64_cameras(cam, quirk):
    """aov_reference.primary_rays — binary32, the kernel's order, the oracle's random numbers — within the derived bound of the model, which
    draws its numbers from its own integer restatement: every test that starts from those rays is anchored here."""
    if cam.W * cam.H > 2500:
        cam = cam.resized(cam.W // 2 + 1, cam.H // 2 - 1)  # (the restatement loops over pixels in Python; the GPU tests run the full sizes)
    for frame in CR.FRAMES[::2]:
        o, d = _restated(cam, frame)
        seen = CR.check_rays(cam, CR.primary_rays(cam, frame, quirk=quirk), o, d, quirk)
        print(cam.name, frame, seen)


VARIANTS = ["flip_v", "swap_jitter", "half_pixel", "hfov_1001", "lens_negated", "lens_not_in_direction", "tan_full_defocus", "frame_plus_one", "column_major"]


def test_checker_accepts_the_model_rounded_to_binary32():
    for cam, quirk in ALL:
        rays = CR.primary_rays(cam, 2, quirk=quirk)
        CR.check_rays(cam, rays, rays.origin.astype(np.float32), rays.direction.astype(np.float32), quirk)


@pytest.mark.parametrize("variant", VARIANTS)
def test_checker_refuses_edited_cameras(variant):
    """each wrong camera, on a lens camera with W != H and on the smallest lens angle of the table, and the restated rays of the right one
    accepted by the same call"""
    for name, W, H in (("level_lens", 33, 17), ("level_lens_small", 7, 64)):
        cam, quirk = CR.camera(name, W, H)
        rays = CR.primary_rays(cam, 2)
        wrong = CR.primary_rays(cam, 2, variant=variant)
        assert not CR.rejects(cam, rays, rays.origin.astype(np.float32), rays.direction.astype(np.float32))
        assert CR.rejects(cam, rays, wrong.origin.astype(np.float32), wrong.direction.astype(np.float32)), "%s passes on %s" % (variant, cam.name)


def test_checker_refuses_a_pinhole_origin_that_is_not_the_position():
    cam, _ = CR.camera("level", 33, 17)
    rays = CR.primary_rays(cam, 1)
    o = rays.origin.astype(np.float32)
    o[5, 1] = np.nextafter(o[5, 1], np.float32(9))
    assert CR.rejects(cam, rays, o, rays.direction.astype(np.float32))
    assert CR.rejects(cam, rays, rays.origin.astype(np.float32)[:-1], rays.direction.astype(np.float32)[:-1])  # (a ray short)


def test_random_numbers_are_the_oracles():
    """the integer restatement against the oracle's orc_rng_init_pixel / orc_rand: two texts of one definition, equal bit for bit"""
    import ctypes as C

    L = O.lib()
    for i, j, W, frame in ((0, 0, 1, 1), (5, 3, 33, 2), (129, 2, 130, 47), (0, 0, 64, 0), (63, 63, 64, 0xfffffff0)):
        st = C.c_uint32(L.orc_rng_init_pixel(i, j, W, frame))
        s = CR.seed([i], [j], W, [frame])
        assert int(s[0]) == st.value
        for _ in range(6):
            s, v = CR.draw(s)
            assert float(L.orc_rand(C.byref(st))) == v[0]


def tiles_order(W, H):
    """NXHIP_ORDER_TILES as include/nexus_hip.h words it: 8 x 8 tiles, row-major inside a tile, tiles left to right in bands of eight rows"""
    out = []
    for band in range(0, H, 8):
        for tile in range(0, W, 8):
            out += [i + j * W for j in range(band, min(band + 8, H)) for i in range(tile, min(tile + 8, W))]
    return np.array(out, np.uint32)


def test_documented_tile_order_is_the_librarys():
    for W, H in ((64, 64), (33, 17), (7, 64), (130, 3), (1, 1)):
        assert np.array_equal(tiles_order(W, H), capi.tile_pixel_map(W, H, 1, 0, 1, tiled=True)), (W, H)


# ---- the lens statistics ----------------------------------------------------------------------------------------------
RINGS, SECTORS = 8, 16
CHI2_DOF = RINGS * SECTORS - 1
CHI2_BAR = CHI2_DOF + 4.5 * np.sqrt(2.0 * CHI2_DOF)  # 127 degrees of freedom: mean 127, sigma sqrt(254); 4.5 sigma = 198.7 (p about 2e-5)
LENS_FRAMES = 64


def disk_chi2(p):
    """chi-square of points p (n, 2) of the unit disk over RINGS x SECTORS polar cells of equal area"""
    r2 = p[:, 0] ** 2 + p[:, 1] ** 2
    ring = np.minimum((r2 * RINGS).astype(int), RINGS - 1)
    sector = np.minimum(((np.arctan2(p[:, 1], p[:, 0]) + np.pi) / (2.0 * np.pi) * SECTORS).astype(int), SECTORS - 1)
    counts = np.bincount(ring * SECTORS + sector, minlength=RINGS * SECTORS)
    e = len(p) / (RINGS * SECTORS)
    return float(np.sum((counts - e) ** 2 / e))


def lens_statistics_rays(variant=None):
    cam, _ = CR.camera("level_lens", 64, 64)
    g = np.tile(np.arange(64 * 64), LENS_FRAMES)
    f = np.repeat(np.arange(1, LENS_FRAMES + 1), 64 * 64)
    return cam, CR.primary_rays(cam, f, g, variant=variant)


def test_lens_points_of_the_model_are_uniform_and_a_radial_disk_is_not():
    cam, rays = lens_statistics_rays()
    chi2 = disk_chi2(rays.lens)
    print("model: chi2 %.1f over %d points, %d degrees of freedom, bar %.1f" % (chi2, len(rays.lens), CHI2_DOF, CHI2_BAR))
    assert chi2 < CHI2_BAR
    assert disk_chi2(lens_statistics_rays("lens_radial")[1].lens) > 10.0 * CHI2_BAR


def test_unclear_share_of_everything_the_gpu_tests_render():
    """the cap the GPU tests enforce (1e-4 of the paths), on the model alone: the table's cameras at frames 1, 2, 47, and the lens statistics"""
    paths = unclear = 0
    for cam, quirk in ALL:
        for frame in CR.FRAMES:
            r = CR.primary_rays(cam, frame, quirk=quirk)
            paths += len(r.pixel)
            unclear += int(r.unclear.sum())
            assert r.unclear.sum() <= 1e-4 * len(r.pixel), (cam.name, frame)
    r = lens_statistics_rays()[1]
    paths += len(r.pixel)
    unclear += int(r.unclear.sum())
    print("unclear: %d of %d paths" % (unclear, paths))
    assert unclear <= 1e-4 * paths


# ---- the pitched camera: a mirrored quirk, pinned ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pitched_up", "pitched_down"])
@pytest.mark.parametrize("maker", [capi.camera_init, O.camera_init], ids=["product", "oracle"])
def test_pitched_camera_is_narrower_by_the_cosine_of_its_pitch(name, maker):
    """right = forward x world_up is not normalised (Camera's constructor, and the reference's): against the camera of the definition the
    viewport vectors and the lens axes are cos 35 degrees long, the horizontal field of view 2 atan(cos 35 tan(hfov / 2)) = 50.62 degrees
    for the 60 asked for.  A measurement of the deviation, not a tolerance: the struct is held to the quirk's model within the host bound
    and to this factor of the definition's."""
    cam, quirk = CR.camera(name, 33, 17)
    assert quirk
    s = maker(*cam.args())
    _check_struct(cam, True, s, "quirk")
    with pytest.raises(AssertionError):
        _check_struct(cam, False, s, "definition")
    ideal, c = cam.struct(False), np.cos(np.radians(35.0))
    n = np.linalg.norm
    for f in ("right", "up", "viewportX", "viewportY"):
        got = np.asarray(s[f], np.float64)
        assert abs(n(got) / n(ideal[f]) - c) < 1e-6, f
        assert n(got / n(got) - ideal[f] / n(ideal[f])) < 1e-6, f  # (the same axis, shorter)
    effective = 2.0 * np.degrees(np.arctan(n(np.asarray(s["viewportX"], np.float64)) / 2.0 / cam.focus))
    assert abs(effective - 2.0 * np.degrees(np.arctan(c * np.tan(np.radians(30.0))))) < 1e-4 and abs(effective - 50.62) < 0.01
    # the lens offsets: the restated rays' origins against the definition's, scaled
    o, _ = _restated(cam, 1)
    want = CR.primary_rays(cam, 1, quirk=False)
    assert np.max(np.abs((o - cam.position) - c * want.offset)) < 1e-6 * cam.lens_radius() + CR.bounds(cam, want)[1]


# ---- depth of field as transport: the frame count, by simulation ------------------------------------------------------
DOF = dict(W=48, H=16, hfov=40.0, focus=4.0, defocus=10.0, frames=1024, edge_per_distance=0.05)


def dof_camera(defocus=None):
    return CR.Camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), DOF["hfov"], DOF["W"], DOF["H"], DOF["focus"], DOF["defocus"] if defocus is None else defocus, name="dof")


def dof_z(coverage, p):
    """z-scores per pixel column of the mean coverage (frames, H, W) against the column's P(hit): Bernoulli samples, so the variance is the
    model's, p (1 - p) / n.  Only columns with n p (1 - p) >= 25 (the normal approximation's domain) give a score, so that the mean of
    z^2 is not diluted by columns that cannot disagree; where p is exactly 0 or 1 the coverage must be exactly that."""
    n = coverage.shape[0] * coverage.shape[1]
    mean = coverage.mean(axis=(0, 1))
    exact = (p == 0.0) | (p == 1.0)
    assert np.array_equal(mean[exact], p[exact]), "a column the model covers fully or not at all"
    use = n * p * (1.0 - p) >= 25.0
    assert use.sum() >= 5
    return _z(mean[use], 0.0, p[use], np.sqrt(p[use] * (1.0 - p[use]) / n))


def dof_check(coverage, d, what):
    """the true model agrees at the bar of tests/test_physics_pins.py; the two controls are refused at it, on the same data"""
    cam, edge = dof_camera(), DOF["edge_per_distance"] * d
    _assert_agree(dof_z(coverage, CR.coverage_model(cam, d, edge)), "%s, d = %g: uniform disk of the lens radius" % (what, d))
    for control in (dict(radius_scale=1.10), dict(radial=True)):
        with pytest.raises(AssertionError):
            _assert_agree(dof_z(coverage, CR.coverage_model(cam, d, edge, **control)), "%s, d = %g: control %s" % (what, d, control))


def dof_model_coverage(d, defocus=None, frames=None):
    cam = dof_camera(defocus)
    N, n = frames or DOF["frames"], DOF["W"] * DOF["H"]
    rays = CR.primary_rays(cam, np.repeat(np.arange(1, N + 1), n), np.tile(np.arange(n), N))
    return CR.coverage_of_rays(rays, d, DOF["edge_per_distance"] * d).reshape(N, DOF["H"], DOF["W"]), rays


@pytest.mark.parametrize("d", [8.0, 2.0])
def test_depth_of_field_simulation_fixes_the_frame_count(d):
    """The estimator of the GPU pin, run on the model's own rays at the same N = 1024 frames of 48 x 16 (16 384 Bernoulli samples per
    column): the true model passes (|z| < 4.5, mean z^2 < 1.6), radius x 1.10 and the radial disk are refused.
    Simulated: d = 8:  6 columns, true max |z| 1.22, mean z^2 0.52; radius x 1.10 max |z| 12.1; radial disk max |z| 26.5.
               d = 2: 12 columns, true max |z| 1.94, mean z^2 1.25; radius x 1.10 max |z| 16.4; radial disk max |z| 29.6."""
    coverage, _ = dof_model_coverage(d)
    dof_check(coverage, d, "model's own rays")


def test_in_the_focal_plane_the_lens_changes_nothing():
    """d = focus on the model: the coverage of a lens ray is the pinhole ray's (same jitter, same focal point)"""
    lens, _ = dof_model_coverage(DOF["focus"], frames=64)
    pin, _ = dof_model_coverage(DOF["focus"], defocus=0.0, frames=64)
    assert np.array_equal(lens, pin) and 0.3 < lens.mean() < 0.6
