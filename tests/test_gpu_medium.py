"""Fog on the device (nxhip_set_medium): the two hooks against the float64 statement of the rule (tests/medium_reference.py, within the bars
tests/test_medium_reference.py derives), transport against closed forms and quadrature — exactly where the rule is deterministic, by z-scores
per 16 x 16 block otherwise (the bars of tests/test_physics_pins.py) — and the wiring: a medium nothing crosses changes no bit, and with fog in
the frame every pass shape gives the same bits.  The oracle does not know the medium; nothing here compares with it."""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen, workloads
from tests import medium_reference as R
from tests import scene_helpers as SH
from tests import test_medium_reference as TR
from tests import test_physics_pins as PP

pytestmark = pytest.mark.gpu

W = H = 64
SCAN = (pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
FAR = np.array((1.0e4, 1.0e4, 1.0e4))


def _scene(cam, quads=(), mats=(), path_length=2, use_mis=False, background=0.0):
    """`quads` with one material each, plus a speck 17 000 units away that no ray meets: a scene needs an instance"""
    meshes = [scenegen.quad(tuple(FAR), tuple(FAR + (1e-3, 0, 0)), tuple(FAR + (1e-3, 1e-3, 0)), tuple(FAR + (0, 1e-3, 0)))] + list(quads)
    materials = [pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0))] + list(mats)
    sc = SH.BuiltScene(meshes, [(k, k, workloads.IDENTITY) for k in range(len(meshes))], materials=np.array(materials, dtype=pod.MAT_DT), camera=cam,
                       settings=workloads.make_settings(use_mis=use_mis, path_length=path_length, background=(1, 1, 1), background_intensity=background))
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    return sc


def _frames(gpu_ctx_factory, scene, medium, frames, lights=None, per_pass=64, transmit=False, light_sampling=pod.LIGHTS_UNIFORM, env_sampling=None, want_medium=True):
    """the per-frame radiance of `frames` frames: (frames, pixels, 3)"""
    ctx = gpu_ctx_factory(W, H)
    scene.light_sampling = light_sampling
    scene.shadow_transmittance = pod.SHADOWS_TRANSMIT if transmit else pod.SHADOWS_OPAQUE
    scene.medium = medium
    scene.upload(ctx)
    if lights is not None:
        ctx.set_analytic_lights(np.array(lights, dtype=pod.ALIGHT_DT))
    if env_sampling is not None:
        ctx.set_env_sampling(env_sampling)
    ctx.set_modes(*SCAN)
    per_pass = min(per_pass, frames)
    ctx.set_frames_per_pass(per_pass)
    ctx.reset_frame_number()
    out = []
    for _ in range(frames // per_pass):
        ctx.render_frame()
        out.append(ctx.read_radiance().reshape(per_pass, W * H, 3))
    assert bool(ctx.debug_pass_flavor() & capi.FLAVOR_MEDIUM) == (want_medium and medium is not None)
    ctx.close()
    return np.concatenate(out)


def _estimate(frames):
    e = PP._Estimate(W, H)
    for f in frames:
        e.add(f)
    return e


def _pin(e, want, what):
    """the estimate agrees with `want` per block and channel (no allowance beyond the number format's), and `want` x 1.05 is refused"""
    rel = e.se / np.maximum(want, 1e-30)
    print("%s: relative standard error of the block means, median %.2g, max %.2g" % (what, np.median(rel), rel.max()))
    assert rel.max() <= 0.02, "frame count too small for the 2 %% bar"
    # (systematic: 2^-22 relative — a block every path of which carries the same binary32 value has no spread, and that value is the rounded one)
    PP._assert_agree(PP._z(e.mean, e.se, want, np.zeros_like(want), systematic=2.0 ** -22), what)
    z = PP._z(e.mean, e.se, want * 1.05, np.zeros_like(want), systematic=2.0 ** -22)
    assert not (np.abs(z).max() < 4.5 and (z * z).mean() < 1.6), "the check has no power"


# ---- 1. the hooks against the reference ------------------------------------------------------------------------------------------------

def test_segment_hook_matches_the_reference(gpu_ctx_factory):
    ctx = gpu_ctx_factory(16, 16)
    ctx.set_medium(TR.hook_medium())
    o, d, t_end, xi, _ = TR.hook_inputs()
    bars, keep, ref = TR.segment_bars()
    t0, L, T, st = (a.astype(np.float64) for a in ctx.medium_segment_batch(o, d, t_end, xi))
    crosses, scat = L > 0, st >= 0
    same = (crosses == ref["crosses"]) & (scat == ref["scatter"])
    print("decisions that differ from float64: %d of %d (cap %d)" % ((~same).sum(), len(same), len(same) // 1000))
    assert (~same).mean() <= 1e-3
    use = same & keep
    dev = {"t0": np.abs(t0 - ref["t0"])[use].max(), "L": np.abs(L - ref["L"])[use].max(), "T": np.abs(T - ref["T"])[use].max(),
           "scatter_t": np.abs(st - ref["scatter_t"])[use].max()}
    print("device deviations", dev, "bars", bars)
    for k in dev:
        assert dev[k] <= bars[k], k
    assert np.all(T[~crosses] == 1.0) and np.all(t0[~crosses] == 0.0) and np.all(st[~scat] == -1.0)
    ctx.close()


@pytest.mark.parametrize("g", TR.HOOK_G)
def test_phase_hook_matches_the_reference(gpu_ctx_factory, g):
    ctx = gpu_ctx_factory(16, 16)
    ctx.set_medium(TR.hook_medium(g))
    (bar_w, bar_p), (d, xi1, xi2, w64, p64) = TR.phase_bars(g)
    w, p = ctx.medium_phase_batch(d, xi1, xi2)
    dev_w = np.sqrt(((w.astype(np.float64) - w64) ** 2).sum(1)).max()
    dev_p = (np.abs(p.astype(np.float64) - p64) / p64).max()
    print("g %.1f: direction %.3g (bar %.3g), pdf %.3g (bar %.3g)" % (g, dev_w, bar_w, dev_p, bar_p))
    assert dev_w <= bar_w and dev_p <= bar_p
    assert np.abs(np.sqrt((w.astype(np.float64) ** 2).sum(1)) - 1.0).max() < 1e-6
    # the directions follow p(c) uniformly in phi: 16 x 16 cells in (cdf of c, phi about d)
    c = (w.astype(np.float64) * d).sum(1)
    u = (1.0 + c) / 2.0 if g == 0.0 else (1.0 - g * g) / (2.0 * g) * (1.0 / np.sqrt(1.0 + g * g - 2.0 * g * c) - 1.0 / (1.0 + g))
    e0 = R.phase_sample(0.0, d.astype(np.float64), np.full(len(d), 0.5), np.zeros(len(d)))[0]  # c = 0, phi = 0: the frame's first axis
    e1 = np.cross(d.astype(np.float64), e0)
    phi = np.arctan2((w * e1).sum(1), (w * e0).sum(1)) % (2.0 * np.pi)
    cells = np.bincount(np.minimum((np.clip(u, 0, 1) * 16).astype(int), 15) * 16 + np.minimum((phi / (2.0 * np.pi) * 16).astype(int), 15), minlength=256)
    e = len(d) / 256.0
    chi2, dof = ((cells - e) ** 2 / e).sum(), 255
    print("chi^2 %.1f on 256 cells: %.2f sigma" % (chi2, (chi2 - dof) / np.sqrt(2 * dof)))
    assert (chi2 - dof) / np.sqrt(2 * dof) < 5
    ctx.close()


# ---- 2. white furnace: exact -------------------------------------------------------------------------------------------------------------

def test_white_furnace_is_exactly_one(gpu_ctx_factory):
    cam = capi.camera_init((0.3, 0.4, 5.0), (0.0, 0.0, -1.0), 40.0, W, H, 5.0, 0.0)
    sc = _scene(cam, path_length=64, use_mis=False, background=1.0)
    fog = pod.make_medium(box_min=(-1, -1, -1), box_max=(1, 1, 1), sigma_t=0.2, g=0.6, albedo=(1, 1, 1))
    r = _frames(gpu_ctx_factory, sc, fog, 64)
    assert r.shape == (64, W * H, 3)
    assert np.all(r.view(np.uint32) == np.float32(1.0).view(np.uint32)), "worst %.9g" % np.abs(r - 1.0).max()


# ---- 3. absorption on the camera segment ---------------------------------------------------------------------------------------------------

def test_absorption_on_the_camera_segment(gpu_ctx_factory):
    le = 2.0
    cam = capi.camera_init((0.2, 0.1, 5.0), (0.0, 0.0, -1.0), 30.0, W, H, 5.0, 0.0)
    wall = scenegen.quad((-6, -6, -3), (6, -6, -3), (6, 6, -3), (-6, 6, -3))
    sc = _scene(cam, [wall], [pod.make_material(pod.MAT_DIFFUSE, albedo=(0, 0, 0), emissive=(1.0, 0.8, 0.6), intensity=le)], path_length=1)
    fog = pod.make_medium(box_min=(-1, -0.6, -1), box_max=(0.7, 1.2, 1), sigma_t=0.7, g=0.3, albedo=(0, 0, 0))
    sub = 4
    pos, dirs = R.camera_rays(cam, W, H, sub)
    want = np.zeros(W * H)
    for k in range(len(dirs)):
        t_end = (-3.0 - pos[2]) / dirs[k][:, 2]
        _, L, _ = R.segment(fog["boxMin"], fog["boxMax"], np.broadcast_to(pos, dirs[k].shape), dirs[k], t_end)
        want += np.exp(-0.7 * L) / len(dirs)
    want = TR.block_means(want)[:, None] * le * np.array((1.0, 0.8, 0.6))[None, :]
    assert want.min() < 0.5 * want.max(), "some blocks look through the box, some past it"
    _pin(_estimate(_frames(gpu_ctx_factory, sc, fog, 256)), want, "absorption")


# ---- 4. / 7. shadow attenuation: deterministic -----------------------------------------------------------------------------------------

SUN_DIR = np.array((0.3, -1.0, 0.2)) / np.linalg.norm((0.3, -1.0, 0.2))
SUN = pod.make_analytic_light(pod.ALIGHT_DIRECTIONAL, direction=tuple(SUN_DIR), colour=(1.0, 0.9, 0.7), intensity=3.0)
SLAB = pod.make_medium(box_min=(-1.5, 1.0, -1.5), box_max=(1.5, 1.5, 2.0), sigma_t=1.3, g=0.2, albedo=(0.8, 0.8, 0.8))
PANE_OPACITY = 0.5


def _slab_scene(pane):
    cam = capi.camera_init((0.0, 0.8, 3.5), np.array((0.0, -0.8, -1.0)) / np.linalg.norm((0.0, -0.8, -1.0)), 40.0, W, H, 5.0, 0.0)
    quads = [scenegen.quad((-8, 0, -8), (-8, 0, 8), (8, 0, 8), (8, 0, -8))]
    mats = [pod.make_material(pod.MAT_DIFFUSE, albedo=(0.6, 0.6, 0.6))]
    if pane:  # a see-through sheet above the slab, larger than its shadow
        quads.append(scenegen.quad((-9, 2.5, -9), (-9, 2.5, 9), (9, 2.5, 9), (9, 2.5, -9)))
        mats.append(pod.make_material(pod.MAT_DIFFUSE, albedo=(0.5, 0.5, 0.5), opacity=PANE_OPACITY))
    return _scene(cam, quads, mats, path_length=2, use_mis=True), cam


def _slab_classes(cam):
    """per pixel: every position of the pixel and of its neighbours lies under the whole slab along the sun / clear of it"""
    sub = 3
    jj, ii = np.mgrid[0:H, 0:W]
    full, clear = np.ones(W * H, bool), np.ones(W * H, bool)
    pos = cam["position"].astype(np.float64)
    for a in np.linspace(-1.0, 2.0, 2 * sub + 1):
        for b in np.linspace(-1.0, 2.0, 2 * sub + 1):
            x, y = ((ii + a) / W).reshape(-1, 1), ((jj + b) / H).reshape(-1, 1)
            d = cam["lowerLeftCorner"].astype(np.float64) + cam["viewportX"].astype(np.float64) * x + cam["viewportY"].astype(np.float64) * y - pos
            assert np.all(d[:, 1] < 0)
            p = pos + d * (-pos[1] / d[:, 1])[:, None]
            _, L, _ = R.segment(SLAB["boxMin"], SLAB["boxMax"], p, np.broadcast_to(-SUN_DIR, p.shape), np.full(len(p), np.inf))
            full &= np.abs(L - 0.5 / -SUN_DIR[1]) < 1e-9
            clear &= L == 0.0
    return full, clear


@pytest.mark.parametrize("pane", [False, True], ids=["slab", "slab under a pane of opacity 0.5"])
def test_shadow_rays_are_attenuated_by_the_slab(gpu_ctx_factory, pane):
    sc, cam = _slab_scene(pane)
    frames = 4
    without = _frames(gpu_ctx_factory, sc, None, frames, lights=[SUN], transmit=pane)
    with_fog = _frames(gpu_ctx_factory, sc, SLAB, frames, lights=[SUN], transmit=pane)
    full, clear = _slab_classes(cam)
    assert full.sum() > 200 and clear.sum() > 200, (full.sum(), clear.sum())
    # the camera is below the slab and sees the floor only: the sun's share is all there is
    assert np.all(without[:, full | clear] > 0)
    assert np.array_equal(with_fog[:, clear].view(np.uint32), without[:, clear].view(np.uint32)), "a request that does not cross the box keeps the default's bits"
    T = np.exp(-1.3 * 0.5 / -SUN_DIR[1])
    bar = TR.segment_bars()[0]["T"] + 2.0 ** -23
    ratio = with_fog[:, full].astype(np.float64) / without[:, full].astype(np.float64)
    print("transmittance %.9g, device ratio %.9g .. %.9g, bar %.3g" % (T, ratio.min(), ratio.max(), bar))
    assert np.abs(ratio - T).max() <= bar
    if pane:  # ... and the pane's factor is in both: the sun alone through the pane is half of the sun
        bare = _frames(gpu_ctx_factory, _slab_scene(False)[0], None, frames, lights=[SUN])
        r2 = without[:, full].astype(np.float64) / bare[:, full].astype(np.float64)
        assert np.abs(r2 - (1.0 - PANE_OPACITY)).max() <= 2.0 ** -22


# ---- 5. single scattering against quadrature ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [0.0, 0.7])
def test_single_scattering_matches_the_quadrature(gpu_ctx_factory, g):
    sc = _scene(TR.ss_camera(), path_length=2, use_mis=False)
    light = pod.make_analytic_light(pod.ALIGHT_POINT, position=tuple(TR.SS_LIGHT), colour=tuple(TR.SS_INTENSITY), intensity=1.0)
    mean, _ = TR.ss_expectation(g, TR.SS_SUB)
    want = mean[:, None] * TR.SS_ALBEDO * TR.SS_INTENSITY[None, :]
    _pin(_estimate(_frames(gpu_ctx_factory, sc, TR.ss_medium(g), TR.SS_FRAMES, lights=[light])), want, "single scattering, g %.1f" % g)


# ---- 6. MIS == naive in fog ----------------------------------------------------------------------------------------------------------------

def _lamp_scene(use_mis):
    cam = capi.camera_init((0.0, 0.0, 4.0), (0.0, 0.0, -1.0), 30.0, W, H, 5.0, 0.0)
    lamp = scenegen.quad((-0.9, -0.3, 0.0), (-0.9, 0.3, 0.0), (-0.5, 0.3, 0.0), (-0.5, -0.3, 0.0))
    return _scene(cam, [lamp], [pod.make_material(pod.MAT_DIFFUSE, albedo=(0, 0, 0), emissive=(1.0, 0.9, 0.8), intensity=6.0)], path_length=3, use_mis=use_mis)


LAMP_FOG = pod.make_medium(box_min=(-1, -1, -1), box_max=(1, 1, 1), sigma_t=0.9, g=0.5, albedo=(0.9, 0.9, 0.9))


@pytest.mark.parametrize("light_sampling", [pod.LIGHTS_UNIFORM, pod.LIGHTS_POWER], ids=["uniform", "power"])
def test_mis_equals_naive_in_fog(gpu_ctx_factory, light_sampling):
    frames = 1024
    mis = _estimate(_frames(gpu_ctx_factory, _lamp_scene(True), LAMP_FOG, frames, light_sampling=light_sampling))
    naive = _estimate(_frames(gpu_ctx_factory, _lamp_scene(False), LAMP_FOG, frames, light_sampling=light_sampling))
    lit = naive.mean.max(1) > 0
    assert lit.sum() >= 12
    print("MIS / naive per block:", np.round(mis.mean[:, 0] / naive.mean[:, 0], 3), "relative standard errors (MIS, naive):", np.round(np.median(mis.se / mis.mean), 4),
          np.round(np.median(naive.se / naive.mean), 4))
    PP._assert_agree(PP._z(mis.mean, mis.se, naive.mean, naive.se)[lit], "MIS against naive in fog")


def test_sampled_environment_in_fog(gpu_ctx_factory):
    rng = np.random.default_rng(3)
    env = (rng.uniform(0.05, 0.3, (16, 32, 3))).astype(np.float32)
    env[3, 20] = (40.0, 36.0, 30.0)
    cam = capi.camera_init((0.0, 0.0, 4.0), (0.0, 0.0, -1.0), 30.0, W, H, 5.0, 0.0)
    est = []
    for sampling in (True, False):
        sc = _scene(cam, path_length=3, use_mis=True)
        sc.hdr_map = env
        est.append(_estimate(_frames(gpu_ctx_factory, sc, LAMP_FOG, 1024, env_sampling=sampling)))
    PP._assert_agree(PP._z(est[0].mean, est[0].se, est[1].mean, est[1].se), "environment sampling on against off in fog")


# ---- 8. nothing crossed ----------------------------------------------------------------------------------------------------------------------

def _cornell_run(gpu_ctx_factory, media, per_pass=1, frames=4, order=pod.ORDER_ROWS, entry=False, in_flight=1):
    """`media`: the medium set before frame k (a list as long as the pass count; False: leave it).  (last frame's radiance, accumulation, flavors)"""
    ctx = gpu_ctx_factory(W, H)
    SH.cornell_scene(W, H, path_length=4).upload(ctx)
    ctx.set_analytic_lights(np.array([SUN], dtype=pod.ALIGHT_DT))
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.set_pixel_order(order)
    ctx.set_entry_points(entry)
    ctx.set_frames_per_pass(per_pass)
    ctx.set_passes_in_flight(in_flight)
    ctx.reset_frame_number()
    flavors = []
    for k in range(frames // per_pass):
        if media[k] is not False:
            ctx.set_medium(media[k])
        ctx.render_frame()
        ctx.accumulate()
        ctx.sync()
        flavors.append(ctx.debug_pass_flavor())
    last, acc = ctx.read_radiance().reshape(per_pass, W * H, 3)[-1], ctx.read_accumulation()
    ctx.close()
    if order == pod.ORDER_TILES:  # back to rows
        pm = capi.tile_pixel_map(W, H, 1, 0, 1, tiled=True)
        rows = [np.zeros_like(last), np.zeros_like(acc)]
        rows[0][pm], rows[1][pm] = last, acc
        last, acc = rows
    return last, acc, flavors


AWAY = pod.make_medium(box_min=(-0.5, -100.5, -100.5), box_max=(0.5, -99.5, -99.5), sigma_t=2.0, g=0.3, albedo=(0.9, 0.9, 0.9))


def test_a_medium_nothing_crosses_changes_no_bit(gpu_ctx_factory):
    plain = _cornell_run(gpu_ctx_factory, [None] * 4)
    away = _cornell_run(gpu_ctx_factory, [AWAY] * 4)
    assert np.array_equal(plain[0].view(np.uint32), away[0].view(np.uint32)) and np.array_equal(plain[1].view(np.uint32), away[1].view(np.uint32))
    assert all(a == p | capi.FLAVOR_MEDIUM and not p & capi.FLAVOR_MEDIUM for a, p in zip(away[2], plain[2]))
    # removed by NULL, and by sigmaT == 0: the flavor word and the frames are the original ones
    off = pod.make_medium(box_min=(-1, -1, -1), box_max=(1, 1, 1), sigma_t=0.0)
    back = _cornell_run(gpu_ctx_factory, [AWAY, None, AWAY, off])
    assert back[2] == [away[2][0], plain[2][1], away[2][2], plain[2][3]]
    assert np.array_equal(back[0].view(np.uint32), plain[0].view(np.uint32)) and np.array_equal(back[1].view(np.uint32), plain[1].view(np.uint32))


# ---- 9. equal bits with fog in the frame -----------------------------------------------------------------------------------------------

IN_FRAME = pod.make_medium(box_min=(-0.8, 0.2, -0.8), box_max=(0.9, 1.9, 0.9), sigma_t=1.1, g=0.4, albedo=(0.9, 0.8, 0.7))


@pytest.fixture(scope="module")
def foggy(gpu_ctx_factory):
    got = _cornell_run(gpu_ctx_factory, [IN_FRAME] * 64, frames=64)
    plain = _cornell_run(gpu_ctx_factory, [None] * 64, frames=64)
    assert np.all(np.isfinite(got[1])) and not np.array_equal(got[1], plain[1]), "the fog did nothing"
    return got


@pytest.mark.parametrize("what,kw", [("4 frames per pass", dict(per_pass=4)), ("64 frames per pass", dict(per_pass=64)), ("tile order", dict(order=pod.ORDER_TILES)),
                                     ("entry points", dict(entry=True)), ("no thin kernel (two passes in flight)", dict(in_flight=2))])
def test_equal_bits_with_fog_in_the_frame(gpu_ctx_factory, foggy, what, kw):
    per_pass = kw.get("per_pass", 1)
    got = _cornell_run(gpu_ctx_factory, [IN_FRAME] * (64 // per_pass), frames=64, **kw)
    assert np.array_equal(got[0].view(np.uint32), foggy[0].view(np.uint32)), what
    assert np.array_equal(got[1].view(np.uint32), foggy[1].view(np.uint32)), what
    assert all(f & capi.FLAVOR_MEDIUM for f in got[2])
