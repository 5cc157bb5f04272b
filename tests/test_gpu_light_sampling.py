"""NXHIP_LIGHTS_POWER in the shading kernels: the wiring (every pipeline, pass shape and pixel split gives the same bits), the
expectation (equal to the default mode's, by z-scores), physics (the form factor of a rectangular emitter whose tessellation the
default mode would sample badly) and what it is for (less noise under unequal lights).

The oracle does not know the mode; nothing here compares with it."""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen, workloads
from tests import light_scenes as LS
from tests import scene_helpers as SH
from tests import test_physics_pins as PP

pytestmark = pytest.mark.gpu

W, H = 64, 48
FRAMES = 4


def _render(gpu_ctx_factory, scene, mode=pod.LIGHTS_POWER, compact=pod.COMPACT_FAST, tail=0, per_pass=1, in_flight=1, pixel_map=None, never_set=False):
    """FRAMES frames with pixel-keyed random numbers: (radiance of the last frame, accumulation), in the order of the context's pixels"""
    ctx = gpu_ctx_factory(W, H)
    if never_set:
        ctx.set_light_sampling = lambda m: None  # (Workload.upload applies the workload's mode: this context never hears of it)
    scene.light_sampling = mode
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, compact, pod.CONDUCTOR_REFERENCE)
    if pixel_map is not None:
        ctx.set_pixel_map(pixel_map)
    ctx.set_tail_bounce(tail)
    ctx.set_frames_per_pass(per_pass)
    ctx.set_passes_in_flight(in_flight)
    ctx.reset_frame_number()
    for _ in range(FRAMES // per_pass):
        ctx.render_frame()
        ctx.accumulate()
    ctx.sync()
    assert ctx.frame_number() == FRAMES
    n = ctx.local_count
    return ctx.read_radiance().reshape(per_pass, n, 3)[-1], ctx.read_accumulation()


def _same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.fixture(scope="module")
def scene():
    return LS.emitter_scene(W, H, path_length=4, objects=True)


@pytest.fixture(scope="module")
def base(gpu_ctx_factory, scene):
    """POWER mode, SCAN pipeline, no tail kernel, one frame per pass, one pass at a time"""
    got = _render(gpu_ctx_factory, scene)
    assert np.all(np.isfinite(got[1])) and got[1].max() > 0
    return got


def test_power_mode_changes_the_frames_and_the_default_mode_ignores_the_setter(gpu_ctx_factory, scene, base):
    uniform = _render(gpu_ctx_factory, scene, mode=pod.LIGHTS_UNIFORM)
    assert not _same(base, uniform), "the mode did nothing"
    assert _same(uniform, _render(gpu_ctx_factory, scene, mode=pod.LIGHTS_UNIFORM, never_set=True))


def test_classic_pipeline_equals_scan(gpu_ctx_factory, scene, base):
    assert _same(base, _render(gpu_ctx_factory, scene, compact=pod.COMPACT_ORDERED))


def test_tail_kernel_equals_the_level_by_level_pass(gpu_ctx_factory, scene, base):
    assert _same(base, _render(gpu_ctx_factory, scene, tail=3))


def test_four_frames_per_pass_equal_four_passes(gpu_ctx_factory, scene, base):
    assert _same(base, _render(gpu_ctx_factory, scene, per_pass=4))


def test_two_passes_in_flight_equal_one(gpu_ctx_factory, scene, base):
    assert _same(base, _render(gpu_ctx_factory, scene, in_flight=2))


def test_a_two_way_pixel_split_equals_the_full_frame(gpu_ctx_factory, scene, base):
    rows = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    for part in (rows[0::2].reshape(-1), rows[1::2].reshape(-1)):
        got = _render(gpu_ctx_factory, scene, pixel_map=part)
        assert _same((base[0][part], base[1][part]), got)


def test_an_environment_map_that_is_not_sampled_changes_nothing(gpu_ctx_factory, base):
    """a black map (it adds +0 to the paths that miss): the pass graph gets its miss type and keeps the continuation rays whose roulette
    is lost, the light sample still knows the mesh lights only"""
    with_map = LS.emitter_scene(W, H, path_length=4, objects=True)
    with_map.hdr_map = np.zeros((4, 8, 4), np.uint8)
    with_map.hdr_map[..., 3] = 255
    with_map.env_sampling = False
    assert _same(base, _render(gpu_ctx_factory, with_map))


def test_switching_the_mode_between_frames_uses_the_graph_of_the_mode(gpu_ctx_factory, scene, base):
    """frames 1-2 in the default mode, 3-4 in POWER mode, on one context: the last frame is POWER mode's frame 4 (pixel-keyed numbers)"""
    ctx = gpu_ctx_factory(W, H)
    scene.light_sampling = pod.LIGHTS_UNIFORM
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.set_tail_bounce(0)
    ctx.reset_frame_number()
    for f in range(FRAMES):
        ctx.set_light_sampling(pod.LIGHTS_POWER if f >= 2 else pod.LIGHTS_UNIFORM)
        ctx.render_frame()
        ctx.accumulate()
    assert np.array_equal(ctx.read_radiance().view(np.uint32), base[0].view(np.uint32))
    ctx.set_light_sampling(pod.LIGHTS_UNIFORM)  # ... and back: the default mode's graph, not the one built last
    ctx.set_frame_number(FRAMES - 1)
    ctx.render_frame()
    uniform = _render(gpu_ctx_factory, scene, mode=pod.LIGHTS_UNIFORM)
    assert np.array_equal(ctx.read_radiance().view(np.uint32), uniform[0].view(np.uint32))


# ---- expectation -------------------------------------------------------------------------------------------------------------

EXPECTATION_FRAMES = 1024  # 64 x 64 pixels in 16 x 16 blocks: the median relative standard error of the lit blocks is then below 2 % in both modes


def test_power_mode_has_the_default_mode_s_expectation(gpu_ctx_factory):
    S = 64
    est = {}
    for mode in (pod.LIGHTS_UNIFORM, pod.LIGHTS_POWER):
        sc = LS.emitter_scene(S, S, path_length=4, objects=True)
        sc.light_sampling = mode
        est[mode] = PP._gpu_estimate(gpu_ctx_factory(S, S), sc, S, S, EXPECTATION_FRAMES)
    a, b = est[pod.LIGHTS_POWER], est[pod.LIGHTS_UNIFORM]
    lit = b.mean > 0.02
    assert lit.mean() > 0.5
    rel = {m: np.median((e.se / np.maximum(e.mean, 1e-9))[lit]) for m, e in est.items()}
    print("median relative standard error of the lit blocks after %d frames: uniform %.4f, power %.4f" % (EXPECTATION_FRAMES, rel[pod.LIGHTS_UNIFORM], rel[pod.LIGHTS_POWER]))
    assert max(rel.values()) < 0.02, "the estimates are too noisy for a pass to mean anything"
    PP._assert_agree(PP._z(a.mean, a.se, b.mean, b.se)[lit], "emitter scene: NXHIP_LIGHTS_POWER against NXHIP_LIGHTS_UNIFORM")


# ---- physics: the form-factor pin of tests/test_physics_pins.py with its emitter cut into one large triangle and 30 slivers ------------

def _fan_light_scene(S, mode):
    x0, x1, z0, z1, h = PP.LIGHT
    floor = scenegen.quad((-8, 0, -8), (-8, 0, 8), (8, 0, 8), (8, 0, -8))
    light = LS.sliver_fan(x0, x1, z0, z1, h, 30)
    assert len(light) == 31
    mats = np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(PP.FLOOR_RHO,) * 3),
                     pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), emissive=(1.0, 1.0, 1.0), intensity=PP.LIGHT_LE)], dtype=pod.MAT_DT)
    eye = np.array((3.0, 0.8, 0.3))
    fwd = np.array((0.0, 0.0, 0.0)) - eye
    cam = capi.camera_init(tuple(eye), fwd / np.linalg.norm(fwd), 20.0, S, S, 5.0, 0.0)
    sc = SH.BuiltScene([floor, light], [(0, 0, workloads.IDENTITY), (1, 1, workloads.IDENTITY)], materials=mats, camera=cam,
                       settings=workloads.make_settings(use_mis=True, path_length=2, background=(1, 1, 1), background_intensity=0.0))
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    sc.light_sampling = mode
    return sc


def test_power_mode_matches_the_form_factor_of_a_badly_tessellated_emitter(gpu_ctx_factory):
    """One light of constant radiance: the mode is area-uniform sampling of the rectangle, whatever its triangles — rho L F(x) pins
    P, the density and the MIS lookup against a closed form (NEE + MIS, paths of two vertices; bars of DESIGN section 2)."""
    S, frames = 64, 4096
    e = PP._gpu_estimate(gpu_ctx_factory(S, S), _fan_light_scene(S, pod.LIGHTS_POWER), S, S, frames)
    want = PP._quad_light_expectation(_fan_light_scene(S, pod.LIGHTS_POWER), S, S)
    rel = np.median(e.se / want)
    print("fan emitter, power mode: median relative standard error %.4f after %d frames" % (rel, frames))
    assert rel < 0.02, "the estimate is too noisy for its pass to mean anything"
    PP._assert_agree(PP._z(e.mean, e.se, want, 0.0, systematic=2e-3), "fan of one large and 30 sliver triangles against the form factor, NXHIP_LIGHTS_POWER")
    # the default mode on the same emitter: the same expectation, more noise (30 of its 31 samples go to half of the area)
    u = PP._gpu_estimate(gpu_ctx_factory(S, S), _fan_light_scene(S, pod.LIGHTS_UNIFORM), S, S, frames)
    PP._assert_agree(PP._z(u.mean, u.se, want, 0.0, systematic=2e-3), "the same fan, NXHIP_LIGHTS_UNIFORM")
    print("median standard error: power %.5f, uniform %.5f" % (np.median(e.se), np.median(u.se)))
    assert np.median(e.se) < np.median(u.se)


# ---- noise ---------------------------------------------------------------------------------------------------------------------

def _two_lights_scene(mode):
    """two equal quads far above a floor, radiance 100 and 0.1; the camera sees the floor only; paths of two vertices"""
    floor = scenegen.quad((-80, 0, -80), (-80, 0, 80), (80, 0, 80), (80, 0, -80))
    panel = scenegen.quad((-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), (-0.5, 0, 0.5))
    mats = np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(0.6, 0.6, 0.6)),
                     pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), emissive=(1.0, 1.0, 1.0), intensity=100.0),
                     pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), emissive=(1.0, 1.0, 1.0), intensity=0.1)], dtype=pod.MAT_DT)
    eye = np.array((0.0, 2.0, 7.0))
    fwd = -eye / np.linalg.norm(eye)
    cam = capi.camera_init(tuple(eye), fwd, 30.0, W, H, 5.0, 0.0)
    sc = SH.BuiltScene([floor, panel], [(0, 0, workloads.IDENTITY), (1, 1, capi.mat4_from_trs((-1.5, 6.0, 0.0))), (1, 2, capi.mat4_from_trs((1.5, 6.0, 0.0)))],
                       materials=mats, camera=cam, settings=workloads.make_settings(use_mis=True, path_length=2, background=(1, 1, 1), background_intensity=0.0))
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    assert len(sc.lights) == 2
    sc.light_sampling = mode
    return sc


def test_power_mode_halves_the_noise_under_a_bright_and_a_dim_light(gpu_ctx_factory):
    """Mean squared error of an 8-frame estimate against a 512-frame POWER image (frames of their own), both modes: mse_power <
    0.5 mse_uniform.  Derived, not measured: with the dim light negligible the uniform estimator is 2 f 1[bright picked], whose
    variance f^2 (1 + 2 c^2) stands against f^2 c^2 (c: the relative deviation of f within the light) — a ratio below 1/2 for every c."""
    ref_ctx = gpu_ctx_factory(W, H)
    _two_lights_scene(pod.LIGHTS_POWER).upload(ref_ctx)
    ref_ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ref_ctx.set_frames_per_pass(64)
    ref_ctx.reset_frame_number()
    for _ in range(512 // 64):
        ref_ctx.render_frame()
        ref_ctx.accumulate()
    ref = ref_ctx.read_accumulation().astype(np.float64)
    assert ref.min() > 0, "every pixel sees the lit floor"
    mse = {}
    for mode in (pod.LIGHTS_UNIFORM, pod.LIGHTS_POWER):
        ctx = gpu_ctx_factory(W, H)
        _two_lights_scene(mode).upload(ctx)
        ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
        ctx.set_frames_per_pass(8)
        ctx.set_frame_number(512)  # frames 513 .. 520: independent of the reference image's
        ctx.render_frame()
        est = ctx.read_radiance().reshape(8, W * H, 3).astype(np.float64).mean(axis=0)
        mse[mode] = float(((est - ref) ** 2).mean())
    ratio = mse[pod.LIGHTS_POWER] / mse[pod.LIGHTS_UNIFORM]
    print("8-frame mean squared error: uniform %.5g, power %.5g, ratio %.4f" % (mse[pod.LIGHTS_UNIFORM], mse[pod.LIGHTS_POWER], ratio))
    assert mse[pod.LIGHTS_POWER] < 0.5 * mse[pod.LIGHTS_UNIFORM]
