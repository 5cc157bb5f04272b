"""NXHIP_LIGHT_IMPORTANCE_POSITION in the shading kernels: the wiring (every pass shape and pixel split gives the same bits; the other
modes and the classic pipeline are untouched), the expectation (POWER mode's, by z-scores; a closed form), the fog's scatter kernel, one
material of each kernel family, what it is for (less noise where a light is far away), and the upper layers.

Pixel-keyed random numbers; bars and helpers are those of tests/test_physics_pins.py.  The oracle does not know the mode."""
import os
import subprocess

import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen
from tests import feature_scenes as FS
from tests import light_scenes as LS
from tests import light_tree_scenes as LTS
from tests import oracle_lib as O
from tests import scene_helpers as SH
from tests import test_gpu_light_sampling as TLS
from tests import test_gpu_medium as TM
from tests import test_physics_pins as PP

pytestmark = pytest.mark.gpu

W, H = 64, 48
FRAMES = 4
POWER, POSITION = pod.LIGHT_IMPORTANCE_POWER, pod.LIGHT_IMPORTANCE_POSITION
SCAN = (pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)


def _render(gpu_ctx_factory, scene, mode=pod.LIGHTS_POWER, importance=POSITION, compact=pod.COMPACT_FAST, tail=0, per_pass=1, in_flight=1, pixel_map=None, never_set=False,
            want_tree=None):
    """FRAMES frames: (radiance of the last frame, accumulation), in the order of the context's pixels"""
    ctx = gpu_ctx_factory(W, H)
    if never_set:
        ctx.set_light_importance = lambda i: None  # (Workload.upload applies the workload's setting: this context never hears of it)
    scene.light_sampling, scene.light_importance = mode, importance
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
    if want_tree is not None:
        assert bool(ctx.debug_pass_flavor() & capi.FLAVOR_LIGHT_TREE) == want_tree
    n = ctx.local_count
    return ctx.read_radiance().reshape(per_pass, n, 3)[-1], ctx.read_accumulation()


_same = TLS._same


@pytest.fixture(scope="module")
def scene():
    return LS.emitter_scene(W, H)


@pytest.fixture(scope="module")
def power(gpu_ctx_factory, scene):
    return _render(gpu_ctx_factory, scene, importance=POWER, want_tree=False)


@pytest.fixture(scope="module")
def position(gpu_ctx_factory, scene):
    got = _render(gpu_ctx_factory, scene, want_tree=True)
    assert np.all(np.isfinite(got[1])) and got[1].max() > 0
    return got


def test_the_setter_with_power_changes_nothing_and_position_changes_the_frames(gpu_ctx_factory, scene, power, position):
    assert _same(power, _render(gpu_ctx_factory, scene, importance=POWER, never_set=True))
    assert not _same(power, position), "the setting did nothing"


def test_uniform_mode_ignores_the_setting(gpu_ctx_factory, scene):
    uniform = _render(gpu_ctx_factory, scene, mode=pod.LIGHTS_UNIFORM, importance=POWER, want_tree=False)
    assert _same(uniform, _render(gpu_ctx_factory, scene, mode=pod.LIGHTS_UNIFORM, importance=POSITION, want_tree=False))


def test_four_frames_per_pass_equal_four_passes(gpu_ctx_factory, scene, position):
    assert _same(position, _render(gpu_ctx_factory, scene, per_pass=4))


def test_two_passes_in_flight_equal_one(gpu_ctx_factory, scene, position):
    assert _same(position, _render(gpu_ctx_factory, scene, in_flight=2))


def test_a_two_way_pixel_split_equals_the_full_frame(gpu_ctx_factory, scene, position):
    rows = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    for part in (rows[0::2].reshape(-1), rows[1::2].reshape(-1)):
        assert _same((position[0][part], position[1][part]), _render(gpu_ctx_factory, scene, pixel_map=part))


def test_the_tail_bounce_setting_is_ignored(gpu_ctx_factory, scene, position):
    assert _same(position, _render(gpu_ctx_factory, scene, tail=2, want_tree=True))


def test_the_classic_pipeline_ignores_the_setting(gpu_ctx_factory, scene):
    assert _same(_render(gpu_ctx_factory, scene, importance=POWER, compact=pod.COMPACT_ORDERED, want_tree=False),
                 _render(gpu_ctx_factory, scene, importance=POSITION, compact=pod.COMPACT_ORDERED, want_tree=False))


def test_switching_between_frames_gives_each_frame_the_bits_of_its_mode(gpu_ctx_factory, scene, power, position):
    """frame 1 POSITION, 2 POWER, 3 POSITION, 4 POWER then POSITION again: every frame is the frame of a context that stayed in its mode"""
    stay = {}
    for importance in (POWER, POSITION):
        ctx = gpu_ctx_factory(W, H)
        scene.light_sampling, scene.light_importance = pod.LIGHTS_POWER, importance
        scene.upload(ctx)
        ctx.set_modes(*SCAN)
        ctx.set_tail_bounce(0)
        ctx.reset_frame_number()
        stay[importance] = []
        for _ in range(FRAMES):
            ctx.render_frame()
            stay[importance].append(ctx.read_radiance().copy())
    assert np.array_equal(stay[POSITION][-1].view(np.uint32), position[0].view(np.uint32)) and np.array_equal(stay[POWER][-1].view(np.uint32), power[0].view(np.uint32))
    ctx = gpu_ctx_factory(W, H)
    scene.light_importance = POSITION
    scene.upload(ctx)
    ctx.set_modes(*SCAN)
    ctx.set_tail_bounce(0)
    ctx.reset_frame_number()
    for f, importance in enumerate((POSITION, POWER, POSITION, POWER)):
        ctx.set_light_importance(importance)
        ctx.render_frame()
        assert np.array_equal(ctx.read_radiance().view(np.uint32), stay[importance][f].view(np.uint32)), "frame %d" % (f + 1)
        assert bool(ctx.debug_pass_flavor() & capi.FLAVOR_LIGHT_TREE) == (importance == POSITION)
    ctx.set_light_importance(POSITION)
    ctx.set_frame_number(FRAMES - 1)
    ctx.render_frame()
    assert np.array_equal(ctx.read_radiance().view(np.uint32), stay[POSITION][-1].view(np.uint32))


# ---- expectation -------------------------------------------------------------------------------------------------------------------

def _agree_with_power(est, what, lit_above=0.02):
    a, b = est[POSITION], est[POWER]
    lit = b.mean > lit_above
    rel = {m: np.median((e.se / np.maximum(e.mean, 1e-9))[lit]) for m, e in est.items()}
    print("%s: median relative standard error of the lit blocks: power %.4f, position %.4f" % (what, rel[POWER], rel[POSITION]))
    assert lit.mean() > 0.25 and max(rel.values()) < 0.02, "the estimates are too noisy for a pass to mean anything"
    PP._assert_agree(PP._z(a.mean, a.se, b.mean, b.se)[lit], "%s: POSITION against POWER" % what)


def test_position_has_power_mode_s_expectation(gpu_ctx_factory):
    S = 64
    est = {}
    for importance in (POWER, POSITION):
        sc = LS.emitter_scene(S, S, path_length=4, objects=True)
        sc.light_sampling, sc.light_importance = pod.LIGHTS_POWER, importance
        est[importance] = PP._gpu_estimate(gpu_ctx_factory(S, S), sc, S, S, 1024)
    _agree_with_power(est, "emitter scene")


def test_position_matches_the_form_factor_of_a_badly_tessellated_emitter(gpu_ctx_factory):
    """the fan emitter of tests/test_gpu_light_sampling.py: rho L F(x) pins P, the density and the MIS lookup together, systematic 2e-3"""
    S, frames = 64, 4096
    sc = TLS._fan_light_scene(S, pod.LIGHTS_POWER)
    sc.light_importance = POSITION
    ctx = gpu_ctx_factory(S, S)
    e = PP._gpu_estimate(ctx, sc, S, S, frames)
    assert ctx.debug_pass_flavor() & capi.FLAVOR_LIGHT_TREE
    want = PP._quad_light_expectation(sc, S, S)
    rel = np.median(e.se / want)
    print("fan emitter, position importance: median relative standard error %.4f after %d frames" % (rel, frames))
    assert rel < 0.02, "the estimate is too noisy for its pass to mean anything"
    PP._assert_agree(PP._z(e.mean, e.se, want, 0.0, systematic=2e-3), "fan of one large and 30 sliver triangles against the form factor, POSITION")


def _two_lamps_in_fog():
    """the lamp scene of tests/test_gpu_medium.py (its builder, its camera, its lamp and material) with a second, dimmer lamp on the other
    side of the fog box — the two triangles of ONE quad share their box, so a single lamp is the same pick in both importances"""
    cam = capi.camera_init((0.0, 0.0, 4.0), (0.0, 0.0, -1.0), 30.0, TM.W, TM.H, 5.0, 0.0)
    lamps = [scenegen.quad((-0.9, -0.3, 0.0), (-0.9, 0.3, 0.0), (-0.5, 0.3, 0.0), (-0.5, -0.3, 0.0)), scenegen.quad((0.6, -0.2, 0.0), (0.6, 0.2, 0.0), (0.9, 0.2, 0.0), (0.9, -0.2, 0.0))]
    mats = [pod.make_material(pod.MAT_DIFFUSE, albedo=(0, 0, 0), emissive=(1.0, 0.9, 0.8), intensity=6.0), pod.make_material(pod.MAT_DIFFUSE, albedo=(0, 0, 0), emissive=(0.6, 0.8, 1.0), intensity=3.0)]
    return TM._scene(cam, lamps, mats, path_length=3, use_mis=True)


def test_position_in_fog(gpu_ctx_factory):
    """two lamps in the fog of tests/test_gpu_medium.py: the scatter kernel's light sample descends the tree from the scatter point"""
    est, frames = {}, {}
    for importance in (POWER, POSITION):
        sc = _two_lamps_in_fog()
        sc.light_importance = importance
        frames[importance] = TM._frames(gpu_ctx_factory, sc, TM.LAMP_FOG, 1024, light_sampling=pod.LIGHTS_POWER)
        est[importance] = TM._estimate(frames[importance])
    assert not np.array_equal(frames[POWER], frames[POSITION]), "the scatter kernel's light sample did not change"
    a, b = est[POSITION], est[POWER]
    lit = b.mean.max(1) > 0
    assert lit.sum() >= 12
    PP._assert_agree(PP._z(a.mean, a.se, b.mean, b.se)[lit], "lamp in fog: POSITION against POWER")


def _families_scene(S, importance):
    """the box of tests/feature_scenes.py (detail-mapped plastic, conductor and diffuse surfaces under a mesh emitter) with one surface
    metal-rough and the pane alpha-masked: the SOLID instance, which holds the METAL and DETAIL cases"""
    sc = FS.all_features_scene(S, S, features=("detail", "power"), path_length=4)
    sc.materials = sc.materials.copy()
    k = next(i for i, m in enumerate(sc.materials) if int(m["type"]) == pod.MAT_PLASTIC)
    rough = pod.make_material(pod.MAT_METALROUGH, albedo=(0.8, 0.6, 0.3), roughness=0.5, metallic=0.7)
    for field in ("emissive", "intensity", "opacity", "diffuseMapId", "emissiveMapId"):
        rough[field] = sc.materials[k][field]
    sc.materials[k] = rough
    alphas = np.array([pod.make_material_alpha()] * len(sc.materials), dtype=pod.ALPHA_DT)
    alphas[-1] = pod.make_material_alpha(pod.ALPHA_MASK, 0.5)
    sc.material_alpha = alphas
    sc.light_importance = importance
    return sc


@pytest.mark.parametrize("family", ["detail", "metal", "solid"])
def test_one_material_of_each_family(gpu_ctx_factory, family):
    S = 48
    est = {}
    for importance in (POWER, POSITION):
        sc = _families_scene(S, importance)
        if family != "solid":
            sc.material_alpha = None
        if family == "detail":
            sc = FS.all_features_scene(S, S, features=("detail", "power"), path_length=4)
            sc.light_importance = importance
        ctx = gpu_ctx_factory(S, S)
        est[importance] = PP._gpu_estimate(ctx, sc, S, S, 1024)
        flavor = ctx.debug_pass_flavor()
        assert bool(flavor & capi.FLAVOR_LIGHT_TREE) == (importance == POSITION) and flavor & capi.FLAVOR_DETAIL
        assert bool(flavor & capi.FLAVOR_METAL) == (family != "detail") and bool(flavor & capi.FLAVOR_SOLID) == (family == "solid")
    _agree_with_power(est, "the %s family" % family)


# ---- noise -------------------------------------------------------------------------------------------------------------------------

def _form_factor_of_panel(p, cx):
    """point-to-rectangle form factor of the 1 x 1 panel centred at (cx, PANEL_H, 0) seen from floor points p[:, (x, z)], by a 64 x 64 midpoint rule"""
    g = (np.arange(64) + 0.5) / 64 - 0.5
    X, Z = np.meshgrid(cx + g, g)
    dx, dz = X[None] - p[:, 0, None, None], Z[None] - p[:, 1, None, None]
    d2 = dx * dx + dz * dz + LTS.PANEL_H ** 2
    return (LTS.PANEL_H ** 2 / (np.pi * d2 * d2)).mean(axis=(1, 2))


def test_position_halves_the_noise_under_a_near_and_a_far_light(gpu_ctx_factory):
    """Mean squared error of an 8-frame estimate against a 512-frame POSITION image (frames of their own): mse_position < 0.5 mse_power.
    Derived as in tests/test_gpu_light_sampling.py: with the far panel negligible, POWER's estimator is 2 f 1[near picked] with variance
    f^2 (1 + 2 c^2), POSITION's has f^2 c'^2."""
    sc = LTS.two_far_panels(W, H, POSITION)
    cam = sc.camera
    pos = cam["position"].astype(np.float64)
    jj, ii = np.mgrid[0:H, 0:W]
    d = cam["lowerLeftCorner"].astype(np.float64) + cam["viewportX"].astype(np.float64) * ((ii + 0.5) / W).reshape(-1, 1) + cam["viewportY"].astype(np.float64) * ((jj + 0.5) / H).reshape(-1, 1) - pos
    assert np.all(d[:, 1] < 0), "every pixel sees the floor"
    p = (pos + d * (-pos[1] / d[:, 1])[:, None])[:, [0, 2]]
    assert np.all(np.hypot(p[:, 0] - LTS.NEAR_X, p[:, 1]) < LTS.PATCH), "... within PATCH of the point under the near panel"
    near, far = _form_factor_of_panel(p, LTS.NEAR_X), _form_factor_of_panel(p, LTS.FAR_X)
    print("far / (near + far) form factor over the visible floor: max %.4g" % (far / (near + far)).max())
    assert np.all(far < 0.01 * (near + far)), "the far panel gives less than 1 % of every visible pixel's radiance"
    ref_ctx = gpu_ctx_factory(W, H)
    sc.upload(ref_ctx)
    ref_ctx.set_modes(*SCAN)
    ref_ctx.set_frames_per_pass(64)
    ref_ctx.reset_frame_number()
    for _ in range(512 // 64):
        ref_ctx.render_frame()
        ref_ctx.accumulate()
    ref = ref_ctx.read_accumulation().astype(np.float64)
    assert ref.min() > 0, "every pixel sees the lit floor"
    mse = {}
    for importance in (POWER, POSITION):
        ctx = gpu_ctx_factory(W, H)
        LTS.two_far_panels(W, H, importance).upload(ctx)
        ctx.set_modes(*SCAN)
        ctx.set_frames_per_pass(8)
        ctx.set_frame_number(512)  # frames 513 .. 520: independent of the reference image's
        ctx.render_frame()
        est = ctx.read_radiance().reshape(8, W * H, 3).astype(np.float64).mean(axis=0)
        mse[importance] = float(((est - ref) ** 2).mean())
    print("8-frame mean squared error: power %.5g, position %.5g, ratio %.4f" % (mse[POWER], mse[POSITION], mse[POSITION] / mse[POWER]))
    assert mse[POSITION] < 0.5 * mse[POWER]


# ---- upper layers ------------------------------------------------------------------------------------------------------------------

def test_set_light_importance_through_the_facade_equals_the_capi_path(gpu_ctx_factory):
    S, frames = 96, 3
    sc = capi.Scene(S, S)
    sc.load_file(SH.GOLDEN + os.sep, "cornell_box_sphere.glb")
    sc.set_camera((0.0, 1.0, 3.9), (0.0, 0.0, -1.0), 40.0, 5.0, 0.0)
    sc.set_render_settings(O.make_settings(use_mis=True, path_length=6))
    sc.update()
    pt = capi.PathTracer(S, S)
    pt.set_modes(*SCAN)
    with pytest.raises(capi.NexusError, match="unknown importance"):
        pt.set_light_importance(7)
    pt.set_light_sampling(pod.LIGHTS_POWER)
    pt.set_light_importance(POSITION)
    pt.update_device_scene(sc)
    for _ in range(frames):
        pt.render(sc)
    scene = SH.glb_scene(os.path.join(SH.GOLDEN, "cornell_box_sphere.glb"), S, S, path_length=6)
    scene.light_sampling, scene.light_importance = pod.LIGHTS_POWER, POSITION
    ctx = gpu_ctx_factory(S, S)
    scene.upload(ctx)
    ctx.set_modes(*SCAN)
    ctx.reset_frame_number()
    for _ in range(frames):
        ctx.render_frame()
        ctx.accumulate()
    assert ctx.debug_pass_flavor() & capi.FLAVOR_LIGHT_TREE
    assert np.array_equal(pt.read_pixels(), ctx.read_rgba8())
    assert np.array_equal(pt.read_accumulation().view(np.uint32), ctx.read_accumulation().view(np.uint32))
    pt.close()


def test_nexus_render_light_sampling_position(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "nexus_render")
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "nexus_render.cpp"), "-o", exe,
           "-L" + os.path.join(root, "nexus_amd", "lib"), "-lnexus_amd", "-Wl,-rpath," + os.path.join(root, "nexus_amd", "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = str(tmp_path / "cornell.ppm")
    r = subprocess.run([exe, "--light-sampling", "position", SH.GOLDEN + os.sep, "cornell_box.glb", out, "64", "64", "3", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    header = b"P6\n64 64\n255\n"
    data = open(out, "rb").read()
    assert data.startswith(header) and len(data) == len(header) + 64 * 64 * 3 and max(data[len(header):]) > 0
    r = subprocess.run([exe, "--light-sampling", "nearest", SH.GOLDEN + os.sep, "cornell_box.glb", out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "position" in r.stderr
