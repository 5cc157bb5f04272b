"""Transparent shadows on the device (nxhip_set_shadow_transmittance): the any-hit TRANSMIT instance against the float64 reference of the
contract (tests/transmittance_reference.py, within the tolerance tests/test_transmittance_reference.py derives), light transport behind
see-through surfaces against closed forms by z-scores per 16 x 16 block (the bars of tests/test_physics_pins.py), and the wiring: every
pipeline, pass shape and pixel split gives the same bits.  The oracle does not know the mode; nothing here compares with it."""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen, workloads
from tests import analytic_light_reference as AR
from tests import scene_helpers as SH
from tests import test_gpu_analytic_lights as AL
from tests import test_physics_pins as PP
from tests import test_transmittance_reference as TR
from tests import transmittance_reference as R

pytestmark = pytest.mark.gpu

W, H = AL.W, AL.H
RHO = AL.RHO
N_UP = AL._tilted(0.0)


# ---- 1. the hook against the reference ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [pod.SHADOWS_OPAQUE, pod.SHADOWS_TRANSMIT], ids=["context opaque", "context transmit"])
def test_hook_matches_the_reference(gpu_ctx_factory, mode):
    """(what dominates the derived tolerance is a 1/256 weight that may round either way in binary32: tests/test_transmittance_reference.py)"""
    scene = TR.hook_scene()
    rays, tmax = TR.hook_rays()
    r64, keep, tol = TR.hook_reference()
    assert 1.0 - keep.mean() <= 0.02, "the reference alone keeps the unclear share at or below 2 %"
    ctx = gpu_ctx_factory(TR.HOOK_W, TR.HOOK_H)
    scene.shadow_transmittance = mode
    scene.upload(ctx)
    got = ctx.trace_transmittance_batch(rays, tmax)  # (runs whatever the context's mode is)
    assert got.dtype == np.float32
    ok, text = R.check(got, r64, tol, what="device")
    print(text)
    assert ok, text
    # the plain hook still answers "occluded" wherever anything was crossed
    occluded = ctx.trace_shadow_batch(rays, tmax)
    assert np.array_equal(occluded[keep] != 0, r64["crossed"][keep] > 0)
    # ... and the counting variant of the instance gives the same bits
    ctx.enable_trace_stats(True)
    assert np.array_equal(ctx.trace_transmittance_batch(rays, tmax).view(np.uint32), got.view(np.uint32))
    ctx.enable_trace_stats(False)
    ctx.close()


# ---- 2. a point light behind a pane ------------------------------------------------------------------------------------------------------

LIGHT = pod.make_analytic_light(pod.ALIGHT_POINT, position=(-0.4, 2.0, 0.2), colour=(1.0, 0.8, 0.6), intensity=7.0)
PANE = AL.OCCLUDER
# the pane of the map case: its shadow covers the image's third block row, the split of its two halves falls between two block columns
# (16 x 16 pixel blocks see trapezoids of the floor; under AL.OCCLUDER no block lies wholly behind one half)
PANE_MAP = (-1.02, -0.15, -0.44, 0.76, 1.0)
ALPHA_HALF = 128
MAP_H = 64


def _pane(with_map):
    return PANE_MAP if with_map else PANE


def _pane_scene(with_map):
    scene = AL._floor_scene(occluder=_pane(with_map))
    scene.materials[-1]["opacity"] = 0.5
    if with_map:  # alpha 128 / 255 on the half of lower z, 0 on the other (the quad's t runs along z)
        img = np.zeros((MAP_H, 2, 4), np.uint8)
        img[..., :3] = 90
        img[:MAP_H // 2, :, 3] = ALPHA_HALF
        scene.materials[-1]["diffuseMapId"] = 0
        scene.diffuse_maps = [img]
    return scene


def _pane_regions(with_map):
    """[(rectangle, T)]: where the pane's o a is constant.  With the map the two halves stop one texel short of where the bilinear lookup
    blends: the middle, and both ends (wrap)."""
    x0, x1, z0, z1, h = _pane(with_map)
    if not with_map:
        return [((x0, x1, z0, z1, h), 0.5)]
    texel, mid = (z1 - z0) / MAP_H, 0.5 * (z0 + z1)
    return [((x0, x1, z0 + texel, mid - texel, h), 1.0 - 0.5 * ALPHA_HALF / 255.0), ((x0, x1, mid + texel, z1 - texel, h), 1.0)]


@pytest.mark.parametrize("with_map", [False, True], ids=["opacity 0.5", "opacity 0.5 x two-block alpha"])
def test_point_light_behind_a_pane(gpu_ctx_factory, with_map):
    scene = _pane_scene(with_map)
    P = AL._floor_points(scene, N_UP, 8)
    centre = AR.table(LIGHT)["centre"]
    # NO camera ray crosses the pane (a pass-through of the camera path would spend a bounce): float64, every sub-pixel position
    assert np.all(AL._visible(np.broadcast_to(AL.EYE, P.shape), P, _pane(with_map))), "a camera ray crosses the pane"
    full = AL._blocks((RHO / np.pi) * AL._direct(LIGHT, P, N_UP)[0].mean(0))
    clear = AL._blocks(AL._visible(P, centre, _pane(with_map)).mean(0)[:, None].astype(np.float64))[:, 0] == 1.0
    want, behind = full.copy(), np.zeros(len(full), bool)
    squared = full.copy()
    for rect, T in _pane_regions(with_map):
        inside = AL._blocks((~AL._visible(P, centre, rect)).mean(0)[:, None].astype(np.float64))[:, 0] == 1.0
        print("T = %.4f: %d blocks wholly behind" % (T, inside.sum()))
        assert inside.sum() >= 1, "no block wholly behind this part of the pane"
        want[inside] *= T
        squared[inside] *= T * T
        behind |= inside
    attenuated = behind & (want[:, 0] < full[:, 0])
    print("blocks: %d wholly behind the pane (%d of them attenuated), %d wholly clear, %d on an edge" % (behind.sum(), attenuated.sum(), clear.sum(), len(full) - behind.sum() - clear.sum()))
    assert attenuated.sum() >= 1 and clear.sum() >= 4 and not np.any(behind & clear)
    use = behind | clear
    scene.shadow_transmittance = pod.SHADOWS_TRANSMIT
    e = AL._estimate(gpu_ctx_factory, scene, [LIGHT], AL.FRAMES)
    AL._pin(e, want, "point light behind a pane", use=use)  # (refuses the expectation x 1.03 too)
    assert not AL._agrees(PP._z(e.mean, e.se, squared, 0.0, systematic=2e-3)[attenuated], "control: T squared"), "the check has no power"
    # the default: the same blocks are exactly black — today's behaviour, which is what fails without the feature
    scene.shadow_transmittance = pod.SHADOWS_OPAQUE
    dark = AL._estimate(gpu_ctx_factory, scene, [LIGHT], 64)
    assert np.all(dark.mean[behind] == 0.0) and np.all(dark.mean[clear] > 0.0)


# ---- 3. MIS == naive through a see-through sheet ---------------------------------------------------------------------------------------------

# The sheet (x0, x1, z0, z1, height) between the floor and the emitter (PP.LIGHT, height 1.2).  One below the eye (height 0.8) would be
# crossed by the camera rays of every block that lies behind it; one above it is so near the emitter that its penumbra is wider than the
# image (a 0.9 high edge: 3.6 along x on the floor).  So the two kinds of block come from two placements: OVER — every segment floor
# point -> emitter point of every block crosses it — and ASIDE — none does (the pass still runs the TRANSMIT instance).
SHEETS = {"over": (-4.0, 4.0, -4.0, 4.0, 0.9), "aside": (-4.0, 4.0, 2.0, 6.0, 0.9)}


def _sheet_scene(use_mis, where):
    base = PP._quad_light_scene(W, H, use_mis)
    x0, x1, z0, z1, h = SHEETS[where]
    sheet = scenegen.quad((x0, h, z0), (x1, h, z0), (x1, h, z1), (x0, h, z1))
    mats = np.append(base.materials, np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), opacity=0.5)], dtype=pod.MAT_DT))
    sc = SH.BuiltScene(list(base.meshes) + [sheet], [(0, 0, workloads.IDENTITY), (1, 1, workloads.IDENTITY), (2, 2, workloads.IDENTITY)], materials=mats, camera=base.camera,
                       # floor, sheet, emitter: the BSDF-sampled side spends a bounce on the pass-through
                       settings=workloads.make_settings(use_mis=use_mis, path_length=3, background=(1, 1, 1), background_intensity=0.0))
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    assert len(sc.lights) == 1
    return sc


def _sheet_expectation(where):
    """rho L F x 0.5 (OVER: every floor point of every block sees every emitter point through the sheet) or rho L F (ASIDE: none does).
    The segment floor point -> emitter point meets the sheet's plane at an affine image of the emitter point: the emitter's four corners
    decide for a rectangle."""
    scene = _sheet_scene(True, where)
    P = AL._floor_points(scene, N_UP, 4)
    assert np.all(AL._visible(np.broadcast_to(AL.EYE, P.shape), P, SHEETS[where])), "a camera ray crosses the sheet"
    x0, x1, z0, z1, h = PP.LIGHT
    vis = np.stack([AL._visible(P, np.array((x, h, z)), SHEETS[where]) for x in (x0, x1) for z in (z0, z1)])  # (corner, sub, pixel)
    assert np.all(~vis) if where == "over" else np.all(vis)
    F = PP._quad_light_expectation(scene, W, H, sub=4)
    return F * (0.5 if where == "over" else 1.0), F


def _sheet_estimate(gpu_ctx_factory, where, use_mis, shadows, light_sampling, frames=4096):
    ctx = gpu_ctx_factory(W, H)
    scene = _sheet_scene(use_mis, where)
    scene.shadow_transmittance, scene.light_sampling = shadows, light_sampling
    e = PP._gpu_estimate(ctx, scene, W, H, frames)
    flavor = ctx.debug_pass_flavor()
    assert bool(flavor & capi.FLAVOR_TRANSMIT) == (shadows == pod.SHADOWS_TRANSMIT), "flavor %#x" % flavor
    ctx.close()
    return e


@pytest.mark.parametrize("light_sampling", [pod.LIGHTS_UNIFORM, pod.LIGHTS_POWER], ids=["uniform", "power"])
def test_mis_equals_naive_through_a_see_through_sheet(gpu_ctx_factory, light_sampling):
    want, F = _sheet_expectation("over")
    naive = _sheet_estimate(gpu_ctx_factory, "over", False, pod.SHADOWS_OPAQUE, light_sampling)
    mis = _sheet_estimate(gpu_ctx_factory, "over", True, pod.SHADOWS_TRANSMIT, light_sampling)
    for name, e in (("useMIS 0", naive), ("useMIS 1, TRANSMIT", mis)):
        print("%s: relative standard error of the block means, median %.2g" % (name, np.median(e.se / want)))
        assert np.median(e.se / want) < 0.05, "the estimate is too noisy for its pass to mean anything"
        assert AL._agrees(PP._z(e.mean, e.se, want, 0.0, systematic=2e-3), name + " against the closed form"), name
    assert AL._agrees(PP._z(mis.mean, mis.se, naive.mean, naive.se), "MIS + TRANSMIT against BSDF sampling alone")
    assert not AL._agrees(PP._z(mis.mean, mis.se, F, 0.0, systematic=2e-3), "control: the unattenuated closed form"), "the check has no power"
    assert not AL._agrees(PP._z(mis.mean, mis.se, want * 1.03, 0.0, systematic=2e-3), "control: expectation x 1.03"), "the check has no power"
    # the default's shadow rays stop at the sheet: the light sample's share is lost and the image is too dark
    opaque = _sheet_estimate(gpu_ctx_factory, "over", True, pod.SHADOWS_OPAQUE, light_sampling, frames=1024)
    assert not AL._agrees(PP._z(opaque.mean, opaque.se, want, 0.0, systematic=2e-3), "control: useMIS 1 in OPAQUE mode")
    assert np.all(opaque.mean < want)


def test_a_sheet_no_segment_crosses_leaves_the_closed_form(gpu_ctx_factory):
    want, F = _sheet_expectation("aside")
    mis = _sheet_estimate(gpu_ctx_factory, "aside", True, pod.SHADOWS_TRANSMIT, pod.LIGHTS_UNIFORM)
    assert np.array_equal(want, F)
    assert AL._agrees(PP._z(mis.mean, mis.se, want, 0.0, systematic=2e-3), "useMIS 1, TRANSMIT, every block clear"), "clear blocks"
    assert not AL._agrees(PP._z(mis.mean, mis.se, want * 1.03, 0.0, systematic=2e-3), "control: expectation x 1.03"), "the check has no power"


# ---- 4. the sampled environment ------------------------------------------------------------------------------------------------------------

SKY_PANE = (-1.8, 0.4, -1.0, 1.0, 1.0)  # above the eye: no camera ray reaches it


def _sky_scene():
    scene = AL._floor_scene(occluder=SKY_PANE)
    scene.materials[-1]["opacity"] = 0.5
    scene.settings = workloads.make_settings(use_mis=True, path_length=3, background=(1, 1, 1), background_intensity=0.0)  # floor, pane, sky
    scene.hdr_map = np.full((4, 8, 4), 255, np.uint8)  # (the sRGB table takes 255 to exactly 1)
    scene.env_sampling = True
    return scene


def _hemisphere_quadrature(P, cells, seed=3):
    """(1 / pi) int T(w) cos dw over the upper hemisphere of every floor point P (sub, pixels, 3), T = 0.5 where the direction meets the
    pane (analytic, AL._visible), else 1: cosine-distributed midpoints of cells x cells in (u, phi), the grid moved by its own offset per
    floor point (fixed seed).  Per pixel."""
    g = (np.arange(cells) + 0.5) / cells
    uu, vv = [a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij")]
    rng = np.random.RandomState(seed)
    pixels = P.shape[1]
    out = np.zeros(pixels)
    for a in range(len(P)):
        shift = rng.rand(pixels, 2)
        u, v = (uu[None, :] + shift[:, 0:1]) % 1.0, (vv[None, :] + shift[:, 1:2]) % 1.0
        r, phi = np.sqrt(u), 2.0 * np.pi * v
        w = np.stack([r * np.cos(phi), np.sqrt(1.0 - u), r * np.sin(phi)], -1)  # (pixels, C, 3), normal +y
        o = np.broadcast_to(P[a][:, None, :], w.shape)
        out += np.where(AL._visible(o, o + w * 100.0, SKY_PANE), 1.0, 0.5).mean(1)
    return out / len(P)


def test_sampled_environment_over_a_pane(gpu_ctx_factory):
    """Every floor point sees a finite pane somewhere, so no block's hemisphere is wholly clear: all blocks are compared with the
    quadrature, which tends to rho c away from the pane."""
    scene = _sky_scene()
    P = AL._floor_points(scene, N_UP, 2)
    assert np.all(AL._visible(np.broadcast_to(AL.EYE, P.shape), P, SKY_PANE)), "a camera ray crosses the pane"
    coarse, fine = AL._blocks(RHO * _hemisphere_quadrature(P, 12)[:, None]), AL._blocks(RHO * _hemisphere_quadrature(P, 24)[:, None])
    residue = (np.abs(fine - coarse) / RHO).max()
    under = fine[:, 0] < 0.8 * RHO
    print("quadrature residue 12 -> 24 cells: max %.3g of rho c; attenuation %.3f .. %.3f, %d blocks below 0.8" % (residue, (fine / RHO).min(), (fine / RHO).max(), under.sum()))
    assert residue < 2e-3 and under.sum() >= 3 and (fine / RHO).max() > 0.93
    want = fine * np.ones((1, 3))
    scene.shadow_transmittance = pod.SHADOWS_TRANSMIT
    e = _estimate(gpu_ctx_factory, scene, AL.FRAMES)
    print("relative standard error of the block means, median %.2g" % np.median(e.se / want))
    assert AL._agrees(PP._z(e.mean, e.se, want, 0.0, systematic=2e-3), "sampled environment over a pane")
    assert not AL._agrees(PP._z(e.mean, e.se, want * 1.03, 0.0, systematic=2e-3), "control: expectation x 1.03")
    assert not AL._agrees(PP._z(e.mean, e.se, np.full_like(want, RHO), 0.0, systematic=2e-3)[under], "control: no pane")
    scene.shadow_transmittance = pod.SHADOWS_OPAQUE
    opaque = _estimate(gpu_ctx_factory, scene, AL.FRAMES)
    assert not AL._agrees(PP._z(opaque.mean, opaque.se, want, 0.0, systematic=2e-3)[under], "control: OPAQUE mode")


def _estimate(gpu_ctx_factory, scene, frames, per_pass=64):
    ctx = gpu_ctx_factory(W, H)
    e = PP._gpu_estimate(ctx, scene, W, H, frames, per_pass=per_pass)
    ctx.close()
    return e


# ---- 5. equal bits ---------------------------------------------------------------------------------------------------------------------------

BOX_FRAMES = AL.BOX_FRAMES
INSIDE = capi.mat4_from_trs((0.1, 1.1, 0.1), (10.0, 30.0, -5.0), (0.6, 1.0, 0.5))   # between the ceiling light and the floor
OUTSIDE = capi.mat4_from_trs((0.0, -1.0, 0.0), (0.0, 0.0, 0.0), (0.5, 1.0, 0.5))    # under the floor: no shadow ray can cross it


def _box_scene(quad):
    base = SH.cornell_scene(W, H, path_length=4)
    if quad is None:
        return base
    placements = [(int(i["bvhIdx"]), int(i["materialId"]), i["transform"].copy()) for i in base.instances]
    placements.append((len(base.meshes), len(base.materials), quad))
    mats = np.append(base.materials, np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(0.8, 0.8, 0.8), opacity=0.7, diffuse_map=0)], dtype=pod.MAT_DT))
    sc = SH.BuiltScene(list(base.meshes) + [scenegen.quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1))], placements, materials=mats, camera=base.camera, settings=base.settings,
                       diffuse_maps=[SH.checker_texture(64, 32, 1, alpha=True)])
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    return sc


def _box_render(gpu_ctx_factory, quad=INSIDE, modes_per_frame=(pod.SHADOWS_TRANSMIT,) * BOX_FRAMES, compact=pod.COMPACT_FAST, tail=0, per_pass=1, in_flight=1, pixel_map=None, stats=False,
                want_flavor=True):
    ctx = gpu_ctx_factory(W, H)
    _box_scene(quad).upload(ctx)
    ctx.set_analytic_lights(AL.BOX_LIGHTS)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, compact, pod.CONDUCTOR_REFERENCE)
    if pixel_map is not None:
        ctx.set_pixel_map(pixel_map)
    ctx.enable_trace_stats(stats)
    ctx.set_tail_bounce(tail)
    ctx.set_frames_per_pass(per_pass)
    ctx.set_passes_in_flight(in_flight)
    ctx.reset_frame_number()
    for f in range(BOX_FRAMES // per_pass):
        ctx.set_shadow_transmittance(modes_per_frame[f * per_pass])
        ctx.render_frame()
        ctx.accumulate()
    ctx.sync()
    flavor = ctx.debug_pass_flavor()
    assert bool(flavor & capi.FLAVOR_TRANSMIT) == want_flavor, "flavor %#x" % flavor
    n = ctx.local_count
    out = ctx.read_radiance().reshape(per_pass, n, 3)[-1], ctx.read_accumulation(), flavor
    ctx.close()
    return out


_same = AL._same
OPAQUE = (pod.SHADOWS_OPAQUE,) * BOX_FRAMES


@pytest.fixture(scope="module")
def box(gpu_ctx_factory):
    got = _box_render(gpu_ctx_factory)
    assert np.all(np.isfinite(got[1])) and got[1].max() > 0
    return got


def test_the_mode_changes_the_frames_and_switching_it_off_restores_the_default(gpu_ctx_factory, box):
    never = _box_render(gpu_ctx_factory, modes_per_frame=OPAQUE, want_flavor=False)
    assert not _same(box, never), "the mode did nothing"
    assert np.all(box[1] >= never[1]), "light through the quad only adds (same random streams, T x radiance in place of nothing)"
    # frames 1-2 TRANSMIT, 3-4 OPAQUE on one context: the last frame and the flavor are the default's
    back = _box_render(gpu_ctx_factory, modes_per_frame=(pod.SHADOWS_TRANSMIT,) * 2 + (pod.SHADOWS_OPAQUE,) * 2, want_flavor=False)
    assert np.array_equal(back[0].view(np.uint32), never[0].view(np.uint32)) and back[2] == never[2]
    forth = _box_render(gpu_ctx_factory, modes_per_frame=(pod.SHADOWS_OPAQUE,) * 2 + (pod.SHADOWS_TRANSMIT,) * 2)
    assert np.array_equal(forth[0].view(np.uint32), box[0].view(np.uint32)) and forth[2] == box[2]


def test_a_repeated_frame_equals_itself(gpu_ctx_factory, box):
    assert _same(box, _box_render(gpu_ctx_factory))


def test_classic_pipeline_equals_scan(gpu_ctx_factory, box):
    assert _same(box, _box_render(gpu_ctx_factory, compact=pod.COMPACT_ORDERED))


def test_four_frames_per_pass_equal_four_passes(gpu_ctx_factory, box):
    assert _same(box, _box_render(gpu_ctx_factory, per_pass=4))


def test_two_passes_in_flight_equal_one(gpu_ctx_factory, box):
    assert _same(box, _box_render(gpu_ctx_factory, in_flight=2))


def test_a_two_way_pixel_split_equals_the_full_frame(gpu_ctx_factory, box):
    rows = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    for part in (rows[0::2].reshape(-1), rows[1::2].reshape(-1)):
        assert _same((box[0][part], box[1][part]), _box_render(gpu_ctx_factory, pixel_map=part))


def test_trace_statistics_do_not_change_the_frames(gpu_ctx_factory, box):
    assert _same(box, _box_render(gpu_ctx_factory, stats=True))


def test_the_tail_kernel_setting_is_ignored(gpu_ctx_factory, box):
    assert _same(box, _box_render(gpu_ctx_factory, tail=3))


def test_an_all_opaque_scene_launches_the_default_kernels(gpu_ctx_factory):
    default = _box_render(gpu_ctx_factory, quad=None, modes_per_frame=OPAQUE, want_flavor=False)
    transmit = _box_render(gpu_ctx_factory, quad=None, want_flavor=False)
    assert _same(default, transmit) and default[2] == transmit[2]


def test_a_see_through_quad_no_shadow_ray_can_cross(gpu_ctx_factory):
    """under the box's floor: the flavor bit is set, the TRANSMIT instance runs, and every frame is the default's"""
    default = _box_render(gpu_ctx_factory, quad=OUTSIDE, modes_per_frame=OPAQUE, want_flavor=False)
    transmit = _box_render(gpu_ctx_factory, quad=OUTSIDE)
    assert _same(default, transmit) and transmit[2] == default[2] | capi.FLAVOR_TRANSMIT
