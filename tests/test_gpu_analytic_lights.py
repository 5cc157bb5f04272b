"""Analytic lights on the device (nxhip_set_analytic_lights): the sampling hook against the float64 reference of the contract
(tests/analytic_light_reference.py, within the tolerance tests/test_analytic_light_reference.py derives), light transport against closed
forms by z-scores per 16 x 16 block (the bars of tests/test_physics_pins.py), and the wiring: every pipeline, pass shape and pixel split
gives the same bits.  The oracle does not know these lights; nothing here compares with it."""
import functools

import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen, workloads
from tests import analytic_light_reference as R
from tests import scene_helpers as SH
from tests import test_analytic_light_reference as TR
from tests import test_bsdf_pins as BP
from tests import test_physics_pins as PP

pytestmark = pytest.mark.gpu

W = H = 64
EYE = np.array((3.0, 0.8, 0.3))
RHO = 0.6
SCAN = (pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)


# ---- 1. the hook against the reference ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hook_ctx(gpu_ctx_factory):
    ctx = gpu_ctx_factory(16, 16)
    ctx.set_analytic_lights(TR.HOOK_LIGHTS)
    return ctx


@pytest.mark.parametrize("k", range(len(TR.HOOK_LIGHTS)), ids=["point", "sphere0.5", "sphere1e-3", "spot", "disc"])
def test_hook_matches_the_reference(hook_ctx, k):
    light = TR.HOOK_LIGHTS[k]
    o, r = TR.hook_inputs(k)
    (bar_d, bar_t, bar_f), keep, ref = TR.hook_tolerance(k)
    direction, tmax, factor, ok = hook_ctx.analytic_light_sample_batch(k, o, r)
    # d <= radius gives ok = 0, everything else a sample
    assert np.array_equal(ok, ref["ok"])
    if float(light["radius"]) > 0:
        assert (~ok).sum() == TR.HOOK_INSIDE
    d64, t64, f64 = direction.astype(np.float64), tmax.astype(np.float64), factor.astype(np.float64)
    dev_d = np.sqrt(((d64 - ref["direction"]) ** 2).sum(1))[keep]
    dev_f = (np.abs(f64 - ref["factor"]).max(1) / ref["unattenuated"].max(1))[keep]
    finite = keep & (ref["tmax"] < 1e29)
    dev_t = (np.abs(t64 - ref["tmax"]) / np.abs(ref["tmax"]))[finite]
    print("direction %.3g (bar %.3g), tmax %.3g (bar %.3g), factor %.3g (bar %.3g); %d of %d draws left out (rim cap, d <= radius)"
          % (dev_d.max(), bar_d, dev_t.max() if finite.any() else 0.0, bar_t, dev_f.max(), bar_f, (~keep).sum(), len(keep)))
    assert dev_d.max() <= bar_d and dev_f.max() <= bar_f
    if finite.any():
        assert dev_t.max() <= bar_t
    else:
        assert np.all(tmax == np.float32(1e30))
    assert (ok & ~keep).mean() <= 1e-3
    # every direction meets the float64 light, or lies within the rim cap
    hit, margin = R.hits_light(light, o, d64)
    assert np.all(hit[ok] | (margin[ok] >= -R.RIM_CAP)), "worst %.3g rad outside" % -margin[ok].min()
    # the draws cover the cone uniformly: 16 x 16 cells in (1 - cos theta, phi)
    if float(ref["q"][ok].max()) > 0:
        u, v = R.cone_coordinates(light, o, d64)
        cells = np.bincount((np.minimum((u[ok] * 16).astype(int), 15) * 16 + np.minimum((v[ok] * 16).astype(int), 15)), minlength=256)
        e = ok.sum() / 256.0
        chi2, dof = ((cells - e) ** 2 / e).sum(), 255
        print("chi^2 %.1f on %d cells: %.2f sigma" % (chi2, 256, (chi2 - dof) / np.sqrt(2 * dof)))
        assert (chi2 - dof) / np.sqrt(2 * dof) < 5
    else:
        assert np.all(dev_d <= bar_d) and np.allclose(t64[ok], ref["d"][ok], rtol=bar_t)


# ---- 2. transport pins -----------------------------------------------------------------------------------------------------------------------

def _tilted(angle):
    """unit normal of the floor plane through the origin, rotated `angle` about z towards +x"""
    return np.array([np.sin(angle), np.cos(angle), 0.0])


def _floor_scene(use_mis=True, mat=None, tilt=0.0, occluder=None, emitter=False):
    """A floor through the origin seen by a camera that sees nothing else; paths of two vertices: the floor point and what its light sample
    (and its BSDF sample) finds.  tilt: the floor's normal leans towards the camera.  occluder: (x0, x1, z0, z1, height), a black quad."""
    n = _tilted(tilt)
    ux, uz = np.array([n[1], -n[0], 0.0]), np.array([0.0, 0.0, 1.0])
    c = [tuple(a * 8 * ux + b * 8 * uz) for a, b in ((-1, -1), (-1, 1), (1, 1), (1, -1))]
    meshes, placements = [scenegen.quad(*c)], [(0, 0, workloads.IDENTITY)]
    mats = [mat if mat is not None else pod.make_material(pod.MAT_DIFFUSE, albedo=(RHO,) * 3)]
    if emitter:
        x0, x1, z0, z1, h = PP.LIGHT
        meshes.append(scenegen.quad((x0, h, z0), (x1, h, z0), (x1, h, z1), (x0, h, z1)))
        placements.append((len(meshes) - 1, len(mats), workloads.IDENTITY))
        mats.append(pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), emissive=(1.0, 1.0, 1.0), intensity=PP.LIGHT_LE))
    if occluder is not None:
        x0, x1, z0, z1, h = occluder
        meshes.append(scenegen.quad((x0, h, z0), (x1, h, z0), (x1, h, z1), (x0, h, z1)))
        placements.append((len(meshes) - 1, len(mats), workloads.IDENTITY))
        mats.append(pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0)))
    fwd = -EYE / np.linalg.norm(EYE)
    cam = capi.camera_init(tuple(EYE), fwd, 20.0, W, H, 5.0, 0.0)
    sc = SH.BuiltScene(meshes, placements, materials=np.array(mats, dtype=pod.MAT_DT), camera=cam,
                       settings=workloads.make_settings(use_mis=use_mis, path_length=2, background=(1, 1, 1), background_intensity=0.0))
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    assert len(sc.lights) == (1 if emitter else 0)
    return sc


def _floor_points(scene, normal, sub):
    """the floor points of sub x sub positions in every pixel: (sub^2, pixels, 3), float64"""
    cam = scene.camera
    pos = cam["position"].astype(np.float64)
    jj, ii = np.mgrid[0:H, 0:W]
    out = []
    for a in range(sub):
        for b in range(sub):
            x = ((ii + (a + 0.5) / sub) / W).reshape(-1, 1)
            y = ((jj + (b + 0.5) / sub) / H).reshape(-1, 1)
            d = cam["lowerLeftCorner"].astype(np.float64) + cam["viewportX"].astype(np.float64) * x + cam["viewportY"].astype(np.float64) * y - pos
            t = -(pos @ normal) / (d @ normal)
            assert np.all(t > 0), "every pixel must see the floor"
            p = pos + d * t[:, None]
            assert np.all(np.abs(p) < 7.5)
            out.append(p)
    return np.stack(out)


def _direct(light, P, normal):
    """closed form, without the albedo: I cos / d^2 x att (POINT, SPOT; the sphere above the horizon), E cos (DIRECTIONAL; the disc above it):
    (..., 3); and the falloff's argument cd x scale + offset before the clamp"""
    T = R.table(light)
    if T["kind"] == R.DIRECTIONAL:
        cos_s = float(-(T["axis"] @ normal))
        assert np.arcsin(cos_s) > 2.0 * np.arcsin(np.sqrt(T["q"] / 2.0))
        return np.ones(P.shape[:-1])[..., None] * (T["power"] * cos_s), np.ones(P.shape[:-1])
    to = T["centre"] - P
    d = np.sqrt((to * to).sum(-1))
    cos_s = (to @ normal) / d
    assert np.all(d * cos_s > T["radius"])
    x = -((to / d[..., None]) @ T["axis"]) * T["scale"] + T["offset"]
    return (np.clip(x, 0.0, 1.0) ** 2 * cos_s / (d * d))[..., None] * T["power"], x


def _blocks(per_pixel):
    ids, nb = PP._block_ids(W, H)
    per_pixel = per_pixel.reshape(W * H, -1)
    return np.stack([np.bincount(ids, weights=per_pixel[:, c], minlength=nb) for c in range(per_pixel.shape[1])], 1) / np.bincount(ids, minlength=nb)[:, None]


def _estimate(gpu_ctx_factory, scene, lights, frames, modes=SCAN, light_sampling=pod.LIGHTS_UNIFORM, per_pass=64):
    ctx = gpu_ctx_factory(W, H)
    scene.light_sampling = light_sampling
    scene.upload(ctx)
    ctx.set_analytic_lights(np.array(lights, dtype=pod.ALIGHT_DT))
    ctx.set_modes(*modes)
    ctx.set_frames_per_pass(per_pass)
    ctx.reset_frame_number()
    e = PP._Estimate(W, H)
    assert frames % per_pass == 0
    for _ in range(frames // per_pass):
        ctx.render_frame()
        r = ctx.read_radiance().reshape(per_pass, W * H, 3)
        for k in range(per_pass):
            e.add(r[k])
    assert ctx.debug_pass_flavor() & capi.FLAVOR_ANALYTIC
    ctx.close()
    return e


def _agrees(z, what):
    z = z[np.isfinite(z)]
    print("%s: %d comparisons, max |z| %.2f, mean z^2 %.2f" % (what, z.size, np.abs(z).max(), (z * z).mean()))
    return np.abs(z).max() < 4.5 and (z * z).mean() < 1.6


def _pin(e, want, what, use=None, systematic=2e-3, extra=0.0):
    """the estimate agrees with `want` per block and channel, and `want` x 1.03 is refused"""
    use = np.ones(len(want), bool) if use is None else use
    rel = np.median((e.se / np.maximum(want, 1e-30))[use])
    print("%s: relative standard error of the block means, median %.2g, max %.2g" % (what, rel, (e.se / np.maximum(want, 1e-30))[use].max()))
    se_w = np.zeros_like(want) + extra
    assert _agrees(PP._z(e.mean, e.se, want, se_w, systematic=systematic)[use], what), what
    assert not _agrees(PP._z(e.mean, e.se, want * 1.03, se_w * 1.03, systematic=systematic)[use], what + ", control: expectation x 1.03"), "the check has no power"


FRAMES = 1024
POINT = pod.make_analytic_light(pod.ALIGHT_POINT, position=(-0.4, 1.5, 0.2), colour=(1.0, 0.8, 0.6), intensity=5.0)
PLAIN = {
    "point": (POINT, 0.0),
    "point, floor tilted 50 degrees": (POINT, np.radians(50.0)),
    "sphere r 0.5 at height 2": (pod.make_analytic_light(pod.ALIGHT_POINT, position=(-0.4, 2.0, 0.2), colour=(1.0, 0.8, 0.6), intensity=7.0, radius=0.5), 0.0),
    "sphere r 2e-3 at height 2": (pod.make_analytic_light(pod.ALIGHT_POINT, position=(-0.4, 2.0, 0.2), colour=(1.0, 0.8, 0.6), intensity=7.0, radius=2e-3), 0.0),
    "delta sun": (pod.make_analytic_light(pod.ALIGHT_DIRECTIONAL, direction=(0.4, -0.8, 0.3), colour=(1.0, 0.9, 0.7), intensity=3.0), 0.0),
    "disc at 40 degrees": (pod.make_analytic_light(pod.ALIGHT_DIRECTIONAL, direction=(-np.cos(np.radians(40)) * 0.8, -np.sin(np.radians(40)), np.cos(np.radians(40)) * 0.6),
                                                   colour=(1.0, 0.9, 0.7), intensity=3.0, angular_radius=0.05), 0.0),
}


@pytest.mark.parametrize("name", list(PLAIN))
def test_direct_light_matches_the_closed_form(gpu_ctx_factory, name):
    light, tilt = PLAIN[name]
    scene = _floor_scene(tilt=tilt)
    n = _tilted(tilt)
    want = _blocks((RHO / np.pi) * _direct(light, _floor_points(scene, n, 8), n)[0].mean(0))
    assert want.min() > 0
    _pin(_estimate(gpu_ctx_factory, scene, [light], FRAMES), want, name)


def test_spot_falloff_band_and_the_dark_outside(gpu_ctx_factory):
    spot = pod.make_analytic_light(pod.ALIGHT_SPOT, position=(2.0, 2.0, 0.1), direction=(0.0, -2.0, 0.0), colour=(1.0, 0.5, 0.25), intensity=9.0, inner_cone=0.25, outer_cone=0.8)
    scene = _floor_scene()
    n = _tilted(0.0)
    value, x = _direct(spot, _floor_points(scene, n, 8), n)
    want = _blocks((RHO / np.pi) * value.mean(0))
    x_mean = _blocks(x.mean(0)[:, None])[:, 0]
    ids, nb = PP._block_ids(W, H)
    x_max = np.array([x.max(0)[ids == b].max() for b in range(nb)])
    x_min = np.array([x.min(0)[ids == b].min() for b in range(nb)])
    dark = x_max < -0.05                                 # wholly outside the outer cone, with a margin of 5 % of the band
    lit = want[:, 0] > 0.02 * want[:, 0].max()
    band = lit & (x_min > 0.05) & (x_max < 0.95)          # wholly inside the falloff band
    print("blocks: %d dark, %d lit, %d of them wholly in the band, %d fully lit" % (dark.sum(), lit.sum(), band.sum(), (x_min >= 1.0).sum()))
    assert dark.sum() >= 2 and band.sum() >= 2
    e = _estimate(gpu_ctx_factory, scene, [spot], FRAMES)
    assert np.all(e.mean[dark] == 0.0), "outside the outer cone the falloff is exactly 0"
    _pin(e, want, "spot", use=lit)
    # att^2, not att: in the band the two differ by the factor x itself
    assert not _agrees(PP._z(e.mean, e.se, want / np.maximum(x_mean, 1e-3)[:, None], 0.0, systematic=2e-3)[band], "spot, control: att not squared")


OCCLUDER = (-1.0, 0.2, -0.5, 0.1, 1.0)  # x0, x1, z0, z1, height


def _visible(P, target, rect=OCCLUDER):
    """does the segment from the floor points P to `target` (broadcast) pass the rectangle (x0, x1, z0, z1, height)?  (analytic: the plane y = height)"""
    x0, x1, z0, z1, h = rect
    t = (h - P[..., 1]) / (target[..., 1] - P[..., 1])
    at = P + (target - P) * t[..., None]
    return ~((t > 0) & (t < 1) & (at[..., 0] > x0) & (at[..., 0] < x1) & (at[..., 2] > z0) & (at[..., 2] < z1))


def test_an_occluder_under_the_point_light(gpu_ctx_factory):
    light = pod.make_analytic_light(pod.ALIGHT_POINT, position=(-0.4, 2.0, 0.2), colour=(1.0, 0.8, 0.6), intensity=7.0)
    scene = _floor_scene(occluder=OCCLUDER)
    n = _tilted(0.0)
    P = _floor_points(scene, n, 8)
    vis = _visible(P, R.table(light)["centre"])
    ids, nb = PP._block_ids(W, H)
    frac = _blocks(vis.mean(0)[:, None].astype(np.float64))[:, 0]
    want = _blocks((RHO / np.pi) * _direct(light, P, n)[0].mean(0))
    umbra, lit = frac == 0.0, frac == 1.0
    # (blocks the shadow's edge crosses: the edge is sharp, sub-pixel positions decide — not compared)
    print("blocks: %d in the umbra, %d lit, %d on the edge" % (umbra.sum(), lit.sum(), nb - umbra.sum() - lit.sum()))
    assert umbra.sum() >= 1 and lit.sum() >= 4
    e = _estimate(gpu_ctx_factory, scene, [light], FRAMES)
    assert np.all(e.mean[umbra] == 0.0)
    _pin(e, want, "point light beside an occluder", use=lit)


def _cone_quadrature(light, P, n, cells, rect=OCCLUDER, to_centre=False, seed=3):
    """float64 quadrature of a sphere light's direct light past a rectangle, over the pixel AND the cone: for each of the sub-pixel floor
    points P (sub^2, pixels, 3) the midpoints of cells x cells in the cone's (u, phi) — the grid moved by its own offset per floor point
    (fixed seed), so that the grids of a block's 256 x sub^2 floor points do not cut the shadow's edge alike and their errors do not add
    up —, the analytic ray-rectangle test along each direction as far as the sphere's near surface (to_centre: as far as the centre's
    distance instead, the wrong shadow ray of a control).  Per pixel (pixels, 3), without the albedo."""
    g = (np.arange(cells) + 0.5) / cells
    uu, vv = [a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij")]
    C, pixels = len(uu), P.shape[1]
    rng = np.random.RandomState(seed)
    out = np.zeros((pixels, 3))
    for a in range(len(P)):
        shift = rng.rand(pixels, 2)
        u, v = (uu[None, :] + shift[:, 0:1]) % 1.0, (vv[None, :] + shift[:, 1:2]) % 1.0
        o = np.repeat(P[a], C, 0)
        s = R.sample(light, o, np.stack([u.ravel(), v.ravel()], 1))
        w = s["direction"]
        vis = _visible(o, o + w * (s["d"] if to_centre else s["tmax"])[:, None], rect)
        out += s["factor"].reshape(pixels, C, 3)[:, 0, :] * np.where(vis, w @ n, 0.0).reshape(pixels, C).mean(1)[:, None]
    return out / len(P)


SPHERE = pod.make_analytic_light(pod.ALIGHT_POINT, position=(-0.4, 2.0, 0.2), colour=(1.0, 0.8, 0.6), intensity=7.0, radius=0.5)


def test_the_penumbra_under_the_sphere(gpu_ctx_factory):
    scene = _floor_scene(occluder=OCCLUDER)
    n = _tilted(0.0)
    P = _floor_points(scene, n, 4)  # 4 x 4 positions in every pixel, as the closed-form cases average over the pixel
    coarse, fine = _blocks((RHO / np.pi) * _cone_quadrature(SPHERE, P, n, 6)), _blocks((RHO / np.pi) * _cone_quadrature(SPHERE, P, n, 12))
    full = _blocks((RHO / np.pi) * _direct(SPHERE, P, n)[0].mean(0))
    # The quadrature's residue, measured by doubling the cell count: 1.5e-3 of the unoccluded value in the worst block between 6 x 6 and
    # 12 x 12 cells per floor point (4 096 floor points per block), which bounds what is left in the finer one.  It must stay under the
    # 2e-3 the comparison allows for the expectation; it is NOT added to the z-scores' denominator.
    residue = (np.abs(fine - coarse) / full).max()
    partial = (fine[:, 0] > 0.02 * full[:, 0]) & (fine[:, 0] < 0.98 * full[:, 0])
    print("quadrature residue 6 -> 12 cells: max %.3g of the unoccluded value; %d blocks in the penumbra, brightest block %.3f of its unoccluded value"
          % (residue, partial.sum(), (fine / full).max()))
    assert partial.sum() >= 3 and residue < 2e-3
    e = _estimate(gpu_ctx_factory, scene, [SPHERE], FRAMES)
    _pin(e, fine, "sphere light behind an occluder", use=fine[:, 0] > 0.02 * full[:, 0])
    assert not _agrees(PP._z(e.mean, e.se, full, 0.0, systematic=2e-3)[partial], "control: the unoccluded closed form in the penumbra")


INSIDE = (-0.7, -0.1, -0.1, 0.5, 1.8)  # a quad INSIDE the sphere, between its near surface and its centre (corners 0.47 from the centre)


def test_the_shadow_ray_ends_at_the_spheres_surface(gpu_ctx_factory):
    """A black quad inside the sphere light occludes nothing: every shadow ray ends at the near intersection with the sphere, in front of
    it, and the floor keeps the unoccluded closed form.  A shadow ray as long as the distance to the CENTRE runs into the quad for most
    directions: that expectation (the same quadrature, rays to_centre) is 48-73 % of the closed form, and the frames must refuse it."""
    scene = _floor_scene(occluder=INSIDE)
    n = _tilted(0.0)
    c, (x0, x1, z0, z1, h) = R.table(SPHERE)["centre"], INSIDE
    assert max(np.linalg.norm(np.array([x, h, z]) - c) for x in (x0, x1) for z in (z0, z1)) < float(SPHERE["radius"])
    want = _blocks((RHO / np.pi) * _direct(SPHERE, _floor_points(scene, n, 8), n)[0].mean(0))
    P = _floor_points(scene, n, 2)
    right = _blocks((RHO / np.pi) * _cone_quadrature(SPHERE, P, n, 8, rect=INSIDE))
    wrong = _blocks((RHO / np.pi) * _cone_quadrature(SPHERE, P, n, 8, rect=INSIDE, to_centre=True))
    print("quadrature with the quad inside: rays to the surface %.5f .. %.5f of the closed form, rays to the centre %.3f .. %.3f"
          % ((right / want).min(), (right / want).max(), (wrong / want).min(), (wrong / want).max()))
    assert np.allclose(right, want, rtol=5e-4) and (wrong / want).max() < 0.8
    e = _estimate(gpu_ctx_factory, scene, [SPHERE], FRAMES)
    _pin(e, want, "sphere light with a quad inside it")
    assert not _agrees(PP._z(e.mean, e.se, wrong, 0.0, systematic=2e-3), "control: shadow rays as long as the distance to the centre")


def test_point_light_under_a_sampled_environment(gpu_ctx_factory):
    """Mesh lights (none here), analytic lights, then the environment: a floor under a uniform white map that the light sample picks too,
    plus a point light, MIS on.  rho L + rho / pi I cos / d^2; nLights = 2 enters the environment's pick, the weight of the BSDF-sampled
    miss (SCAN: the material launch's miss type; CLASSIC: the one-item logic kernel's ANALYTIC instance) and the analytic factor.  The
    two pipelines give the same frames bit for bit."""
    n = _tilted(0.0)
    est = {}
    for name, modes in (("scan", SCAN), ("classic", (pod.RNG_PIXEL_KEYED, pod.COMPACT_ORDERED, pod.CONDUCTOR_EXTENDED))):
        scene = _floor_scene()
        scene.hdr_map = np.full((4, 8, 4), 255, np.uint8)  # (the sRGB table takes 255 to exactly 1)
        scene.env_sampling = True
        est[name] = _estimate(gpu_ctx_factory, scene, [POINT], FRAMES, modes=modes)
    point = _blocks((RHO / np.pi) * _direct(POINT, _floor_points(_floor_scene(), n, 8), n)[0].mean(0))
    sky = np.full_like(point, RHO * 1.0)
    assert np.array_equal(est["scan"].s, est["classic"].s) and np.array_equal(est["scan"].s2, est["classic"].s2)
    e = est["scan"]
    print("relative standard error of the block means, median %.2g" % np.median(e.se / (sky + point)))
    assert _agrees(PP._z(e.mean, e.se, sky + point, 0.0, systematic=2e-3), "environment + point, MIS")
    assert not _agrees(PP._z(e.mean, e.se, 1.25 * sky + point, 0.0, systematic=2e-3), "control: the environment's part x 1.25")
    assert not _agrees(PP._z(e.mean, e.se, sky + 1.25 * point, 0.0, systematic=2e-3), "control: the point's part x 1.25")
    assert not _agrees(PP._z(e.mean, e.se, (sky + point) * 1.03, 0.0, systematic=2e-3), "control: expectation x 1.03")


MIXED_POINT = pod.make_analytic_light(pod.ALIGHT_POINT, position=(-1.5, 1.0, 0.8), colour=(1.0, 1.0, 1.0), intensity=16.0)


@functools.lru_cache(maxsize=None)
def _mixed_expectation():
    scene = _floor_scene(emitter=True)
    n = _tilted(0.0)
    emitter = PP._quad_light_expectation(scene, W, H, sub=4)
    point = _blocks((RHO / np.pi) * _direct(MIXED_POINT, _floor_points(scene, n, 4), n)[0].mean(0))
    return emitter * (RHO / PP.FLOOR_RHO), point


def _check_mixed(e, what):
    emitter, point = _mixed_expectation()
    assert 0.2 < np.median(emitter / point) < 5.0, "both parts must matter"
    rel = np.median(e.se / (emitter + point))
    print("%s: relative standard error, median %.2g" % (what, rel))
    assert _agrees(PP._z(e.mean, e.se, emitter + point, 0.0, systematic=2e-3), what)
    assert not _agrees(PP._z(e.mean, e.se, 1.25 * emitter + point, 0.0, systematic=2e-3), what + ", control: the emitter's part x 1.25")
    assert not _agrees(PP._z(e.mean, e.se, emitter + 1.25 * point, 0.0, systematic=2e-3), what + ", control: the point's part x 1.25")


@pytest.mark.parametrize("mode", [pod.LIGHTS_UNIFORM, pod.LIGHTS_POWER], ids=["uniform", "power"])
def test_mesh_emitter_and_point_light_under_mis(gpu_ctx_factory, mode):
    """rho L F + rho / pi I cos / d^2: nLights = 2 in the mesh light's pdf, in the emissive hit's weight and in the analytic factor"""
    _check_mixed(_estimate(gpu_ctx_factory, _floor_scene(emitter=True), [MIXED_POINT], 4096, light_sampling=mode), "emitter + point, MIS")


def test_mesh_emitter_and_point_light_without_mis(gpu_ctx_factory):
    """useMIS = 0: BSDF sampling finds the emitter, the analytic-only light sample (nLights := A) the point"""
    _check_mixed(_estimate(gpu_ctx_factory, _floor_scene(use_mis=False, emitter=True), [MIXED_POINT], 4096), "emitter + point, useMIS 0")


GLOSSY = {
    "conductor r0.3": BP.MATS["conductor r0.3"],
    "plastic": pod.make_material(pod.MAT_PLASTIC, albedo=(0.6, 0.4, 0.2), roughness=0.45, ior=1.5),
}


@pytest.mark.parametrize("name", list(GLOSSY))
def test_glossy_floor_under_the_point_light(gpu_ctx_factory, name):
    """f cos from the published-formula evaluators of tests/test_bsdf_pins.py, Eval's validity rule (pdf > 1e-4) applied, x I / d^2"""
    mat = GLOSSY[name]
    light = pod.make_analytic_light(pod.ALIGHT_POINT, position=(-2.8, 1.0, -0.1), colour=(1.0, 0.9, 0.8), intensity=6.0)  # where the floor mirrors it towards the camera
    scene = _floor_scene(mat=mat)
    lob = BP.Lobes(mat)
    Pl, WI = BP._pixel_geometry(scene, W, H)  # the floor's local frame: (x, z, height)
    c = R.table(light)["centre"]
    to = np.array([c[0], c[2], c[1]])[None, :] - Pl
    d2 = (to * to).sum(1)
    wo = to / np.sqrt(d2)[:, None]
    want = np.zeros((W * H, 3))
    for k in range(W * H):
        f, p = lob.eval(WI[k], wo[k][None, :])
        want[k] = np.where(p[0] > 1e-4, f[0], 0.0) * R.table(light)["power"] / d2[k]
    want = _blocks(want)
    lit = want.max(1) > 0.05 * want.max()
    assert lit.mean() > 0.3
    _pin(_estimate(gpu_ctx_factory, scene, [light], FRAMES), want, name + " floor", use=lit, systematic=1e-2)


# ---- 3. equal bits ---------------------------------------------------------------------------------------------------------------------------

BOX_LIGHTS = np.array([
    pod.make_analytic_light(pod.ALIGHT_POINT, position=(0.4, 1.2, 0.3), colour=(1.0, 0.8, 0.6), intensity=0.8, radius=0.05),
    pod.make_analytic_light(pod.ALIGHT_SPOT, position=(-0.5, 1.8, 0.0), direction=(0.2, -1.0, 0.1), colour=(0.4, 0.6, 1.0), intensity=2.0, inner_cone=0.3, outer_cone=0.6),
    pod.make_analytic_light(pod.ALIGHT_DIRECTIONAL, direction=(0.2, -0.5, -1.0), colour=(1.0, 1.0, 0.9), intensity=0.7, angular_radius=0.02),
], dtype=pod.ALIGHT_DT)
BOX_FRAMES = 4  # (three frames and one more, so that four frames per pass divide them)


def _box_render(gpu_ctx_factory, compact=pod.COMPACT_FAST, tail=0, per_pass=1, in_flight=1, pixel_map=None, lights=BOX_LIGHTS, force_general=None, power_from=None, then_none=False,
                want_flavor=True):
    ctx = gpu_ctx_factory(W, H)
    scene = SH.cornell_scene(W, H, path_length=4)
    scene.upload(ctx)
    if lights is not None:
        ctx.set_analytic_lights(lights)
    if then_none:
        ctx.set_analytic_lights(np.zeros(0, pod.ALIGHT_DT))
    ctx.set_modes(pod.RNG_PIXEL_KEYED, compact, pod.CONDUCTOR_REFERENCE)
    if pixel_map is not None:
        ctx.set_pixel_map(pixel_map)
    if force_general is not None:
        ctx.debug_pass_flavor(force_general=force_general)
    ctx.set_tail_bounce(tail)
    ctx.set_frames_per_pass(per_pass)
    ctx.set_passes_in_flight(in_flight)
    ctx.reset_frame_number()
    for f in range(BOX_FRAMES // per_pass):
        if power_from is not None:
            ctx.set_light_sampling(pod.LIGHTS_POWER if power_from[f] else pod.LIGHTS_UNIFORM)
        ctx.render_frame()
        ctx.accumulate()
    ctx.sync()
    flavor = ctx.debug_pass_flavor()
    assert bool(flavor & capi.FLAVOR_ANALYTIC) == want_flavor, "flavor %#x" % flavor
    n = ctx.local_count
    out = ctx.read_radiance().reshape(per_pass, n, 3)[-1], ctx.read_accumulation(), flavor
    ctx.close()
    return out


def _same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.fixture(scope="module")
def box(gpu_ctx_factory):
    got = _box_render(gpu_ctx_factory)
    assert np.all(np.isfinite(got[1])) and got[1].max() > 0
    return got


def test_the_lights_change_the_frames_and_removing_them_restores_the_default(gpu_ctx_factory, box):
    never = _box_render(gpu_ctx_factory, lights=None, want_flavor=False)
    assert not _same(box, never), "the lights did nothing"
    removed = _box_render(gpu_ctx_factory, then_none=True, want_flavor=False)
    assert _same(never, removed) and never[2] == removed[2]


def test_classic_pipeline_equals_scan(gpu_ctx_factory, box):
    assert _same(box, _box_render(gpu_ctx_factory, compact=pod.COMPACT_ORDERED))


def test_tail_kernel_equals_the_level_by_level_pass(gpu_ctx_factory, box):
    assert _same(box, _box_render(gpu_ctx_factory, tail=2))
    assert _same(box, _box_render(gpu_ctx_factory, tail=3))


def test_four_frames_per_pass_equal_four_passes(gpu_ctx_factory, box):
    assert _same(box, _box_render(gpu_ctx_factory, per_pass=4))


def test_two_passes_in_flight_equal_one(gpu_ctx_factory, box):
    assert _same(box, _box_render(gpu_ctx_factory, in_flight=2))


def test_a_two_way_pixel_split_equals_the_full_frame(gpu_ctx_factory, box):
    rows = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    for part in (rows[0::2].reshape(-1), rows[1::2].reshape(-1)):
        assert _same((box[0][part], box[1][part]), _box_render(gpu_ctx_factory, pixel_map=part))


def test_the_map_free_instance_equals_the_general_one(gpu_ctx_factory, box):
    assert box[2] & capi.FLAVOR_NO_MAPS, "the Cornell box names no map"
    general = _box_render(gpu_ctx_factory, force_general=capi.FLAVOR_IDENTITY | capi.FLAVOR_NO_MAPS)
    assert not general[2] & capi.FLAVOR_NO_MAPS and _same(box, general)


def test_switching_power_sampling_between_frames(gpu_ctx_factory, box):
    """frames 1-2 uniform, 3-4 POWER on one context: the last frame is the POWER context's frame 4; and all-uniform is the base"""
    power = _box_render(gpu_ctx_factory, power_from=[True] * 4)
    mixed = _box_render(gpu_ctx_factory, power_from=[False, False, True, True])
    assert np.array_equal(mixed[0].view(np.uint32), power[0].view(np.uint32))
    assert _same(box, _box_render(gpu_ctx_factory, power_from=[False] * 4))
    back = _box_render(gpu_ctx_factory, power_from=[True, True, False, False])
    assert np.array_equal(back[0].view(np.uint32), box[0].view(np.uint32))
