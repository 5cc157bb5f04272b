"""Direct light on a normal-mapped floor under analytic lights, behind a see-through pane, through an absorbing density grid: the float64
expectation with EVERY factor, composed from the references the per-feature tests already hold — no new physics.  For the floor point x
the camera sees through the pixel position s:

    E[radiance] = T_grid(eye -> x) x sum over the lights l of
                  closed_form_l(x, ns(x), rho) x (1 - opacity x alpha)^[the segment x -> l crosses the pane] x T_grid(x -> l)

    T_grid       exp(-optical_depth)                   tests/grid_medium_reference.py
    ns           shading_frame, as test_gpu_detail_maps._reference calls it   tests/detail_reference.py
    closed_form  with ns as the normal                 tests/analytic_light_reference.py (restated for arrays of points: closed_form_many;
                                                       tests/test_feature_product_reference.py holds the two against each other)
    the pane     transmittance                         tests/transmittance_reference.py

averaged over sub x sub positions per pixel (test_gpu_analytic_lights._floor_points), then over 16 x 16 pixel blocks.  Every factor has a
switch, so the same text gives the expectation with any one factor, or any one light, left out: what a kernel instance that dropped it
would render.  The medium absorbs only (albedo 0) and every surface but the floor is black, so at a path length of 2 the product is the
whole expectation.

The scene is here too (scene(), LIGHTS, MEDIUM, density()), shared by the CPU file that shows it can tell the factors apart and by
tests/test_gpu_feature_products.py."""
import functools

import numpy as np

from nexus_amd import pod, scenegen, workloads
from tests import analytic_light_reference as AR
from tests import grid_medium_reference as G
from tests import medium_reference as MR
from tests import scene_helpers as SH
from tests import test_gpu_analytic_lights as AL
from tests import test_gpu_detail_maps as DM
from tests import transmittance_reference as TRN

W = H = 64
RHO = DM.RHO
EYE = DM.EYE
N_UP = np.array([0.0, 1.0, 0.0])
UV_REPEAT = 24.0
BLOCKS = 16

# ---- the scene ---------------------------------------------------------------------------------------------------------------------------------

# the fog: an absorbing box between the floor and the lights, across part of the camera segments (the eye, at height 0.8, is outside it:
# x = 3 against the box's 1.2); a grid whose dimensions are no multiples of the 8-voxel brick
BOX_MIN, BOX_MAX = (-1.5, 0.2, -1.5), (1.2, 0.7, 1.5)
SIGMA_T = 0.6
GRID_SHAPE = (13, 9, 20)  # (nz, ny, nx)
MEDIUM = pod.make_medium(box_min=BOX_MIN, box_max=BOX_MAX, sigma_t=SIGMA_T, g=0.0, albedo=(0, 0, 0))

# the pane: a black see-through sheet at height 2, above the eye (no camera ray reaches it) and below every light
PANE = (-6.0, 3.2, -4.1, 3.9, 2.0)  # x0, x1, z0, z1, height
PANE_OPACITY = 0.5
PANE_ALPHA = (255, 102)  # the two blocks of its alpha map along z: 1 - 0.5 x 1 = 0.5 and 1 - 0.5 x 0.4 = 0.8
MAP_H = 64

LIGHTS = {
    "point": pod.make_analytic_light(pod.ALIGHT_POINT, position=(-0.5, 2.5, 0.4), colour=(1.0, 0.8, 0.6), intensity=9.0),
    "spot": pod.make_analytic_light(pod.ALIGHT_SPOT, position=(1.6, 1.8, -0.6), direction=(-0.55, -1.0, 0.25), colour=(0.5, 0.8, 1.0), intensity=14.0, inner_cone=0.35,
                                    outer_cone=1.2),
    "sun": pod.make_analytic_light(pod.ALIGHT_DIRECTIONAL, direction=(-0.6, -0.7, 0.3), colour=(1.0, 0.9, 0.7), intensity=1.6),
}
ALL = tuple(LIGHTS)
FACTORS = ("fog_camera", "fog_shadow", "pane", "detail")


def light_array(names=ALL):
    return np.array([LIGHTS[n] for n in names], dtype=pod.ALIGHT_DT)


def normal_map():
    """the varying 4 x 4 map of test_gpu_detail_maps.test_a_varying_map_matches_the_quadrature: leaning towards the camera's side"""
    rng = np.random.RandomState(2)
    img = np.zeros((4, 4, 4), np.uint8)
    img[..., 0] = rng.randint(128, 240, (4, 4))
    img[..., 1] = rng.randint(64, 193, (4, 4))
    img[..., 2] = rng.randint(200, 256, (4, 4))
    return img


def density():
    """a Gaussian puff of density 0.2 .. 1.8 on the grid's voxel centres, off centre"""
    nz, ny, nx = GRID_SHAPE
    z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    r2 = ((x - 0.55) / 0.35) ** 2 + ((y - 0.5) / 0.6) ** 2 + ((z - 0.45) / 0.4) ** 2
    return (0.2 + 1.6 * np.exp(-r2)).astype(np.float32)


def pane_alpha_map():
    img = np.zeros((MAP_H, 2, 4), np.uint8)
    img[..., :3] = 90
    img[:MAP_H // 2, :, 3], img[MAP_H // 2:, :, 3] = PANE_ALPHA
    return img


EMITTER = (-0.9, 0.3, -0.5, 0.2, 1.2)  # x0, x1, z0, z1, height: above the eye and the box, below the pane; only scene(emitter=...) places it


def scene(fog=True, pane=True, detail=True, transmit=True, path_length=2, use_mis=True, medium=None, emitter=0.0, hdr_map=None, pane_rect=None):
    """the floor of test_gpu_detail_maps._floor_scene (instance 0, material 0) and the pane above it; the features as scene fields, applied by
    Workload.upload.  The lights are the caller's (set_analytic_lights).  For the estimator pairs: `medium` in place of the absorbing MEDIUM,
    `emitter` > 0 the radiance of a mesh emitter at EMITTER, `hdr_map` a sampled environment, `pane_rect` in place of PANE."""
    img = normal_map()
    base = DM._floor_scene(normal_map=img, uv_repeat=UV_REPEAT)
    x0, x1, z0, z1, h = PANE if pane_rect is None else pane_rect
    sheet = scenegen.quad((x0, h, z0), (x1, h, z0), (x1, h, z1), (x0, h, z1))
    mats = [pod.make_material(pod.MAT_DIFFUSE, albedo=(RHO,) * 3), pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), opacity=PANE_OPACITY, diffuse_map=0)]
    meshes, placements = [base.meshes[0]], [(0, 0, workloads.IDENTITY)]
    if pane:
        meshes.append(sheet)
        placements.append((len(meshes) - 1, 1, workloads.IDENTITY))
    if emitter > 0.0:
        x0, x1, z0, z1, h = EMITTER
        meshes.append(scenegen.quad((x0, h, z0), (x1, h, z0), (x1, h, z1), (x0, h, z1)))
        placements.append((len(meshes) - 1, 2, workloads.IDENTITY))
        mats.append(pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), emissive=(1.0, 0.9, 0.8), intensity=emitter))
    mats = np.array(mats, dtype=pod.MAT_DT)
    sc = SH.BuiltScene(meshes, placements, materials=mats, camera=base.camera, diffuse_maps=[pane_alpha_map()], hdr_map=hdr_map,
                       settings=workloads.make_settings(use_mis=use_mis, path_length=path_length, background=(1, 1, 1), background_intensity=0.0))
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    sc.env_sampling = hdr_map is not None
    if detail:
        sc.normal_maps = [img]
        sc.material_detail = np.array([pod.make_material_detail(0, -1, 1.0)] + [pod.make_material_detail()] * (len(mats) - 1), dtype=pod.DETAIL_DT)
    sc.shadow_transmittance = pod.SHADOWS_TRANSMIT if transmit else pod.SHADOWS_OPAQUE
    if fog:
        sc.medium, sc.medium_density = (MEDIUM if medium is None else medium), density()
    return sc


def pane_surface(with_map=True):
    """the pane as the transmittance reference takes it: world-space triangles and texture coordinates of the quad the scene places"""
    x0, x1, z0, z1, h = PANE
    q = scenegen.quad((x0, h, z0), (x1, h, z0), (x1, h, z1), (x0, h, z1))
    pos = np.stack([q["pos%d" % k] for k in range(3)], 1)
    uvs = np.stack([q["texCoord%d" % k] for k in range(3)], 1)
    return TRN.Surface(pos, uvs, opacity=PANE_OPACITY, rgba8=pane_alpha_map() if with_map else None)


# ---- the factors -------------------------------------------------------------------------------------------------------------------------------

def closed_form_many(light, P, normals, rho):
    """analytic_light_reference.closed_form for points P (n, 3) with one normal each (n, 3), lights of radius 0: (n, 3); a light below the
    normal's horizon gives 0.  Also the spot falloff's argument before the clamp (1 for the other kinds)."""
    T = AR.table(light)
    assert float(T["radius"]) == 0.0 and float(T["q"]) == 0.0, "delta lights only: the closed forms hold for any normal"
    if T["kind"] == AR.DIRECTIONAL:
        cos_s = -(normals @ T["axis"])
        return rho / np.pi * np.maximum(cos_s, 0.0)[:, None] * T["power"][None, :], np.ones(len(P))
    to = T["centre"][None, :] - P
    d = np.sqrt((to * to).sum(1))
    cos_s = (to * normals).sum(1) / d
    x = -((to / d[:, None]) @ T["axis"]) * T["scale"] + T["offset"]
    return rho / np.pi * (np.clip(x, 0.0, 1.0) ** 2 * np.maximum(cos_s, 0.0) / (d * d))[:, None] * T["power"][None, :], x


def shadow_segment(light, P):
    """the shadow segment from the floor points P towards the light: unit directions (n, 3) and lengths (n,), inf for the sun"""
    T = AR.table(light)
    if T["kind"] == AR.DIRECTIONAL:
        return np.broadcast_to(-T["axis"], P.shape).copy(), np.full(len(P), np.inf)
    to = T["centre"][None, :] - P
    d = np.sqrt((to * to).sum(1))
    return to / d[:, None], d


PANELS = 24  # of 8 Gauss-Legendre nodes per segment in the box: tests/test_feature_product_reference.py measures what that leaves against 256


def grid_transmittance(o, d, t_end, panels=PANELS):
    """exp(-optical depth) of the segments (o, d, t_end) through the density grid; the quadrature runs over the segments that cross the box"""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    _, _, crosses = MR.segment(np.asarray(BOX_MIN, np.float32), np.asarray(BOX_MAX, np.float32), o, d, t_end)
    T = np.ones(len(o))
    if crosses.any():
        T[crosses] = np.exp(-G.optical_depth(density(), MEDIUM["boxMin"], MEDIUM["boxMax"], SIGMA_T, o[crosses], d[crosses], np.asarray(t_end, np.float64)[crosses], panels=panels))
    return T


@functools.lru_cache(maxsize=None)
def factors(sub):
    """every factor of the product at the sub x sub positions of every pixel, computed once: a dict of arrays with the leading shape
    (sub^2, pixels) —
      t_camera                       T_grid(eye -> x)
      fell_back                      the view is below the mapped horizon there (the shading normal went back to N)
    and per light name
      mapped, flat                   closed_form with ns / with N as the normal: (sub^2, pixels, 3)
      t_shadow                       T_grid(x -> l)
      t_pane, crossed, unclear       the pane's factor, its crossing count, and transmittance_reference's EDGE band (a crossing that may go
                                     either way in binary32), from the pane without its map so that the weight rule does not enter
      falloff                        the spot falloff's argument before the clamp"""
    sc = scene()
    img = normal_map()
    P = AL._floor_points(sc, N_UP, sub)
    S, n = len(P), P.shape[1]
    out = dict(t_camera=np.ones((S, n)), fell_back=np.zeros((S, n), bool), P=P)
    per = {name: dict(mapped=np.zeros((S, n, 3)), flat=np.zeros((S, n, 3)), t_shadow=np.ones((S, n)), t_pane=np.ones((S, n)), crossed=np.zeros((S, n), np.int64),
                      unclear=np.zeros((S, n), bool), falloff=np.ones((S, n))) for name in ALL}
    surface, bare = pane_surface(True), pane_surface(False)
    for k in range(S):
        p = P[k]
        ref = DM._reference(sc, p, img)
        out["fell_back"][k] = ref["fell_back"]
        to = p - EYE[None, :]
        dist = np.sqrt((to * to).sum(1))
        out["t_camera"][k] = grid_transmittance(np.broadcast_to(EYE, p.shape), to / dist[:, None], dist)
        for name in ALL:
            f = per[name]
            f["mapped"][k], f["falloff"][k] = closed_form_many(LIGHTS[name], p, ref["ns"], RHO)
            f["flat"][k] = closed_form_many(LIGHTS[name], p, np.broadcast_to(N_UP, p.shape), RHO)[0]
            d, length = shadow_segment(LIGHTS[name], p)
            f["t_shadow"][k] = grid_transmittance(p, d, length)
            tmax = np.where(np.isfinite(length), length, 1.0e3)  # (the pane is 2 above the floor: a sun ray meets it within 1 000 units or never)
            t = TRN.transmittance(p, d, tmax, [surface])
            f["t_pane"][k], f["crossed"][k] = t["T"], t["crossed"]
            f["unclear"][k] = TRN.transmittance(p, d, tmax, [bare])["unclear"]
    out.update(per)
    return out


def blocks(per_pixel):
    """means over the 16 x 16 pixel blocks: (16, channels)"""
    return AL._blocks(np.asarray(per_pixel, np.float64))


def expectation(sub=4, fog_camera=True, fog_shadow=True, pane=True, detail=True, lights=ALL):
    """block means (16, 3) of the product, with the factors the switches name and the lights of `lights`"""
    F = factors(sub)
    total = np.zeros(F["t_camera"].shape + (3,))
    for name in lights:
        f = F[name]
        term = f["mapped"] if detail else f["flat"]
        if fog_shadow:
            term = term * f["t_shadow"][..., None]
        if pane:
            term = term * f["t_pane"][..., None]
        total = total + term
    if fog_camera:
        total = total * F["t_camera"][..., None]
    return blocks(total.mean(0))


def unattenuated(sub=4):
    """the mapped floor under all the lights, no fog and no pane: what a block's product is held against"""
    return expectation(sub, fog_camera=False, fog_shadow=False, pane=False)


def _any_in_block(mask):
    """mask (sub^2, pixels) -> (16,): true in some position of some pixel of the block"""
    return blocks(mask.any(0)[:, None].astype(np.float64))[:, 0] > 0


DARK = 0.05


def left_out(sub=4):
    """{reason: (16,) bool}: the blocks that are not compared, each for a reason decided from the reference alone —
      pane edge   the shadow segments of one light do not all cross the pane alike: a pane edge's shadow runs through the block
                  (segments in transmittance_reference's EDGE band, 1e-5 wide, lie along the quad's diagonal too, where either answer is
                  the same crossing: they are counted by unclear_share and allowed for, not left out)
      alpha edge  the pane's factor varies among the crossing segments of one light: the two alpha blocks' seam (or the wrap at the map's
                  ends) falls in the block
      cone rim    the spot falloff's argument changes sign in the block
      horizon     a view falls below the mapped horizon (fell_back)
      dark        the product is below DARK of the unattenuated value"""
    F = factors(sub)
    edge, seam = np.zeros(BLOCKS, bool), np.zeros(BLOCKS, bool)
    jj, ii = np.mgrid[0:H, 0:W]
    ids = ((jj // 16) * (W // 16) + ii // 16).reshape(-1)
    for name in ALL:
        f = F[name]
        edge |= _any_in_block(f["crossed"] > 0) & _any_in_block(f["crossed"] == 0)
        through = f["crossed"] > 0
        for b in range(BLOCKS):
            t = f["t_pane"][:, ids == b][through[:, ids == b]]
            seam[b] |= t.size > 0 and t.max() - t.min() > 1e-9
    x = F["spot"]["falloff"]
    rim = _any_in_block(x < 0.0) & _any_in_block(x > 0.0)
    full, bare = expectation(sub), unattenuated(sub)
    return {"pane edge": edge, "alpha edge": seam & ~edge, "cone rim": rim, "horizon": _any_in_block(F["fell_back"]), "dark": np.any(full < DARK * bare, 1)}


def kept(sub=4):
    out = np.zeros(BLOCKS, bool)
    for mask in left_out(sub).values():
        out |= mask
    return ~out


def unclear_share(sub=4):
    """the largest share, over the blocks and the lights, of shadow segments in the EDGE band: a crossing counted or not changes that
    segment's term by at most its own size, so the share bounds the relative change of a block mean"""
    F = factors(sub)
    return max(float(blocks(F[name]["unclear"].mean(0)[:, None]).max()) for name in ALL)


# The sub-pixel quadrature's residue: the largest relative difference between sub = 4 and sub = 8 over the kept blocks, as
# tests/test_feature_product_reference.py measures it (and holds this constant to: not below the measurement, not above twice it).
QUADRATURE_TERM = 7.0e-5
# ... and a bound on unclear_share(4), asserted there too
UNCLEAR_TERM = 5.0e-4
# what the device comparison allows the expectation, relative: the two together
SYSTEMATIC = QUADRATURE_TERM + UNCLEAR_TERM


# ---- one integral, two estimators: the scene of the MIS / BSDF-sampling pair ---------------------------------------------------------------------

# Everything on, and a medium that SCATTERS; paths of three vertices.  The two estimators agree only where every light path one of them
# finds is within the other's reach, and a path's pass-through of the pane spends a bounce while a shadow ray's does not: a light sample at
# the last vertex that may take one (vertex 2 of 3) THROUGH the pane has no BSDF-sampled twin within three bounces.  So what BSDF sampling
# must find lies where no such twin is needed:
#   the mesh emitter  below the pane;
#   the point light   is sampled by the light sample alone under either setting (useMIS 0: the analytic-only light sample), through the
#                     pane (the TRANSMIT any-hit launch behind medium_shadow_grid) — the pane is just wide enough for its shadow segments;
#   the environment   radiates only in a band about the horizon, below PAIR_BAND_TOP; from every point of the fog box every point of the pane
#                     lies higher than that (pair_pane_elevation), so no light sample of a scattering vertex crosses the pane towards
#                     a lit direction.  That leaves vertex 2 on the FLOOR, far enough away to see the pane that low: pair_bound().
PAIR_PANE = (-1.7, 0.1, -0.3, 0.7, 2.0)
PAIR_FOG = pod.make_medium(box_min=BOX_MIN, box_max=BOX_MAX, sigma_t=1.5, g=0.5, albedo=(0.9, 0.9, 0.9))
PAIR_EMITTER = 4.0
PAIR_LIGHT = pod.make_analytic_light(pod.ALIGHT_POINT, position=(-0.5, 2.5, 0.4), colour=(1.0, 0.8, 0.6), intensity=4.0)
PAIR_ENV_ROWS, PAIR_ENV_LIT = 32, (14, 18)  # of 32 rows of 5.625 degrees the four about the horizon are lit
PAIR_ENV_MAX = 2.0
# the bilinear lookup blends row 14 into row 13 and is 0 from row 13's centre upwards: polar angle 13.5 / 32 x pi, elevation 14.06 degrees
PAIR_BAND_TOP = np.pi / 2.0 - (PAIR_ENV_LIT[0] - 0.5) / PAIR_ENV_ROWS * np.pi


def pair_environment():
    env = np.zeros((PAIR_ENV_ROWS, 2 * PAIR_ENV_ROWS, 3), np.float32)
    env[PAIR_ENV_LIT[0]:PAIR_ENV_LIT[1]] = np.random.default_rng(3).uniform(0.3, 1.0, (PAIR_ENV_LIT[1] - PAIR_ENV_LIT[0], 2 * PAIR_ENV_ROWS, 3))
    env[15, 40] = (PAIR_ENV_MAX, 1.9, 1.8)
    return env


def pair_scene(use_mis):
    return scene(path_length=3, use_mis=use_mis, medium=PAIR_FOG, emitter=PAIR_EMITTER, hdr_map=pair_environment(), pane_rect=PAIR_PANE)


def pair_pane_elevation(n=9):
    """the lowest elevation (radians) at which a point of the fog box sees a point of the pane: over a grid on the box and on the pane (the
    minimum lies on their boundaries, which the grids include)"""
    x0, x1, z0, z1, h = PAIR_PANE
    bx, by, bz = (np.linspace(BOX_MIN[k], BOX_MAX[k], n) for k in range(3))
    box = np.stack(np.meshgrid(bx, by, bz, indexing="ij"), -1).reshape(-1, 3)
    pane = np.stack(np.meshgrid(np.linspace(x0, x1, n), [h], np.linspace(z0, z1, n), indexing="ij"), -1).reshape(-1, 3)
    to = pane[None, :, :] - box[:, None, :]
    return float(np.arcsin(to[..., 1] / np.sqrt((to * to).sum(-1))).min())


def pair_bound():
    """What the light sample of a floor vertex 2 can collect through the pane from the lit band, at most — the radiance by which MIS may
    exceed BSDF sampling, by construction.  A pane element dA seen from the floor at elevation e is h / sin e away and subtends
    dA sin e / (h / sin e)^2 = dA sin^3 e / h^2; the floor's BSDF weighs it with cos / pi = sin e / pi; the band ends at e = PAIR_BAND_TOP:
        at most  albedo of the fog x rho x L_max x A sin^4(PAIR_BAND_TOP) / (pi h^2)
    (vertex 2 on the floor follows a scattering vertex 1; transmittances, the pane's factor and the MIS weight are at most 1)."""
    x0, x1, z0, z1, h = PAIR_PANE
    return float(PAIR_FOG["albedo"].max()) * RHO * PAIR_ENV_MAX * (x1 - x0) * (z1 - z0) * np.sin(PAIR_BAND_TOP) ** 4 / (np.pi * h * h)
