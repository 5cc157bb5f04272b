"""Algorithm-independent pins of the geometry: hit records, any-hit, the instance inverse, the first-hit features and the
environment lookup against float64 geometry (tests/geometry_reference.py), in the style of tests/test_physics_pins.py.

Every other geometric test compares the device with the oracle's tree walk, that walk with the oracle's brute force, and the
feature buffers with a restatement that takes u, v and triIdx from the oracle's hit record: an error common to both sides — u and v
attached to the wrong vertices, a normal carried by M instead of M^-T, the facing flip under a mirrored instance, a sign in a
cofactor of the inverse, the texture's v direction, the seam of the latitude/longitude map, the pixel -> ray mapping of a pixel
order — would pass them all.  Here each side is compared with geometry, not with the other side: the oracle on the CPU, the device
under -m gpu (wide kernel, thin kernel with mid-traversal hand-over, every device BLAS builder, device TLAS + device-side refit;
features with both pixel orders, entry points on and off).

Scene G (hit records): 8 instances of displaced_torus(24, 12), random_soup(300, size=0.15), height_field(8); two placement sets —
`ordinary` (scales 0.5-1.5) and `extreme` (every third instance scaled 1/20-20 per axis, every fourth mirrored); 4 000 rays, half
random_rays, half interior_rays.  Scene F (features): 48 x 32 pinhole camera, the torus mirrored and scaled (1, 2.5, 0.6), the
height field plain and mirrored, a 64 x 32 ramp texture (R along x, G along y), a plain material, a 64 x 32 8-bit ramp as
environment, pathLength 1; plus 200 directions at the seam of the map and 200 near its poles through the oracle's lookup.

Rays the float64 answer calls unclear (geometry_reference.MARGIN = 1e-3: runner-up that close to the winner, a plane crossed that
close to a triangle's edge, a crossing that close to tmax) are left out; their share of the hits is asserted to stay under 2 %.

Numbers.  MEASURED below is the ORACLE's worst deviation from the float64 reference on exactly these inputs (x86-64 CPU; the oracle
is not under test here, the device must equal it bit for bit elsewhere); each bound is 4 x that (a device build may differ from
the oracle on ties only, which the margins remove; the factor covers reseeding, not new error).

                               measured (oracle, CPU)     bound        unclear share of hits
  hitDistance, relative        ordinary 9.69e-6           3.88e-5      closest 0.98 %, any-hit 1.14 %
                               extreme  1.12e-5           4.48e-5      closest 0.93 %, any-hit 1.26 %
  u, v absolute                ordinary 1.74e-4           6.96e-4
                               extreme  9.06e-5           3.63e-4
  inverse, relative to |inv|   ordinary 1.38e-7           5.52e-7
                               extreme  1.64e-7           6.56e-7
  inverse x M - identity       ordinary 1.88e-7           7.52e-7
                               extreme  2.99e-6           1.20e-5
  normal (F), absolute         1.14e-5                    4.56e-5      frame 1: 0.73 %, frame 3: 0.65 %
  depth (F), relative          1.05e-6                    4.20e-6
  albedo (F), absolute         1.95e-3                    7.80e-3
  environment, image (F)       8.53e-5                    3.42e-4
  environment, seam and poles  1.94e-3                    7.76e-3

(The albedo and environment figures are the 8-bit fractional weights of the texture unit's bilinear filter, 1 / 512 of the step
between two texels, at the one place where the step is the whole ramp: the wrap-around column.)  Conditions that are not
measurements: the bounds of hitDistance, u / v and the normal stay under 1e-3, those of albedo and environment under half a step
of the ramp (2 / 255 in code, decoded where the decoding is steepest: 0.0177).  The environment of the image's missing pixels has
a bound of its own: they see a dark part of the ramp, where a shift of half a texel is smaller than the seam's bound.

Observed where: every figure above on the CPU (oracle walk and oracle brute force alike; host inverse through instance_init,
mat4_invert and the oracle's).  On an MI355X all 15 device cases gave the same figures to every printed digit — the records are
the oracle's bit for bit — including the device-side inverse after set_instance_transforms; the seam / pole directions go
through the device's own lookup too (nxhip_env_eval_batch).

The inputs were changed once, not a cap: hitDistance is compared relatively, but its error is absolute (about 1e-7 here: the
rounding of the origin's coordinates, eps x |origin| / |direction| in object space), so rays starting 1e-4 in front of the triangle
they hit gave 7.4e-4 (ordinary) and 5.7e-4 (extreme) relative and a hit at t = 0.06 under a 0.055 scale 1.7e-4.  3 000 rays of each
kind are drawn and the first 2 000 kept whose float64 answer is a miss or a hit at t >= T_MIN = 0.1 (docs/NOTEBOOK.md N18).

The checker is tested itself: the oracle's own records after a deliberate edit — u <-> v, triIdx + 1, hitDistance x (1 + 1e-3),
normals through M, the facing flip dropped under mirrored instances, texture v -> 1 - v, the environment's u shifted by half a
texel, one element of the inverse with the wrong sign — must each be refused.
"""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen
from tests import aov_reference as R
from tests import geometry_reference as G
from tests import oracle_lib as O
from tests import scene_helpers as SH

MEASURED = {
    "ordinary": dict(t=9.69e-6, uv=1.74e-4, inv=1.38e-7, prod=1.88e-7),
    "extreme": dict(t=1.12e-5, uv=9.06e-5, inv=1.64e-7, prod=2.99e-6),
    "features": dict(normal=1.14e-5, depth=1.05e-6, albedo=1.95e-3, env_image=8.53e-5, env=1.94e-3),
}
BOUND = {k: {q: 4.0 * x for q, x in v.items()} for k, v in MEASURED.items()}
MAX_UNCLEAR = 0.02
HALF_RAMP_STEP = float(G.srgb_decode(255) - G.srgb_decode(253))  # 2 / 255 in code where the decoding is steepest

N_INST = 8
T_MIN = 0.1
W, H = 48, 32
FRAMES = (1, 3)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- scene G ------------------------------------------------------------------------------------------------------------

def _meshes_g():
    return [scenegen.displaced_torus(24, 12), scenegen.random_soup(300, size=0.15), scenegen.height_field(8)]


def _transforms(kind):
    rng = np.random.RandomState(11 if kind == "ordinary" else 12)
    out = []
    for i in range(N_INST):
        scale = rng.uniform(0.5, 1.5, 3)
        if kind == "extreme":
            if i % 3 == 0:
                scale = np.exp(rng.uniform(np.log(1.0 / 20.0), np.log(20.0), 3))
            if i % 4 == 3:
                scale[rng.randint(3)] *= -1.0  # mirrored
        out.append(capi.mat4_from_trs(rng.uniform(-1.5, 1.5, 3), rng.uniform(0, 360, 3), scale))
    return np.array(out, dtype=np.float32)


def _scene_g(kind):
    def make():
        meshes = _meshes_g()
        xfs = _transforms(kind)
        scene = SH.BuiltScene(meshes, [(i % 3, 0, xfs[i]) for i in range(N_INST)])
        world = G.World(scene.meshes, [i % 3 for i in range(N_INST)], xfs)
        # hitDistance is compared RELATIVELY, and its absolute error does not shrink with it (it is the rounding of the origin's own
        # coordinates): a ray that starts within T_MIN of the surface it hits is an ill-conditioned input, not a probe of anything.
        # 3 000 rays of each kind are drawn and the first 2 000 kept whose float64 answer is a miss or a hit at T_MIN or beyond.
        drawn = [scenegen.random_rays(3000, seed=21, radius=6.0, target_extent=1.5), scenegen.interior_rays(3000, seed=22, extent=2.5)]
        rays = np.concatenate([r[np.flatnonzero(world.closest(r)["t"] >= T_MIN)[:2000]] for r in drawn])
        assert len(rays) == 4000
        ref = world.closest(rays)
        rng = np.random.RandomState(23)
        tmax = (np.where(ref["hit"], ref["t"], rng.uniform(1.0, 8.0, len(rays))) * rng.uniform(0.5, 1.5, len(rays))).astype(np.float32)
        occ, occ_unclear, _ = world.occluded(rays, tmax)
        return dict(kind=kind, scene=scene, xfs=xfs, world=world, rays=rays, ref=ref, tmax=tmax, occ=occ, occ_unclear=occ_unclear)

    return _cached(("G", kind), make)


# ---- the checks: records against the float64 reference ---------------------------------------------------------------------

def _check_hits(got, g, what):
    """hit/miss and ids equal on every clear ray, hitDistance relative, u against w1, v against w2"""
    ref, b = g["ref"], BOUND[g["kind"]]
    clear = ~ref["unclear"]
    n_hits = int(ref["hit"].sum())
    share = float(ref["unclear"].sum()) / n_hits
    got_hit = got["hitDistance"] < pod.MISS_DISTANCE
    sel = clear & ref["hit"] & got_hit
    et = float(np.max(np.abs(got["hitDistance"][sel].astype(np.float64) - ref["t"][sel]) / ref["t"][sel]))
    eu = float(np.max(np.abs(got["u"][sel].astype(np.float64) - ref["w"][sel, 1])))
    ev = float(np.max(np.abs(got["v"][sel].astype(np.float64) - ref["w"][sel, 2])))
    print("%s: %d rays, %d hits (%.3f), unclear %.4f of the hits; hit/miss differs on %d clear rays, ids on %d; hitDistance %.3g relative (bound %.3g), u %.3g, v %.3g (bound %.3g)" % (
        what, len(got), n_hits, ref["hit"].mean(), share, int((got_hit != ref["hit"])[clear].sum()),
        int(((got["instanceIdx"].astype(np.int64) != ref["inst"]) | (got["triIdx"].astype(np.int64) != ref["tri"]))[sel].sum()), et, b["t"], eu, ev, b["uv"]))
    assert share <= MAX_UNCLEAR
    assert ref["hit"].mean() >= 0.30
    assert np.array_equal(got_hit[clear], ref["hit"][clear])
    assert np.array_equal(got["instanceIdx"][sel].astype(np.int64), ref["inst"][sel])
    assert np.array_equal(got["triIdx"][sel].astype(np.int64), ref["tri"][sel])
    assert et <= b["t"]
    assert eu <= b["uv"] and ev <= b["uv"]
    return dict(t=et, uv=max(eu, ev), unclear=share)


def _check_shadow(got, g, what):
    clear = ~g["occ_unclear"]
    share = float(g["occ_unclear"].sum()) / int(g["ref"]["hit"].sum())
    wrong = int((np.asarray(got).astype(bool) != g["occ"])[clear].sum())
    print("%s: any-hit, %d of %d rays occluded, unclear %.4f of the hits, %d clear rays differ" % (what, int(g["occ"].sum()), len(g["occ"]), share, wrong))
    assert share <= MAX_UNCLEAR
    assert 0.1 < g["occ"].mean() < 0.9
    assert wrong == 0
    return dict(unclear=share)


def _check_inverse(inv32, m32, kind, what):
    """the inverse relative to the float64 inverse's largest element, and inverse x M against the identity"""
    M = np.asarray(m32, np.float64).reshape(-1, 4, 4)
    got = np.asarray(inv32, np.float64).reshape(-1, 4, 4)
    want = np.linalg.inv(M)
    rel = float(np.max(np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))))
    prod = float(np.max(np.abs(got @ M - np.eye(4))))
    b = BOUND[kind]
    print("%s: inverse of %d placements, %.3g relative (bound %.3g), inverse x M - 1 %.3g (bound %.3g)" % (what, len(M), rel, b["inv"], prod, b["prod"]))
    assert rel <= b["inv"]
    assert prod <= b["prod"]
    return dict(inv=rel, prod=prod)


# ---- scene F --------------------------------------------------------------------------------------------------------------

def _ramp(w, h, blue):
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 0] = np.round(np.arange(w) * 255.0 / (w - 1)).astype(np.uint8)[None, :]
    img[..., 1] = np.round(np.arange(h) * 255.0 / (h - 1)).astype(np.uint8)[:, None]
    img[..., 2] = blue
    img[..., 3] = 255
    return img


PLAIN = (0.25, 0.5, 0.75)


def _scene_f():
    def make():
        meshes = [scenegen.displaced_torus(24, 12), scenegen.height_field(8)]
        xfs = np.array([
            capi.mat4_from_trs((-1.3, 0.7, 0.0), (35, 20, 10), (-1.0, 1.0, 1.0)),        # torus, mirrored
            capi.mat4_from_trs((1.5, 0.2, -0.3), (60, -30, 15), (1.0, 2.5, 0.6)),        # torus, non-uniform scale
            capi.mat4_from_trs((0.0, -1.2, 0.5), (10, 25, -5), (2.0, 1.5, 1.6)),         # height field
            capi.mat4_from_trs((0.3, 1.4, -2.5), (80, 10, 20), (1.8, -1.0, 1.2)),        # height field, mirrored
        ], dtype=np.float32)
        mesh_of = [0, 0, 1, 1]
        material_of = [0, 1, 0, 1]
        mats = np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(0.7, 0.7, 0.7), diffuse_map=0), pod.make_material(pod.MAT_DIFFUSE, albedo=PLAIN)], dtype=pod.MAT_DT)
        cam = capi.camera_init((0.2, 0.9, 6.0), np.array((-0.03, -0.1, -1.0)) / np.linalg.norm((-0.03, -0.1, -1.0)), 50.0, W, H, 5.0, 0.0)
        sc = SH.BuiltScene(meshes, [(mesh_of[i], material_of[i], xfs[i]) for i in range(4)], materials=mats, camera=cam,
                           settings=O.make_settings(use_mis=False, path_length=1), diffuse_maps=[_ramp(64, 32, 40)], hdr_map=_ramp(64, 32, 128))
        world = G.World(sc.meshes, mesh_of, xfs)
        frames = {}
        for f in FRAMES:
            rays = R.primary_rays(cam, W, H, f)
            ref = world.closest(rays)
            tc = world.texcoord(ref)
            albedo = np.where((np.asarray(material_of)[np.where(ref["hit"], ref["inst"], 0)] == 0)[:, None], G.texture(sc.diffuse_maps[0], tc[:, 0], tc[:, 1]), np.asarray(PLAIN, np.float32).astype(np.float64))
            frames[f] = dict(rays=rays, ref=ref, albedo=albedo, normal=world.normal(ref, rays), env=G.texture(sc.hdr_map, *G.latlong(rays["direction"])))
        return dict(scene=sc, world=world, frames=frames, mirrored=np.linalg.det(xfs.reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)) < 0)

    return _cached("F", make)


def _check_features(albedo4, nd4, radiance, fr, what):
    """coverage, depth, normal, albedo of the clear pixels that hit; radiance of the clear pixels that miss = the environment"""
    ref, b = fr["ref"], BOUND["features"]
    clear = ~ref["unclear"]
    hit = ref["hit"]
    share = float(ref["unclear"].sum()) / int(hit.sum())
    covered = albedo4[:, 3] == 1.0
    sel = clear & hit & covered
    miss = clear & ~hit
    ez = float(np.max(np.abs(nd4[sel, 3].astype(np.float64) - ref["t"][sel]) / ref["t"][sel]))
    en = float(np.max(np.abs(nd4[sel, 0:3].astype(np.float64) - fr["normal"][sel])))
    ea = float(np.max(np.abs(albedo4[sel, 0:3].astype(np.float64) - fr["albedo"][sel])))
    ee = float(np.max(np.abs(np.asarray(radiance, np.float64).reshape(-1, 3)[miss] - fr["env"][miss])))
    print("%s: hit share %.3f, unclear %.4f of the hits, coverage differs on %d clear pixels; depth %.3g relative (bound %.3g), normal %.3g (%.3g), albedo %.3g (%.3g), environment %.3g (%.3g)" % (
        what, hit.mean(), share, int((covered != hit)[clear].sum()), ez, b["depth"], en, b["normal"], ea, b["albedo"], ee, b["env_image"]))
    assert share <= MAX_UNCLEAR
    assert 0.2 < hit.mean() < 0.8
    assert set(np.unique(albedo4[:, 3])) <= {0.0, 1.0}
    assert np.array_equal(covered[clear], hit[clear])
    assert np.all(nd4[clear & ~hit] == 0.0) and np.all(albedo4[clear & ~hit] == 0.0)
    assert ez <= b["depth"]
    assert en <= b["normal"]
    assert ea <= b["albedo"]
    assert ee <= b["env_image"]
    return dict(depth=ez, normal=en, albedo=ea, env=ee, unclear=share)


def _check_environment(rgb, directions, env_map, what):
    want = G.texture(env_map, *G.latlong(directions))
    err = float(np.max(np.abs(np.asarray(rgb, np.float64) - want)))
    print("%s: %d directions, environment %.3g (bound %.3g)" % (what, len(want), err, BOUND["features"]["env"]))
    assert err <= BOUND["features"]["env"]
    return dict(env=err)


def _aimed_directions():
    """200 directions at the seam of the map (d.x < 0, d.z = +-1e-4) and 200 near its two poles, unit length in float32"""
    rng = np.random.RandomState(31)
    elevation = rng.uniform(-1.4, 1.4, 200)
    seam = np.stack([-np.cos(elevation), np.sin(elevation), np.zeros(200)], axis=1)
    seam[:, 2] = np.where(np.arange(200) % 2 == 0, 1e-4, -1e-4)
    polar = rng.uniform(0.0, 0.02, 200)
    az = rng.uniform(-np.pi, np.pi, 200)
    poles = np.stack([np.sin(polar) * np.cos(az), np.cos(polar) * np.where(np.arange(200) % 2 == 0, 1.0, -1.0), np.sin(polar) * np.sin(az)], axis=1)
    d = np.concatenate([seam, poles])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    assert np.all(d[:200, 0] < 0) and np.all(np.abs(d[:200, 2]) < 2e-4) and np.all(np.abs(d[200:, 1]) > 0.999) and np.all(np.abs(d) <= 1.0)
    return d


def _oracle_features(sc, frame):
    """(albedo4, normalDepth4, radiance) of one frame on the CPU: the restated primary ray traced by the oracle, the shading normal in
    float32, the radiance of the oracle's wavefront (pathLength 1: the environment on a miss)"""
    albedo, depth, hits, rays = R.primary_features(sc, W, H, frame)
    n32, _flip = R.shading_normals(sc, hits, rays, np.float32)
    w = O.Wavefront(sc.oracle(), W * H, None, pod.RNG_PIXEL_KEYED, pod.CONDUCTOR_REFERENCE)
    w.render(frame)
    radiance = np.array(w.radiance(), np.float32).reshape(-1, 3)
    w.close()
    return albedo, np.concatenate([n32, depth[:, None]], axis=1).astype(np.float32), radiance, hits, rays


# ---- the oracle, on the CPU -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ordinary", "extreme"])
def test_oracle_hit_records(kind):
    g = _scene_g(kind)
    orc = g["scene"].oracle()
    _check_hits(orc.trace_closest(g["rays"]), g, "oracle walk, %s" % kind)
    _check_hits(orc.brute_closest(g["rays"]), g, "oracle brute force, %s" % kind)


@pytest.mark.parametrize("kind", ["ordinary", "extreme"])
def test_oracle_any_hit(kind):
    g = _scene_g(kind)
    orc = g["scene"].oracle()
    _check_shadow(orc.trace_any(g["rays"], g["tmax"]), g, "oracle walk, %s" % kind)
    _check_shadow(orc.brute_any(g["rays"], g["tmax"]), g, "oracle brute force, %s" % kind)


@pytest.mark.parametrize("kind", ["ordinary", "extreme"])
def test_host_inverse(kind):
    g = _scene_g(kind)
    _check_inverse(g["scene"].instances["invTransform"], g["xfs"], kind, "instance_init, %s" % kind)
    _check_inverse(np.array([capi.mat4_invert(m) for m in g["xfs"]]), g["xfs"], kind, "mat4_invert, %s" % kind)
    _check_inverse(np.array([O.mat4_invert(m) for m in g["xfs"]]), g["xfs"], kind, "oracle's inverse, %s" % kind)


@pytest.mark.parametrize("frame", FRAMES)
def test_oracle_features(frame):
    f = _scene_f()
    albedo, nd, radiance, _hits, _rays = _oracle_features(f["scene"], frame)
    _check_features(albedo, nd, radiance, f["frames"][frame], "oracle, frame %d" % frame)


def test_oracle_environment_at_the_seam_and_the_poles():
    f = _scene_f()
    d = _aimed_directions()
    _check_environment(f["scene"].oracle().sample_background(d), d, f["scene"].hdr_map, "oracle, seam and poles")


def test_bounds_meet_their_conditions():
    for kind in ("ordinary", "extreme"):
        assert BOUND[kind]["t"] <= 1e-3 and BOUND[kind]["uv"] <= 1e-3
    assert BOUND["features"]["normal"] <= 1e-3
    assert 0.017 < HALF_RAMP_STEP < 0.018
    assert BOUND["features"]["albedo"] < HALF_RAMP_STEP and BOUND["features"]["env"] < HALF_RAMP_STEP


# ---- the checker itself: the oracle's records after a deliberate edit must be refused ----------------------------------------------

def _refused(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


@pytest.mark.parametrize("kind", ["ordinary", "extreme"])
def test_checker_refuses_edited_hit_records(kind):
    g = _scene_g(kind)
    hits = g["scene"].oracle().trace_closest(g["rays"])
    _check_hits(hits, g, "unedited")
    hit = hits["hitDistance"] < pod.MISS_DISTANCE
    swapped = hits.copy()
    swapped["u"], swapped["v"] = hits["v"], hits["u"]
    _refused(_check_hits, swapped, g, "u <-> v")
    moved = hits.copy()
    moved["triIdx"] = np.where(hit, hits["triIdx"] + 1, hits["triIdx"])
    _refused(_check_hits, moved, g, "triIdx + 1")
    longer = hits.copy()
    longer["hitDistance"] = np.where(hit, hits["hitDistance"] * np.float32(1.0 + 1e-3), hits["hitDistance"])
    _refused(_check_hits, longer, g, "hitDistance x (1 + 1e-3)")
    # a single record is enough
    k = int(np.flatnonzero(hit & ~g["ref"]["unclear"])[7])
    one = hits.copy()
    one["u"][k], one["v"][k] = hits["v"][k], hits["u"][k]
    assert abs(float(hits["u"][k]) - float(hits["v"][k])) > 2 * BOUND[kind]["uv"]
    _refused(_check_hits, one, g, "u <-> v of one ray")
    occ = g["scene"].oracle().trace_any(g["rays"], g["tmax"])
    flipped = occ.copy()
    k = int(np.flatnonzero(~g["occ_unclear"])[5])
    flipped[k] ^= 1
    _refused(_check_shadow, flipped, g, "one shadow ray flipped")


@pytest.mark.parametrize("kind", ["ordinary", "extreme"])
def test_checker_refuses_a_wrong_cofactor_sign(kind):
    g = _scene_g(kind)
    inv = np.array(g["scene"].instances["invTransform"], np.float32).reshape(-1, 16).copy()
    for cell in (1, 6, 8, 3):  # (0,1), (1,2), (2,0) of the linear part, and one of the translation
        wrong = inv.copy()
        wrong[:, cell] = -wrong[:, cell]
        _refused(_check_inverse, wrong, g["xfs"], kind, "cell %d negated" % cell)
        one = inv.copy()
        one[2, cell] = -one[2, cell]
        _refused(_check_inverse, one, g["xfs"], kind, "cell %d of one placement negated" % cell)


def test_checker_refuses_edited_features():
    f = _scene_f()
    sc = f["scene"]
    frame = FRAMES[0]
    fr = f["frames"][frame]
    albedo, nd, radiance, hits, rays = _oracle_features(sc, frame)
    _check_features(albedo, nd, radiance, fr, "unedited")
    hit = hits["hitDistance"] < pod.MISS_DISTANCE
    # normals carried by M instead of M^-T: the restatement with transform^T in the place of the inverse
    through_m = SH.BuiltScene.__new__(SH.BuiltScene)
    through_m.__dict__.update(sc.__dict__)
    through_m.instances = sc.instances.copy()
    through_m.instances["invTransform"] = np.swapaxes(sc.instances["transform"].reshape(-1, 4, 4), 1, 2).reshape(sc.instances["invTransform"].shape)
    n_m, _ = R.shading_normals(through_m, hits, rays, np.float32)
    edited = nd.copy()
    edited[:, 0:3] = n_m
    _refused(_check_features, albedo, edited, radiance, fr, "normals through M")
    # the facing flip dropped under the mirrored instances
    _n, flip = R.shading_normals(sc, hits, rays, np.float32)
    under_mirror = hit & f["mirrored"][np.where(hit, hits["instanceIdx"], 0)] & flip
    assert under_mirror.sum() > 20
    edited = nd.copy()
    edited[under_mirror, 0:3] *= -1.0
    _refused(_check_features, albedo, edited, radiance, fr, "no facing flip under mirrored instances")
    # ... and the flip decided by the world-space winding, which a mirror reverses: every normal under a mirrored instance negated
    edited = nd.copy()
    edited[hit & f["mirrored"][np.where(hit, hits["instanceIdx"], 0)], 0:3] *= -1.0
    _refused(_check_features, albedo, edited, radiance, fr, "facing from the world-space winding")
    # texture v -> 1 - v: the same map upside down
    upside_down = SH.BuiltScene.__new__(SH.BuiltScene)
    upside_down.__dict__.update(sc.__dict__)
    upside_down.diffuse_maps = [np.ascontiguousarray(sc.diffuse_maps[0][::-1])]
    flipped_albedo = R.primary_features(upside_down, W, H, frame)[0]
    _refused(_check_features, flipped_albedo, nd, radiance, fr, "texture v -> 1 - v")
    # u <-> v reaches the texture coordinates and the normal
    swapped = hits.copy()
    swapped["u"], swapped["v"] = hits["v"], hits["u"]
    n_s, _ = R.shading_normals(sc, swapped, rays, np.float32)
    edited = nd.copy()
    edited[:, 0:3] = n_s
    _refused(_check_features, albedo, edited, radiance, fr, "normals from u <-> v")
    # depth and coverage
    edited = nd.copy()
    edited[:, 3] *= np.float32(1.0 + 1e-3)
    _refused(_check_features, albedo, edited, radiance, fr, "depth x (1 + 1e-3)")
    # the environment's u shifted by half a texel = the direction turned about y by half a texel's angle
    a = 2.0 * np.pi * 0.5 / sc.hdr_map.shape[1]
    d = np.asarray(rays["direction"], np.float64)
    turned = np.stack([np.cos(a) * d[:, 0] - np.sin(a) * d[:, 2], d[:, 1], np.sin(a) * d[:, 0] + np.cos(a) * d[:, 2]], axis=1).astype(np.float32)
    _refused(_check_features, albedo, nd, sc.oracle().sample_background(turned), fr, "environment u + half a texel")
    aimed = _aimed_directions()
    d = aimed.astype(np.float64)
    turned = np.stack([np.cos(a) * d[:, 0] - np.sin(a) * d[:, 2], d[:, 1], np.sin(a) * d[:, 0] + np.cos(a) * d[:, 2]], axis=1).astype(np.float32)
    _refused(_check_environment, sc.oracle().sample_background(turned), aimed, sc.hdr_map, "environment u + half a texel, seam and poles")
    # a row-major frame read as if it were in tile order (the pixel -> ray mapping of a pixel order)
    pm = capi.tile_pixel_map(W, H, 1, 0, 1, tiled=True)
    _refused(_check_features, albedo[pm], nd[pm], radiance[pm], fr, "pixels in another order")


# ---- the device ---------------------------------------------------------------------------------------------------------------

def _device_g(gpu_ctx_factory, variant, kind):
    """a context holding scene G's placement set `kind`, configured as `variant`"""
    g = _scene_g(kind)
    ctx = gpu_ctx_factory(64, 64)
    if variant.startswith("builder"):
        ctx.set_device_builder(int(variant[len("builder"):]))
        g["scene"].upload(ctx, device_bvh=True)
    else:
        g["scene"].upload(ctx)
    if variant == "thin":
        ctx.debug_set_thin(lanes=64, iters=5, in_hooks=True, any_time=True)
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ordinary", "extreme"])
@pytest.mark.parametrize("variant", ["wide", "thin", "builder0", "builder16", "builder-1"])
def test_gpu_hit_records_and_any_hit(gpu_ctx_factory, variant, kind):
    g = _scene_g(kind)
    ctx = _device_g(gpu_ctx_factory, variant, kind)
    _check_hits(ctx.trace_batch(g["rays"]), g, "device %s, %s" % (variant, kind))
    if variant == "thin":
        handed = ctx.debug_thin_counts()[0]
        print("handed to the thin kernel: %d closest-hit rays" % handed)
        assert handed > 500
    _check_shadow(ctx.trace_shadow_batch(g["rays"], g["tmax"]), g, "device %s, %s" % (variant, kind))
    if variant == "thin":
        assert ctx.debug_thin_counts()[1] > 100


@pytest.mark.gpu
def test_gpu_device_tlas_refit_and_device_side_inverse(gpu_ctx_factory):
    """rebuild_tlas from the ordinary placements, then set_instance_transforms to the extreme ones: the refit, the tight boxes and the
    inverse formed on the device"""
    before, g = _scene_g("ordinary"), _scene_g("extreme")
    ctx = gpu_ctx_factory(64, 64)
    before["scene"].upload(ctx)
    nodes, _idx = ctx.rebuild_tlas(before["scene"].instances)
    _check_hits(ctx.trace_batch(before["rays"]), before, "device TLAS, ordinary")
    ctx.set_instance_transforms(np.arange(N_INST, dtype=np.uint32), g["xfs"])
    _nodes, insts = ctx.read_tlas(len(nodes), N_INST)
    assert np.array_equal(insts["transform"].reshape(-1, 16).view(np.uint32), g["xfs"].view(np.uint32))
    _check_inverse(insts["invTransform"], g["xfs"], "extreme", "device-side inverse")
    _check_hits(ctx.trace_batch(g["rays"]), g, "device TLAS refitted to the extreme placements")
    _check_shadow(ctx.trace_shadow_batch(g["rays"], g["tmax"]), g, "device TLAS refitted to the extreme placements")
    # ... and back
    ctx.set_instance_transforms(np.arange(N_INST, dtype=np.uint32), before["xfs"])
    _check_inverse(ctx.read_tlas(len(nodes), N_INST)[1]["invTransform"], before["xfs"], "ordinary", "device-side inverse")
    _check_hits(ctx.trace_batch(before["rays"]), before, "device TLAS refitted back")


@pytest.mark.gpu
@pytest.mark.parametrize("entry", [False, True])
@pytest.mark.parametrize("order", [pod.ORDER_ROWS, pod.ORDER_TILES])
def test_gpu_features_and_environment(gpu_ctx_factory, order, entry):
    f = _scene_f()
    ctx = gpu_ctx_factory(W, H)
    f["scene"].upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.set_pixel_order(order)
    ctx.set_entry_points(entry)
    ctx.reset_frame_number()
    ctx.set_aov(True)
    pm = capi.tile_pixel_map(W, H, 1, 0, 1, tiled=True)
    for frame in range(1, max(FRAMES) + 1):
        ctx.render_frame()
        ctx.accumulate()
        if frame not in FRAMES:
            continue
        albedo, nd = ctx.read_aov_frame()
        radiance = ctx.read_radiance().reshape(-1, 3)
        if order == pod.ORDER_TILES:  # back to rows
            rows = [np.zeros_like(x) for x in (albedo, nd, radiance)]
            for dst, src in zip(rows, (albedo, nd, radiance)):
                dst[pm] = src
            albedo, nd, radiance = rows
        _check_features(albedo, nd, radiance, f["frames"][frame], "device, order %d, entry points %s, frame %d" % (order, entry, frame))


@pytest.mark.gpu
def test_gpu_environment_at_the_seam_and_the_poles(gpu_ctx_factory):
    """the device twin of test_oracle_environment_at_the_seam_and_the_poles: the product's own background lookup on lone directions"""
    f = _scene_f()
    ctx = gpu_ctx_factory(W, H)
    f["scene"].upload(ctx)
    d = _aimed_directions()
    rgb, _pdf, _texel = ctx.env_eval_batch(d, with_pdf=False)
    _check_environment(rgb, d, f["scene"].hdr_map, "device, seam and poles")
