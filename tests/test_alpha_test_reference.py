"""The float64 reference of the alpha-test rule (tests/alpha_test_reference.py) against closed forms, the hook tests' scene and ray sets
(shared with tests/test_gpu_alpha_test.py), the share of rays the reference leaves out on exactly those sets, and the bars a binary32
implementation is held to.  No GPU, no product kernel."""
import functools

import numpy as np

from nexus_amd import capi, pod, scenegen, workloads
from tests import alpha_test_reference as A
from tests import scene_helpers as SH

HOOK_RAYS = 4096
HOOK_W = HOOK_H = 64  # the context the scene is uploaded to


def block_map(alphas, size=128, seed=3):
    """size x size RGBA8, alpha constant on 2 x 2 blocks of size / 2 texels (alphas[row][column]); colours random: they must not matter.
    Large blocks keep the share of bilinear footprints that straddle a block edge, where a 1/256 weight may round either way, at 1/32."""
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, size=(size, size, 4)).astype(np.uint8)
    img[..., 3] = np.kron(np.asarray(alphas, np.uint8), np.ones((size // 2, size // 2), np.uint8))
    return img


def _sheet(y, half=2.0):
    return scenegen.quad((-half, y, -half), (half, y, -half), (half, y, half), (-half, y, half))


def _surface(y, **kw):
    q = _sheet(y)
    return A.Surface(np.stack([q["pos0"], q["pos1"], q["pos2"]], 1), np.stack([q["texCoord0"], q["texCoord1"], q["texCoord2"]], 1), **kw)


def _down_rays(n, seed, extent=1.9, top=3.0):
    rng = np.random.RandomState(seed)
    o = np.stack([rng.uniform(-extent, extent, n), np.full(n, top), rng.uniform(-extent, extent, n)], 1)
    return o, np.tile((0.0, -1.0, 0.0), (n, 1))


# ---- self-checks ----------------------------------------------------------------------------------------------------------------------------

ALPHAS = [[0, 255], [100, 180]]


def test_cutoff_zero_rejects_nothing_and_cutoff_one_everything_below_255():
    o, d = _down_rays(2000, 1)
    img = block_map(ALPHAS)
    wall = _surface(0.0)
    r = A.trace(o, d, np.inf, [_surface(1.0, rgba8=img, mode=A.MASK, cutoff=0.0), wall])
    assert np.all(r["inst"] == 0) and np.all(r["rejected"] == 0) and np.allclose(r["t"], 2.0) and np.all(r["occluded"]) and np.all(r["T"] == 0.0)
    below = block_map([[0, 254], [100, 180]])
    r = A.trace(o, d, np.inf, [_surface(1.0, rgba8=below, mode=A.MASK, cutoff=1.0), wall])
    assert np.all(r["inst"] == 1) and np.all(r["rejected"] == 1) and np.allclose(r["t"], 3.0)
    # ... and without the wall nothing is left: a miss, not occluded, T untouched
    r = A.trace(o, d, np.inf, [_surface(1.0, rgba8=below, mode=A.MASK, cutoff=1.0)])
    assert np.all(r["inst"] == -1) and np.all(np.isinf(r["t"])) and not r["occluded"].any() and np.all(r["T"] == 1.0)


def test_blocks_decide_by_their_alpha_and_the_three_modes_differ():
    o, d = _down_rays(4000, 2)
    img = block_map(ALPHAS)
    s, t = (o[:, 0] + 2.0) / 4.0, (o[:, 2] + 2.0) / 4.0
    inner = (np.abs((s * 128.0) % 64.0 - 32.0) < 31.0) & (np.abs((t * 128.0) % 64.0 - 32.0) < 31.0)
    alpha = np.asarray(ALPHAS)[(t * 2).astype(int), (s * 2).astype(int)] / 255.0
    wall = _surface(0.0)
    for opacity, cutoff in ((1.0, 0.5), (0.6, 0.25), (1.0, 0.25)):
        r = A.trace(o, d, np.inf, [_surface(1.0, opacity=opacity, rgba8=img, mode=A.MASK, cutoff=cutoff), wall])
        want = opacity * alpha >= cutoff
        assert np.array_equal(r["inst"][inner] == 0, want[inner]) and 0.2 < want[inner].mean() < 0.8
        assert np.all(r["T"][inner] == 0.0)  # (the wall is solid either way)
        assert not r["unclear"][inner].any()
    # OPAQUE ignores the map; BLEND keeps every crossing and multiplies 1 - o a into T
    r = A.trace(o, d, 2.5, [_surface(1.0, rgba8=img, mode=A.OPAQUE), wall])
    assert np.all(r["inst"] == 0) and np.all(r["T"] == 0.0)
    r = A.trace(o, d, 2.5, [_surface(1.0, opacity=0.6, rgba8=img, mode=A.BLEND), wall])  # (tmax ends the rays in front of the wall)
    assert np.all(r["inst"] == 0) and np.all(r["occluded"]) and np.allclose(r["T"][inner], 1.0 - 0.6 * alpha[inner], rtol=1e-13)
    # MASK: what survives is solid for T as well, what is rejected leaves it untouched
    r = A.trace(o, d, 2.5, [_surface(1.0, opacity=0.6, rgba8=img, mode=A.MASK, cutoff=0.25), wall])
    assert set(np.unique(r["T"][inner])) == {0.0, 1.0} and np.array_equal(r["T"][inner] == 0.0, (0.6 * alpha >= 0.25)[inner])


def test_a_case_at_the_cutoff_or_on_a_block_edge_is_left_out():
    o, d = _down_rays(4000, 3)
    r = A.trace(o, d, np.inf, [_surface(1.0, rgba8=block_map([[0, 255], [255, 255]]), mode=A.MASK, cutoff=1.0)])
    s, t = (o[:, 0] + 2.0) / 4.0, (o[:, 2] + 2.0) / 4.0
    full = (s > 0.55) & (s < 0.95) & (t > 0.05) & (t < 0.45)  # the block of alpha 255: s = cutoff exactly
    assert full.sum() > 100 and r["unclear"][full].all()
    o, d = _down_rays(40000, 4)
    r = A.trace(o, d, np.inf, [_surface(1.0, rgba8=block_map(ALPHAS), mode=A.MASK, cutoff=0.5)])
    s, t = (o[:, 0] + 2.0) / 4.0, (o[:, 2] + 2.0) / 4.0
    inner = (np.abs((s * 128.0) % 64.0 - 32.0) < 31.0) & (np.abs((t * 128.0) % 64.0 - 32.0) < 31.0)
    assert 0.0 < r["unclear"].mean() < 2e-3 and not r["unclear"][inner].any()  # (only where a footprint straddles two blocks)


# ---- the hook tests' scene and rays (CPU side; the GPU test uploads the same scene) ---------------------------------------------------------

def strip_mesh(quads=150, y=-0.1, half=2.0):
    """2 x quads triangles side by side along x: a BLAS deep enough that a ray which gets here descends and uses its stack"""
    x = np.linspace(-half, half, quads + 1)
    p = []
    for k in range(quads):
        a, b = (x[k], y, -half), (x[k + 1], y, -half)
        c, e = (x[k + 1], y, half), (x[k], y, half)
        p += [[a, b, c], [a, c, e]]
    return pod.make_triangles(np.asarray(p, np.float32))


# instance -> (mesh, material); materials -> (opacity, map, mode, cutoff)
TILTED = capi.mat4_from_trs((0.3, -0.6, -0.2), (8.0, 25.0, -6.0), (0.8, 1.0, 0.7))
MATERIALS = [dict(opacity=1.0, map=0, mode=A.MASK, cutoff=0.5),      # 0
             dict(opacity=0.6, map=0, mode=A.MASK, cutoff=0.25),     # 1
             dict(opacity=1.0, map=1, mode=A.MASK, cutoff=1.0),      # 2: every alpha of its map is below 255: all holes
             dict(opacity=0.5, map=-1, mode=A.BLEND, cutoff=0.5),    # 3: the strip
             dict(opacity=1.0, map=0, mode=A.OPAQUE, cutoff=0.5),    # 4
             dict(opacity=1.0, map=-1, mode=A.BLEND, cutoff=0.5)]    # 5: the back wall


@functools.lru_cache(maxsize=None)
def hook_scene():
    """Three parallel MASK quads (cutoffs 0.5, 0.25 with opacity 0.6, 1.0), the third one's mesh a second time in a rotated,
    non-uniformly scaled instance, a 300-triangle strip (BLEND, opacity 0.5) behind them, an OPAQUE quad under half of it and an opaque wall."""
    meshes = [_sheet(2.0), _sheet(1.5), _sheet(1.0), strip_mesh(),
              scenegen.quad((-0.5, -0.3, -2), (2, -0.3, -2), (2, -0.3, 2), (-0.5, -0.3, 2)),
              scenegen.quad((-3, -0.5, -3), (3, -0.5, -3), (3, -0.5, 3), (-3, -0.5, 3))]
    placements = [(0, 0, workloads.IDENTITY), (1, 1, workloads.IDENTITY), (2, 2, workloads.IDENTITY), (2, 0, TILTED),
                  (3, 3, workloads.IDENTITY), (4, 4, workloads.IDENTITY), (5, 5, workloads.IDENTITY)]
    mats = np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(0.5, 0.5, 0.5), opacity=m["opacity"], diffuse_map=m["map"]) for m in MATERIALS], dtype=pod.MAT_DT)
    cam = capi.camera_init((0.0, 5.0, 0.0), (0.0, -1.0, 0.0), 40.0, HOOK_W, HOOK_H, 5.0, 0.0)  # (the hooks ignore it; an upload wants one of the context's size)
    sc = SH.BuiltScene(meshes, placements, materials=mats, camera=cam, settings=workloads.make_settings(use_mis=True, path_length=2),
                       diffuse_maps=[block_map(ALPHAS), block_map([[0, 254], [100, 180]], seed=4)])
    sc.material_alpha = np.array([pod.make_material_alpha(m["mode"], m["cutoff"]) for m in MATERIALS], dtype=pod.ALPHA_DT)
    return sc


def surfaces_of(scene, modes=True):
    """the scene as the reference sees it: every instance's triangles in world space (float64 arithmetic on the uploaded binary32 numbers)"""
    out = []
    for inst in scene.instances:
        tris = scene.blas[int(inst["bvhIdx"])][1]
        M = inst["transform"].reshape(4, 4).astype(np.float64)
        pos = np.stack([tris[k].astype(np.float64) @ M[:3, :3].T + M[:3, 3] for k in ("pos0", "pos1", "pos2")], 1)
        uv = np.stack([tris[k].astype(np.float64) for k in ("texCoord0", "texCoord1", "texCoord2")], 1)
        mid = int(inst["materialId"])
        m = scene.materials[mid]
        rgba8 = scene.diffuse_maps[int(m["diffuseMapId"])] if int(m["diffuseMapId"]) != -1 else None
        al = scene.material_alpha[mid] if (modes and scene.material_alpha is not None) else None
        out.append(A.Surface(pos, uv, opacity=float(m["opacity"]), rgba8=rgba8, mode=int(al["mode"]) if al is not None else A.BLEND,
                             cutoff=float(al["cutoff"]) if al is not None else 0.5))
    return out


@functools.lru_cache(maxsize=None)
def hook_rays(seed=5):
    """origins above the stack, aimed at points of the scene's interior on the wall's level; a tenth of them point up; the shadow rays'
    tmax between 0.2 and 1.3 times the way to the target, so that some end between two sheets"""
    rng = np.random.RandomState(seed)
    n = HOOK_RAYS
    o = np.stack([rng.uniform(-1.8, 1.8, n), rng.uniform(2.3, 3.0, n), rng.uniform(-1.8, 1.8, n)], 1)
    target = np.stack([rng.uniform(-1.8, 1.8, n), np.full(n, -0.5), rng.uniform(-1.8, 1.8, n)], 1)
    d = target - o
    length = np.linalg.norm(d, axis=1)
    d /= length[:, None]
    d[::10] *= -1.0
    tmax = length * rng.uniform(0.2, 1.3, n)
    rays = np.zeros(n, pod.RAY_DT)
    rays["origin"], rays["direction"] = o.astype(np.float32), d.astype(np.float32)
    return rays, tmax.astype(np.float32)


@functools.lru_cache(maxsize=None)
def hook_reference(closest):
    """(r64, r32, keep) of the closest-hit set (no tmax) or of the shadow set (the rays' tmax)"""
    rays, tmax = hook_rays()
    r64, r32 = A.both(rays["origin"], rays["direction"], np.full(len(rays), np.inf, np.float32) if closest else tmax, surfaces_of(hook_scene()))
    return r64, r32, A.kept(r64, r32)


def record_bars(r64, r32, keep):
    """t, u, v: 4 x the worst deviation of the reference's own binary32 run from its float64 run on the same inputs (the project's convention)"""
    dev, same = A.record_deviation(r64, r32, keep)
    return {k: 4.0 * v for k, v in dev.items()}, same


def test_the_hook_rays_cover_the_cases_and_the_reference_leaves_out_little():
    for closest in (True, False):
        r64, r32, keep = hook_reference(closest)
        left = 1.0 - keep.mean()
        per_inst = np.bincount(r64["inst"][r64["inst"] >= 0], minlength=7)
        print("%s rays: left out %.3g (bar %.3g); closest instance counts %s, misses %d; rejected crossings per ray up to %d, rays with one %d" % (
            "closest-hit" if closest else "shadow", left, A.MAX_LEFT_OUT, per_inst.tolist(), (r64["inst"] < 0).sum(), r64["rejected"].max(), (r64["rejected"] > 0).sum()))
        assert left <= A.MAX_LEFT_OUT, "the reference alone must keep the left-out share within the bar"
        assert (r64["rejected"] > 0).sum() > 1000 and r64["rejected"].max() >= 3
        # the float32 run agrees with the float64 run on what it names, on the kept rays
        assert np.array_equal(r64["tri"][keep], r32["tri"][keep]) and np.array_equal(r64["inst"][keep], r32["inst"][keep])
        assert np.array_equal(r64["occluded"][keep], r32["occluded"][keep])
    r64, r32, keep = hook_reference(True)
    per_inst = np.bincount(r64["inst"][r64["inst"] >= 0], minlength=7)
    assert per_inst[2] == 0, "the cutoff-1 quad is all holes"
    assert all(per_inst[k] >= 50 for k in (0, 1, 3, 4)), "every other surface is some ray's closest crossing (the strip behind holes included)"
    assert (r64["inst"] < 0).sum() >= 300  # (the rays that point up)
    bars, same = record_bars(r64, r32, keep)
    print("bars (4 x binary32's own worst): t %.3g, u %.3g, v %.3g over %d rays" % (bars["t"], bars["u"], bars["v"], same.sum()))
    assert 0.0 < bars["t"] < 1e-4 and 0.0 < bars["u"] < 1e-4 and 0.0 < bars["v"] < 1e-4
    # the shadow set: MASK, BLEND and OPAQUE crossings all decide some ray's T; some rays end between two sheets
    r64, r32, keep = hook_reference(False)
    assert ((r64["T"] > 0) & (r64["T"] < 1)).sum() > 100 and (r64["T"] == 0).sum() > 500 and (r64["T"] == 1).sum() > 500
    far = hook_reference(True)[0]
    assert (far["crossings"] > r64["crossings"]).sum() > 500
    # without the table the same rays name the carrier quads: what a stub would return
    rays, _ = hook_rays()
    blend = A.trace(rays["origin"].astype(np.float64), rays["direction"].astype(np.float64), np.inf, surfaces_of(hook_scene(), modes=False))
    assert (blend["inst"][keep] != hook_reference(True)[0]["inst"][keep]).mean() > 0.3
