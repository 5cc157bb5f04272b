"""Scenes of the light-sampling tests (tests/test_gpu_light_table.py, tests/test_gpu_light_sampling.py)."""
import numpy as np

from nexus_amd import capi, pod, scenegen, workloads
from tests import scene_helpers as SH

PANEL_BIG = capi.mat4_from_trs((1.0, 2.75, -0.5), (0, 0, 0), (3, 3, 3))
TORUS_AT = capi.mat4_from_trs((0.25, 0.75, 0.5), (30, 0, 20), (1, 1, 1))
TORUS_INSTANCE, PANEL_BIG_INSTANCE = 3, 2


def light_torus(seed=3, amp=0.06):
    return scenegen.displaced_torus(12, 8, seed=seed, major=0.4, minor=0.15, amp=amp)


def emitter_scene(W=64, H=48, path_length=4, objects=False):
    """a quad BLAS used by two emissive instances (one scaled x 3) with different materials, an emissive displaced torus, an emissive
    textured quad and a floor that emits nothing; objects: plus a diffuse and a plastic torus"""
    floor = scenegen.quad((-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4))
    panel = scenegen.quad((-0.25, 0, -0.25), (0.25, 0, -0.25), (0.25, 0, 0.25), (-0.25, 0, 0.25))
    screen = scenegen.quad((-1.5, 0.25, -2.5), (1.5, 0.25, -2.5), (1.5, 1.75, -2.5), (-1.5, 1.75, -2.5))
    meshes = [floor, panel, light_torus(), screen]
    mats = [
        pod.make_material(pod.MAT_DIFFUSE, albedo=(0.7, 0.7, 0.7)),
        pod.make_material(pod.MAT_DIFFUSE, albedo=(0.5, 0.5, 0.5), emissive=(1.0, 0.9, 0.8), intensity=20.0),
        pod.make_material(pod.MAT_DIFFUSE, albedo=(0.5, 0.5, 0.5), emissive=(0.2, 0.4, 1.0), intensity=1.5),
        pod.make_material(pod.MAT_DIFFUSE, albedo=(0.5, 0.5, 0.5), emissive=(1.0, 0.3, 0.1), intensity=4.0),
        pod.make_material(pod.MAT_DIFFUSE, albedo=(0.5, 0.5, 0.5), emissive=(1.0, 1.0, 1.0), intensity=2.0, emissive_map=0),
    ]
    placements = [
        (0, 0, workloads.IDENTITY),
        (1, 1, capi.mat4_from_trs((-1.25, 2.5, 0.25), (0, 0, 0), (1, 1, 1))),
        (1, 2, PANEL_BIG),
        (2, 3, TORUS_AT),
        (3, 4, workloads.IDENTITY),
    ]
    assert placements[TORUS_INSTANCE][0] == 2 and placements[PANEL_BIG_INSTANCE][2] is PANEL_BIG
    if objects:
        meshes += [scenegen.displaced_torus(24, 12, seed=5, major=0.5, minor=0.2)]
        mats += [pod.make_material(pod.MAT_DIFFUSE, albedo=(0.8, 0.5, 0.3)), pod.make_material(pod.MAT_PLASTIC, albedo=(0.3, 0.7, 0.4), roughness=0.3, ior=1.5)]
        placements += [(4, 5, capi.mat4_from_trs((-1.5, 0.5, 0.75), (0, 0, 0), (1, 1, 1))), (4, 6, capi.mat4_from_trs((1.5, 0.5, 1.0), (60, 20, 0), (1, 1, 1)))]
    cam = capi.camera_init((0.0, 1.5, 5.0), (0.0, -0.12, -0.99) / np.linalg.norm((0.0, -0.12, -0.99)), 55.0, W, H, 5.0, 0.0)
    sc = SH.BuiltScene(meshes, placements, materials=np.array(mats, dtype=pod.MAT_DT), camera=cam,
                       settings=workloads.make_settings(use_mis=True, path_length=path_length, background=(1, 1, 1), background_intensity=0.0),
                       emissive_maps=[workloads.checker_texture(32, 16, 6)])
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    assert [int(l) for l in sc.lights["meshId"]] == [1, 2, 3, 4]
    return sc


def one_light_scene(light_mesh, intensity=5.0):
    """`light_mesh` as the only light, over a floor (table tests: no camera needed beyond a valid one)"""
    floor = scenegen.quad((-4, -1, -4), (-4, -1, 4), (4, -1, 4), (4, -1, -4))
    mats = np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(0.7, 0.7, 0.7)),
                     pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), emissive=(1.0, 1.0, 1.0), intensity=intensity)], dtype=pod.MAT_DT)
    cam = capi.camera_init((0.0, 1.0, 5.0), (0.0, 0.0, -1.0), 50.0, 64, 48, 5.0, 0.0)
    sc = SH.BuiltScene([floor, light_mesh], [(0, 0, workloads.IDENTITY), (1, 1, workloads.IDENTITY)], materials=mats, camera=cam,
                       settings=workloads.make_settings(use_mis=True, path_length=3, background=(1, 1, 1), background_intensity=0.0))
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    return sc


def sliver_fan(x0, x1, z0, z1, y, slivers):
    """the rectangle [x0, x1] x [z0, z1] at height y as a fan around its corner (x0, z0): one large triangle (half of it) and `slivers`
    thin ones that share the other half — every triangle has the rectangle's normal (0, -1, 0) side facing down like the quad's"""
    c = np.array((x0, y, z0))
    far = np.array((x1, y, z1))
    tris = [(c, np.array((x1, y, z0)), far)]
    edge = np.linspace(0.0, 1.0, slivers + 1)
    for a, b in zip(edge[:-1], edge[1:]):  # along the side z = z1, from (x1, z1) back to (x0, z1)
        tris.append((c, far + a * (np.array((x0, y, z1)) - far), far + b * (np.array((x0, y, z1)) - far)))
    return pod.make_triangles(np.asarray(tris, np.float32))


def slivers_and_a_slab(n=4000):
    """one large triangle and n slivers of a ten-thousandth of its area each, axis-aligned and untransformed (their binary32 areas are
    exact products): long walks, and thousands of guide slots that land on the one large entry"""
    big = [((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0))]
    xs = 5.0 + np.arange(n) * (1.0 / 1024.0)
    thin = [((x, 0.0, 0.0), (x + 1.0 / 2048.0, 0.0, 0.0), (x, 0.0, 3.25)) for x in xs]
    order = np.random.RandomState(4).permutation(n + 1)
    return pod.make_triangles(np.asarray(big + thin, np.float32)[order])
