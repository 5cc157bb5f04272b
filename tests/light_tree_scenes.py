"""Scenes of the light tree's tests (tests/test_gpu_light_tree.py, tests/test_gpu_light_importance.py)."""
import numpy as np

from nexus_amd import capi, pod, scenegen, workloads
from tests import scene_helpers as SH

GROUPS, QUADS_PER_GROUP = 5, 8
# five of a cube's corners, 40 apart: the groups differ in the top bit of some axis of the Morton code
GROUP_AT = np.array([(0.0, 3.0, 0.0), (40.0, 3.0, 0.0), (0.0, 43.0, 0.0), (0.0, 3.0, 40.0), (40.0, 43.0, 40.0)])


def _panel_group(seed=2):
    """eight small quads (side 0.2 .. 0.5) scattered within 1.5 of the origin, facing down"""
    rng = np.random.RandomState(seed)
    tris = []
    for _ in range(QUADS_PER_GROUP):
        c = rng.uniform(-1.5, 1.5, 3)
        s = rng.uniform(0.1, 0.25)
        tris.append(scenegen.quad(c + (-s, 0, -s), c + (s, 0, -s), c + (s, 0, s), c + (-s, 0, s)))
    return np.concatenate(tris)


def clustered_panels(W=64, H=48):
    """5 groups of 8 small emissive quads (16 triangles each; one mesh, five instances with different materials), the groups 40 apart,
    over a floor: 80 entries, G = 128"""
    floor = scenegen.quad((-10, 0, -10), (-10, 0, 50), (50, 0, 50), (50, 0, -10))
    mats = [pod.make_material(pod.MAT_DIFFUSE, albedo=(0.7, 0.7, 0.7))]
    mats += [pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), emissive=(1.0, 0.8, 0.6), intensity=2.0 + 3.0 * g) for g in range(GROUPS)]
    placements = [(0, 0, workloads.IDENTITY)] + [(1, 1 + g, capi.mat4_from_trs(tuple(GROUP_AT[g]), (0, 0, 0), (1, 1, 1))) for g in range(GROUPS)]
    cam = capi.camera_init((2.0, 1.5, 8.0), (0.0, 0.0, -1.0), 50.0, W, H, 5.0, 0.0)
    sc = SH.BuiltScene([floor, _panel_group()], placements, materials=np.array(mats, dtype=pod.MAT_DT), camera=cam,
                       settings=workloads.make_settings(use_mis=True, path_length=3, background=(1, 1, 1), background_intensity=0.0))
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    assert len(sc.lights) == GROUPS
    return sc


def tiny_light(n):
    """n = 1, 2 or 3 triangles of different sizes as one light"""
    tris = np.asarray([((-0.5, 2.0, -0.5), (0.5, 2.0, -0.5), (0.5, 2.0, 0.5)), ((1.0, 2.5, 0.0), (1.75, 2.5, 0.0), (1.0, 2.5, 0.4)), ((-2.0, 1.5, 1.0), (-1.7, 1.5, 1.0), (-2.0, 1.9, 1.3))],
                      np.float32)[:n]
    return pod.make_triangles(tris)


NEAR_X, FAR_X, PANEL_H, PATCH = -20.0, 20.0, 3.0, 3.0
NOISE_RADIANCE, NOISE_RHO = 10.0, 0.6


def two_far_panels(W, H, importance):
    """two equal 1 x 1 panels of equal radiance at height 3, at x = -20 and x = +20, over a diffuse floor; the camera, below the
    panels' height, looks down on the floor under the first panel and sees only floor within PATCH of that point; paths of two vertices"""
    floor = scenegen.quad((-80, 0, -80), (-80, 0, 80), (80, 0, 80), (80, 0, -80))
    panel = scenegen.quad((-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), (-0.5, 0, 0.5))
    mats = np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(NOISE_RHO,) * 3),
                     pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), emissive=(1.0, 1.0, 1.0), intensity=NOISE_RADIANCE)], dtype=pod.MAT_DT)
    eye = np.array((NEAR_X + 2.0, 2.0, 0.3))  # below the panels' height, looking down at 45 degrees: no ray can reach a panel first
    fwd = np.array((NEAR_X, 0.0, 0.0)) - eye
    cam = capi.camera_init(tuple(eye), fwd / np.linalg.norm(fwd), 30.0, W, H, 5.0, 0.0)
    sc = SH.BuiltScene([floor, panel], [(0, 0, workloads.IDENTITY), (1, 1, capi.mat4_from_trs((NEAR_X, PANEL_H, 0.0))), (1, 1, capi.mat4_from_trs((FAR_X, PANEL_H, 0.0)))],
                       materials=mats, camera=cam, settings=workloads.make_settings(use_mis=True, path_length=2, background=(1, 1, 1), background_intensity=0.0))
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    assert len(sc.lights) == 2
    sc.light_sampling = pod.LIGHTS_POWER
    sc.light_importance = importance
    return sc
