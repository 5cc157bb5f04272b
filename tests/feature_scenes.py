"""The fixture scene with every shading feature at once, for the tests that compare ways of rendering bit for bit
(tests/test_gpu_feature_products.py, tests/test_gpu_adaptive.py): the box of tests/test_gpu_detail_maps.py — plastic, conductor and diffuse
surfaces with normal and roughness maps under a mesh emitter — with analytic lights, a see-through textured pane, a scattering fog grid
and a sampled float environment added.  Each feature has a switch: the scene a context would hold had it never been given the others."""
import numpy as np

from nexus_amd import capi, pod, scenegen, workloads
from tests import scene_helpers as SH
from tests import test_gpu_analytic_lights as AL
from tests import test_gpu_detail_maps as DM

FEATURES = ("analytic", "transmit", "detail", "medium", "grid", "power", "aov", "entry", "env")
ALL_ON = frozenset(FEATURES)

LIGHTS = AL.BOX_LIGHTS
FOG = pod.make_medium(box_min=(-0.9, 0.1, -0.9), box_max=(1.0, 1.7, 1.0), sigma_t=1.8, g=0.4, albedo=(0.9, 0.8, 0.7))
PANE = capi.mat4_from_trs((0.1, 1.9, 0.2), (8.0, 25.0, -5.0), (0.9, 1.0, 0.8))  # between the lamp (height 2.6) and the box (up to 1.2)


def fog_grid():
    """20 x 9 x 13 voxels (x, y, z) — no multiple of the 8-voxel brick —: a lumpy puff with an empty corner"""
    z, y, x = np.meshgrid(np.linspace(-1, 1, 13), np.linspace(-1, 1, 9), np.linspace(-1, 1, 20), indexing="ij")
    body = np.maximum(0.0, 1.0 - ((x - 0.1) ** 2 + (y + 0.1) ** 2 + z ** 2) / 1.3) ** 2
    return (1.7 * body * (1.0 + 0.3 * np.sin(5.0 * x + 1.0) * np.sin(4.0 * y) * np.sin(6.0 * z + 0.3))).astype(np.float32)


def environment():
    env = np.random.default_rng(5).uniform(0.05, 0.4, (16, 32, 3)).astype(np.float32)
    env[4, 9] = (9.0, 8.0, 6.5)
    return env


class FeatureScene(SH.BuiltScene):
    """a BuiltScene whose upload also applies what the scene fields do not carry: the analytic lights, the feature buffers, the entry points"""
    features = ALL_ON

    def upload(self, ctx, **kw):
        super().upload(ctx, **kw)
        ctx.set_analytic_lights(LIGHTS if "analytic" in self.features else np.zeros(0, pod.ALIGHT_DT))
        ctx.set_aov("aov" in self.features)
        ctx.set_entry_points("entry" in self.features)


def all_features_scene(width, height, features=ALL_ON, path_length=4):
    features = frozenset(features)
    assert features <= ALL_ON
    base = DM._box_scene()
    placements = [(int(i["bvhIdx"]), int(i["materialId"]), i["transform"].copy()) for i in base.instances]
    placements.append((len(base.meshes), len(base.materials), PANE))
    mats = np.append(base.materials, np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(0.8, 0.8, 0.8), opacity=0.6, diffuse_map=0)], dtype=pod.MAT_DT))
    cam = capi.camera_init((0.3, 1.4, 3.6), tuple(np.array([-0.05, -0.25, -1.0]) / np.linalg.norm([-0.05, -0.25, -1.0])), 45.0, width, height, 5.0, 0.0)
    sc = FeatureScene(list(base.meshes) + [scenegen.quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1))], placements, materials=mats, camera=cam,
                      settings=workloads.make_settings(use_mis=True, path_length=path_length), diffuse_maps=[SH.checker_texture(64, 32, 1, alpha=True)],
                      hdr_map=environment() if "env" in features else None)
    sc.features = features
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    sc.env_sampling = "env" in features
    # (the maps are uploaded whether or not the table names them: a context that turns the table on later finds them)
    sc.normal_maps, sc.roughness_maps = base.normal_maps, base.roughness_maps
    sc.detail_table = np.append(base.material_detail, np.array([pod.make_material_detail()], dtype=pod.DETAIL_DT))
    sc.material_detail = sc.detail_table if "detail" in features else None
    sc.light_sampling = pod.LIGHTS_POWER if "power" in features else pod.LIGHTS_UNIFORM
    sc.shadow_transmittance = pod.SHADOWS_TRANSMIT if "transmit" in features else pod.SHADOWS_OPAQUE
    sc.medium = FOG if "medium" in features else None
    sc.medium_density = fog_grid() if "grid" in features else None
    return sc
