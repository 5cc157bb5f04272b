"""Deforming meshes through the kept C++ host API: nexus::AssetManager::UpdateMeshTriangles + Scene::Update +
PathTracer::UpdateDeviceScene + Render give the image the bare C-ABI gives with nxhip_update_blas, in the three TLAS modes — the
host's rebuild (the reference's behaviour), the host refit (Scene::SetTlasRefit) and the device's tree (Scene::SetDeviceTlasBuild).
CPU part: the scene's bookkeeping."""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen
from tests import deform_meshes as D
from tests import oracle_lib as O
from tests import scene_helpers as SH

W = H = 64
M = 7
# (mesh, material, position, rotation in degrees, scale): the wavy grid as the light, face down, and once more as a surface;
# a floor, a wall and a torus
PLACEMENTS = [(0, 0, (0.0, 2.4, 0.0), (180, 0, 0), (0.7, 1.5, 0.7)), (1, 1, (0, 0, 0), (0, 0, 0), (1, 1, 1)), (2, 2, (0, 0, 0), (0, 0, 0), (1, 1, 1)),
              (3, 3, (0.2, 0.5, -0.2), (25, 30, 0), (1, 1, 1)), (0, 2, (-1.0, 0.3, 0.6), (10, 40, 5), (0.5, 1.0, 0.5))]
EYE, FORWARD, HFOV = (0.0, 1.2, 4.2), tuple(np.array((0.0, -0.05, -1.0)) / np.linalg.norm((0.0, -0.05, -1.0))), 45.0


def _meshes():
    return [D.base_grid(M), scenegen.quad((-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2)), scenegen.quad((-2, 0, -2), (2, 0, -2), (2, 3, -2), (-2, 3, -2)),
            scenegen.displaced_torus(24, 12, seed=3, major=0.45, minor=0.18)]


def _materials():
    return np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(0.8, 0.8, 0.8), emissive=(1.0, 0.95, 0.9), intensity=18.0),
                     pod.make_material(pod.MAT_DIFFUSE, albedo=(0.7, 0.7, 0.7)), pod.make_material(pod.MAT_DIFFUSE, albedo=(0.7, 0.3, 0.25)),
                     pod.make_material(pod.MAT_PLASTIC, albedo=(0.3, 0.5, 0.8), roughness=0.4, ior=1.5)], dtype=pod.MAT_DT)


def _facade(mode):
    sc = capi.Scene(W, H)
    if mode == "refit":
        sc.set_tlas_refit(True)
    if mode == "device":
        sc.set_device_tlas(True)
    mats = [sc.add_material(m) for m in _materials()]
    meshes = [sc.add_mesh(t) for t in _meshes()]
    for mesh, mat, pos, rot, scale in PLACEMENTS:
        sc.create_instance(meshes[mesh], mats[mat], pos, rot, scale)
    sc.set_camera(EYE, FORWARD, HFOV, 5.0, 0.0)
    sc.set_render_settings(O.make_settings(use_mis=True, path_length=4))
    sc.update()
    return sc


def test_a_deformed_mesh_invalidates_the_scene_until_the_update():
    sc = _facade("rebuild")
    assert sc.instance_count() == len(PLACEMENTS) and sc.light_count() == 1
    sc.update_mesh(0, D.deformed_grid(M))
    sc.update()
    assert sc.instance_count() == len(PLACEMENTS) and sc.light_count() == 1
    with pytest.raises(capi.NexusError):   # a refit keeps the topology
        sc.update_mesh(0, D.deformed_grid(M)[:-1])
    with pytest.raises(capi.NexusError):
        sc.update_mesh(9, D.deformed_grid(M))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["rebuild", "refit", "device"])
def test_facade_with_a_deformed_mesh_equals_the_capi_path(gpu_ctx_factory, mode):
    moved = D.deformed_grid(M)
    modes = (pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    # the facade: two frames, the mesh deforms, two more
    sc = _facade(mode)
    pt = capi.PathTracer(W, H)
    pt.set_modes(*modes)
    pt.update_device_scene(sc)
    for _ in range(2):
        pt.render(sc)
    base_px = pt.read_pixels().copy()
    sc.update_mesh(0, moved)
    sc.update()
    pt.update_device_scene(sc)
    for _ in range(2):
        pt.render(sc)
    assert pt.frame_number() == 4
    got_rad, got_px = pt.read_radiance().copy(), pt.read_pixels().copy()
    pt.close()
    sc.close()

    # the C-ABI with the same inputs
    scene = SH.BuiltScene(_meshes(), [(mesh, mat, capi.mat4_from_trs(pos, rot, scale)) for mesh, mat, pos, rot, scale in PLACEMENTS], materials=_materials(),
                          camera=capi.camera_init(EYE, FORWARD, HFOV, W, H, 5.0, 0.0), settings=O.make_settings(use_mis=True, path_length=4))
    scene.lights = SH.mesh_lights(scene.instances, scene.materials)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    if mode == "device":
        ctx.rebuild_tlas(scene.instances)
    ctx.set_modes(*modes)
    ctx.reset_frame_number()
    for _ in range(2):
        ctx.render_frame()
        ctx.accumulate()
    assert np.array_equal(base_px, ctx.read_rgba8())
    ctx.update_blas(0, moved)
    if mode == "rebuild":  # the reference's way with a changed instance: bounds from the new root, a new tree
        after = D.host_deformed(scene, {0: moved})
        nodes, idx = capi.tlas_build(after.instances)
        ctx.set_tlas(nodes, idx, after.instances)
    for _ in range(2):
        ctx.render_frame()
        ctx.accumulate()
    want_rad, want_px = ctx.read_radiance(), ctx.read_rgba8()
    assert SH.frames_identical(got_rad, want_rad, "facade against the C-ABI, %s" % mode)
    assert np.array_equal(got_px, want_px), "%d of %d pixels differ" % (int((got_px != want_px).sum()), got_px.size)
    assert not np.array_equal(got_px, base_px)
