"""Skinned meshes through the kept C++ host API: Scene::SetSkins + CreateMeshInstanceFromFile read tests/golden/skinned_bar.glb with its
skin, Scene::JointPalette evaluates a pose, PathTracer::PoseMesh has the device blend and refit, and Scene::Update +
PathTracer::UpdateDeviceScene + Render give the image the bare C-ABI gives (loaders.load_glb + animation.joint_palette +
nxhip_pose_blas), in the three TLAS modes — the host's rebuild, the host refit (Scene::SetTlasRefit) and the device's tree
(Scene::SetDeviceTlasBuild).  Then a pose that throws the bar 3.5 x its extent outward, out of every old box: no hit may be lost
against float64 geometry.  CPU part: the scene's bookkeeping."""
import ctypes as C
import os

import numpy as np
import pytest

from nexus_amd import animation, capi, loaders, pod
from tests import deform_meshes as D
from tests import geometry_reference as G
from tests import oracle_lib as O
from tests import scene_helpers as SH
from tests import skin_cases as K

W = H = 64
FILE = "skinned_bar.glb"
EYE, FORWARD, HFOV = (0.0, 1.2, 4.2), tuple(np.array((0.0, -0.05, -1.0)) / np.linalg.norm((0.0, -0.05, -1.0))), 45.0
MODES = (pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
BAR = 0  # the skinned mesh: the file's first primitive


def _facade(mode, skins=True):
    sc = capi.Scene(W, H)
    if mode == "refit":
        sc.set_tlas_refit(True)
    if mode == "device":
        sc.set_device_tlas(True)
    sc.set_skins(skins)
    sc.load_file(SH.GOLDEN + os.sep, FILE)
    sc.set_camera(EYE, FORWARD, HFOV, 5.0, 0.0)
    sc.set_render_settings(O.make_settings(use_mis=True, path_length=4))
    sc.update()
    return sc


def _device_context(pt):
    """the path tracer's own context, not owned (as Renderer.device_context wraps its one)"""
    ctx = capi.Context.__new__(capi.Context)
    ctx.L = capi.lib()
    ctx.h = C.c_void_p(ctx.L.nxs_pathtracer_device_context(pt.h))
    ctx.width, ctx.height, ctx.local_count, ctx.frames_per_pass = W, H, W * H, 1
    ctx.close = lambda: None
    return ctx


def test_a_scene_keeps_its_skins_only_when_asked():
    sc = _facade("rebuild")
    assert sc.instance_count() == 4 and sc.light_count() == 1 and sc.animation_count() == 2 and sc.mesh_joint_count(BAR) == 2
    assert sc.joint_palette(BAR, 0, 0.5).shape == (2, 12)
    sc.close()
    sc = _facade("rebuild", skins=False)
    assert sc.instance_count() == 4 and sc.animation_count() == 0 and sc.mesh_joint_count(BAR) == 0
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["rebuild", "refit", "device"])
def test_facade_with_a_posed_mesh_equals_the_capi_path(gpu_ctx_factory, mode):
    # the facade: two frames, the bar bends (animation 0 at t = 0.5), two more
    sc = _facade(mode)
    pt = capi.PathTracer(W, H)
    pt.set_modes(*MODES)
    pt.update_device_scene(sc)
    for _ in range(2):
        pt.render(sc)
    base_px = pt.read_pixels().copy()
    pt.pose_mesh(sc, BAR, sc.joint_palette(BAR, 0, 0.5))
    sc.update()
    pt.update_device_scene(sc)
    for _ in range(2):
        pt.render(sc)
    assert pt.frame_number() == 4
    got_rad, got_px = pt.read_radiance().copy(), pt.read_pixels().copy()
    with pytest.raises(capi.NexusError):
        pt.pose_mesh(sc, 1, sc.joint_palette(BAR, 0, 0.5))  # the floor has no skin
    with pytest.raises(capi.NexusError):
        pt.pose_mesh(sc, BAR, np.zeros((3, 12), np.float32))  # another joint count
    pt.close()
    sc.close()

    # the C-ABI with the same inputs
    path = os.path.join(SH.GOLDEN, FILE)
    ls = loaders.load_glb(path, skins=True)
    skin = ls.skins[0]
    assert skin["mesh"] == BAR
    scene = SH.glb_scene(path, W, H, path_length=4, eye=EYE, forward=FORWARD, hfov=HFOV)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    if mode == "device":
        ctx.rebuild_tlas(scene.instances)
    ctx.set_modes(*MODES)
    ctx.reset_frame_number()
    for _ in range(2):
        ctx.render_frame()
        ctx.accumulate()
    assert np.array_equal(base_px, ctx.read_rgba8())
    ctx.set_blas_skin(BAR, skin["corners"], len(skin["joints"]))
    ctx.pose_blas(BAR, animation.joint_palette(ls, skin, 0, 0.5))
    if mode == "rebuild":  # the reference's way with a changed instance: bounds from the new root, a new tree
        after = D.host_deformed(scene, {BAR: ctx.read_blas_triangles(BAR, len(scene.meshes[BAR]))})
        nodes, idx = capi.tlas_build(after.instances)
        ctx.set_tlas(nodes, idx, after.instances)
    for _ in range(2):
        ctx.render_frame()
        ctx.accumulate()
    want_rad, want_px = ctx.read_radiance(), ctx.read_rgba8()
    assert SH.frames_identical(got_rad, want_rad, "facade against the C-ABI, %s" % mode)
    assert np.array_equal(got_px, want_px), "%d of %d pixels differ" % (int((got_px != want_px).sum()), got_px.size)
    assert not np.array_equal(got_px, base_px), "the bent bar renders like the straight one"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["rebuild", "refit", "device"])
def test_a_pose_that_leaves_every_old_box_loses_no_hits(mode):
    from tests.test_gpu_blas_refit import _check_against_geometry, _conditioned

    path = os.path.join(SH.GOLDEN, FILE)
    scene = SH.glb_scene(path, W, H, path_length=4, eye=EYE, forward=FORWARD, hfov=HFOV)  # (the meshes and where the file places them)
    bar = scene.meshes[BAR]
    outward = K.palette("outward", 2, K.corner_positions(bar).max() - K.corner_positions(bar).min(), 4)
    sc = _facade(mode)
    pt = capi.PathTracer(W, H)
    pt.set_modes(*MODES)
    pt.update_device_scene(sc)
    pt.render(sc)
    pt.pose_mesh(sc, BAR, outward)
    sc.update()
    pt.update_device_scene(sc)
    ctx = _device_context(pt)
    posed = ctx.read_blas_triangles(BAR, len(bar))
    p = K.corner_positions(posed)
    assert p[:, 1].min() > K.corner_positions(bar)[:, 1].max() + 1.0, "the pose stays near the bind pose: the test shows nothing"
    xfs = np.array([np.asarray(i["transform"], np.float32).reshape(16) for i in scene.instances])
    world = G.World([posed] + scene.meshes[1:], [int(i["bvhIdx"]) for i in scene.instances], xfs)
    # rays into the room, and rays aimed at where the bar now is
    centre = (p.astype(np.float64).mean(0) * 1.25 + np.array([0.5, 0.25, -0.75]))
    aimed = D.rays_for(1500, 43, extent=0.5)
    aimed["origin"] += centre.astype(np.float32)
    rays, ref = _conditioned(world, np.concatenate([D.rays_for(1500, 41, extent=2.0), aimed]), 2000)
    got = ctx.trace_batch(rays)
    on_bar = ref["hit"] & (ref["inst"] == 0)
    assert on_bar.sum() > 100, "hardly a ray reaches the posed bar"
    _check_against_geometry(got, ref, "facade, %s TLAS, after a 3.5 x outward pose" % mode)
    pt.close()
    sc.close()
