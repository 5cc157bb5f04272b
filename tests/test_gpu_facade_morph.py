"""Morph targets through the kept C++ host API: Scene::SetMorphs + SetSkins + CreateMeshInstanceFromFile read tests/golden/morph_bar.glb,
Scene::MorphWeights and JointPalette evaluate a pose inside the weights animation, the PathTracer::PoseMesh overload that takes weights
has the device blend deltas and joints and refit, and the image and the triangles are those of the bare C-ABI (loaders.load_glb +
animation.morph_weights + Context.pose_blas_morph), bit for bit.  CPU part: the scene's bookkeeping."""
import os

import numpy as np
import pytest

from nexus_amd import animation, capi, loaders
from tests import deform_meshes as D
from tests import oracle_lib as O
from tests import scene_helpers as SH
from tests.test_gpu_facade_pose import BAR, EYE, FORWARD, H, HFOV, MODES, W, _device_context

FILE = "morph_bar.glb"
T = 0.3  # between the first two keys of the weights animation (2); the elbow bends by animation 0 at the same time


def _facade(mode, morphs=True):
    sc = capi.Scene(W, H)
    if mode == "refit":
        sc.set_tlas_refit(True)
    sc.set_skins(True)
    sc.set_morphs(morphs)
    sc.load_file(SH.GOLDEN + os.sep, FILE)
    sc.set_camera(EYE, FORWARD, HFOV, 5.0, 0.0)
    sc.set_render_settings(O.make_settings(use_mis=True, path_length=4))
    sc.update()
    return sc


def test_a_scene_keeps_its_morphs_only_when_asked():
    sc = _facade("rebuild")
    assert sc.instance_count() == 4 and sc.animation_count() == 3 and sc.mesh_target_count(BAR) == 3 and sc.mesh_joint_count(BAR) == 2
    assert np.array_equal(sc.morph_weights(BAR), [0.0, 0.25, 0.0])
    sc.close()
    sc = _facade("rebuild", morphs=False)
    assert sc.instance_count() == 4 and sc.animation_count() == 3 and sc.mesh_target_count(BAR) == 0 and sc.mesh_joint_count(BAR) == 2
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["rebuild", "refit"])
def test_facade_with_a_morphed_and_posed_mesh_equals_the_capi_path(gpu_ctx_factory, mode):
    # the facade: two frames, the bar morphs and bends, two more
    sc = _facade(mode)
    pt = capi.PathTracer(W, H)
    pt.set_modes(*MODES)
    pt.update_device_scene(sc)
    for _ in range(2):
        pt.render(sc)
    base_px = pt.read_pixels().copy()
    weights, palette = sc.morph_weights(BAR, 2, T), sc.joint_palette(BAR, 0, T)
    assert np.count_nonzero(weights) == 2
    pt.pose_mesh_morph(sc, BAR, weights, palette)
    sc.update()
    pt.update_device_scene(sc)
    for _ in range(2):
        pt.render(sc)
    assert pt.frame_number() == 4
    got_rad, got_px = pt.read_radiance().copy(), pt.read_pixels().copy()
    n = len(loaders.load_glb(os.path.join(SH.GOLDEN, FILE)).meshes[BAR])
    got_tris = _device_context(pt).read_blas_triangles(BAR, n)
    with pytest.raises(capi.NexusError):
        pt.pose_mesh_morph(sc, 1, weights)  # the floor has no targets
    with pytest.raises(capi.NexusError):
        pt.pose_mesh_morph(sc, BAR, weights[:2], palette)  # another target count
    with pytest.raises(capi.NexusError):
        pt.pose_mesh_morph(sc, BAR, weights)  # a skinned mesh needs its palette
    pt.close()
    sc.close()

    # the Python route with the same inputs
    path = os.path.join(SH.GOLDEN, FILE)
    ls = loaders.load_glb(path, skins=True, morphs=True)
    morph, skin = ls.morphs[0], ls.skins[0]
    assert morph["mesh"] == skin["mesh"] == BAR
    w, pal = animation.morph_weights(ls, morph, 2, T), animation.joint_palette(ls, skin, 0, T)
    assert w.tobytes() == weights.tobytes()
    scene = SH.glb_scene(path, W, H, path_length=4, eye=EYE, forward=FORWARD, hfov=HFOV)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(*MODES)
    ctx.reset_frame_number()
    for _ in range(2):
        ctx.render_frame()
        ctx.accumulate()
    assert np.array_equal(base_px, ctx.read_rgba8())
    ctx.set_blas_morph(BAR, morph["deltas"])
    ctx.set_blas_skin(BAR, skin["corners"], len(skin["joints"]))
    ctx.pose_blas_morph(BAR, w, palette)  # (the palette of the C++ evaluation: two binary64 evaluations may differ in the last place)
    assert np.max(np.abs(pal.astype(np.float64) - palette)) <= 2.0 ** -22
    want_tris = ctx.read_blas_triangles(BAR, n)
    assert got_tris.tobytes() == want_tris.tobytes()
    assert want_tris.tobytes() != scene.meshes[BAR].tobytes()
    if mode == "rebuild":  # the reference's way with a changed instance: bounds from the new root, a new tree
        after = D.host_deformed(scene, {BAR: want_tris})
        nodes, idx = capi.tlas_build(after.instances)
        ctx.set_tlas(nodes, idx, after.instances)
    for _ in range(2):
        ctx.render_frame()
        ctx.accumulate()
    want_rad, want_px = ctx.read_radiance(), ctx.read_rgba8()
    assert SH.frames_identical(got_rad, want_rad, "facade against the Python route, %s" % mode)
    assert np.array_equal(got_px, want_px), "%d of %d pixels differ" % (int((got_px != want_px).sum()), got_px.size)
    assert not np.array_equal(got_px, base_px), "the morphed bar renders like the bind pose"
