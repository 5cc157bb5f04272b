"""Detail maps through the kept C++ API: nexus::Scene loads tests/golden/detail_maps.glb (normalTexture, metallicRoughnessTexture),
PathTracer::Render renders it; the RGBA8 image and the accumulation are those of the same maps set through the C-ABI
(nxhip_upload_texture kind 3 / 4, nxhip_set_material_detail).  AssetManager::ClearMaterialDetails — what nexus_render --no-detail-maps
calls — gives the frames of a context whose table was removed."""
import os

import numpy as np
import pytest

from nexus_amd import capi, loaders, pod
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

W = H = 64
FRAMES = 3
EYE, FORWARD = (0.0, 1.6, 4.5), (0.0, -0.2425356, -0.9701425)
MODES = (pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)


def _capi_frames(gpu_ctx_factory, glb, with_detail, removed=False):
    scene = SH.glb_scene(glb, W, H, path_length=3, eye=EYE, forward=FORWARD)
    ls = loaders.load_glb(glb)
    if with_detail:
        ids, per_kind = [], {"normal": [], "roughness": []}
        for kind, px in ls.detail_textures:  # ids are positions in the per-kind lists, as AssetManager::AddTexture hands them out
            ids.append(len(per_kind[kind]))
            per_kind[kind].append(px)
        scene.normal_maps, scene.roughness_maps = per_kind["normal"], per_kind["roughness"]
        scene.material_detail = np.array([pod.make_material_detail(ids[n] if n >= 0 else -1, ids[r] if r >= 0 else -1, s) for n, r, s in
                                          zip(ls.material_normal_texture, ls.material_roughness_texture, ls.material_normal_scale)], dtype=pod.DETAIL_DT)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    if removed:
        ctx.set_material_detail([])
    ctx.set_modes(*MODES)
    ctx.reset_frame_number()
    for _ in range(FRAMES):
        ctx.render_frame()
        ctx.accumulate()
    out = ctx.read_rgba8().copy(), ctx.read_accumulation().copy(), ctx.debug_pass_flavor(), scene.settings
    ctx.close()
    return out


def test_a_glb_with_detail_maps_through_the_facade_equals_the_capi_path(gpu_ctx_factory):
    glb = os.path.join(SH.GOLDEN, "detail_maps.glb")
    px, acc, flavor, settings = _capi_frames(gpu_ctx_factory, glb, True)
    assert flavor & capi.FLAVOR_DETAIL
    assert acc.max() > 0.05 and (acc.max(1) > 0).mean() > 0.3, "the file's lamp lights the floor"
    flat_px, flat_acc, flat_flavor, _ = _capi_frames(gpu_ctx_factory, glb, False)
    removed = _capi_frames(gpu_ctx_factory, glb, True, removed=True)
    assert not flat_flavor & capi.FLAVOR_DETAIL and not np.array_equal(acc, flat_acc), "the maps change the image"
    assert np.array_equal(removed[1].view(np.uint32), flat_acc.view(np.uint32)) and removed[2] == flat_flavor

    sc = capi.Scene(W, H)
    sc.load_file(SH.GOLDEN + os.sep, "detail_maps.glb")
    d = sc.material_details()
    assert d["normalMapId"].tolist() == [0, -1, -1, -1] and d["roughnessMapId"].tolist() == [0, 0, -1, -1]
    assert np.array_equal(d["normalScale"], np.float32([0.8, 1.0, 1.0, 1.0]))
    sc.set_camera(EYE, FORWARD, 40.0, 5.0, 0.0)
    sc.set_render_settings(settings)
    sc.update()
    pt = capi.PathTracer(W, H)
    pt.set_modes(*MODES)
    pt.update_device_scene(sc)
    for _ in range(FRAMES):
        pt.render(sc)
    assert pt.frame_number() == FRAMES
    assert np.array_equal(pt.read_pixels(), px)
    assert np.array_equal(pt.read_accumulation().view(np.uint32), acc.view(np.uint32))
    # --no-detail-maps: the table goes, the textures stay where they are; the frames are those of a context without a table
    sc.clear_material_details()
    assert len(sc.material_details()) == 0
    pt.update_device_scene(sc)
    pt.reset_frame_number()
    for _ in range(FRAMES):
        pt.render(sc)
    assert np.array_equal(pt.read_pixels(), flat_px)
    assert np.array_equal(pt.read_accumulation().view(np.uint32), flat_acc.view(np.uint32))
    # ... and a detail record set by hand brings the floor's maps back
    sc.set_material_detail(0, pod.make_material_detail(0, 0, 0.8))
    sc.set_material_detail(1, pod.make_material_detail(-1, 0, 1.0))
    pt.update_device_scene(sc)
    pt.reset_frame_number()
    for _ in range(FRAMES):
        pt.render(sc)
    assert np.array_equal(pt.read_accumulation().view(np.uint32), acc.view(np.uint32))
    pt.close()
    sc.close()
