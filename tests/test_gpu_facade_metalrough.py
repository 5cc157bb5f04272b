"""The metallic-roughness option through the kept C++ API: nexus::Scene with SetMetalRoughMaterials(true) loads
tests/golden/metal_rough.glb and PathTracer::Render renders it; the RGBA8 image and the accumulation are those of the same tables — the
Python reader's, option on — uploaded through the C-ABI.  With the option off the file renders as it always did, and differently."""
import os

import numpy as np
import pytest

from nexus_amd import capi, loaders, pod
from tests import oracle_lib as O
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

W = H = 64
FRAMES = 3
EYE, FORWARD = (0.0, 1.6, 4.5), (0.0, -0.2425356, -0.9701425)
MODES = (pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
GLB = os.path.join(SH.GOLDEN, "metal_rough.glb")


def _capi_frames(gpu_ctx_factory, metal_rough):
    """SH.glb_scene with the reader's option, plus the file's detail table"""
    ls = loaders.load_glb(GLB, metal_rough=metal_rough)
    placements = [(inst["mesh"], inst["material"], capi.mat4_from_trs(inst["position"], inst["rotation"], inst["scale"])) for inst in ls.instances]
    cam = capi.camera_init(EYE, FORWARD, 40.0, W, H, 5.0, 0.0)
    settings = O.make_settings(use_mis=True, path_length=3, background=(1, 1, 1), background_intensity=0.0)
    scene = SH.BuiltScene(ls.meshes, placements, materials=ls.materials.copy(), camera=cam, settings=settings)
    scene.lights = SH.mesh_lights(scene.instances, scene.materials)
    ids, per_kind = [], {"normal": [], "roughness": []}
    for kind, px in ls.detail_textures:
        ids.append(len(per_kind[kind]))
        per_kind[kind].append(px)
    scene.normal_maps, scene.roughness_maps = per_kind["normal"], per_kind["roughness"]
    scene.material_detail = np.array([pod.make_material_detail(ids[n] if n >= 0 else -1, ids[r] if r >= 0 else -1, s) for n, r, s in
                                      zip(ls.material_normal_texture, ls.material_roughness_texture, ls.material_normal_scale)], dtype=pod.DETAIL_DT)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(*MODES)
    ctx.reset_frame_number()
    for _ in range(FRAMES):
        ctx.render_frame()
        ctx.accumulate()
    out = ctx.read_rgba8().copy(), ctx.read_accumulation().copy(), ctx.debug_pass_flavor(), settings, ctx.read_material_queue_sizes(pod.MAT_METALROUGH)
    ctx.close()
    return out


def _facade_frames(settings, metal_rough):
    sc = capi.Scene(W, H)
    if metal_rough is not None:
        sc.set_metal_rough(metal_rough)
    sc.load_file(SH.GOLDEN + os.sep, "metal_rough.glb")
    sc.set_camera(EYE, FORWARD, 40.0, 5.0, 0.0)
    sc.set_render_settings(settings)
    sc.update()
    pt = capi.PathTracer(W, H)
    pt.set_modes(*MODES)
    pt.update_device_scene(sc)
    for _ in range(FRAMES):
        pt.render(sc)
    out = pt.read_pixels().copy(), pt.read_accumulation().copy()
    pt.close()
    sc.close()
    return out


def test_a_glb_read_as_metallic_roughness_through_the_facade_equals_the_capi_path(gpu_ctx_factory):
    px, acc, flavor, settings, sizes = _capi_frames(gpu_ctx_factory, True)
    assert flavor & capi.FLAVOR_METAL and flavor & capi.FLAVOR_DETAIL and sizes[1] > 0
    assert acc.max() > 0.05 and (acc.max(1) > 0).mean() > 0.3, "the file's lamp lights the floor"
    off_px, off_acc, off_flavor, _, off_sizes = _capi_frames(gpu_ctx_factory, False)
    assert not off_flavor & capi.FLAVOR_METAL and np.all(off_sizes == 0)
    assert not np.array_equal(acc, off_acc), "gold is not yellow plastic"
    got_px, got_acc = _facade_frames(settings, True)
    assert np.array_equal(got_px, px) and np.array_equal(got_acc.view(np.uint32), acc.view(np.uint32))
    for option in (False, None):  # switched off, and never touched: the default
        got_px, got_acc = _facade_frames(settings, option)
        assert np.array_equal(got_px, off_px) and np.array_equal(got_acc.view(np.uint32), off_acc.view(np.uint32))
