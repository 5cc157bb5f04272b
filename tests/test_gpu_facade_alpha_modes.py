"""Scene::SetMaterialAlphaModes through the C view (nxs_scene_set_material_alpha_modes): tests/golden/alpha_cutout.glb read by the C++ loader
with the option on and rendered through the façade gives the RGBA8 image and the accumulation of the bare C-ABI path with the same
table (nxhip_set_material_alpha), and not those of the default, in which alpha blends."""
import os

import numpy as np
import pytest

from nexus_amd import capi, loaders, pod
from tests import oracle_lib as O
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

W = H = 64
FRAMES = 3
NAME = "alpha_cutout.glb"
EYE, FORWARD, HFOV = (0.0, 0.7, 3.6), (0.0, 0.1, -1.0), 50.0


def _direct(gpu_ctx_factory, alpha_modes):
    path = os.path.join(SH.GOLDEN, NAME)
    scene = SH.glb_scene(path, W, H, path_length=4, eye=EYE, forward=tuple(np.asarray(FORWARD) / np.linalg.norm(FORWARD)), hfov=HFOV)
    if alpha_modes:
        scene.material_alpha = loaders.load_glb(path, alpha_modes=True).material_alpha
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.reset_frame_number()
    for _ in range(FRAMES):
        ctx.render_frame()
        ctx.accumulate()
    out = ctx.read_rgba8(), ctx.read_accumulation(), ctx.debug_pass_flavor()
    ctx.close()
    return out


def _facade(alpha_modes):
    sc = capi.Scene(W, H)
    sc.set_material_alpha_modes(alpha_modes)
    sc.load_file(SH.GOLDEN + os.sep, NAME)
    sc.set_camera(EYE, tuple(np.asarray(FORWARD) / np.linalg.norm(FORWARD)), HFOV, 5.0, 0.0)
    sc.set_render_settings(O.make_settings(use_mis=True, path_length=4, background=(1, 1, 1), background_intensity=0.0))
    sc.update()
    pt = capi.PathTracer(W, H)
    pt.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    pt.update_device_scene(sc)
    for _ in range(FRAMES):
        pt.render(sc)
    out = pt.read_pixels(), pt.read_accumulation()
    pt.close()
    sc.close()
    return out


def test_set_material_alpha_modes_reaches_the_context(gpu_ctx_factory):
    px, acc, flavor = _direct(gpu_ctx_factory, True)
    assert flavor & capi.FLAVOR_ALPHA_TEST and flavor & capi.FLAVOR_SOLID
    got = _facade(True)
    assert np.array_equal(got[0], px)
    assert np.array_equal(got[1].view(np.uint32), acc.view(np.uint32))
    # off — the default — the façade renders the blend, which is another image
    px0, acc0, flavor0 = _direct(gpu_ctx_factory, False)
    assert not flavor0 & (capi.FLAVOR_ALPHA_TEST | capi.FLAVOR_SOLID) and not np.array_equal(acc0, acc)
    off = _facade(False)
    assert np.array_equal(off[1].view(np.uint32), acc0.view(np.uint32))
