"""Fog through the kept C++ API: Scene::SetMedium over tests/golden/punctual_lights.glb rendered by PathTracer::Render gives the bits of the same
medium set through the C-ABI (nxhip_set_medium); ClearMedium gives the bits of a scene that never had one."""
import os

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

W = H = 64
FRAMES = 3
EYE, FORWARD = (0.0, 1.6, 4.5), (0.0, -0.2425356, -0.9701425)
FOG = pod.make_medium(box_min=(-3.0, 0.0, -3.0), box_max=(3.0, 3.0, 3.0), sigma_t=0.4, g=0.5, albedo=(0.9, 0.9, 0.9))


def _capi_route(gpu_ctx_factory, medium):
    glb = os.path.join(SH.GOLDEN, "punctual_lights.glb")
    scene = SH.glb_scene(glb, W, H, path_length=3, eye=EYE, forward=FORWARD)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_analytic_lights(capi.load_scene_analytic_lights(glb))
    ctx.set_medium(medium)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.reset_frame_number()
    for _ in range(FRAMES):
        ctx.render_frame()
        ctx.accumulate()
    out = ctx.read_rgba8(), ctx.read_accumulation(), bool(ctx.debug_pass_flavor() & capi.FLAVOR_MEDIUM), scene.settings
    ctx.close()
    return out


def test_set_medium_through_the_facade_equals_the_capi_path(gpu_ctx_factory):
    px_fog, acc_fog, on, settings = _capi_route(gpu_ctx_factory, FOG)
    px, acc, off, _ = _capi_route(gpu_ctx_factory, None)
    assert on and not off and not np.array_equal(acc_fog, acc), "the fog shows"

    sc = capi.Scene(W, H)
    sc.load_file(SH.GOLDEN + os.sep, "punctual_lights.glb")
    assert sc.medium() is None
    sc.set_medium(FOG)
    assert sc.medium().tobytes() == FOG.tobytes()
    sc.set_camera(EYE, FORWARD, 40.0, 5.0, 0.0)
    sc.set_render_settings(settings)
    sc.update()
    pt = capi.PathTracer(W, H)
    pt.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    pt.update_device_scene(sc)
    for _ in range(FRAMES):
        pt.render(sc)
    assert np.array_equal(pt.read_pixels(), px_fog)
    assert np.array_equal(pt.read_accumulation().view(np.uint32), acc_fog.view(np.uint32))
    # ClearMedium reaches the device with the next update: the bits of a scene that never had one
    sc.set_medium(None)
    assert sc.medium() is None
    pt.update_device_scene(sc)
    pt.reset_frame_number()
    for _ in range(FRAMES):
        pt.render(sc)
    assert np.array_equal(pt.read_pixels(), px)
    assert np.array_equal(pt.read_accumulation().view(np.uint32), acc.view(np.uint32))
    pt.close()
    sc.close()
