"""Analytic lights through the kept C++ API: nexus::Scene loads tests/golden/punctual_lights.glb (KHR_lights_punctual), PathTracer::Render
renders it; the RGBA8 image and the accumulation are those of the same records set through the C-ABI (nxhip_set_analytic_lights)."""
import os

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

W = H = 64
FRAMES = 3
EYE, FORWARD = (0.0, 1.6, 4.5), (0.0, -0.2425356, -0.9701425)


def test_a_glb_with_punctual_lights_through_the_facade_equals_the_capi_path(gpu_ctx_factory):
    glb = os.path.join(SH.GOLDEN, "punctual_lights.glb")
    scene = SH.glb_scene(glb, W, H, path_length=3, eye=EYE, forward=FORWARD)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_analytic_lights(capi.load_scene_analytic_lights(glb))
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.reset_frame_number()
    for _ in range(FRAMES):
        ctx.render_frame()
        ctx.accumulate()
    px, acc = ctx.read_rgba8(), ctx.read_accumulation()
    assert ctx.debug_pass_flavor() & capi.FLAVOR_ANALYTIC
    assert acc.max() > 0.05 and (acc.max(1) > 0).mean() > 0.3, "the file's lights light the floor (it holds no emitter)"

    sc = capi.Scene(W, H)
    sc.load_file(SH.GOLDEN + os.sep, "punctual_lights.glb")
    assert len(sc.analytic_lights()) == 4 and sc.light_count() == 0
    sc.set_camera(EYE, FORWARD, 40.0, 5.0, 0.0)
    sc.set_render_settings(scene.settings)
    sc.update()
    pt = capi.PathTracer(W, H)
    pt.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    pt.update_device_scene(sc)
    for _ in range(FRAMES):
        pt.render(sc)
    assert pt.frame_number() == FRAMES
    assert np.array_equal(pt.read_pixels(), px)
    assert np.array_equal(pt.read_accumulation().view(np.uint32), acc.view(np.uint32))
    # a light added by hand reaches the device with the next update, and removing every light returns to the image without any
    extra = sc.add_analytic_light(pod.make_analytic_light(pod.ALIGHT_POINT, position=(0.0, 1.0, 1.0), intensity=3.0))
    pt.update_device_scene(sc)
    pt.reset_frame_number()
    pt.render(sc)
    with_extra = pt.read_radiance().copy()
    for _ in range(extra + 1):
        sc.remove_analytic_light(0)
    pt.update_device_scene(sc)
    pt.reset_frame_number()
    pt.render(sc)
    assert not np.array_equal(with_extra, pt.read_radiance()) and pt.read_radiance().max() == 0.0
    pt.close()
    sc.close()
