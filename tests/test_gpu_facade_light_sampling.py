"""PathTracer::SetLightSampling through the C view (nxs_pathtracer_set_light_sampling): cornell_box_sphere.glb read by the C++ loader and
rendered in NXHIP_LIGHTS_POWER gives the RGBA8 image and the accumulation of the bare C-ABI path in the same mode."""
import ctypes as C
import os

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import oracle_lib as O
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

W = H = 96
FRAMES = 3


def _direct(gpu_ctx_factory, mode):
    scene = SH.glb_scene(os.path.join(SH.GOLDEN, "cornell_box_sphere.glb"), W, H, path_length=6)
    scene.light_sampling = mode
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.reset_frame_number()
    for _ in range(FRAMES):
        ctx.render_frame()
        ctx.accumulate()
    return ctx.read_rgba8(), ctx.read_accumulation()


def test_set_light_sampling_through_the_facade_equals_the_capi_path(gpu_ctx_factory):
    sc = capi.Scene(W, H)
    sc.load_file(SH.GOLDEN + os.sep, "cornell_box_sphere.glb")
    sc.set_camera((0.0, 1.0, 3.9), (0.0, 0.0, -1.0), 40.0, 5.0, 0.0)
    sc.set_render_settings(O.make_settings(use_mis=True, path_length=6))
    sc.update()
    pt = capi.PathTracer(W, H)
    pt.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    with pytest.raises(capi.NexusError, match="unknown mode"):
        pt.set_light_sampling(7)
    pt.set_light_sampling(pod.LIGHTS_POWER)
    pt.update_device_scene(sc)
    for _ in range(FRAMES):
        pt.render(sc)
    assert pt.frame_number() == FRAMES
    px, acc = _direct(gpu_ctx_factory, pod.LIGHTS_POWER)
    assert np.array_equal(pt.read_pixels(), px)
    assert np.array_equal(pt.read_accumulation().view(np.uint32), acc.view(np.uint32))
    # the façade's context is in the mode: it has a light table (the default mode refuses the hook), with the light's two triangles
    L = capi.lib()
    n = C.c_uint32(0)
    assert L.nxhip_read_light_table(L.nxs_pathtracer_device_context(pt.h), None, None, 0, None, C.byref(n)) == 0 and n.value == 2
    pt.set_light_sampling(pod.LIGHTS_UNIFORM)
    assert L.nxhip_read_light_table(L.nxs_pathtracer_device_context(pt.h), None, None, 0, None, C.byref(n)) != 0
    pt.close()
