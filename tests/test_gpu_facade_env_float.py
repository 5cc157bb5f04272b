"""Scene::AddHDRMapFloat on the device: the Cornell box of tests/test_host_facade.py under a float sun map, rendered through
nexus::Scene / PathTracer (PathTracer::UpdateDeviceScene -> nxhip_upload_env_float, then nxhip_set_env_sampling on the path tracer's
context: the call sequence of examples/nexus_render --env-float --env-sampling), gives the bits of the bare C-ABI path
(Context.upload_env_float of the same array).  Both ways a map reaches the scene (the array, the .hdr file) and both ways it reaches
the device (with the textures, and alone under hdrDirty, replacing an 8-bit map)."""
import ctypes as C
import os

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import env_float_reference as F
from tests import scene_helpers as SH
from tests.test_host_facade import _cornell_facade

pytestmark = pytest.mark.gpu

W = H = 96
FRAMES = 3


def _sun():
    """the 32 x 16 sun map as a Radiance file holds it (RGBE and back), so that the array and the file are the same texels"""
    return F.rgbe_to_float(F.float_to_rgbe(F.sun_map()))


def _sampling_on(pt):
    L = capi.lib()
    capi.check(L.nxhip_set_env_sampling(C.c_void_p(L.nxs_pathtracer_device_context(pt.h)), 1), "nxhip_set_env_sampling")


def _stored(pt):
    """the float map the path tracer's context holds (nxhip_read_env_float on the handle itself: a capi.Context wrapped round it would
    destroy the path tracer's context when it is collected)"""
    L = capi.lib()
    h = C.c_void_p(L.nxs_pathtracer_device_context(pt.h))
    width, height = C.c_uint32(0), C.c_uint32(0)
    capi.check(L.nxhip_read_env_float(h, None, 0, C.byref(width), C.byref(height)), "nxhip_read_env_float")
    out = np.zeros((height.value, width.value, 3), np.float32)
    capi.check(L.nxhip_read_env_float(h, capi._ptr(out), width.value * height.value, C.byref(width), C.byref(height)), "nxhip_read_env_float")
    return out


def _frames(pt, sc):
    pt.reset_frame_number()
    for _ in range(FRAMES):
        pt.render(sc)
    assert pt.frame_number() == FRAMES
    return pt.read_pixels(), pt.read_accumulation()


@pytest.fixture(scope="module")
def direct(gpu_ctx_factory):
    scene = SH.cornell_scene(W, H, path_length=4)
    scene.hdr_map = _sun()
    scene.env_sampling = True
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.reset_frame_number()
    for _ in range(FRAMES):
        ctx.render_frame()
        ctx.accumulate()
    px, acc = ctx.read_rgba8(), ctx.read_accumulation()
    # the map lights the box: the same scene without it is another image
    ctx.clear_textures()
    ctx.reset_frame_number()
    for _ in range(FRAMES):
        ctx.render_frame()
        ctx.accumulate()
    assert not np.array_equal(px, ctx.read_rgba8())
    return px, acc


def test_a_float_map_through_the_facade_equals_the_capi_path(direct):
    img = _sun()
    assert img.dtype == np.float32 and img.max() > 3e4
    sc = _cornell_facade(W, H, 4, before_meshes=lambda s: s.set_hdr_map_float(img))
    pt = capi.PathTracer(W, H)
    try:
        pt.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
        pt.update_device_scene(sc)
        assert np.array_equal(_stored(pt).view(np.uint32), img.view(np.uint32))
        _sampling_on(pt)
        px, acc = _frames(pt, sc)
        assert np.array_equal(px, direct[0])
        assert np.array_equal(acc.view(np.uint32), direct[1].view(np.uint32))
    finally:
        pt.close()
        sc.close()


def test_a_float_file_replaces_an_eight_bit_map_on_the_device(direct, tmp_path):
    """... under hdrDirty alone (the textures are not dirty the second time), with the sampler already on: the new map gets new tables"""
    img = _sun()
    (tmp_path / "sun.hdr").write_bytes(F.write_hdr(F.float_to_rgbe(F.sun_map()), True))
    sc = _cornell_facade(W, H, 4, before_meshes=lambda s: s.set_hdr_map(SH.checker_texture(128, 64, 3)))
    pt = capi.PathTracer(W, H)
    try:
        pt.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
        pt.update_device_scene(sc)
        _sampling_on(pt)
        eight, _acc = _frames(pt, sc)
        assert not np.array_equal(eight, direct[0])
        with pytest.raises(capi.NexusError):
            _stored(pt)  # (an 8-bit map is no float map)
        sc.add_hdr_map_file_float(str(tmp_path) + os.sep, "sun.hdr")
        sc.update()
        pt.update_device_scene(sc)
        assert np.array_equal(_stored(pt).view(np.uint32), img.view(np.uint32))
        px, acc = _frames(pt, sc)
        assert np.array_equal(px, direct[0])
        assert np.array_equal(acc.view(np.uint32), direct[1].view(np.uint32))
    finally:
        pt.close()
        sc.close()
