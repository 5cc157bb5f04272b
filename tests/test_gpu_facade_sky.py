"""Scene::SetSky on the device: the Cornell box of tests/test_host_facade.py under a generated sky, rendered through nexus::Scene /
PathTracer (PathTracer::UpdateDeviceScene -> nxhip_set_sky, then nxhip_set_env_sampling on the path tracer's context: the call sequence of
examples/nexus_render --sky --env-sampling), gives the bits of the bare C-ABI path (Context.set_sky of the same record).  Both ways the sky
reaches the device (with the textures, and alone under hdrDirty, replacing an 8-bit map), ClearSky, and the sun record of --sky-sun."""
import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import scene_helpers as SH
from tests.test_gpu_facade_env_float import _sampling_on, _stored
from tests.test_host_facade import _cornell_facade
from tests.test_sky import direction

pytestmark = pytest.mark.gpu

W = H = 64
FRAMES = 3
SKY = pod.Sky(sunDirection=direction(30.0, 25.0), width=64, height=32, sunDisc=1, sunAngularRadius=0.1, sunIrradiance=(20.0, 20.0, 20.0))
NO_DISC = pod.Sky(sunDirection=direction(30.0, 25.0), width=64, height=32, sunAngularRadius=0.02, sunIrradiance=(20.0, 20.0, 20.0))


def _direct(gpu_ctx_factory, sky, lights=()):
    scene = SH.cornell_scene(W, H, path_length=4)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_sky(sky)
    ctx.set_env_sampling(True)
    ctx.set_analytic_lights(list(lights))
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.reset_frame_number()
    for _ in range(FRAMES):
        ctx.render_frame()
        ctx.accumulate()
    return ctx.read_rgba8(), ctx.read_accumulation(), ctx.read_env_float()


def _frames(pt, sc):
    pt.reset_frame_number()
    for _ in range(FRAMES):
        pt.render(sc)
    assert pt.frame_number() == FRAMES
    return pt.read_pixels(), pt.read_accumulation()


def test_a_sky_through_the_facade_equals_the_capi_path(gpu_ctx_factory):
    px, acc, texels = _direct(gpu_ctx_factory, SKY)
    sc = _cornell_facade(W, H, 4, before_meshes=lambda s: s.set_sky(SKY))
    pt = capi.PathTracer(W, H)
    try:
        pt.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
        pt.update_device_scene(sc)
        assert np.array_equal(_stored(pt).view(np.uint32), texels.view(np.uint32))
        _sampling_on(pt)
        got_px, got_acc = _frames(pt, sc)
        assert np.array_equal(got_px, px) and np.array_equal(got_acc.view(np.uint32), acc.view(np.uint32))
        # ClearSky: no environment any more (the textures go up again without one)
        sc.set_sky(None)
        sc.update()
        pt.update_device_scene(sc)
        with pytest.raises(capi.NexusError):
            _stored(pt)
        dark, _acc = _frames(pt, sc)
        assert not np.array_equal(dark, px)
    finally:
        pt.close()
        sc.close()


def test_a_sky_replaces_an_eight_bit_map_on_the_device_and_is_replaced_by_one(gpu_ctx_factory):
    """... under hdrDirty alone (the textures are not dirty the second time), with the sampler already on: the new map gets new tables"""
    px, acc, texels = _direct(gpu_ctx_factory, SKY)
    sc = _cornell_facade(W, H, 4, before_meshes=lambda s: s.set_hdr_map(SH.checker_texture(128, 64, 3)))
    pt = capi.PathTracer(W, H)
    try:
        pt.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
        pt.update_device_scene(sc)
        _sampling_on(pt)
        eight, _acc = _frames(pt, sc)
        assert not np.array_equal(eight, px)
        sc.set_sky(SKY)
        sc.update()
        pt.update_device_scene(sc)
        assert np.array_equal(_stored(pt).view(np.uint32), texels.view(np.uint32))
        got_px, got_acc = _frames(pt, sc)
        assert np.array_equal(got_px, px) and np.array_equal(got_acc.view(np.uint32), acc.view(np.uint32))
        sc.set_hdr_map(SH.checker_texture(128, 64, 3))  # AddHDRMap replaces the sky
        sc.update()
        pt.update_device_scene(sc)
        with pytest.raises(capi.NexusError):
            _stored(pt)
        again, _acc = _frames(pt, sc)
        assert np.array_equal(again, eight)
    finally:
        pt.close()
        sc.close()


def test_the_sun_record_of_sky_sun_is_the_librarys(gpu_ctx_factory):
    """nexus_render --sky-sun: Scene::SetSky without a disc + Scene::AddAnalyticLight(nxhip_sky_sun_light's record) — the frames of
    Context.set_sky + Context.set_analytic_lights of that record, bit for bit; and the record is the sky's sun"""
    L = capi.lib()
    sun = capi.sky_sun_light(NO_DISC)
    raw = np.zeros(1, dtype=pod.ALIGHT_DT)
    capi.check(L.nxhip_sky_sun_light(capi._ptr(np.ascontiguousarray(NO_DISC).reshape(1)), capi._ptr(raw)), "nxhip_sky_sun_light")
    assert sun.tobytes() == raw[0].tobytes()
    assert sun["type"] == pod.ALIGHT_DIRECTIONAL and sun["angularRadius"] == np.float32(0.02) and np.all(sun["colour"] > 0) and np.all(sun["colour"] < 20.0)
    assert np.max(np.abs(sun["direction"].astype(np.float64) + direction(30.0, 25.0))) < 1e-7
    px, acc, _texels = _direct(gpu_ctx_factory, NO_DISC, lights=[sun])
    plain, _acc, _t = _direct(gpu_ctx_factory, NO_DISC)
    assert not np.array_equal(px, plain)  # the record lights the box
    sc = _cornell_facade(W, H, 4, before_meshes=lambda s: (s.set_sky(NO_DISC), s.add_analytic_light(sun)))
    pt = capi.PathTracer(W, H)
    try:
        pt.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
        pt.update_device_scene(sc)
        _sampling_on(pt)
        got_px, got_acc = _frames(pt, sc)
        assert np.array_equal(got_px, px) and np.array_equal(got_acc.view(np.uint32), acc.view(np.uint32))
    finally:
        pt.close()
        sc.close()
