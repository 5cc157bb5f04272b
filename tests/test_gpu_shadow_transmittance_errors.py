"""nxhip_set_shadow_transmittance / nxhip_trace_transmittance_batch: what they refuse, with a status and without a launch."""
import ctypes as C

import numpy as np
import pytest

from nexus_amd import capi, pod, workloads
from tests import scene_helpers as SH
from tests import test_transmittance_reference as TR

pytestmark = pytest.mark.gpu

INVALID, TIMEOUT = 1, 6


def _err():
    msg = capi.lib().nxhip_last_error()
    return msg.decode() if msg else ""


def _hook(ctx, rays, tmax, count, out):
    L = capi.lib()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return L.nxhip_trace_transmittance_batch(ctx.h, ptr(rays), ptr(tmax), count, ptr(out))


def test_an_unknown_mode_is_refused(gpu_ctx_factory):
    ctx = gpu_ctx_factory(TR.HOOK_W, TR.HOOK_H)
    for mode in (2, -1, 7):
        with pytest.raises(capi.NexusError, match="unknown mode"):
            ctx.set_shadow_transmittance(mode)
    ctx.set_shadow_transmittance(pod.SHADOWS_TRANSMIT)
    ctx.set_shadow_transmittance(pod.SHADOWS_OPAQUE)
    L = capi.lib()
    assert L.nxhip_set_shadow_transmittance(None, 1) == INVALID


def test_the_hook_refuses_what_it_cannot_follow(gpu_ctx_factory):
    rays, tmax = TR.hook_rays()
    rays, tmax = rays[:64].copy(), tmax[:64].copy()
    out = np.full(64, -1.0, np.float32)
    ctx = gpu_ctx_factory(TR.HOOK_W, TR.HOOK_H)
    # before a TLAS
    assert _hook(ctx, rays, tmax, 64, out) == INVALID and "TLAS" in _err()
    scene = TR.hook_scene()
    scene.upload(ctx)
    # null buffers (a count of 0 asks for nothing)
    for args in ((None, tmax, out), (rays, None, out), (rays, tmax, None)):
        assert _hook(ctx, *args[:2], 64, args[2]) == INVALID and "null buffer" in _err()
    assert _hook(ctx, None, None, 0, None) == 0
    # a material that names a diffuse map nobody uploaded: a status, not a launch
    ctx.clear_textures()
    assert _hook(ctx, rays, tmax, 64, out) == INVALID and "diffuse map" in _err()
    assert np.all(out == -1.0), "nothing was written"
    ctx.upload_texture("diffuse", scene.diffuse_maps[0])
    assert _hook(ctx, rays, tmax, 64, out) == 0 and np.all((out >= 0.0) & (out <= 1.0))
    # ... and without materials
    bare = gpu_ctx_factory(TR.HOOK_W, TR.HOOK_H)
    for nodes, tris, idx in scene.blas:
        bare.upload_blas(nodes, tris, idx)
    bare.set_tlas(scene.tlas_nodes, scene.tlas_idx, scene.instances)
    assert _hook(bare, rays, tmax, 64, out) == INVALID and "materials" in _err()


def test_both_calls_on_a_dead_context_answer_timeout():
    """(the expiry is a limit of 0 ms on a pass that takes milliseconds, as tests/test_gpu_api_errors.py stages it)"""
    Wd = Hd = 256
    scene = workloads.config2(Wd, Hd, 128, 64, 8, cls=SH.BuiltScene)
    ctx = capi.Context(Wd, Hd)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    ctx.set_frames_per_pass(64)
    ctx.render_frame()
    with pytest.raises(capi.NexusError, match="status 6"):
        ctx.sync_timeout(0)
    rays, tmax = TR.hook_rays()
    out = np.zeros(8, np.float32)
    assert _hook(ctx, rays[:8].copy(), tmax[:8].copy(), 8, out) == TIMEOUT
    with pytest.raises(capi.NexusError, match="status 6"):
        ctx.set_shadow_transmittance(pod.SHADOWS_TRANSMIT)
    ctx.close()
