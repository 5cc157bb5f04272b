"""nxhip_set_material_alpha: what it, the render and the ray-batch hooks refuse, with a status and without a launch."""
import ctypes as C

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import scene_helpers as SH
from tests import test_alpha_test_reference as AT

pytestmark = pytest.mark.gpu

INVALID = 1


def _err():
    msg = capi.lib().nxhip_last_error()
    return msg.decode() if msg else ""


def _table(*entries):
    return np.array([pod.make_material_alpha(m, c) for m, c in entries], dtype=pod.ALPHA_DT)


def test_bad_tables_are_refused_and_the_previous_one_stays(gpu_ctx_factory):
    scene = AT.hook_scene()
    ctx = gpu_ctx_factory(AT.HOOK_W, AT.HOOK_H)
    scene.upload(ctx)
    rays, _ = AT.hook_rays()
    before = ctx.trace_batch(rays[:512])
    n = len(scene.materials)
    for mode in (3, 7, 0xFFFFFFFF):
        with pytest.raises(capi.NexusError, match="unknown mode"):
            ctx.set_material_alpha(_table(*([(mode, 0.5)] + [(pod.ALPHA_BLEND, 0.5)] * (n - 1))))
    for cutoff in (float("nan"), float("inf"), -0.01, 1.01):
        with pytest.raises(capi.NexusError, match="cutoff"):
            ctx.set_material_alpha(_table(*([(pod.ALPHA_MASK, cutoff)] + [(pod.ALPHA_BLEND, 0.5)] * (n - 1))))
    # (only a MASK entry's cutoff is looked at)
    ctx.set_material_alpha(_table(*([(pod.ALPHA_BLEND, float("nan")), (pod.ALPHA_OPAQUE, 7.0)] + [(pod.ALPHA_BLEND, 0.5)] * (n - 2))))
    ctx.set_material_alpha(scene.material_alpha)
    with pytest.raises(capi.NexusError, match="cutoff"):
        ctx.set_material_alpha(_table(*([(pod.ALPHA_MASK, 2.0)] * n)))
    assert SH.hit_records_equal(before, ctx.trace_batch(rays[:512])), "a refused table changes nothing"
    # a null array with a count, and a null context
    L = capi.lib()
    assert L.nxhip_set_material_alpha(ctx.h, None, 3) == INVALID and "null array" in _err()
    assert L.nxhip_set_material_alpha(None, None, 0) == INVALID
    assert L.nxhip_set_material_alpha(ctx.h, None, 0) == 0  # (clears)
    ctx.close()


def test_a_count_that_is_not_the_material_count_is_refused_at_render_time(gpu_ctx_factory):
    scene = AT.hook_scene()
    ctx = gpu_ctx_factory(AT.HOOK_W, AT.HOOK_H)
    scene.upload(ctx)
    ctx.set_material_alpha(scene.material_alpha[:-1])  # (accepted: a table may be set before its materials are)
    with pytest.raises(capi.NexusError, match="one entry per material"):
        ctx.render_frame()
    rays, tmax = AT.hook_rays()
    for call in (lambda: ctx.trace_batch(rays[:64]), lambda: ctx.trace_shadow_batch(rays[:64], tmax[:64]), lambda: ctx.trace_transmittance_batch(rays[:64], tmax[:64])):
        with pytest.raises(capi.NexusError, match="one entry per material"):
            call()
    ctx.set_material_alpha(scene.material_alpha)
    ctx.render_frame()
    ctx.sync()
    ctx.close()


def test_a_mask_material_on_a_mesh_light_is_refused_at_render_time(gpu_ctx_factory):
    W = H = 32
    scene = SH.cornell_scene(W, H, path_length=2)
    assert len(scene.lights) >= 1
    light_material = int(scene.instances[int(scene.lights[0]["meshId"])]["materialId"])
    table = _table(*[(pod.ALPHA_MASK if k == light_material else pod.ALPHA_BLEND, 0.5) for k in range(len(scene.materials))])
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_material_alpha(table)
    with pytest.raises(capi.NexusError, match="mesh light"):
        ctx.render_frame()
    # OPAQUE on an emitter is fine, and so is MASK on any other material
    table["mode"][light_material] = pod.ALPHA_OPAQUE
    ctx.set_material_alpha(table)
    ctx.render_frame()
    other = _table(*[(pod.ALPHA_BLEND if k == light_material else pod.ALPHA_MASK, 0.5) for k in range(len(scene.materials))])
    ctx.set_material_alpha(other)
    ctx.render_frame()
    ctx.sync()
    ctx.close()
