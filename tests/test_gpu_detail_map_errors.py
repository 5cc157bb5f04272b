"""nxhip_set_material_detail refuses what its contract lists (include/nexus_hip.h) with NXHIP_ERR_INVALID and the previous table stays in
place; a render refuses a table that does not fit the materials or names a texture that is not there; after each refusal the previous
state renders the previous frame."""
import ctypes as C

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import test_gpu_detail_maps as DM

pytestmark = pytest.mark.gpu

W = H = DM.W
INVALID = 1  # NXHIP_ERR_INVALID


def _frame(ctx):
    ctx.reset_frame_number()
    ctx.render_frame()
    return ctx.read_radiance().view(np.uint32).copy()


@pytest.fixture(scope="module")
def ctx_scene(gpu_ctx_factory):
    c = gpu_ctx_factory(W, H)
    scene = DM._box_scene()
    scene.upload(c)
    c.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    c.set_frames_per_pass(1)
    return c, scene


def _with(table, index, **fields):
    t = table.copy()
    for k, v in fields.items():
        t[index][k] = v
    return t


def test_every_refused_table_leaves_the_previous_one(ctx_scene):
    ctx, scene = ctx_scene
    good = scene.material_detail
    want = _frame(ctx)
    L = ctx.L
    refused = {
        "a normal map id below -1": _with(good, 0, normalMapId=-2),
        "a roughness map id below -1": _with(good, 1, roughnessMapId=-7),
        "a normalScale that is not a number": _with(good, 2, normalScale=np.nan),
        "an infinite normalScale": _with(good, 0, normalScale=-np.inf),
    }
    for what, table in refused.items():
        assert L.nxhip_set_material_detail(ctx.h, table.ctypes.data_as(C.c_void_p), len(table)) == INVALID, what
        with pytest.raises(capi.NexusError):
            ctx.set_material_detail(table)
        assert np.array_equal(_frame(ctx), want), what
    assert L.nxhip_set_material_detail(ctx.h, None, 4) == INVALID
    assert L.nxhip_set_material_detail(None, good.ctypes.data_as(C.c_void_p), 4) == INVALID
    assert np.array_equal(_frame(ctx), want)
    # what is allowed: a negative and a zero scale, NULL with count 0
    ctx.set_material_detail(_with(good, 0, normalScale=-1.0))
    ctx.set_material_detail(_with(good, 0, normalScale=0.0))
    assert L.nxhip_set_material_detail(ctx.h, None, 0) == 0
    ctx.set_material_detail(good)
    assert np.array_equal(_frame(ctx), want)


def test_a_render_refuses_a_table_that_does_not_fit(ctx_scene):
    ctx, scene = ctx_scene
    good = scene.material_detail
    ctx.set_material_detail(good)
    want = _frame(ctx)
    L = ctx.L
    unfit = {
        "one entry too few": good[:3],
        "one entry too many": np.concatenate([good, good[:1]]),
        "a normal map that has not been uploaded": _with(good, 2, normalMapId=1),
        "a roughness map that has not been uploaded": _with(good, 0, roughnessMapId=5),
    }
    for what, table in unfit.items():
        ctx.set_material_detail(table)  # (accepted: the table may come before its textures and its materials)
        assert L.nxhip_render_frame(ctx.h) == INVALID, what
        with pytest.raises(capi.NexusError):
            ctx.shading_frame_batch(0, [0], [[0.2, 0.2]], [[0.0, -1.0, 0.0]])
        ctx.set_material_detail(good)
        assert np.array_equal(_frame(ctx), want), what
    # clearing the textures leaves the table naming maps that are gone
    ctx.clear_textures()
    assert L.nxhip_render_frame(ctx.h) == INVALID
    for img in scene.normal_maps:
        ctx.upload_texture("normal", img)
    for img in scene.roughness_maps:
        ctx.upload_texture("roughness", img)
    assert np.array_equal(_frame(ctx), want)


def test_the_hooks_refuse_bad_arguments(ctx_scene):
    ctx, scene = ctx_scene
    ctx.set_material_detail(scene.material_detail)
    uv, d = np.full((2, 2), 0.25, np.float32), np.tile(np.float32([0.0, -1.0, 0.0]), (2, 1))
    ns, rough, fell = ctx.shading_frame_batch(0, [0, 1], uv, d)
    assert ns.shape == (2, 3) and np.all(np.isfinite(ns))
    with pytest.raises(capi.NexusError):
        ctx.shading_frame_batch(len(scene.instances), [0, 1], uv, d)
    with pytest.raises(capi.NexusError):
        ctx.shading_frame_batch(0, [0, len(scene.meshes[0])], uv, d)
    L = ctx.L
    assert L.nxhip_shading_frame_batch(ctx.h, 0, None, None, None, 2, None, None, None) == INVALID
    assert L.nxhip_shading_frame_batch(ctx.h, 0, None, None, None, 0, None, None, None) == 0
    for kind in ("normal", "roughness"):
        with pytest.raises(capi.NexusError):
            ctx.tex2d_batch(kind, 1, uv)
        with pytest.raises(capi.NexusError):
            ctx.tex2d_batch(kind, -1, uv)
    img = np.zeros((2, 2, 4), np.uint8)
    assert L.nxhip_upload_texture(ctx.h, 5, img.ctypes.data_as(C.c_void_p), 2, 2, None) == INVALID
