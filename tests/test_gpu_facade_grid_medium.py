"""The fog density grid through the kept C++ API: Scene::SetMediumDensity with tests/golden/fog_puff.npy (read by IMGLoader::LoadNPYGrid)
over tests/golden/punctual_lights.glb rendered by PathTracer::Render gives the bits of the same grid set through the C-ABI
(nxhip_set_medium_density); ClearMediumDensity gives the bits of the homogeneous medium."""
import os

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import scene_helpers as SH
from tests import test_gpu_facade_medium as FM

pytestmark = pytest.mark.gpu

W = H = 64
FRAMES = 3
FOG = pod.make_medium(box_min=(-2.0, 0.0, -2.0), box_max=(2.0, 3.0, 2.0), sigma_t=1.2, g=0.5, albedo=(0.9, 0.9, 0.9))


def _capi_route(gpu_ctx_factory, grid):
    glb = os.path.join(SH.GOLDEN, "punctual_lights.glb")
    scene = SH.glb_scene(glb, W, H, path_length=3, eye=FM.EYE, forward=FM.FORWARD)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_analytic_lights(capi.load_scene_analytic_lights(glb))
    ctx.set_medium(FOG)
    ctx.set_medium_density(grid)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.reset_frame_number()
    for _ in range(FRAMES):
        ctx.render_frame()
        ctx.accumulate()
    out = ctx.read_rgba8(), ctx.read_accumulation(), bool(ctx.debug_pass_flavor() & capi.FLAVOR_MEDIUM_GRID), scene.settings
    ctx.close()
    return out


def test_set_medium_density_through_the_facade_equals_the_capi_path(gpu_ctx_factory):
    with open(os.path.join(SH.GOLDEN, "fog_puff.npy"), "rb") as f:
        puff = capi.decode_npy_grid(f.read())
    assert puff.shape == (16, 16, 16)
    px_grid, acc_grid, on, settings = _capi_route(gpu_ctx_factory, puff)
    px, acc, off, _ = _capi_route(gpu_ctx_factory, None)
    assert on and not off and not np.array_equal(acc_grid, acc), "the grid shows"

    sc = capi.Scene(W, H)
    sc.load_file(SH.GOLDEN + os.sep, "punctual_lights.glb")
    assert sc.medium_density() is None
    sc.set_medium(FOG)
    sc.set_medium_density(puff)
    assert np.array_equal(sc.medium_density().view(np.uint32), puff.view(np.uint32))
    sc.set_camera(FM.EYE, FM.FORWARD, 40.0, 5.0, 0.0)
    sc.set_render_settings(settings)
    sc.update()
    pt = capi.PathTracer(W, H)
    pt.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    pt.update_device_scene(sc)
    for _ in range(FRAMES):
        pt.render(sc)
    assert np.array_equal(pt.read_pixels(), px_grid)
    assert np.array_equal(pt.read_accumulation().view(np.uint32), acc_grid.view(np.uint32))
    # ClearMediumDensity reaches the device with the next update: the bits of the homogeneous medium
    sc.set_medium_density(None)
    assert sc.medium_density() is None and sc.medium() is not None
    pt.update_device_scene(sc)
    pt.reset_frame_number()
    for _ in range(FRAMES):
        pt.render(sc)
    assert np.array_equal(pt.read_pixels(), px)
    assert np.array_equal(pt.read_accumulation().view(np.uint32), acc.view(np.uint32))
    pt.close()
    sc.close()
