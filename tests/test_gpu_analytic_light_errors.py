"""nxhip_set_analytic_lights refuses what its contract lists (include/nexus_hip.h) with NXHIP_ERR_INVALID before anything is allocated, and
the previous table stays in place: the next frame is the frame that table gives."""
import ctypes as C

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

W = H = 32
GOOD = np.array([
    pod.make_analytic_light(pod.ALIGHT_POINT, position=(0.4, 1.2, 0.3), intensity=0.8, radius=0.05),
    pod.make_analytic_light(pod.ALIGHT_SPOT, position=(-0.5, 1.8, 0.0), direction=(0.2, -1.0, 0.1), intensity=2.0, inner_cone=0.3, outer_cone=0.6),
    pod.make_analytic_light(pod.ALIGHT_DIRECTIONAL, direction=(0.2, -0.5, -1.0), intensity=0.7, angular_radius=0.02),
], dtype=pod.ALIGHT_DT)


def _bad(index, **fields):
    lights = GOOD.copy()
    for k, v in fields.items():
        lights[index][k] = v
    return lights


REFUSED = {
    "a position that is not finite": _bad(0, position=(np.nan, 0, 0)),
    "an infinite radius": _bad(0, radius=np.inf),
    "an intensity that is not a number": _bad(1, intensity=np.nan),
    "an infinite colour": _bad(2, colour=(1, np.inf, 1)),
    "a cone angle that is not a number": _bad(1, innerConeAngle=np.nan),
    "a direction that is not finite": _bad(2, direction=(0, -np.inf, 0)),
    "an angular radius that is not a number": _bad(2, angularRadius=np.nan),
    "a negative radius": _bad(0, radius=-0.1),
    "a negative intensity": _bad(0, intensity=-1.0),
    "a negative colour component": _bad(1, colour=(1, -0.5, 1)),
    "a negative angular radius": _bad(2, angularRadius=-0.01),
    "an angular radius of pi / 2": _bad(2, angularRadius=np.float32(np.pi / 2)),
    "an angular radius above pi / 2": _bad(2, angularRadius=2.0),
    "a spot's direction of length 0": _bad(1, direction=(0, 0, 0)),
    "a sun's direction of length 0": _bad(2, direction=(0, 0, 0)),
    "a point light's direction of length 0": _bad(0, direction=(0, 0, 0)),
    "a negative inner cone angle": _bad(1, innerConeAngle=-0.1),
    "inner equal to outer": _bad(1, innerConeAngle=0.6, outerConeAngle=0.6),
    "inner above outer": _bad(1, innerConeAngle=0.7, outerConeAngle=0.6),
    "an outer cone angle above pi / 2": _bad(1, outerConeAngle=1.7),
    "an unknown type": _bad(0, type=3),
}


def _frame(ctx):
    ctx.reset_frame_number()
    ctx.render_frame()
    return ctx.read_radiance().view(np.uint32).copy()


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    c = gpu_ctx_factory(W, H)
    SH.cornell_scene(W, H, path_length=3).upload(c)
    c.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    c.set_frames_per_pass(1)
    return c


def test_every_refused_input_leaves_the_previous_table(ctx):
    without = _frame(ctx)
    ctx.set_analytic_lights(GOOD)
    want = _frame(ctx)
    assert not np.array_equal(want, without)
    L = ctx.L
    for what, lights in REFUSED.items():
        assert L.nxhip_set_analytic_lights(ctx.h, lights.ctypes.data_as(C.c_void_p), len(lights)) == 1, what  # NXHIP_ERR_INVALID
        with pytest.raises(capi.NexusError):
            ctx.set_analytic_lights(lights)
        assert np.array_equal(_frame(ctx), want), what
    # a null array with a count, and more lights than the random number that picks can tell apart (refused before the array is read)
    assert L.nxhip_set_analytic_lights(ctx.h, None, 3) == 1
    assert L.nxhip_set_analytic_lights(ctx.h, GOOD.ctypes.data_as(C.c_void_p), (1 << 23) - 1) == 1
    assert L.nxhip_set_analytic_lights(None, GOOD.ctypes.data_as(C.c_void_p), 3) == 1
    assert np.array_equal(_frame(ctx), want)
    # with a table in place nxhip_set_lights is held to the same bound (the count is refused before the array is read)
    one = np.zeros(1, pod.LIGHT_DT)
    assert L.nxhip_set_lights(ctx.h, one.ctypes.data_as(C.c_void_p), (1 << 23) - 3) == 1
    assert np.array_equal(_frame(ctx), want)
    # what is allowed at the edges: pi / 2 as the outer angle, radius 0, a direction of any length
    ctx.set_analytic_lights(_bad(1, outerConeAngle=np.float32(np.pi / 2)))
    ctx.set_analytic_lights(_bad(0, direction=(0, 0, 1e-20), radius=0.0))
    ctx.set_analytic_lights(GOOD)
    assert np.array_equal(_frame(ctx), want)
    ctx.set_analytic_lights(np.zeros(0, pod.ALIGHT_DT))
    assert np.array_equal(_frame(ctx), without)


def test_the_hook_refuses_bad_arguments(ctx):
    ctx.set_analytic_lights(GOOD)
    o, r = np.zeros((4, 3), np.float32), np.full((4, 2), 0.5, np.float32)
    assert len(ctx.analytic_light_sample_batch(0, o, r)[1]) == 4
    with pytest.raises(capi.NexusError):
        ctx.analytic_light_sample_batch(3, o, r)
    for bad in (1.0, -0.1, np.nan):
        rr = r.copy()
        rr[2, 1] = bad
        with pytest.raises(capi.NexusError):
            ctx.analytic_light_sample_batch(0, o, rr)
    oo = o.copy()
    oo[1, 0] = np.inf
    with pytest.raises(capi.NexusError):
        ctx.analytic_light_sample_batch(0, oo, r)
    ctx.set_analytic_lights(np.zeros(0, pod.ALIGHT_DT))
    with pytest.raises(capi.NexusError):
        ctx.analytic_light_sample_batch(0, o, r)
