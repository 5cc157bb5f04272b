"""nxhip_set_medium's refusals: every validation case leaves the previous medium in effect (verified by a rendered frame), a render in a mode
the medium cannot run in says so, and the hooks need a medium."""
import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import scene_helpers as SH
from tests import test_gpu_medium as GM

pytestmark = pytest.mark.gpu

W = H = 64


def _frame(ctx):
    ctx.reset_frame_number()
    ctx.render_frame()
    return ctx.read_radiance().copy()


def test_refusals_leave_the_previous_medium_in_effect(gpu_ctx_factory):
    ctx = gpu_ctx_factory(W, H)
    SH.cornell_scene(W, H, path_length=4).upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    plain = _frame(ctx)
    ctx.set_medium(GM.IN_FRAME)
    foggy = _frame(ctx)
    assert not np.array_equal(plain, foggy)
    good = dict(box_min=(-1, -1, -1), box_max=(1, 1, 1), sigma_t=0.5, g=0.2, albedo=(0.5, 0.5, 0.5))
    bad = {
        "a field is not finite": [dict(good, sigma_t=np.nan), dict(good, g=np.inf), dict(good, box_min=(-np.inf, -1, -1)), dict(good, box_max=(1, np.nan, 1)),
                                  dict(good, albedo=(0.5, np.nan, 0.5))],
        "sigmaT may not be negative": [dict(good, sigma_t=-0.1)],
        "albedo": [dict(good, albedo=(0.5, 1.5, 0.5)), dict(good, albedo=(-0.1, 0.5, 0.5))],
        "0.99": [dict(good, g=0.995), dict(good, g=-1.0)],
        "boxMin must be below boxMax": [dict(good, box_min=(1, -1, -1)), dict(good, box_min=(-1, 2, -1)), dict(good, box_max=(1, 1, -1))],
    }
    for message, cases in bad.items():
        for kw in cases:
            with pytest.raises(capi.NexusError, match=message):
                ctx.set_medium(pod.make_medium(**kw))
            assert np.array_equal(_frame(ctx).view(np.uint32), foggy.view(np.uint32)), kw
    # modes the medium cannot run in: refused with a message that says so; the medium removed, they render
    for modes in ((pod.RNG_PIXEL_KEYED, pod.COMPACT_ORDERED), (pod.RNG_REFERENCE_SLOT, pod.COMPACT_FAST)):
        ctx.set_modes(modes[0], modes[1], pod.CONDUCTOR_REFERENCE)
        with pytest.raises(capi.NexusError, match="NX_COMPACT_FAST.*NX_RNG_PIXEL_KEYED"):
            ctx.render_frame()
        ctx.set_medium(None)
        ctx.render_frame()
        ctx.sync()
        ctx.set_medium(GM.IN_FRAME)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    assert np.array_equal(_frame(ctx).view(np.uint32), foggy.view(np.uint32))
    ctx.close()


def test_the_hooks_need_a_medium(gpu_ctx_factory):
    ctx = gpu_ctx_factory(16, 16)
    o, d, te, xi = np.zeros((1, 3), np.float32), np.array([[0, 0, 1]], np.float32), np.ones(1, np.float32), np.zeros(1, np.float32)
    for medium in (None, pod.make_medium(sigma_t=0.0)):
        ctx.set_medium(medium)
        with pytest.raises(capi.NexusError, match="no medium"):
            ctx.medium_segment_batch(o, d, te, xi)
        with pytest.raises(capi.NexusError, match="no medium"):
            ctx.medium_phase_batch(d, xi, xi)
    ctx.set_medium(pod.make_medium(sigma_t=1.0))
    with pytest.raises(capi.NexusError, match="xi must be in"):
        ctx.medium_segment_batch(o, d, te, np.ones(1, np.float32))
    with pytest.raises(capi.NexusError, match="finite"):
        ctx.medium_phase_batch(np.array([[np.nan, 0, 1]], np.float32), xi, xi)
    t0, L, T, st = ctx.medium_segment_batch(o, d, te, xi)  # from the box's corner along z, one unit: all of it inside
    assert (float(t0[0]), float(L[0]), float(st[0])) == (0.0, 1.0, 0.0) and abs(float(T[0]) - np.exp(-1.0)) < 1e-6
    ctx.close()
