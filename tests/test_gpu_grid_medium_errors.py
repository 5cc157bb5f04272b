"""nxhip_set_medium_density's refusals: every validation case leaves the previous grid in effect (verified by a rendered frame), a grid too
thick for the walk's bound is refused by the render and by the walking hook with a message that names the bound, the hooks need a medium
and a grid, and a `make release` library refuses the hooks."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import scene_helpers as SH
from tests import test_gpu_grid_medium as GG
from tests import test_grid_medium_reference as TR

W = H = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(ctx):
    ctx.reset_frame_number()
    ctx.render_frame()
    return ctx.read_radiance().copy()


@pytest.mark.gpu
def test_refusals_leave_the_previous_grid_in_effect(gpu_ctx_factory):
    ctx = gpu_ctx_factory(W, H)
    SH.cornell_scene(W, H, path_length=4).upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.set_medium(GG.IN_FRAME)
    homogeneous = _frame(ctx)
    ctx.set_medium_density(TR.puff())
    puffy = _frame(ctx)
    assert not np.array_equal(homogeneous, puffy)
    good = np.full((3, 4, 5), 0.5, np.float32)

    def poisoned(value):
        g = good.copy()
        g[1, 2, 3] = value
        return g

    L = ctx.L
    raw = good.ctypes.data_as(C.c_void_p)
    # (more than 2^27 voxels cannot be reached with dimensions of at most 512: 512^3 is 2^27 — the dimension check answers first)
    for dims, message in (((0, 4, 3), "a dimension is 0"), ((5, 0, 3), "a dimension is 0"), ((5, 4, 0), "a dimension is 0"), ((513, 1, 1), "exceeds 512"),
                          ((1, 1, 4000000000), "exceeds 512")):
        assert L.nxhip_set_medium_density(ctx.h, raw, *dims) == 1, dims  # NXHIP_ERR_INVALID (validated before the voxels are read)
        assert message in L.nxhip_last_error().decode(), dims
        assert np.array_equal(_frame(ctx).view(np.uint32), puffy.view(np.uint32)), dims
    for grid, message in ((poisoned(-0.25), "negative or not finite"), (poisoned(np.nan), "negative or not finite"), (poisoned(np.inf), "negative or not finite"),
                          (poisoned(-np.inf), "negative or not finite"), (np.zeros((2, 2, 2), np.float32), "maximum is 0"), (np.ones((1, 1, 513), np.float32), "exceeds 512")):
        with pytest.raises(capi.NexusError, match=message):
            ctx.set_medium_density(grid)
        assert np.array_equal(_frame(ctx).view(np.uint32), puffy.view(np.uint32)), message
    assert ctx.debug_pass_flavor() & capi.FLAVOR_MEDIUM_GRID
    ctx.set_medium_density(None)
    assert np.array_equal(_frame(ctx).view(np.uint32), homogeneous.view(np.uint32))
    ctx.close()


@pytest.mark.gpu
def test_a_grid_too_thick_for_the_walk_is_refused_with_the_bound(gpu_ctx_factory):
    ctx = gpu_ctx_factory(W, H)
    SH.cornell_scene(W, H, path_length=4).upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    puff = TR.puff()
    diag = float(np.linalg.norm(GG.IN_FRAME["boxMax"].astype(np.float64) - GG.IN_FRAME["boxMin"].astype(np.float64)))
    thick = GG.IN_FRAME.copy()
    thick["sigmaT"] = 1.01 * 512.0 / (float(puff.max()) * diag)
    fine = GG.IN_FRAME.copy()
    fine["sigmaT"] = 0.99 * 512.0 / (float(puff.max()) * diag)
    ctx.set_medium_density(puff)
    ctx.set_medium(thick)  # (the setters take it: the product is a render's business)
    o, d, te, seed = np.array([[0, 1, 3]], np.float32), np.array([[0, 0, -1]], np.float32), np.full(1, np.inf, np.float32), np.ones(1, np.uint32)
    with pytest.raises(capi.NexusError, match=r"exceeds 512 mean free paths.*lower sigmaT"):
        ctx.render_frame()
    with pytest.raises(capi.NexusError, match=r"exceeds 512"):
        ctx.medium_track_batch(o, d, te, seed)
    ctx.set_medium(thick)
    ctx.set_medium_density(None)  # the homogeneous medium has no bound to keep
    ctx.render_frame()
    ctx.sync()
    ctx.set_medium_density(puff)
    ctx.set_medium(fine)
    ctx.render_frame()
    ctx.sync()
    st, T, steps = ctx.medium_track_batch(o, d, te, seed)
    assert (steps[0, 0] & 0xffff) < 4096 and (steps[0, 1] & 0xffff) < 4096
    ctx.close()


@pytest.mark.gpu
def test_the_hooks_need_a_medium_and_a_grid(gpu_ctx_factory):
    ctx = gpu_ctx_factory(16, 16)
    o, d, te, seed = np.zeros((1, 3), np.float32), np.array([[0, 0, 1]], np.float32), np.ones(1, np.float32), np.ones(1, np.uint32)
    with pytest.raises(capi.NexusError, match="no density grid"):
        ctx.read_medium_majorants()
    for medium, grid in ((None, None), (pod.make_medium(sigma_t=1.0), None), (None, np.ones((2, 2, 2), np.float32)), (pod.make_medium(sigma_t=0.0), np.ones((2, 2, 2), np.float32))):
        ctx.set_medium(medium)
        ctx.set_medium_density(grid)
        with pytest.raises(capi.NexusError, match="needs a medium"):
            ctx.medium_density_batch(o)
        with pytest.raises(capi.NexusError, match="needs a medium"):
            ctx.medium_track_batch(o, d, te, seed)
    ctx.set_medium(pod.make_medium(sigma_t=1.0))
    ctx.set_medium_density(np.ones((2, 2, 2), np.float32))
    with pytest.raises(capi.NexusError, match="seed may not be 0"):
        ctx.medium_track_batch(o, d, te, np.zeros(1, np.uint32))
    with pytest.raises(capi.NexusError, match="finite"):
        ctx.medium_density_batch(np.array([[np.nan, 0, 0]], np.float32))
    st, T, steps = ctx.medium_track_batch(o, d, te, seed)  # from the unit box's corner along z: one brick, at most a few collisions
    assert (steps[0, 0] & 0xffff) >= 1 and 0.0 <= float(T[0]) <= 1.0
    ctx.close()


def test_a_release_library_refuses_the_grid_hooks():
    """no GPU needed: the hooks refuse before they look at their context"""
    assert shutil.which("/opt/rocm/bin/hipcc"), "the release library cannot be built without the compiler"
    out = os.path.join(ROOT, "nexus_amd", "lib", "release", "libnexus_amd.so")
    subprocess.run(["make", "-C", ROOT, "-j", "8", "release"], check=True, capture_output=True, timeout=900)
    L = C.CDLL(out)
    L.nxhip_last_error.restype = C.c_char_p
    for name in ("nxhip_read_medium_majorants", "nxhip_medium_density_batch", "nxhip_medium_track_batch"):
        fn = getattr(L, name)
        fn.restype = C.c_int
        assert fn(None, None, 0, None, None, None, None, None, None) != 0 and b"built without the test hooks" in L.nxhip_last_error(), name
    L.nxhip_set_medium_density.restype = C.c_int
    assert L.nxhip_set_medium_density(None, None, 0, 0, 0) != 0 and b"built without" not in L.nxhip_last_error(), "the setter is no hook"
