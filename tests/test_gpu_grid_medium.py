"""Fog density grids on the device (nxhip_set_medium_density): the majorant bricks bit for bit against numpy, the lookup and the walk's hooks
against the float64 statement of the rule (tests/grid_medium_reference.py, within the bars tests/test_grid_medium_reference.py derives),
transport against quadrature of the trilinear field — exactly where the rule is deterministic, by z-scores per 16 x 16 block otherwise (the
bars of tests/test_physics_pins.py) — and the wiring: a grid without a medium changes no bit, removing it gives the homogeneous bits, and
with the puff in the frame every pass shape gives the same bits.  The oracle does not know the medium; nothing here compares with it."""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen
from tests import grid_medium_reference as G
from tests import medium_reference as R
from tests import scene_helpers as SH
from tests import test_gpu_medium as GM
from tests import test_grid_medium_reference as TR
from tests import test_medium_reference as TM
from tests import test_physics_pins as PP

pytestmark = pytest.mark.gpu

W = H = 64


def _frames(gpu_ctx_factory, scene, medium, grid, frames, **kw):
    """GM._frames with the grid beside the medium (Workload.upload applies both); the grid's flavor bit is checked by the wiring tests"""
    scene.medium_density = grid
    return GM._frames(gpu_ctx_factory, scene, medium, frames, **kw)


# ---- 1. bricks -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", TR.SHAPES, ids=["1x1x1", "8x8x8", "9x8x8", "20x13x18"])
def test_device_bricks_equal_numpy_bit_for_bit(gpu_ctx_factory, shape):
    ctx = gpu_ctx_factory(16, 16)
    grid = TR.shape_grid(shape)
    ctx.set_medium_density(grid)
    got = ctx.read_medium_majorants()
    want = G.bricks(grid)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ctx.close()


# ---- 2. the lookup hook --------------------------------------------------------------------------------------------------------------------

def test_lookup_hook_matches_the_reference(gpu_ctx_factory):
    ctx = gpu_ctx_factory(16, 16)
    m, grid, p = TR.hook_medium(), TR.hook_grid(), TR.lookup_points()
    ctx.set_medium(m)
    ctx.set_medium_density(grid)
    bar, r64 = TR.lookup_bar()
    rho, maj = ctx.medium_density_batch(p)
    dev = np.abs(rho.astype(np.float64) - r64).max()
    print("lookup: device deviation %.3g, bar %.3g" % (dev, bar))
    assert 0.0 < bar < 1e-5 and dev <= bar
    b = G.brick_of(m["boxMin"], m["boxMax"], grid.shape, p, np.float32)
    want = G.bricks(grid)[b[:, 2], b[:, 1], b[:, 0]]
    assert (maj != want).mean() <= 1e-3, "the point's brick"
    assert np.all(rho.astype(np.float64) <= maj.astype(np.float64) * (1.0 + 2.0 ** -23)), "a majorant under the lookup"
    ctx.close()


def test_a_constant_grid_returns_the_constant_exactly(gpu_ctx_factory):
    ctx = gpu_ctx_factory(16, 16)
    ctx.set_medium(TR.hook_medium())
    for shape, value in (((5, 9, 11), 0.7), ((1, 1, 1), 1.0), ((8, 8, 9), 3.1)):
        ctx.set_medium_density(np.full(shape, value, np.float32))
        rho, maj = ctx.medium_density_batch(TR.lookup_points())
        assert np.all(rho.view(np.uint32) == np.float32(value).view(np.uint32)) and np.all(maj == np.float32(value)), (shape, value)
    ctx.close()


# ---- 3. the track hook -----------------------------------------------------------------------------------------------------------------------

def test_track_hook_matches_the_reference(gpu_ctx_factory):
    ctx = gpu_ctx_factory(16, 16)
    ctx.set_medium(TR.hook_medium())
    ctx.set_medium_density(TR.hook_grid())
    o, d, t_end, seed = TR.hook_inputs()
    bars, keep, (flight, ratio) = TR.track_bars()
    st, T, steps = ctx.medium_track_batch(o, d, t_end, seed)
    got = np.stack([steps[:, 0], steps[:, 1], (st >= 0).astype(np.uint32)], 1)
    same = np.all(got == TR.decisions(flight, ratio), 1)
    print("decision sequences that differ from float64: %d of %d (cap %d)" % ((~same).sum(), len(same), len(same) // 1000))
    assert (~same).mean() <= 1e-3
    use = same & keep
    dev = {"scatter_t": np.abs(st.astype(np.float64) - flight["scatter_t"])[use].max(), "T": np.abs(T.astype(np.float64) - ratio["T"])[use].max()}
    print("device deviations", dev, "bars", bars)
    for k in dev:
        assert dev[k] <= bars[k], k
    none = (steps[:, 1] >> 16) == 0
    assert none.sum() > 1000 and np.all(T[none].view(np.uint32) == np.float32(1.0).view(np.uint32)), "T is exactly 1 where no collision happened"
    assert np.all(st[~(st >= 0)] == -1.0) and np.all(steps[~flight["crosses"]] == 0)
    iters = (steps[:, 0] & 0xffff)[flight["crosses"]]
    print("iterations per crossing ray: mean %.2f, max %d" % (iters.mean(), iters.max()))
    ctx.close()


# ---- 4. white furnace: exact -----------------------------------------------------------------------------------------------------------------

def test_white_furnace_is_exactly_one(gpu_ctx_factory):
    cam = capi.camera_init((0.3, 0.4, 5.0), (0.0, 0.0, -1.0), 40.0, W, H, 5.0, 0.0)
    sc = GM._scene(cam, path_length=64, use_mis=False, background=1.0)
    fog = pod.make_medium(box_min=(-1, -1, -1), box_max=(1, 1, 1), sigma_t=0.5, g=0.6, albedo=(1, 1, 1))
    r = _frames(gpu_ctx_factory, sc, fog, TR.puff(), 64)
    assert r.shape == (64, W * H, 3)
    assert np.all(r.view(np.uint32) == np.float32(1.0).view(np.uint32)), "worst %.9g" % np.abs(r - 1.0).max()


# ---- 5. absorption on the camera segment -------------------------------------------------------------------------------------------------

def test_absorption_on_the_camera_segment(gpu_ctx_factory):
    le, sigma = 2.0, 1.5
    cam = capi.camera_init((0.2, 0.1, 5.0), (0.0, 0.0, -1.0), 30.0, W, H, 5.0, 0.0)
    wall = scenegen.quad((-6, -6, -3), (6, -6, -3), (6, 6, -3), (-6, 6, -3))
    sc = GM._scene(cam, [wall], [pod.make_material(pod.MAT_DIFFUSE, albedo=(0, 0, 0), emissive=(1.0, 0.8, 0.6), intensity=le)], path_length=1)
    fog = pod.make_medium(box_min=(-1, -0.6, -1), box_max=(0.7, 1.2, 1), sigma_t=sigma, g=0.3, albedo=(0, 0, 0))
    # the puff on a floor of 0.1: a block that only grazes the puff's empty rim would expect a fraction of ONE absorbed path in 65 536, and
    # the block means' spread says nothing about an expectation that small; with the floor every block that sees the box absorbs thousands
    grid = TR.puff() + np.float32(0.1)
    pos, dirs = R.camera_rays(cam, W, H, 4)
    want = np.zeros(W * H)
    for k in range(len(dirs)):
        t_end = (-3.0 - pos[2]) / dirs[k][:, 2]
        tau = G.optical_depth(grid, fog["boxMin"], fog["boxMax"], sigma, np.broadcast_to(pos, dirs[k].shape), dirs[k], t_end, panels=32)
        want += np.exp(-tau) / len(dirs)
    want = TM.block_means(want)[:, None] * le * np.array((1.0, 0.8, 0.6))[None, :]
    assert want.min() < 0.6 * want.max(), "some blocks look through the puff, some past it"
    GM._pin(GM._estimate(_frames(gpu_ctx_factory, sc, fog, grid, 256)), want, "absorption through the puff")


# ---- 6. shadow rays: ratio tracking ----------------------------------------------------------------------------------------------------------

SLAB_SIGMA = 2.0
SLAB_EMPTY_X = -0.9 + 1.5 / 3.0  # the first of the three bricks along x ends here
# (above the patch of floor the slab scene's camera sees, x in [-0.55, 0.55], z in [1.6, 2.9], displaced against the sun; the camera is below it)
SLAB = pod.make_medium(box_min=(-0.9, 1.0, 1.0), box_max=(0.6, 1.5, 3.4), sigma_t=SLAB_SIGMA, g=0.2, albedo=(0.8, 0.8, 0.8))


def slab_grid():
    """24 x 4 x 24 voxels (x, y, z) over the slab: lumpy, and 0 for x < 12 voxels — the bricks of the first 8 voxels along x are empty"""
    z, y, x = np.meshgrid(np.arange(24), np.arange(4), np.arange(24), indexing="ij")
    f = 0.8 + 0.5 * np.sin(0.6 * x) * np.cos(0.5 * z + 0.4) + 0.1 * y
    f[:, :, :12] = 0.0
    return f.astype(np.float32)


def slab_expectation(cam, grid):
    """per pixel: E[T] along the sun direction from the floor, and whether every sun ray of the pixel and of its neighbours stays in the
    empty bricks (world x below SLAB_EMPTY_X) or clear of the box"""
    sub = 3
    pos = cam["position"].astype(np.float64)
    jj, ii = np.mgrid[0:H, 0:W]
    want, untouched = np.zeros(W * H), np.ones(W * H, bool)
    offsets = np.linspace(-1.0, 2.0, 2 * sub + 1)
    inner = 0
    for a in offsets:
        for b in offsets:
            x, y = ((ii + a) / W).reshape(-1, 1), ((jj + b) / H).reshape(-1, 1)
            d = cam["lowerLeftCorner"].astype(np.float64) + cam["viewportX"].astype(np.float64) * x + cam["viewportY"].astype(np.float64) * y - pos
            assert np.all(d[:, 1] < 0), "the camera looks down: no camera ray crosses the slab"
            p = pos + d * (-pos[1] / d[:, 1])[:, None]
            to_sun = np.broadcast_to(-GM.SUN_DIR, p.shape)
            t0, L, crosses = R.segment(SLAB["boxMin"], SLAB["boxMax"], p, to_sun, np.full(len(p), np.inf))
            x_in, x_out = p[:, 0] + to_sun[:, 0] * t0, p[:, 0] + to_sun[:, 0] * (t0 + L)
            untouched &= ~crosses | (np.maximum(x_in, x_out) < SLAB_EMPTY_X - 1e-3)
            if 0.0 <= a <= 1.0 and 0.0 <= b <= 1.0:
                want += np.exp(-G.optical_depth(grid, SLAB["boxMin"], SLAB["boxMax"], SLAB_SIGMA, p, to_sun, np.full(len(p), np.inf), panels=16))
                inner += 1
    return want / inner, untouched


def test_shadow_rays_meet_the_quadrature_and_empty_bricks_change_no_bit(gpu_ctx_factory):
    sc, cam = GM._slab_scene(False)
    grid = slab_grid()
    M = G.bricks(grid)
    assert np.all(M[:, :, 0] == 0) and np.all(M[:, :, 1:] > 0)
    frames = 64
    without = _frames(gpu_ctx_factory, sc, None, None, frames, lights=[GM.SUN], want_medium=False)
    with_fog = _frames(gpu_ctx_factory, sc, SLAB, grid, frames, lights=[GM.SUN])
    assert np.all(without > 0), "the camera sees the lit floor only"
    want, untouched = slab_expectation(cam, grid)
    assert untouched.sum() > 200 and (want < 0.7).sum() > 200, (untouched.sum(), (want < 0.7).sum())
    assert np.array_equal(with_fog[:, untouched].view(np.uint32), without[:, untouched].view(np.uint32)), "a request that meets no brick with M > 0 keeps the default's bits"
    ratio = with_fog.astype(np.float64) / without.astype(np.float64)
    assert ratio.max() <= 1.0 + 2.0 ** -22
    GM._pin(GM._estimate(ratio), np.repeat(TM.block_means(want)[:, None], 3, 1), "with / without the grid against E[T] along the sun")


# ---- 7. a grid of 1.0 is the homogeneous medium ------------------------------------------------------------------------------------------

def test_a_grid_of_ones_agrees_with_the_homogeneous_medium(gpu_ctx_factory):
    frames = 512
    homogeneous = GM._estimate(_frames(gpu_ctx_factory, GM._lamp_scene(True), GM.LAMP_FOG, None, frames))
    ones = GM._estimate(_frames(gpu_ctx_factory, GM._lamp_scene(True), GM.LAMP_FOG, np.ones((4, 9, 5), np.float32), frames))
    lit = homogeneous.mean.max(1) > 0
    assert lit.sum() >= 12
    PP._assert_agree(PP._z(ones.mean, ones.se, homogeneous.mean, homogeneous.se)[lit], "a grid of 1.0 against the homogeneous medium")


# ---- 8. MIS == naive in the puff -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("light_sampling", [pod.LIGHTS_UNIFORM, pod.LIGHTS_POWER], ids=["uniform", "power"])
def test_mis_equals_naive_in_the_puff(gpu_ctx_factory, light_sampling):
    frames = 1024
    fog = pod.make_medium(box_min=(-1, -1, -1), box_max=(1, 1, 1), sigma_t=1.5, g=0.5, albedo=(0.9, 0.9, 0.9))
    mis = GM._estimate(_frames(gpu_ctx_factory, GM._lamp_scene(True), fog, TR.puff(), frames, light_sampling=light_sampling))
    naive = GM._estimate(_frames(gpu_ctx_factory, GM._lamp_scene(False), fog, TR.puff(), frames, light_sampling=light_sampling))
    lit = naive.mean.max(1) > 0
    assert lit.sum() >= 12
    print("MIS / naive per block:", np.round(mis.mean[:, 0] / naive.mean[:, 0], 3))
    PP._assert_agree(PP._z(mis.mean, mis.se, naive.mean, naive.se)[lit], "MIS against naive in the puff")


# ---- 9. wiring -------------------------------------------------------------------------------------------------------------------------------

def _cornell_run(gpu_ctx_factory, fog, per_pass=1, frames=4, order=pod.ORDER_ROWS, entry=False, in_flight=1):
    """`fog`: (medium, grid) set before pass k — (medium,) alone: the grid is left as it is; False: both are — in a list as long as the pass
    count.  (last frame's radiance, accumulation, flavors)"""
    ctx = gpu_ctx_factory(W, H)
    SH.cornell_scene(W, H, path_length=4).upload(ctx)
    ctx.set_analytic_lights(np.array([GM.SUN], dtype=pod.ALIGHT_DT))
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.set_pixel_order(order)
    ctx.set_entry_points(entry)
    ctx.set_frames_per_pass(per_pass)
    ctx.set_passes_in_flight(in_flight)
    ctx.reset_frame_number()
    flavors = []
    for k in range(frames // per_pass):
        if fog[k] is not False:
            ctx.set_medium(fog[k][0])
            if len(fog[k]) > 1:
                ctx.set_medium_density(fog[k][1])
        ctx.render_frame()
        ctx.accumulate()
        ctx.sync()
        flavors.append(ctx.debug_pass_flavor())
    last, acc = ctx.read_radiance().reshape(per_pass, W * H, 3)[-1], ctx.read_accumulation()
    ctx.close()
    if order == pod.ORDER_TILES:  # back to rows
        pm = capi.tile_pixel_map(W, H, 1, 0, 1, tiled=True)
        rows = [np.zeros_like(last), np.zeros_like(acc)]
        rows[0][pm], rows[1][pm] = last, acc
        last, acc = rows
    return last, acc, flavors


def _same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


IN_FRAME = pod.make_medium(box_min=(-0.8, 0.2, -0.8), box_max=(0.9, 1.9, 0.9), sigma_t=2.5, g=0.4, albedo=(0.9, 0.8, 0.7))


def test_wiring_of_the_grid(gpu_ctx_factory):
    puff = TR.puff()
    plain = _cornell_run(gpu_ctx_factory, [(None, None)] * 4)
    homogeneous = _cornell_run(gpu_ctx_factory, [(IN_FRAME, None)] * 4)
    assert not _same(plain, homogeneous)
    # a grid with no medium set: no bit, no flavor
    alone = _cornell_run(gpu_ctx_factory, [(None, puff)] * 4)
    assert _same(alone, plain) and alone[2] == plain[2]
    # with the medium: exactly the grid's bit more than the homogeneous run, and other frames
    both = _cornell_run(gpu_ctx_factory, [(IN_FRAME, puff)] * 4)
    assert all(b == h | capi.FLAVOR_MEDIUM_GRID and not h & capi.FLAVOR_MEDIUM_GRID and h & capi.FLAVOR_MEDIUM for b, h in zip(both[2], homogeneous[2]))
    assert not _same(both, homogeneous) and not _same(both, plain) and np.all(np.isfinite(both[1]))
    # set_medium leaves the grid alone: the medium removed and set again gives the grid's frames
    again = _cornell_run(gpu_ctx_factory, [(IN_FRAME, puff), (None,), (IN_FRAME,), False])
    assert np.array_equal(again[0].view(np.uint32), both[0].view(np.uint32)) and again[2] == [both[2][0], plain[2][1], both[2][2], both[2][3]]
    # the grid removed: the homogeneous run's bits and flavors (frames 1 .. 3 decide the last frame; the accumulation is compared on a run that
    # never rendered with the grid)
    removed = _cornell_run(gpu_ctx_factory, [(IN_FRAME, puff), (IN_FRAME, None), False, False])
    assert np.array_equal(removed[0].view(np.uint32), homogeneous[0].view(np.uint32)) and removed[2][1:] == homogeneous[2][1:] and removed[2][0] == both[2][0]
    # a box nothing crosses: the plain run's bits
    away = _cornell_run(gpu_ctx_factory, [(GM.AWAY, puff)] * 4)
    assert _same(away, plain) and all(a == p | capi.FLAVOR_MEDIUM | capi.FLAVOR_MEDIUM_GRID for a, p in zip(away[2], plain[2]))


# ---- 10. equal bits with the puff in the frame -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def puffy(gpu_ctx_factory):
    got = _cornell_run(gpu_ctx_factory, [(IN_FRAME, TR.puff())] * 64, frames=64)
    assert np.all(np.isfinite(got[1])) and all(f & capi.FLAVOR_MEDIUM_GRID for f in got[2])
    return got


@pytest.mark.parametrize("what,kw", [("4 frames per pass", dict(per_pass=4)), ("64 frames per pass", dict(per_pass=64)), ("tile order", dict(order=pod.ORDER_TILES)),
                                     ("entry points", dict(entry=True)), ("two passes in flight", dict(in_flight=2))])
def test_equal_bits_with_the_puff_in_the_frame(gpu_ctx_factory, puffy, what, kw):
    per_pass = kw.get("per_pass", 1)
    got = _cornell_run(gpu_ctx_factory, [(IN_FRAME, TR.puff())] * (64 // per_pass), frames=64, **kw)
    assert _same(got, puffy), what
    assert all(f & capi.FLAVOR_MEDIUM_GRID for f in got[2])
