"""nxhip_denoise on the device (include/nexus_hip.h): the edge-avoiding a-trous filter against its numpy restatement
(tests/aov_reference.py atrous), the invariants of the definition, and that it actually denoises.

Tolerance of the device comparison, derived here and printed: 8 x the deviation of a float32 numpy run of the same definition from
the float64 one, both measured as the largest absolute difference relative to the reference image's largest value.

It must actually denoise: Cornell box 256 x 256, 16 accumulated frames against the same context's 4 096-frame accumulation, relative
MSE of the tonemapped image over three seeds.  The bar is the ratio denoised / noisy measured on an MI355X with the default
parameters, x 1.25 for the spread between seeds: see profiles/r09_denoise.txt (sweep and measurement).
"""
import ctypes as C

import numpy as np
import pytest

from nexus_amd import pod
from tests import aov_reference as R
from tests import oracle_lib as O
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

W, H = 257, 131  # no dimension a multiple of a tile

# profiles/r09_denoise.txt: ratio of the relative MSEs (denoised / noisy) with the default parameters, mean of the three seeds
MEASURED_RATIO = 0.2327
RATIO_BAR = MEASURED_RATIO * 1.25


def _filter_ctx(factory, colour, albedo, nd, order=pod.ORDER_ROWS, w=W, h=H):
    """A context whose accumulation and feature buffers hold the given row-major images"""
    ctx = factory(w, h)
    pm = None
    if order == pod.ORDER_TILES:
        ctx.set_pixel_order(order)
        from nexus_amd import capi
        pm = capi.tile_pixel_map(w, h, 1, 0, 1, tiled=True)
    ctx.set_aov(True)
    flat = [np.ascontiguousarray(x, np.float32).reshape(w * h, -1) for x in (colour, albedo, nd)]
    if pm is not None:
        flat = [x[pm] for x in flat]
    ctx.write_accumulation(flat[0], 1)
    ctx.write_aov(flat[1], flat[2])
    return ctx


def test_device_filter_matches_the_definition(gpu_ctx_factory):
    colour, albedo, nd = R.synthetic_inputs(W, H)
    ctx = _filter_ctx(gpu_ctx_factory, colour, albedo, nd)
    p = dict(R.DEFAULTS)
    for it in (1, 2, 3, 4, 5):
        q = dict(p, iterations=it)
        want = R.atrous(colour, albedo, nd, **q, dtype=np.float64)
        single = R.atrous(colour, albedo, nd, **q, dtype=np.float32)
        tol = 8.0 * R.rel_dev(single, want)
        ctx.denoise(**q)
        got = ctx.read_denoised().reshape(H, W, 3)
        dev = R.rel_dev(got, want)
        moved = R.rel_dev(want, colour)
        print("iterations %d: device against float64 %.3g, tolerance %.3g (8 x float32 numpy's %.3g); the filter itself moves the image by %.3g" % (
            it, dev, tol, tol / 8.0, moved))
        assert np.isfinite(got).all()
        assert moved > 1e-2  # (the inputs give the filter something to do)
        assert 0.0 < tol < 1e-4 and dev <= tol


def test_definition_invariants_on_the_device(gpu_ctx_factory):
    colour, albedo, nd = R.synthetic_inputs(W, H, seed=11)
    ctx = _filter_ctx(gpu_ctx_factory, colour, albedo, nd)
    # iterations = 0 copies
    ctx.denoise(iterations=0)
    assert R.same_bits(ctx.read_denoised().reshape(H, W, 3), colour)
    # two runs: equal bits
    ctx.denoise()
    first = ctx.read_denoised()
    ctx.denoise()
    assert R.same_bits(ctx.read_denoised(), first)
    # a constant image is a fixed point, to rounding (R.FIXED_POINT_BOUND)
    const = np.empty_like(colour)
    const[...] = (0.25, 0.5, 2.0)
    ctx.write_accumulation(const.reshape(-1, 3), 1)
    ctx.denoise()
    assert np.max(np.abs(ctx.read_denoised().reshape(H, W, 3) - const)) <= R.FIXED_POINT_BOUND * 2.0
    # a hard normal edge, sigmaNormal 0.05: |dN|^2 = 2, exp(-800) = 0 — left of the edge NOTHING depends on the colours right of it
    edge = W // 2
    a2 = np.zeros_like(albedo); a2[...] = (0.5, 0.5, 0.5, 1.0)
    n2 = np.zeros_like(nd); n2[..., 3] = 4.0
    n2[:, :edge, 0] = 1.0
    n2[:, edge:, 1] = 1.0
    ctx.write_aov(a2.reshape(-1, 4), n2.reshape(-1, 4))
    other = colour.copy()
    other[:, edge:] = np.random.RandomState(9).uniform(0, 50, other[:, edge:].shape)
    outs = []
    for img in (colour, other):
        ctx.write_accumulation(img.reshape(-1, 3), 1)
        ctx.denoise(sigma_normal=0.05)
        outs.append(ctx.read_denoised().reshape(H, W, 3))
    assert R.same_bits(outs[0][:, :edge], outs[1][:, :edge])
    assert not R.same_bits(outs[0][:, edge:], outs[1][:, edge:])
    assert np.isfinite(outs[1]).all()


def test_pixel_order_does_not_matter_and_the_accumulation_is_left_alone(gpu_ctx_factory):
    colour, albedo, nd = R.synthetic_inputs(W + 7, H + 5, seed=5)  # 264 x 136: whole 8 x 8 tiles, as the tile order needs
    w, h = W + 7, H + 5
    rows = _filter_ctx(gpu_ctx_factory, colour, albedo, nd, w=w, h=h)
    tiles = _filter_ctx(gpu_ctx_factory, colour, albedo, nd, order=pod.ORDER_TILES, w=w, h=h)
    before = rows.read_accumulation(), rows.read_rgba8(), rows.read_aov()
    for it in (0, 2, 5):
        rows.denoise(iterations=it)
        tiles.denoise(iterations=it)
        assert R.same_bits(rows.read_denoised(), tiles.read_denoised())
        px = rows.read_denoised_rgba8()
        assert np.array_equal(px, tiles.read_denoised_rgba8())
        # the RGBA8 image is the tonemap of the float image
        img = rows.read_denoised()
        want = np.array([O.lib().orc_tonemap_rgba8(O._ptr(np.ascontiguousarray(img[k]))) for k in range(0, len(img), 7)], np.uint32)
        assert np.array_equal(px[::7], want)
    after = rows.read_accumulation(), rows.read_rgba8(), rows.read_aov()
    assert R.same_bits(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert R.same_bits(before[2][0], after[2][0]) and R.same_bits(before[2][1], after[2][1])


def test_parameters_are_checked(gpu_ctx_factory):
    from nexus_amd import capi
    colour, albedo, nd = R.synthetic_inputs(64, 32)
    ctx = _filter_ctx(gpu_ctx_factory, colour, albedo, nd, w=64, h=32)
    with pytest.raises(capi.NexusError, match="read_denoised"):
        ctx.read_denoised()
    for bad in (dict(iterations=7), dict(sigma_color=0.0), dict(sigma_normal=-1.0), dict(sigma_albedo=float("nan")), dict(sigma_depth=float("inf"))):
        with pytest.raises(capi.NexusError, match="nxhip_denoise"):
            ctx.denoise(**bad)
    assert ctx.L.nxhip_denoise(ctx.h, None) == 0  # NULL: the defaults
    ctx.denoise(sigma_depth=1e-30, sigma_color=1e-25)  # squares underflow: still no NaN
    assert np.isfinite(ctx.read_denoised()).all()


def _tonemapped(rgb):
    """the library's tonemap curve without the 8-bit rounding (PathTracer.cu:37-62)"""
    x = np.asarray(rgb, np.float64) * 0.6
    x = np.clip((x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14), 0.0, 1.0)
    return x ** 0.45454545454


def rel_mse(img, truth):
    a, b = _tonemapped(img), _tonemapped(truth)
    return float(np.mean((a - b) ** 2 / (b ** 2 + 1e-2)))


def measure_denoising(factory, seeds=(5000, 6000, 7000), frames=16, truth_frames=4096, params=None, size=256):
    """[(noisy rMSE, denoised rMSE)] per seed; seed = offset of the frame numbers the 16 frames are rendered with (beyond the ground truth's)"""
    sc = SH.cornell_scene(size, size, path_length=4)
    ctx = factory(size, size)
    sc.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.reset_frame_number()
    ctx.set_frames_per_pass(16)
    ctx.render(truth_frames)
    truth = ctx.read_accumulation()
    ctx.set_frames_per_pass(1)
    ctx.reset_frame_number()
    ctx.set_aov(True)
    out = []
    for seed in seeds:
        # frames seed + 1 .. seed + 16, each read back and averaged here: a 16-frame accumulation that starts anywhere in the sequence
        ctx.set_frame_number(seed)
        rad, alb, nd = [], [], []
        for _ in range(frames):
            ctx.render_frame()
            ctx.accumulate()
            rad.append(ctx.read_radiance())
            a, n = ctx.read_aov_frame()
            alb.append(a)
            nd.append(n)
        ctx.write_accumulation(R.running_mean32(rad), frames)
        ctx.write_aov(R.running_mean32(alb), R.running_mean32(nd))
        noisy = ctx.read_accumulation()
        for p in (params if isinstance(params, list) else [params]):
            ctx.denoise(**(p or {}))
            out.append((seed, p, rel_mse(noisy, truth), rel_mse(ctx.read_denoised(), truth)))
    ctx.close()
    return out


def test_it_actually_denoises(gpu_ctx_factory):
    res = measure_denoising(gpu_ctx_factory)
    ratios = []
    for seed, _p, noisy, denoised in res:
        print("seed %d: relative MSE of the tonemapped image noisy %.5f, denoised %.5f, ratio %.3f (bar %.3f)" % (seed, noisy, denoised, denoised / noisy, RATIO_BAR))
        ratios.append(denoised / noisy)
        assert denoised < noisy
    assert max(ratios) <= RATIO_BAR
