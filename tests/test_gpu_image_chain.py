"""The displayed image on the device: running mean (accumulate_kernel), tonemap and RGBA8 pack (nx_tonemap.h) against float64.

Reference: tests/image_reference.py (the curve from its definition in float64 / mpmath, the allowed 8-bit levels with a derived
band, the running mean in exact binary32 and in float64), itself held against mpmath and against the oracle's twin on the CPU by
tests/test_image_reference.py.  The device is reached through nxhip_compose_tiles (a tonemap of any float4 buffer) and
nxhip_accumulate_external (the running mean of any radiance) on caller-owned device memory (tests/hip_buffers.py), and at the end
through a real render.

Threshold neighbourhoods: the offsets are {0, +-1, +-2, +-16, +-256, +-65536} binary32 ulps, 255 x 11 = 2805 inputs.  At +-256 ulps
the reference decides levels 20 .. 246 only (21 levels stay inside the band: at low levels and at the flat top of the curve 256 ulps
move the level by less than 2e-4); at +-65536 ulps it decides every level.  Both facts are asserted for the reference before the
device is looked at.
"""
import numpy as np
import pytest

from nexus_amd import pod
from tests import image_reference as R
from tests import oracle_lib as O
from tests import scene_helpers as SH
from tests.hip_buffers import DeviceBuffers

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL8 = 0x5A17C3E9
SENTINEL_ACC = f32(-7777.25)


def _float4(rgb, w=np.nan):
    rgb = np.asarray(rgb, f32).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([rgb, np.full((len(rgb), 1), w, f32)], axis=1))


def _oracle_tonemap(rgb4):
    rgb4 = np.ascontiguousarray(rgb4, f32)
    L = O.lib()
    return np.array([L.orc_tonemap_rgba8(O._ptr(rgb4[i])) for i in range(len(rgb4))], np.uint32)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _subset_permutation(n_full, count, seed):
    """`count` distinct pixels of n_full in a seeded order"""
    return np.ascontiguousarray(np.random.default_rng(seed).permutation(n_full)[:count], np.uint32)


def _compose(ctx, dev, src4, dst_map=None, rgba8=True):
    """nxhip_compose_tiles of src4 (count, 4) into sentinel-filled full-image buffers -> (accumulation (n_full, 4), rgba8 (n_full,))"""
    n_full = ctx.width * ctx.height
    assert len(src4) <= n_full and (dst_map is None or (len(dst_map) == len(src4) and int(dst_map.max()) < n_full))
    d_acc = dev.upload(np.full((n_full, 4), SENTINEL_ACC, f32))
    d_px = dev.upload(np.full(n_full, SENTINEL8, np.uint32))
    ctx.compose_tiles(dev.upload(src4), len(src4), dev.upload(dst_map) if dst_map is not None else None, d_acc, d_px if rgba8 else None)
    ctx.sync()
    return dev.download(d_acc, (n_full, 4), f32), dev.download(d_px, n_full, np.uint32)


def _assert_display(rgb, rgba8, what, cap=None):
    bad, undecided = R.display_check(rgb, rgba8)
    print("%s: %d pixels, undecided share %.4f" % (what, len(np.asarray(rgb).reshape(-1, 3)), undecided))
    rgb = np.asarray(rgb, f32).reshape(-1, 3)
    assert not bad, "%s: (radiance, packed) outside the allowed levels: %r" % (what, [(float(rgb[i, k % 3]), hex(int(np.asarray(rgba8).reshape(-1)[i]))) for i, k in bad[:8]])
    if cap is not None:
        assert undecided <= cap, what
    return undecided


# ---- (a) the tonemap -----------------------------------------------------------------------------------------


def test_tonemap_thresholds_through_a_scatter(gpu_ctx_factory):
    """Every level's threshold and its neighbourhood, the channels of a pixel at different levels; count = 2805 (no multiple of
    the block) through a dstMap that is a permutation of a subset; pixels outside the map keep their bytes."""
    W, H = 64, 48
    T = R.threshold_inputs()
    lo, hi = R.levels_allowed(T)
    col = {o: j for j, o in enumerate(R.ULP_OFFSETS)}
    L = np.arange(1, 256)
    # the reference first: decided where the offsets are far enough, so the check below cannot pass by leaving everything out
    assert np.array_equal(lo[:, col[65536]], L) and np.array_equal(hi[:, col[65536]], L)
    assert np.array_equal(lo[:, col[-65536]], L - 1) and np.array_equal(hi[:, col[-65536]], L - 1)
    assert np.array_equal(lo[19:246, col[256]], L[19:246]) and np.array_equal(hi[19:246, col[256]], L[19:246])
    assert np.array_equal(lo[19:246, col[-256]], L[19:246] - 1) and np.array_equal(hi[19:246, col[-256]], L[19:246] - 1)

    rgb = R.rotate_channels(T.reshape(-1))
    assert len(rgb) == 2805
    src = _float4(rgb)
    dst_map = _subset_permutation(W * H, len(src), seed=31)
    ctx = gpu_ctx_factory(W, H)
    with DeviceBuffers() as dev:
        acc, px = _compose(ctx, dev, src, dst_map)
        acc_only, px_untouched = _compose(ctx, dev, src, dst_map, rgba8=False)
    _assert_display(rgb, px[dst_map], "thresholds on the device")
    assert np.array_equal(px[dst_map], _oracle_tonemap(src))  # device and oracle, bit for bit
    # the copy is the source, the fourth component included; with no RGBA8 destination the copy alone is written
    assert np.array_equal(_bits(acc[dst_map]), _bits(src)) and np.array_equal(_bits(acc_only), _bits(acc))
    assert np.all(px_untouched == SENTINEL8)
    outside = np.setdiff1d(np.arange(W * H), dst_map)
    assert len(outside) == W * H - 2805
    assert np.all(px[outside] == SENTINEL8) and np.all(acc[outside] == SENTINEL_ACC)


@pytest.mark.parametrize("name", ["log", "uniform"])
def test_tonemap_sweeps(gpu_ctx_factory, name):
    """3000 radiances log-spaced over [1e-30, 1e19] / uniform on [0, 13]: allowed levels, decided ones exact, and along the log
    sweep (spacing far above an ulp) no step down"""
    W, H = 64, 48
    values = R.log_sweep() if name == "log" else R.uniform_sweep()
    rgb = R.rotate_channels(values)
    grey = np.repeat(values[:, None], 3, axis=1)
    ctx = gpu_ctx_factory(W, H)
    with DeviceBuffers() as dev:
        _, px = _compose(ctx, dev, _float4(rgb))
        _, px_grey = _compose(ctx, dev, _float4(grey))
    _assert_display(rgb, px[:3000], "%s sweep on the device" % name, cap=R.UNDECIDED_CAP)
    _assert_display(grey, px_grey[:3000], "%s sweep, grey, on the device" % name, cap=R.UNDECIDED_CAP)
    assert np.array_equal(px[:3000], _oracle_tonemap(_float4(rgb))) and np.array_equal(px_grey[:3000], _oracle_tonemap(_float4(grey)))
    assert np.all(px[3000:] == SENTINEL8)
    lv, _ = R.unpack_levels(px_grey[:3000])
    assert np.array_equal(lv[:, 0], lv[:, 1]) and np.array_equal(lv[:, 0], lv[:, 2])  # the three channels are one text
    if name == "log":
        assert np.all(np.diff(lv[:, 0]) >= 0) and lv[0, 0] == 0 and lv[-1, 0] == 255


def test_tonemap_specials(gpu_ctx_factory):
    """The table of the display contract (nx_tonemap.h), one pixel per row and channel, NaN in the fourth component.
    With the text before the saturation the rows R.SPECIALS_OVERFLOW (2e19 and brighter, +inf) display 0 and fail here."""
    W, H = 64, 48
    rgb, want = R.special_pixels()
    special = want >= 0
    src = _float4(rgb)
    plain = _float4(np.array([R.SPECIAL_COMPANIONS + (0.0,)], f32))
    ctx = gpu_ctx_factory(W, H)
    with DeviceBuffers() as dev:
        _, px = _compose(ctx, dev, np.concatenate([src, plain]))
    lv, alpha = R.unpack_levels(px[:len(src) + 1])
    wrong = [(float(rgb[i][special[i]][0]), int(lv[i][special[i]][0]), int(want[i][special[i]][0])) for i in range(len(rgb)) if lv[i][special[i]][0] != want[i][special[i]][0]]
    assert not wrong, "(radiance, level on the device, level of the table): %r" % wrong
    assert np.all(alpha == 255)
    for i in range(len(rgb)):  # a special in one channel does not change the other two
        assert lv[i][~special[i]].tolist() == lv[-1][:2].tolist(), rgb[i]
    _assert_display(rgb, px[:len(src)], "the table on the device")
    assert np.array_equal(px[:len(src)], _oracle_tonemap(src))


# ---- (b) the running mean ------------------------------------------------------------------------------------


def _radiance4(frames, stride):
    """(slices, count, 3) -> the external layout [slices][stride] of float4: NaN in every fourth component and in the padding"""
    slices, count, _ = frames.shape
    out = np.full((slices, stride, 4), np.nan, f32)
    out[:, :count, :3] = frames
    return out


def _state(ctx, dev):
    """the context's full accumulation as float4 (fourth component included) and its RGBA8 image"""
    n_full = ctx.width * ctx.height
    ctx.sync()
    return dev.download(ctx.accumulation_device_ptr(), (n_full, 4), f32, capacity=n_full * 16), ctx.read_full_rgba8()


def _fill_accumulation_with_nan(ctx, dev):
    """the context's accumulation, fourth component included, straight through its device pointer"""
    n_full = ctx.width * ctx.height
    ctx.sync()  # (nothing the context has queued may land after the copy)
    dev.write(ctx.accumulation_device_ptr(), np.full((n_full, 4), np.nan, f32), capacity=n_full * 16)


def _nan_agnostic_equal(a, b):
    """bit-equal, except that any NaN equals any NaN (sign and payload of a NaN that arithmetic produced are the hardware's choice)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def test_running_mean_grid(gpu_ctx_factory):
    """slices x sliceStride x firstFrame x dstMap: accumulation bit-equal to the binary32 statement, RGBA8 per the tonemap contract,
    padding never read, pixels outside the map untouched, and the float64 mean within 8 x what binary32 costs"""
    W, H = 67, 3
    n_full = W * H
    ctx = gpu_ctx_factory(W, H)
    seed = 100
    points = 0
    with DeviceBuffers() as dev:
        for mapped in (False, True):  # (unmapped first: the mapped points then find an image that is not the one they write)
            count = 150 if mapped else n_full
            dst_map = _subset_permutation(n_full, count, seed=77) if mapped else None
            d_map = dev.upload(dst_map) if mapped else None
            idx = dst_map if mapped else np.arange(n_full)
            for first in (1, 2, 7):
                for slices in (1, 2, 5):
                    for stride in (count, count + 13):
                        seed += 1
                        frames = R.heavy_tail_radiance(slices, count, seed)
                        if first > 1:
                            start = R.running_mean32(R.heavy_tail_radiance(first - 1, n_full, seed + 1000))
                            ctx.write_accumulation(start, first - 1)
                        else:  # the result must not depend on what the accumulation held: NaN, fourth component included
                            start = np.full((n_full, 3), np.nan, f32)
                            _fill_accumulation_with_nan(ctx, dev)
                        acc0, px0 = _state(ctx, dev)
                        src = _radiance4(frames, stride)
                        assert src.shape[0] * src.shape[1] >= (slices - 1) * stride + count
                        ctx.accumulate_external(dev.upload(src), count, first, d_map, slices=slices, slice_stride=stride)
                        acc, px = _state(ctx, dev)
                        what = "map %s, first frame %d, %d slices, stride %d" % (mapped, first, slices, stride)

                        want = R.running_mean32(frames, first, start[idx])
                        assert np.array_equal(_bits(acc[idx, :3]), _bits(want)), what
                        assert np.all(_bits(acc[idx, 3]) == 0), what  # the fourth component stays 0
                        assert np.array_equal(_bits(ctx.read_full_accumulation()[idx]), _bits(want)), what
                        assert np.isfinite(acc[idx]).all(), what  # neither the padding nor the pre-fill shows
                        bad, _ = R.display_check(want, px[idx])
                        assert not bad, (what, bad[:8])
                        assert np.array_equal(px[idx], _oracle_tonemap(_float4(want))), what
                        outside = np.setdiff1d(np.arange(n_full), idx)
                        assert len(outside) == n_full - count
                        assert np.array_equal(_bits(acc[outside]), _bits(acc0[outside])) and np.array_equal(px[outside], px0[outside]), what
                        if mapped:
                            assert not np.array_equal(px[idx], px0[idx]), what  # (the image was another one before)
                        ok, deviation, bar = R.mean_within_bar(acc[idx, :3], frames, first, start[idx])
                        assert ok, (what, deviation, bar)
                        points += 1
    assert points == 36


def test_running_mean_long_run_and_large_frame_numbers(gpu_ctx_factory):
    """One call with 4096 slices of heavy-tailed radiance; and five frames from 2^24 - 2 on, where float(frame) rounds"""
    W, H = 64, 1
    ctx = gpu_ctx_factory(W, H)
    frames = R.heavy_tail_radiance(4096, W, seed=11)
    with DeviceBuffers() as dev:
        _fill_accumulation_with_nan(ctx, dev)
        ctx.accumulate_external(dev.upload(_radiance4(frames, W)), W, 1, None, slices=4096, slice_stride=W)
        acc = ctx.read_full_accumulation()
        px = ctx.read_full_rgba8()
        want = R.running_mean32(frames)
        assert np.array_equal(_bits(acc), _bits(want))
        ok, deviation, bar = R.mean_within_bar(acc, frames)
        print("running mean on the device, 4096 slices x %d pixels: relative deviation from float64 %.3g (bar %.3g = 8 x the binary32 statement's)" % (W, deviation, bar))
        assert ok
        assert not R.display_check(want, px)[0]

        first = 2 ** 24 - 2
        start = R.running_mean32(R.heavy_tail_radiance(3, W, seed=10))
        late = R.heavy_tail_radiance(5, W, seed=9)
        ctx.write_accumulation(start, first - 1)
        ctx.accumulate_external(dev.upload(_radiance4(late, W + 5)), W, first, None, slices=5, slice_stride=W + 5)
        want = R.running_mean32(late, first, start)
        assert np.array_equal(_bits(ctx.read_full_accumulation()), _bits(want))
        assert not np.array_equal(_bits(want), _bits(start))
        # one frame per call is the same run
        ctx.write_accumulation(start, first - 1)
        for k in range(5):
            ctx.accumulate_external(dev.upload(_radiance4(late[k:k + 1], W)), W, first + k, None)
        assert np.array_equal(_bits(ctx.read_full_accumulation()), _bits(want))


def test_non_finite_samples_stay_in_their_channel(gpu_ctx_factory):
    """One +inf, one NaN and one 3e38 sample in frame 1, three further frames: every other pixel and channel is bit-equal to the
    run without them; the poisoned channels follow the binary32 statement (inf, then NaN for good; 3e38 stays finite) and are
    displayed per the table.  This pins what the accumulation does today; rejecting such samples is another feature."""
    W, H = 67, 3
    n = W * H
    clean = R.heavy_tail_radiance(4, n, seed=21)
    poisoned = clean.copy()
    spots = ((5, 0, np.inf), (70, 1, np.nan), (140, 2, 3e38))
    for p, k, v in spots:
        poisoned[0, p, k] = v
    mask = np.zeros((n, 3), bool)
    for p, k, _ in spots:
        mask[p, k] = True
    runs = []
    with DeviceBuffers() as dev:
        for rad in (clean, poisoned):
            ctx = gpu_ctx_factory(W, H)
            states = []
            for f in range(4):
                ctx.accumulate_external(dev.upload(_radiance4(rad[f:f + 1], n)), n, f + 1, None)
                states.append((ctx.read_full_accumulation(), ctx.read_full_rgba8()))
            runs.append(states)
    for f in range(4):
        (acc_c, px_c), (acc_p, px_p) = runs[0][f], runs[1][f]
        want = R.running_mean32(poisoned[:f + 1])
        assert np.array_equal(_bits(acc_p)[~mask], _bits(acc_c)[~mask]), f
        assert np.array_equal(_bits(acc_c), _bits(R.running_mean32(clean[:f + 1]))), f
        assert _nan_agnostic_equal(acc_p, want), f
        lv_c, _ = R.unpack_levels(px_c)
        lv_p, alpha = R.unpack_levels(px_p)
        assert np.array_equal(lv_p[~mask], lv_c[~mask]) and np.all(alpha == 255), f
        assert not R.display_check(acc_p, px_p)[0], f
        # the table: +inf 255 (frame 1), NaN 0, a finite 3e38 / (f + 1) far above the clamp 255
        assert lv_p[5, 0] == (255 if f == 0 else 0) and lv_p[70, 1] == 0 and lv_p[140, 2] == 255, f
    a = runs[1][3][0]
    assert np.isnan(a[5, 0]) and np.isnan(a[70, 1]) and np.isfinite(a[140, 2])
    assert np.isposinf(runs[1][0][0][5, 0])


# ---- (c) the chain on a real render ----------------------------------------------------------------------


def test_rendered_image_satisfies_the_display_contract(gpu_ctx_factory):
    W, H = 64, 48
    scene = SH.cornell_scene(W, H, path_length=3)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.reset_frame_number()
    ctx.set_aov(True)
    for _ in range(3):
        ctx.render_frame()
        ctx.accumulate()
    acc, px = ctx.read_accumulation(), ctx.read_rgba8()
    assert np.isfinite(acc).all() and acc.max() > 0
    _assert_display(acc, px, "rendered image", cap=R.UNDECIDED_CAP)
    ctx.denoise()
    den, px_den = ctx.read_denoised(), ctx.read_denoised_rgba8()
    assert not np.array_equal(_bits(den), _bits(acc))
    _assert_display(den, px_den, "denoised image", cap=R.UNDECIDED_CAP)
    assert len(np.unique(R.unpack_levels(px)[0])) > 50  # (a picture, not a flat field)
