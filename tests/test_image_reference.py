"""The display reference (tests/image_reference.py) held against mpmath, and the oracle's tonemap held against the reference.

No GPU.  The device runs the same checks on the same inputs in tests/test_gpu_image_chain.py."""
import numpy as np
import pytest

from tests import aov_reference as AOV
from tests import image_reference as R
from tests import oracle_lib as O

f32 = np.float32


def oracle_tonemap(rgb):
    rgb = np.ascontiguousarray(rgb, f32).reshape(-1, 3)
    L = O.lib()
    return np.array([L.orc_tonemap_rgba8(O._ptr(rgb[i])) for i in range(len(rgb))], np.uint32)


# ---- the reference against mpmath --------------------------------------------------------------------------


def test_level64_agrees_with_50_digits():
    th = R.level_thresholds()
    assert len(th) == 255
    assert all(b > a for a, b in zip(th, th[1:])) and th[0] > 0  # strictly increasing
    assert abs(float(th[-1]) - 12.0694) < 1e-4  # the curve's clamp
    # at the thresholds the 50-digit level is the integer, and float64 agrees to its own precision
    worst = 0.0
    for L, c in enumerate(th, start=1):
        assert abs(R.level_mp(c, clamp=False) - L) < 1e-40, L
        worst = max(worst, abs(float(R.level64(float(c))) - L))
    rng = np.random.default_rng(7)
    sweep = np.concatenate([10.0 ** rng.uniform(-30, 19, 300), rng.uniform(0, 13, 300), -(10.0 ** rng.uniform(-6, 18, 50))])
    for c in sweep:
        worst = max(worst, abs(float(R.level64(c)) - float(R.level_mp(float(c)))))
    print("level64 against 50 digits: worst %.3g of a level (band %.3g)" % (worst, R.BAND))
    assert worst < 1e-9  # float64: 2^-53 relative per operation, a dozen operations, 255 levels: 4e-13


def test_band_derived_and_measured():
    """the band's derivation in numbers, and the measurement that stands beside it: binary32 numpy against level64"""
    rng = np.random.default_rng(1)
    c = np.concatenate([10.0 ** rng.uniform(-6, 3, 200000), rng.uniform(0, 13, 200000)]).astype(f32)
    x = c * f32(0.6)
    q = (x * (f32(2.51) * x + f32(0.03))) / (x * (f32(2.43) * x + f32(0.59)) + f32(0.14))
    q = np.clip(q, f32(0), f32(1))
    y = (q.astype(np.float64) ** R.EXPONENT).astype(f32) * f32(255.0)
    measured = float(np.max(np.abs(y.astype(np.float64) - R.level64(c))))
    print("band: derived %.3g of a level, used %.3g; binary32 against float64 on %d radiances: %.3g (on 4 million: %.3g)"
          % (R.BAND_DERIVED, R.BAND, len(c), measured, R.BAND_MEASURED))
    assert abs(R.BAND_DERIVED - 1.478e-4) < 1e-7 and R.BAND_DERIVED <= R.BAND
    assert measured <= R.BAND_DERIVED
    # and on these inputs no decided level of the binary32 statement mismatches
    lo, hi = R.levels_allowed(c)
    lv = np.floor(y).astype(np.int64)
    assert np.all((lv >= lo) & (lv <= hi))


def test_allowed_sets_at_the_edges():
    lo, hi = R.levels_allowed(np.array([0.0, -0.0, 13.0, float("inf"), float("nan"), float("-inf"), -1.0, -3e38, -1.95e19, -1.9e19], np.float64))
    assert lo.tolist() == [0, 0, 255, 255, 0, 0, 255, 0, 0, 255]
    assert hi.tolist() == [0, 0, 255, 255, 0, 0, 255, 0, 255, 255]
    # a threshold itself is undecided by construction, and its two candidates are L - 1 and L
    th = np.array([float(c) for c in R.level_thresholds()])
    lo, hi = R.levels_allowed(th)
    assert np.array_equal(lo, np.arange(0, 255)) and np.array_equal(hi, np.arange(1, 256))


def test_threshold_inputs_are_decided_where_they_are_far_enough():
    """2^16 ulps away from a threshold every level is decided, and on the side the offset says; 256 ulps away the levels 20 .. 246
    are (below them, and at the flat top, 256 ulps move the level by less than the band: 21 levels stay undecided there)"""
    T = R.threshold_inputs()
    assert T.shape == (255, 11) and T.size == 2805
    lo, hi = R.levels_allowed(T)
    L = np.arange(1, 256)
    col = {o: j for j, o in enumerate(R.ULP_OFFSETS)}
    assert np.array_equal(lo[:, col[65536]], L) and np.array_equal(hi[:, col[65536]], L)
    assert np.array_equal(lo[:, col[-65536]], L - 1) and np.array_equal(hi[:, col[-65536]], L - 1)
    mid = slice(19, 246)  # levels 20 .. 246
    assert np.array_equal(lo[mid, col[256]], L[mid]) and np.array_equal(hi[mid, col[256]], L[mid])
    assert np.array_equal(lo[mid, col[-256]], L[mid] - 1) and np.array_equal(hi[mid, col[-256]], L[mid] - 1)
    print("thresholds: levels undecided at +256 ulps: %s" % (np.flatnonzero(lo[:, col[256]] != hi[:, col[256]]) + 1).tolist())


# ---- the oracle twin ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["thresholds", "log", "uniform"])
def test_oracle_tonemap_lies_in_the_allowed_set(name):
    values = {"thresholds": lambda: R.threshold_inputs().reshape(-1), "log": R.log_sweep, "uniform": R.uniform_sweep}[name]()
    rgb = R.rotate_channels(values)
    out = oracle_tonemap(rgb)
    bad, undecided = R.display_check(rgb, out)
    print("oracle tonemap, %s: %d pixels, undecided share %.4f" % (name, len(rgb), undecided))
    assert not bad, [(rgb[i, k % 3], hex(out[i])) for i, k in bad[:8]]
    if name != "thresholds":  # (the neighbourhoods of the thresholds are undecided by construction: membership only)
        assert undecided <= R.UNDECIDED_CAP
    if name == "log":
        lv, _ = R.unpack_levels(oracle_tonemap(np.repeat(values[:, None], 3, axis=1)))
        assert np.all(np.diff(lv[:, 0]) >= 0) and lv[0, 0] == 0 and lv[-1, 0] == 255


def test_oracle_specials():
    """the table of the display contract (nx_tonemap.h), one pixel per row and channel; a special value in one channel leaves the
    other two alone; the fourth component of the input is not read"""
    rgb, want = R.special_pixels()
    lo, hi = R.levels_allowed(rgb)
    special = want >= 0
    assert np.array_equal(lo[special], want[special]) and np.array_equal(hi[special], want[special])  # the reference says what the table says
    rgba = np.concatenate([rgb, np.full((len(rgb), 1), np.nan, f32)], axis=1)
    L = O.lib()
    out = np.array([L.orc_tonemap_rgba8(O._ptr(rgba[i])) for i in range(len(rgba))], np.uint32)
    lv, alpha = R.unpack_levels(out)
    wrong = [(float(rgb[i][special[i]][0]), int(lv[i][special[i]][0]), int(want[i][special[i]][0])) for i in range(len(rgb)) if lv[i][special[i]][0] != want[i][special[i]][0]]
    assert not wrong, "(radiance, level, level of the table): %r" % wrong
    assert np.all(alpha == 255)
    plain = R.unpack_levels(oracle_tonemap(np.array([R.SPECIAL_COMPANIONS + (0.0,)], f32)))[0][0][:2]
    for i in range(len(rgb)):
        assert lv[i][~special[i]].tolist() == plain.tolist(), rgb[i]
    bad, _ = R.display_check(rgb, out)
    assert not bad


# ---- running means -----------------------------------------------------------------------------------------


def test_running_mean32_extends_the_feature_buffers_reference():
    rad = R.heavy_tail_radiance(9, 50, seed=3)
    assert R.same_bits(R.running_mean32(rad), AOV.running_mean32(list(rad)))
    # a run split in two, the second part started from the first part's result, is the same run
    for cut in (1, 4, 8):
        head = R.running_mean32(rad[:cut])
        assert R.same_bits(R.running_mean32(rad[cut:], cut + 1, head), R.running_mean32(rad))
    # with first frame 1 the starting value is not read
    assert R.same_bits(R.running_mean32(rad, 1, np.full((50, 3), np.nan, f32)), R.running_mean32(rad))
    m = R.running_mean64(rad)
    assert np.allclose(R.running_mean64(rad[4:], 5, R.running_mean64(rad[:4])), m, rtol=1e-14, atol=0)
    assert np.allclose(m, rad.astype(np.float64).mean(axis=0), rtol=1e-14, atol=0)


def test_long_run_drift_of_the_binary32_running_mean():
    """4096 frames of heavy-tailed radiance: how far the binary32 update drifts from the float64 mean.  The figure is the
    reference's own; the device is held to 8 x it (tests/test_gpu_image_chain.py)."""
    rad = R.heavy_tail_radiance(4096, 256, seed=11)
    dev = R.relative_deviation(R.running_mean32(rad), R.running_mean64(rad))
    print("running mean, 4096 frames x 256 pixels, binary32 against float64: largest relative deviation %.3g" % dev)
    # each update rounds three times (difference, quotient, sum) relative to values of the mean's size or, for the difference, the
    # sample's; the errors of 4096 updates add up at worst linearly: 3 * 4096 * 2^-24 = 7.3e-4, and as a random walk to about
    # sqrt(3 * 4096) * 2^-24 = 6.6e-6.  Measured with this seed: 3.7e-6.
    assert 0 < dev < 3 * 4096 * 2.0 ** -24


def test_off_by_one_frame_counter_is_refused():
    rad = R.heavy_tail_radiance(5, 201, seed=5)
    ok, dev, bar = R.mean_within_bar(R.running_mean32(rad), rad)
    assert ok and dev * R.MEAN_BAR_FACTOR == bar
    # the frame numbers one too high: frame 1 folded as "frame 2" into an accumulation of zeros, and so on
    late = R.running_mean32(rad, 2, np.zeros((201, 3), f32))
    ok, dev, bar = R.mean_within_bar(late, rad)
    print("off-by-one frame counter at 5 frames: deviation %.3g against a bar of %.3g" % (dev, bar))
    assert not ok and dev > 1000 * bar
    # ... and one too low from the second frame on (frame 2 folded as frame 1 replaces the mean)
    early = R.running_mean32(rad[1:], 1)
    assert not R.mean_within_bar(early, rad)[0]
    # with a start: frames 7 .. 11 counted as 8 .. 12
    start = R.running_mean32(R.heavy_tail_radiance(6, 201, seed=6))
    assert R.mean_within_bar(R.running_mean32(rad, 7, start), rad, 7, start)[0]
    assert not R.mean_within_bar(R.running_mean32(rad, 8, start), rad, 7, start)[0]


def test_frame_numbers_at_the_edge_of_binary32_integers():
    """float(frame) rounds from 2^24 on: the binary32 statement divides by what the conversion gives, not by the integer"""
    first = 2 ** 24 - 2
    assert [float(f32(first + k)) for k in range(5)] == [16777214.0, 16777215.0, 16777216.0, 16777216.0, 16777218.0]
    rad = R.heavy_tail_radiance(5, 64, seed=9)
    start = R.running_mean32(R.heavy_tail_radiance(3, 64, seed=10))
    a = start.copy()
    for k in range(5):
        a = a + (rad[k] - a) / f32(float(f32(first + k)))
    assert R.same_bits(R.running_mean32(rad, first, start), a)


def test_non_finite_samples_in_the_binary32_statement():
    """+inf stays +inf for its frame and is NaN from the next one on; 3e38 stays finite; NaN stays NaN"""
    r = np.ones((4, 3), f32)
    r[0] = (np.inf, np.nan, 3e38)
    a1, a2, a4 = R.running_mean32(r[:1]), R.running_mean32(r[:2]), R.running_mean32(r)
    assert np.isposinf(a1[0]) and np.isnan(a1[1]) and a1[2] == f32(3e38)
    assert np.isnan(a2[0]) and np.isnan(a2[1]) and np.isfinite(a2[2])
    assert np.isnan(a4[0]) and np.isnan(a4[1]) and np.isfinite(a4[2])
