"""The displayed image from the definition: running mean, tonemap curve, 8-bit level.  float64 and mpmath; shares no text with
nx_tonemap.h or the oracle.

TEST INFRASTRUCTURE ONLY.  The definition (PathTracer.cu:37-62, 480-496; Utils/Utils.h:51-54), per colour channel c:

    x = 0.6 c       N = x (2.51 x + 0.03)       D = x (2.43 x + 0.59) + 0.14
    y = 255 clip(N / D, 0, 1) ** 0.45454545454          the real-valued level            (level64)
    the byte written is floor(y), as a binary32 evaluation rounds y                      (levels_allowed)

N / D increases strictly on c >= 0 (d/dx: (1.408 x^2 + 0.7028 x + 0.0042) / D^2 > 0), from 0 at c = 0 through 1 at the curve's
clamp, x = (0.56 + sqrt(0.3584)) / 0.16 = 7.2417, c = 12.0694, towards 2.51 / 2.43.  D has no real root (0.59^2 < 4 * 2.43 * 0.14),
so there is no pole for negative c either.

The band.  levels_allowed admits floor of every point of [y - BAND, y + BAND].  BAND bounds how far a CORRECT binary32 evaluation
can lie from y, for c >= 0, where every term of N and D is positive and no subtraction amplifies an error: a sum or product of
values with relative errors e1, e2 has at most max(e1, e2) (sum) or e1 + e2 (product), plus its own rounding u = 2^-24.  To first
order the relative errors simply add up, so they are counted:

    ahead of the power
      the product with 0.6            1 rounding + the constant 0.6f (not a binary32 number: up to u)           = 2
        ... and N / D answers a relative change of x with at most twice that (N grows like x .. x^2, D like
        1 .. x^2: the elasticity of N / D lies in [-1, 2])                                                        x 2  -> 4
      N: 2.51 x, + 0.03, the product with x       3 roundings + the constants 2.51f, 0.03f                       = 5
      D: 2.43 x, + 0.59, the product with x, + 0.14   4 roundings + the constants 2.43f, 0.59f, 0.14f            = 7
      the division                                                                                               = 1
                                                                                                            sum  = 17
      the exponent 0.45454545454 damps them: 17 * 0.45454545454                                                  = 7.73
    after the power
      nxf_pow's result rounded to float, the product with 255                                                    = 2
      (nxf_pow itself works in binary64: 1e-16, not counted; the first clamp is exact)
                                                                                                          total  = 9.73 u

9.73 * 2^-24 = 5.8e-7 relative, times at most 255 levels: BAND_DERIVED = 1.48e-4 of a level, rounded up to BAND = 2e-4 (the figure
the band was specified at).  MEASURED: a numpy binary32 statement of the same operations against level64 on 4 million radiances
(log-uniform over [1e-6, 1e3] and uniform over [0, 13]) deviates by at most 4.2e-5 of a level; tests/test_image_reference.py repeats
that measurement on 400 000 and prints it.  Where the unclamped N / D is above 1 + 1e-6 (nine roundings ahead of the clamp: 5.4e-7)
the clamp decides and the level is exactly 255; below -1e-6 exactly 0.

Outside c >= 0 the curve is "what it is" and the specials are pinned by the display contract of nx_tonemap.h:

    NaN, -inf                                  0
    c <= -1.98e19                              0     both polynomials overflow in binary32, inf / inf = NaN, which displays 0
    -1.98e19 < c < -1.93e19                    0 or 255: N overflows at 0.6 |c| = sqrt(FLT_MAX / 2.51) = 1.164e19 (c = 1.941e19),
                                               D only at sqrt(FLT_MAX / 2.43) = 1.183e19 (c = 1.972e19); between them inf / D = 255
    finite c < 0 above that                    the band rule (N / D > 1 below c = -0.0199 .. : -1 displays 255); the band's derivation
                                               does not cover the cancellation in 2.51 x + 0.03 near x = -0.012, where N / D is
                                               within 1e-6 of 0 and the level is 0 either way
    c above the clamp, FLT_MAX, +inf           255   (N / D -> 2.51 / 2.43)
"""
import functools

import numpy as np

f32 = np.float32

EXPONENT = 0.45454545454
ROUNDINGS_AHEAD_OF_POW = 17  # the docstring's count
ROUNDINGS_AFTER_POW = 2
BAND_DERIVED = (ROUNDINGS_AHEAD_OF_POW * EXPONENT + ROUNDINGS_AFTER_POW) * 2.0 ** -24 * 255.0  # 1.48e-4 of a level
BAND = 2e-4
BAND_MEASURED = 4.2e-5  # numpy binary32 against level64, 4 million radiances (see above)
assert BAND_DERIVED <= BAND
SATURATED = 1e-6  # N / D beyond [0, 1] by more than this: the clamp decides
UNDECIDED_CAP = 0.01  # of a sweep
NEG_OVERFLOW_BOTH = -1.98e19  # at and below: N and D overflow in binary32
NEG_OVERFLOW_ANY = -1.93e19  # above: neither does


def quotient64(c):
    """the unclamped N / D in float64; +-inf: the limit 2.51 / 2.43; NaN stays NaN"""
    c = np.asarray(c, np.float64)
    x = 0.6 * c
    with np.errstate(invalid="ignore", over="ignore"):
        q = (x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)  # (a binary32 radiance squared stays far inside binary64)
    return np.where(np.isinf(c), 2.51 / 2.43, q)


def level64(rgb):
    """the real-valued level per channel, 255 clip(N / D, 0, 1) ** 0.45454545454 (NaN for a NaN)"""
    return 255.0 * np.clip(quotient64(rgb), 0.0, 1.0) ** EXPONENT


def levels_allowed(rgb, band=BAND):
    """(lo, hi), int arrays shaped like rgb: the 8-bit values lo .. hi are what a correct binary32 evaluation may write for the channel.
    An input is DECIDED where lo == hi."""
    c = np.asarray(rgb, np.float64)
    q = quotient64(c)
    y = 255.0 * np.clip(np.nan_to_num(q, nan=0.0), 0.0, 1.0) ** EXPONENT
    lo = np.floor(np.clip(y - band, 0.0, 255.0)).astype(np.int64)
    hi = np.floor(np.clip(y + band, 0.0, 255.0)).astype(np.int64)
    up, down = q > 1.0 + SATURATED, q < -SATURATED
    lo, hi = np.where(up, 255, lo), np.where(up, 255, hi)
    lo, hi = np.where(down, 0, lo), np.where(down, 0, hi)
    # the pinned specials
    black = np.isnan(c) | (c <= NEG_OVERFLOW_BOTH)
    either = (c > NEG_OVERFLOW_BOTH) & (c < NEG_OVERFLOW_ANY)
    lo, hi = np.where(black | either, 0, lo), np.where(black, 0, np.where(either, 255, hi))
    return lo, hi


def unpack_levels(rgba8):
    """uint32 RGBA8 (n,) -> (levels (n, 3) int64, alpha (n,) int64); channel k sits at bits 8 k"""
    p = np.asarray(rgba8, np.uint32).astype(np.int64).reshape(-1)
    return np.stack([(p >> (8 * k)) & 0xFF for k in range(3)], axis=1), (p >> 24) & 0xFF


def display_check(rgb, rgba8, band=BAND):
    """The tonemap contract applied to rgb (n, 3) float32 against the packed image rgba8 (n,).
    -> (bad, undecided): bad = indices (pixel, channel) whose level is outside the allowed set (a decided input: not the exact level),
    plus (pixel, 3) where alpha is not 255; undecided = the share of channels whose allowed set has two elements."""
    rgb = np.asarray(rgb, f32).reshape(-1, 3)
    got, alpha = unpack_levels(rgba8)
    assert got.shape == rgb.shape, (got.shape, rgb.shape)
    lo, hi = levels_allowed(rgb, band)
    bad = [tuple(ix) for ix in np.argwhere((got < lo) | (got > hi))] + [(int(i), 3) for i in np.flatnonzero(alpha != 255)]
    return bad, float(np.mean(lo != hi))


# ---- mpmath ------------------------------------------------------------------------------------------------


def _mp():
    import mpmath

    return mpmath


def level_mp(c, clamp=True):
    """the level of radiance c (a float, an mpf or a string) at 50 digits; clamp=False: N / D is not clipped above 1 (bisection)"""
    mp = _mp()
    with mp.workdps(50):
        x = mp.mpf("0.6") * mp.mpf(c)
        q = (x * (mp.mpf("2.51") * x + mp.mpf("0.03"))) / (x * (mp.mpf("2.43") * x + mp.mpf("0.59")) + mp.mpf("0.14"))
        q = max(q, mp.mpf(0))
        if clamp:
            q = min(q, mp.mpf(1))
        return 255 * mp.power(q, mp.mpf("0.45454545454"))


@functools.lru_cache(maxsize=None)
def level_thresholds():
    """c_L for L = 1 .. 255 with level(c_L) = L, as a tuple of mpf: bisection at 50 digits on the strictly increasing unclamped curve.
    c_255 is the curve's clamp, about 12.0694.  (level = L is bisected as N / D = (L / 255) ** (1 / 0.45454545454): the same equation,
    with the power taken once per level instead of once per step; test_image_reference.py holds the result against level_mp.)"""
    mp = _mp()
    out = []
    with mp.workdps(50):
        k = [mp.mpf(s) for s in ("0.6", "2.51", "0.03", "2.43", "0.59", "0.14")]
        lo = mp.mpf(0)
        for L in range(1, 256):
            target = mp.power(mp.mpf(L) / 255, 1 / mp.mpf("0.45454545454"))
            a, b = lo, mp.mpf(13)  # N / D > 1 at 13; thresholds increase, so the last one bounds the next from below
            while b - a > mp.mpf(10) ** -45:
                m = (a + b) / 2
                x = k[0] * m
                if x * (k[1] * x + k[2]) < target * (x * (k[3] * x + k[4]) + k[5]):  # (D > 0)
                    a = m
                else:
                    b = m
            out.append((a + b) / 2)
            lo = a
    return tuple(out)


# ---- the input sets of the display tests -------------------------------------------------------------------

# Binary32 ulps around float32(c_L): 11 offsets, 255 x 11 = 2805 inputs.  The far pair is 2^16 ulps (0.4 .. 0.8 % of c): 256 ulps
# move the level by about L * 0.45 * 3e-5 times the curve's elasticity, which is inside the band at low levels and at the flat top
# (FAR_DECIDED_FROM), so only the far pair is decided at EVERY level.
ULP_OFFSETS = (0, 1, -1, 2, -2, 16, -16, 256, -256, 65536, -65536)


def threshold_inputs():
    """float32 (255, 11): float32(c_L) moved by each of ULP_OFFSETS"""
    base = np.array([float(c) for c in level_thresholds()], np.float64).astype(f32)
    bits = base.view(np.int32).astype(np.int64)  # positive floats: consecutive integers are consecutive floats
    return np.stack([(bits + o).astype(np.int32).view(f32) for o in ULP_OFFSETS], axis=1)


def log_sweep():
    return np.logspace(-30.0, 19.0, 3000).astype(f32)


def uniform_sweep():
    return np.sort(np.random.default_rng(20240611).uniform(0.0, 13.0, 3000)).astype(f32)


def rotate_channels(values):
    """n radiances -> (n, 3): pixel j holds values j, j + n/3, j + 2n/3 (mod n), so every value appears in every channel and the
    channels of one pixel sit at different levels"""
    v = np.asarray(values, f32).reshape(-1)
    n = len(v)
    j = np.arange(n)
    return np.stack([v[j], v[(j + n // 3) % n], v[(j + 2 * (n // 3)) % n]], axis=1)


FLT_MAX = float(np.finfo(f32).max)
# the table of the display contract: (radiance, level)
SPECIALS = (
    (0.0, 0), (-0.0, 0), (1e-45, 0), (1e-39, 0), (1.1754942e-38, 0),
    (12.1, 255), (13.0, 255), (1e3, 255), (1.6e9, 255), (1.7e9, 255), (1e15, 255), (1e19, 255), (1.9e19, 255), (1.95e19, 255),
    (2e19, 255), (1e30, 255), (3e38, 255), (FLT_MAX, 255), (float("inf"), 255),
    (-1.0, 255), (-1e10, 255), (-1e19, 255), (-1e-3, 0), (-1e-2, 0), (-1e-45, 0),
    (float("nan"), 0), (float("-inf"), 0), (-2e19, 0), (-1e30, 0), (-3e38, 0), (-FLT_MAX, 0),
)
# the rows today's fix changes: with the parent's text the polynomials overflow and these display 0
SPECIALS_OVERFLOW = (2e19, 1e30, 3e38, FLT_MAX, float("inf"))
SPECIAL_COMPANIONS = (0.18, 1.0)  # what the other two channels of a table pixel hold


def special_pixels():
    """-> (rgb (rows * 3, 3) float32, want (rows * 3, 3) int, or -1 where the companions' level is whatever the curve says):
    one pixel per row of SPECIALS and channel, the special in that channel, the companions in the other two"""
    rgb, want = [], []
    for value, level in SPECIALS:
        for k in range(3):
            px = [SPECIAL_COMPANIONS[0], SPECIAL_COMPANIONS[1]]
            px.insert(k, value)
            w = [-1, -1]
            w.insert(k, level)
            rgb.append(px)
            want.append(w)
    return np.array(rgb, f32), np.array(want, np.int64)


# ---- running means -----------------------------------------------------------------------------------------


def running_mean64(frames, first_frame=1, start=None):
    """the mean of frames 1 .. first_frame - 1 + len(frames) in float64, where `start` is the mean of the first first_frame - 1"""
    fr = np.asarray(frames, np.float64)
    total = fr.sum(axis=0)
    if first_frame == 1:
        return total / len(fr)
    return (np.asarray(start, np.float64) * (first_frame - 1) + total) / (first_frame - 1 + len(fr))


def running_mean32(frames, first_frame=1, start=None):
    """accumulate_kernel's update in exact binary32: frame k folds r as a += (r - a) / float(k), frame 1 as a = r.  The frames are
    numbered first_frame, first_frame + 1, ..; a first frame other than 1 starts from `start` (with 1 it is not read).
    float(k) rounds to nearest even from 2^24 on, as the conversion of the kernel's uint32 does."""
    a = None if first_frame == 1 else np.array(start, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, r in enumerate(frames, start=first_frame):
            r = np.asarray(r, f32)
            a = r.copy() if k == 1 else a + (r - a) / f32(k)
    return a


def relative_deviation(a, mean64):
    """the largest |a - mean64| / |mean64| over the elements"""
    m = np.asarray(mean64, np.float64)
    return float(np.max(np.abs(np.asarray(a, np.float64) - m) / np.abs(m)))


MEAN_BAR_FACTOR = 8.0


def mean_within_bar(candidate, frames, first_frame=1, start=None):
    """Is `candidate` as close to the float64 mean as a binary32 running mean can be expected to be?  The bar is 8 x the deviation of
    running_mean32 from running_mean64, formed from the two references alone.  -> (ok, deviation of the candidate, bar)"""
    m64 = running_mean64(frames, first_frame, start)
    bar = MEAN_BAR_FACTOR * relative_deviation(running_mean32(frames, first_frame, start), m64)
    dev = relative_deviation(candidate, m64)
    return dev <= bar, dev, bar


def heavy_tail_radiance(frames, pixels, seed):
    """float32 (frames, pixels, 3): exponential radiance, 1 % of the samples scaled by 100 (fireflies)"""
    rng = np.random.default_rng(seed)
    r = rng.exponential(1.0, (frames, pixels, 3))
    r *= np.where(rng.random(r.shape) < 0.01, 100.0, 1.0)
    return r.astype(f32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
