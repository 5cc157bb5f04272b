"""Algorithm-independent pins of environment importance sampling (nxhip_set_env_sampling): the tables, the cdf inversion, the
directions and their pdf against float64 mathematics (tests/env_reference.py), and the light transport under a map against
quadrature — in the style of tests/test_geometry_pins.py and tests/test_physics_pins.py.

tests/test_gpu_env_sampling.py compares device frames with the oracle's restatement of the same estimator, which carries the same
texts: a missing 1 / cos(latitude), the 2 pi^2 of the map's Jacobian, a row counted from the wrong pole, an azimuth mirrored between
the sampler and the lookup, a light count off by one, a guide bucket off by one would be common to both sides or invisible in a
3 % image mean.  Here each side is compared with mathematics, not with the other side: the oracle on the CPU (orc_env_sample_batch,
orc_env_eval_batch, orc_env_distribution), the device under -m gpu (nxhip_read_env_tables, nxhip_env_sample_batch,
nxhip_env_eval_batch: one hook kernel over the product's own env_invert, env_direction, env_uv, env_pdf, env_texel,
sample_background).

Maps (coloured: a warm sun, a bluish sky): A 32 x 16 — dim sky, a 3 x 3 texel sun off every symmetry axis, three black bottom rows,
one row of random texels; S — A's layout with the sun moved across the seam, 6-40 degrees above the horizon (the glossy floor's
mirror direction); B 128 x 64 — as A, plus a row of 104 white texels followed by 24 black ones (a black step is about 1e-8
of the row's sum: the float32 cdf has plateaus there, asserted); C 7 x 5 — odd sizes, fewer texels than guide buckets; D 1 x 1;
E 64 x 32 — all black, only the 1e-6 floor.

Numbers.  The bounds that are derived or are conditions:
  cdf            |cdf32 - cdf64| <= 2^-23: two binary32 roundings of values <= 1 (as tests/test_gpu_light_table.py)
  picks          exact: the texel picked equals searchsorted on the float32 tables read back, on both axes; no plateau entry is
                 ever picked; every pick has density > 0
  unit length    | |d| - 1 | <= 4 ulp = 4 x 2^-23
  round trip     texel of env_uv(direction) != texel picked on at most 1e-3 of the draws
  pdf, caps      for |d.y| > 0.999 the device forms 1 - d.y^2 in binary32: the bound there is the pdf bound below plus
                 2^-22 / cos(latitude)^2 (two roundings of magnitude <= 1 divided by cos^2, with a factor 2); cos >= 1e-6 as documented
  histogram      chi-square of 200 000 draws against p64 over the texels that expect >= 5: (chi2 - dof) / sqrt(2 dof) < 5
  transport      |z| < 4.5 per 8 x 8 block and channel, mean z^2 < 1.6 (test_physics_pins._assert_agree), systematic 1e-3 (pixel-
                 centre evaluation, shadow-ray origin offset, quadrature residue < 2e-5); median relative standard error with
                 sampling on <= 0.5 % on the device, <= 2 % on the oracle twin; the same data must refuse the expectation x 1.03
                 (device) / x 1.10 (oracle twin)
The pdf is compared at the direction as returned, on the draws whose float64 map coordinates lie at least 1e-4 texel (x cos(latitude)
along a row: u is ill-conditioned near the poles) from a texel's edge: a float32 direction is known to about 1e-7, 2e-6 texel at 128
columns, so on those the texel is not in question; the rest — 4e-4 of uniform draws plus the polar rows — must stay under 1 % and are
held, with the same bound, against the pdf of their own texel or of one of the eight around it, whichever is nearest.

MEASURED is the ORACLE's worst deviation from float64 on exactly these inputs (x86-64 CPU); each such bound is 4 x that (the factor
covers reseeding, not new error), on the condition stated beside it.

                                 measured (oracle, CPU)          bound      condition   device (MI355X)
  density, relative              3.00e-7 (B; A 1.88e-7)          1.20e-6                3.00e-7
  direction, |d32 - d64|         6.61e-7 (C; B 5.32e-7)          2.64e-6    < 1e-5      6.61e-7
  pdf, relative, |d.y| <= 0.999  7.27e-6 (D; A 5.85e-6)          2.91e-5                7.27e-6
  1 - integral of the pdf        1.21e-7 (C; A 1.79e-8)          4.84e-7    < 1e-3      1.21e-7
(The pdf's figure is the binary32 1 - d.y^2 at the caps' rim: 2^-24 / (1 - 0.999^2) = 3e-5, halved by the square root.)
For the record, not bounds (oracle and device alike): marginal cdf 3.6e-8, row cdfs 6.9e-8 (2^-23 = 1.19e-7); | |d| - 1 | 1.06e-7; round
trip 0 of 200 000 draws on every map; 0.04-0.07 % of the draws unclear; histogram z 0.26 (A), -0.08 (B); 21 plateau entries in B.
On an MI355X every figure above came out the same to every printed digit: tables, picks, directions and pdf are the oracle's bit
for bit, through the guided search where the oracle searches the whole array.

Transport as measured.  Oracle twin, 256 frames: every estimator within max |z| 3.3, mean z^2 0.80-1.30 of albedo x irradiance / pi;
median relative standard error 0.94-1.09 % with the sampler on, 1.15-1.44 % with the hidden emitter beside it (floor 2 %), 2.1-2.6 %
without the sampler; expectation x 1.10 refused with mean z^2 57-109.  Device, 4 096 frames: max |z| 3.1, mean z^2 0.69-1.29; 0.23-0.28 % with the sampler on, 0.29-0.36 % with the hidden
emitter (floor 0.5 %), 0.53-0.66 % without the sampler; expectation x 1.03 refused with mean z^2 78-131.  The hidden emitter changes no
estimate's expectation in either light-sampling mode; in POWER mode the frames are those of UNIFORM mode bit for bit (the emitter's
own samples are all rejected, so the factor on the mesh lights' pdf, lightCount / nLights, is not reached by that scene: the last
test of this file reaches it, with an emitter that contributes — the rectangular emitter of test_physics_pins under a one-colour map,
radiance = rho (L F + c (1 - F)) from the closed-form form factor; oracle twin: 48 comparisons, max |z| 2.3, mean z^2 0.92; device, UNIFORM and POWER
alike — two equal triangles, so the table's pick is the uniform one —: max |z| 0.76, mean z^2 0.16, the emitter's part x 1.25 refused).
Glossy floor, 48 comparisons each at 1 % systematic, sampler off and on alike: under map A (the floor mirrors the dim sky: the
light pdf is small against the lobe's, so this case pins the SUM of light samples and weighted misses) max |z| 1.4, mean z^2 0.32;
under map S (A's layout with the sun where the floor mirrors the camera: the two pdfs are of one size) max |z| 0.8, mean z^2 0.12,
and the expectation of an estimator whose miss weight carries the light pdf x 0.5 / x 2 — a light count off by one in that one
place — lies +2.1 .. +2.5 % / -3.9 .. -5.4 % away and is refused (mean z^2 5.9 / 21; device 5.9 / 22, with map A at max |z| 1.5,
mean z^2 0.27 and map S at 0.6, 0.08).

The checker is tested itself: the oracle's own outputs after a deliberate edit — pdf x cos(latitude) (the Jacobian dropped),
pdf x 2, v -> 1 - v, the azimuth mirrored, u shifted by half a texel, the picked index + 1 on 1 % of the picks — must each be
refused.

Found while writing these: nothing wrong in the product — no bound exceeded, no non-finite value near the poles (normalize3 never
yields |y| > 1 for (eps, +-1, eps): the sum of squares is >= 1, so the reciprocal root is <= 1), no factor off.
"""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen, workloads
from tests import env_reference as E
from tests import geometry_reference as G
from tests import oracle_lib as O
from tests import scene_helpers as SH
from tests import test_bsdf_pins as BP
from tests import test_physics_pins as PP
from tests.test_physics_pins import _assert_agree, _z

MEASURED = dict(density=3.00e-7, direction=6.61e-7, pdf=7.27e-6, integral=1.21e-7)
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
CDF_BOUND = 2.0 ** -23
UNIT_BOUND = 4.0 * 2.0 ** -23
ROUND_TRIP_MAX = 1e-3
EDGE_MARGIN = 1e-4
MAX_UNCLEAR = 0.01
CAP = 0.999
N_RANDOM = 200_000
GUIDE = 64

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- the maps ------------------------------------------------------------------------------------------------------------------

SKY, SUN = (10, 14, 24), (255, 214, 150)


def _sun_map(W, H, sun_xy, random_row, seed, white_row=None):
    img = np.zeros((H, W, 4), np.uint8)
    img[..., 3] = 255
    img[..., 0:3] = SKY
    img[sun_xy[1]:sun_xy[1] + 3, sun_xy[0]:sun_xy[0] + 3, 0:3] = SUN
    img[random_row, :, 0:3] = np.random.RandomState(seed).randint(0, 256, (W, 3))
    if white_row is not None:
        img[white_row, :, 0:3] = 0
        img[white_row, :104, 0:3] = 255
    img[H - 3:, :, 0:3] = 0
    return img


def _map(name):
    def make():
        if name == "A":
            return _sun_map(32, 16, (9, 3), 8, 41)
        if name == "S":  # A's layout with the sun across the seam, 6 .. 40 degrees above the horizon: where the glossy floor below mirrors the camera
            return np.roll(_sun_map(32, 16, (14, 5), 8, 41), 17, axis=1)
        if name == "B":
            return _sun_map(128, 64, (37, 13), 30, 42, white_row=40)
        if name == "C":
            img = np.zeros((5, 7, 4), np.uint8)
            img[..., 3] = 255
            img[..., 0:3] = np.random.RandomState(43).randint(0, 64, (5, 7, 3))
            img[1, 4, 0:3] = SUN
            return img
        if name == "D":
            img = np.zeros((1, 1, 4), np.uint8)
            img[0, 0] = SUN + (255,)
            return img
        assert name == "E"
        img = np.zeros((32, 64, 4), np.uint8)
        img[..., 3] = 255
        return img

    return _cached(("map", name), make)


def _dist(name):
    return _cached(("dist", name), lambda: E.distribution(_map(name)))


# ---- the two sides: the same three calls on the oracle and on the device ---------------------------------------------------------

class _OracleSide:
    what = "oracle"

    def __init__(self, name):
        sc = SH.BuiltScene([scenegen.quad((-1, 0, -1), (-1, 0, 1), (1, 0, 1), (1, 0, -1))], [(0, 0, workloads.IDENTITY)], hdr_map=_map(name))
        sc.env_sampling = True
        self.scene = sc  # (owns the buffers behind the oracle's view)
        self.orc = sc.oracle()

    def tables(self):
        return self.orc.env_tables()

    def sample(self, r):
        return self.orc.env_sample_batch(r)

    def eval(self, d):
        return self.orc.env_eval_batch(d)


class _DeviceSide:
    what = "device"

    def __init__(self, ctx, name):
        ctx.clear_textures()
        ctx.upload_texture("hdr", _map(name))
        ctx.set_env_sampling(True)
        self.ctx = ctx

    def tables(self):
        return self.ctx.read_env_tables()

    def sample(self, r):
        return self.ctx.env_sample_batch(r)

    def eval(self, d):
        return self.ctx.env_eval_batch(d)


def _oracle_side(name):
    return _cached(("oracle", name), lambda: _OracleSide(name))


# ---- tables --------------------------------------------------------------------------------------------------------------------

def _plateaus(cdf32):
    """entries of a cdf (last axis) that no r can pick: cdf[i] == cdf[i - 1] (cdf[-1] = 0)"""
    prev = np.concatenate([np.zeros(cdf32.shape[:-1] + (1,), np.float32), cdf32[..., :-1]], axis=-1)
    return cdf32 == prev


def _check_tables(tables, name, what):
    marginal, row, density = tables
    img, want = _map(name), _dist(name)
    H, W = img.shape[:2]
    assert marginal.shape == (H,) and row.shape == (H, W) and density.shape == (H, W), what
    assert marginal.dtype == np.float32 and row.dtype == np.float32 and density.dtype == np.float32
    assert np.all(np.diff(marginal) >= 0) and np.all(np.diff(row, axis=1) >= 0), what
    assert marginal[-1] == np.float32(1.0) and np.all(row[:, -1] == np.float32(1.0)), what
    em = float(np.max(np.abs(marginal.astype(np.float64) - want["marginal"])))
    er = float(np.max(np.abs(row.astype(np.float64) - want["row"])))
    ed = float(np.max(np.abs(density.astype(np.float64) - want["density"]) / want["density"]))
    print("%s, map %s (%d x %d): marginal cdf %.3g, row cdfs %.3g (bound %.3g); density %.3g relative (bound %.3g); %d plateau entries" % (
        what, name, W, H, em, er, CDF_BOUND, ed, BOUND["density"], int(_plateaus(row).sum() + _plateaus(marginal).sum())))
    assert em <= CDF_BOUND and er <= CDF_BOUND, what
    assert np.all(density > 0), what
    assert ed <= BOUND["density"], what
    return dict(marginal=em, row=er, density=ed)


# ---- picks ---------------------------------------------------------------------------------------------------------------------

def _special_values(cdf32):
    """0, 1 - 2^-24, every cdf value and every guide boundary b / 64, each with its two float neighbours; those in [0, 1)"""
    at = np.concatenate([np.asarray(cdf32, np.float32), (np.arange(GUIDE + 1) / float(GUIDE)).astype(np.float32)])
    r = np.concatenate([np.array([0.0, 1.0 - 2.0 ** -24], np.float32), at, np.nextafter(at, np.float32(-1)), np.nextafter(at, np.float32(2))])
    return np.unique(r[(r >= 0) & (r < 1)])


def _random_values(n, seed):
    return (np.random.RandomState(seed).randint(0, 1 << 24, n) / float(1 << 24)).astype(np.float32)


def _pick_inputs(marginal, row):
    """(r1, r2) pairs: the special values of the marginal cdf with random r2; for every row that can be picked, an r1 inside it with
    the special values of that row's cdf; N_RANDOM random pairs (multiples of 2^-24) last"""
    s1 = _special_values(marginal)
    parts = [np.stack([s1, _random_values(len(s1), 51)], axis=1)]
    lo = np.concatenate([[0.0], marginal[:-1].astype(np.float64)])
    for y in range(len(marginal)):
        inside = np.float32(0.5 * (lo[y] + float(marginal[y])))
        if not (lo[y] <= inside < marginal[y]):
            continue  # (a plateau of the marginal cdf: no r1 picks this row)
        s2 = _special_values(row[y])
        parts.append(np.stack([np.full(len(s2), inside, np.float32), s2], axis=1))
    parts.append(np.stack([_random_values(N_RANDOM, 52), _random_values(N_RANDOM, 53)], axis=1))
    return np.concatenate(parts).astype(np.float32)


def _check_picks(r, texel, tables, what):
    marginal, row, density = tables
    H, W = row.shape
    assert len(r) >= 100_000 + 3 * (H + GUIDE)
    y, x = np.divmod(texel.astype(np.int64), W)
    want_y = E.pick(marginal, r[:, 0])
    assert np.array_equal(y, want_y), what
    want_x = E.pick(row, (want_y, r[:, 1]))
    wrong = int((x != want_x).sum())
    print("%s: %d picks (%d x %d), %d differ from searchsorted on the tables read back" % (what, len(r), W, H, wrong))
    assert wrong == 0, what
    assert not np.any(_plateaus(marginal)[y]) and not np.any(_plateaus(row)[y, x]), what
    assert np.all(density[y, x] > 0), what


# ---- directions and pdf of the draws ----------------------------------------------------------------------------------------------

def _check_directions(r, d, texel, tables, what):
    """unit length; distance to the float64 direction of the same point of the same texel, formed from the same float32 tables"""
    marginal, row, _ = tables
    H, W = row.shape
    y, x = np.divmod(texel.astype(np.int64), W)
    fy = E.fraction(marginal, y, r[:, 0])
    fx = E.fraction(row, x, r[:, 1], rows=y)
    want = E.direction(x, y, fx, fy, W, H)
    d64 = d.astype(np.float64)
    unit = float(np.max(np.abs(np.linalg.norm(d64, axis=1) - 1.0)))
    err = float(np.max(np.linalg.norm(d64 - want, axis=1)))
    print("%s: %d draws, | |d| - 1 | %.3g (bound %.3g), |d32 - d64| %.3g (bound %.3g)" % (what, len(r), unit, UNIT_BOUND, err, BOUND["direction"]))
    assert unit <= UNIT_BOUND, what
    assert err <= BOUND["direction"], what
    return dict(unit=unit, direction=err)


def _check_round_trip(texel_of_direction, texel_picked, what):
    share = float(np.mean(texel_of_direction != texel_picked))
    print("%s: texel of env_uv(direction) differs from the texel picked on %.3g of %d draws (at most %.3g)" % (what, share, len(texel_picked), ROUND_TRIP_MAX))
    assert share <= ROUND_TRIP_MAX, what
    return share


def _check_pdf(d, pdf, name, what):
    """pdf per solid angle at the direction as returned against p64 W H / (2 pi^2 cos(latitude)) of the direction's texel — for the
    draws whose texel is in question (within EDGE_MARGIN of an edge), of that texel or one of its neighbours; inside the polar caps (|d.y| > 0.999) the device forms 1 - d.y^2 in binary32, whose two roundings of magnitude <= 1 the
    square root's argument carries relative to cos^2: there the bound grows by 2^-22 / cos(latitude)^2"""
    p64 = _dist(name)["p"]
    H, W = p64.shape
    d64 = d.astype(np.float64)
    cos = E.cos_latitude(d64)
    u, v = G.latlong(d64)
    ex = np.minimum(u * W - np.floor(u * W), np.ceil(u * W) - u * W) * cos
    ey = np.minimum(v * H - np.floor(v * H), np.ceil(v * H) - v * H)
    clear = (np.minimum(ex, ey) >= EDGE_MARGIN) if W * H > 1 else np.ones(len(d), bool)
    want = E.pdf(p64, d64)
    rel = np.abs(pdf.astype(np.float64) - want) / want
    # an unclear draw may belong to the texel next door: it is held against the nearest of the pdfs of its texel and the eight around it
    x, y, _ = E.texel_of(d64, W, H)
    scale = W * H / (2.0 * np.pi ** 2 * cos)
    near = np.full(len(d), np.inf)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            other = p64[np.clip(y + dy, 0, H - 1), (x + dx) % W] * scale
            near = np.minimum(near, np.abs(pdf.astype(np.float64) - other) / other)
    rel = np.where(clear, rel, near)
    cap = np.abs(d64[:, 1]) > CAP
    worst = float(rel[clear & ~cap].max())
    over = rel - np.where(cap, 2.0 ** -22 / cos ** 2, 0.0)
    print("%s: %d draws, %.4f unclear (worst against a neighbouring texel %.3g), %d in the polar caps; pdf %.3g relative outside the caps (bound %.3g), %.3g beyond the caps' allowance inside" % (
        what, len(d), 1.0 - clear.mean(), float(over[~clear].max()) if (~clear).any() else 0.0, int(cap.sum()), worst, BOUND["pdf"],
        float(over[clear & cap].max()) if (clear & cap).any() else 0.0))
    assert np.all(np.isfinite(pdf)) and np.all(pdf > 0), what
    assert 1.0 - clear.mean() <= MAX_UNCLEAR, what
    assert np.all(over <= BOUND["pdf"]), what
    return dict(pdf=worst)


def _check_histogram(texel, name, what):
    p = _dist(name)["p"].reshape(-1)
    n = len(texel)
    expected = n * p
    use = expected >= 5.0
    counts = np.bincount(texel.astype(np.int64), minlength=len(p)).astype(np.float64)
    # (the texels that expect less, together, are one more cell)
    chi2 = float((((counts - expected) ** 2 / expected)[use]).sum())
    dof = int(use.sum())
    rest = expected[~use].sum()
    if rest >= 5.0:
        chi2 += float((counts[~use].sum() - rest) ** 2 / rest)
        dof += 1
    dof -= 1
    z = (chi2 - dof) / np.sqrt(2.0 * dof)
    print("%s: %d draws over %d texels, %d cells expect >= 5: chi2 %.1f, z %.2f (bar 5)" % (what, n, len(p), dof + 1, chi2, z))
    assert dof >= 50 and z < 5.0, what
    return z


def _check_pdf_integral(side, name):
    """the eval hook's pdf on the centres of an 8 x 8 sub-grid per texel: sum pdf cos(latitude) d(theta) d(phi) = 1"""
    H, W = _map(name).shape[:2]
    d, _u, _v, dw = E.sphere_grid(W, H, 8)
    _rgb, pdf, texel = side.eval(d.astype(np.float32))
    total = float((pdf.astype(np.float64) * dw).sum())
    want_texel = (np.arange(H * 8)[:, None] // 8 * W + np.arange(W * 8)[None, :] // 8).reshape(-1)
    print("%s, map %s: the pdf integrates to 1 %+.3g over %d directions (bound %.3g)" % (side.what, name, total - 1.0, len(d), BOUND["integral"]))
    assert np.array_equal(texel.astype(np.int64), want_texel)
    assert abs(total - 1.0) <= BOUND["integral"]
    return abs(total - 1.0)


def _draws(side, name):
    """what one side gives for the map's pick inputs: (tables, r, direction, pdf, texel picked, texel of env_uv(direction))"""
    tables = side.tables()
    r = _pick_inputs(tables[0], tables[1])
    d, pdf, texel = side.sample(r)
    _rgb, _pdf, back = side.eval(d)
    return tables, r, d, pdf, texel, back


def _check_side(side, name):
    tables, r, d, pdf, texel, back = _draws(side, name)
    what = "%s, map %s" % (side.what, name)
    _check_picks(r, texel, tables, what)
    rnd = slice(len(r) - N_RANDOM, len(r))  # (the special values sit ON texel edges: directions and pdf are judged on the random draws)
    out = _check_directions(r[rnd], d[rnd], texel[rnd], tables, what)
    out["round_trip"] = _check_round_trip(back[rnd], texel[rnd], what)
    out.update(_check_pdf(d[rnd], pdf[rnd], name, what))
    return out


# ---- near the poles -------------------------------------------------------------------------------------------------------------

def _near_pole_directions():
    """normalize3 of (eps, +-1, eps), eps from 1e-3 down to 1e-20, by the device's own rule a * (1 / sqrt(dot(a, a))) in binary32 —
    the sum of squares formed with separate roundings and with fused multiply-adds alike"""
    eps = np.float32(10.0) ** -np.arange(3, 21, dtype=np.float32)
    a = np.stack([np.concatenate([eps, eps]), np.concatenate([np.ones_like(eps), -np.ones_like(eps)]), np.concatenate([eps, eps])], axis=1).astype(np.float32)
    plain = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    fused = (a.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    out = []
    for dot in (plain, fused):
        assert dot.dtype == np.float32
        inv = np.float32(1.0) / np.sqrt(dot)
        out.append(a * inv[:, None])
    d = np.concatenate(out).astype(np.float32)
    assert np.all(np.abs(d[:, 1]) <= np.float32(1.0)), "a normalised direction must not leave [-1, 1]: asin is NaN beyond"
    return d


def _check_near_poles(side):
    rgb, pdf, _texel = side.eval(_near_pole_directions())
    print("%s: %d directions within 1e-3 .. 1e-20 of the poles: colour and pdf finite, largest pdf %.3g" % (side.what, len(pdf), float(pdf.max())))
    assert np.all(np.isfinite(rgb)) and np.all(np.isfinite(pdf)) and np.all(pdf > 0)


# ---- the oracle, on the CPU -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_oracle_tables(name):
    _check_tables(_oracle_side(name).tables(), name, "oracle")


def test_map_b_has_cdf_plateaus():
    _marginal, row, _density = _oracle_side("B").tables()
    assert _plateaus(row).sum() >= 1
    assert _plateaus(row)[40, 104:].sum() >= 1, "the white row's black tail must not resolve in binary32"


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_oracle_picks_directions_and_pdf(name):
    _check_side(_oracle_side(name), name)


@pytest.mark.parametrize("name", ["A", "B"])
def test_oracle_histogram(name):
    side = _oracle_side(name)
    _d, _pdf, texel = side.sample(np.stack([_random_values(N_RANDOM, 61), _random_values(N_RANDOM, 62)], axis=1))
    _check_histogram(texel, name, "oracle, map %s" % name)


@pytest.mark.parametrize("name", ["A", "C"])
def test_oracle_pdf_integrates_to_one(name):
    _check_pdf_integral(_oracle_side(name), name)


def test_oracle_near_the_poles():
    _check_near_poles(_oracle_side("A"))


def test_bounds_meet_their_conditions():
    assert 0.0 < BOUND["direction"] < 1e-5
    assert 0.0 < BOUND["integral"] < 1e-3
    assert 0.0 < BOUND["density"] < 1e-5 and 0.0 < BOUND["pdf"] < 1e-4


# ---- the checker itself: the oracle's outputs after a deliberate edit must be refused ------------------------------------------------

def _refused(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def test_checker_refuses_edited_samples():
    name = "A"
    side = _oracle_side(name)
    tables, r, d, pdf, texel, _back = _draws(side, name)
    rnd = slice(len(r) - N_RANDOM, len(r))
    r_, d_, pdf_, texel_ = r[rnd], d[rnd], pdf[rnd], texel[rnd]
    _check_directions(r_, d_, texel_, tables, "unedited")
    _check_pdf(d_, pdf_, name, "unedited")
    _check_picks(r, texel, tables, "unedited")
    cos = E.cos_latitude(d_).astype(np.float32)
    _refused(_check_pdf, d_, pdf_ * cos, name, "pdf x cos(latitude): the Jacobian dropped")
    _refused(_check_pdf, d_, pdf_ * np.float32(2.0), name, "pdf x 2")
    _refused(_check_directions, r_, d_ * np.array([1, -1, 1], np.float32), texel_, tables, "v -> 1 - v")
    _refused(_check_directions, r_, d_ * np.array([1, 1, -1], np.float32), texel_, tables, "azimuth mirrored")
    # ... and the pdf of the mirrored directions is not the pdf of the draws either (an azimuth mirrored between sampler and lookup)
    _refused(_check_pdf, d_ * np.array([1, 1, -1], np.float32), pdf_, name, "azimuth mirrored between the sampler and the lookup")
    _refused(_check_pdf, d_ * np.array([1, -1, 1], np.float32), pdf_, name, "rows counted from the other pole in the lookup")
    a = 2.0 * np.pi * 0.5 / _map(name).shape[1]
    turned = np.stack([np.cos(a) * d_[:, 0] - np.sin(a) * d_[:, 2], d_[:, 1], np.sin(a) * d_[:, 0] + np.cos(a) * d_[:, 2]], axis=1).astype(np.float32)
    _refused(_check_directions, r_, turned, texel_, tables, "u shifted by half a texel")
    moved = texel.copy()
    some = np.random.RandomState(71).rand(len(texel)) < 0.01
    moved[some] = np.minimum(texel[some] + 1, tables[1].size - 1)
    _refused(_check_picks, r, moved, tables, "picked index + 1 on 1 % of the picks")
    # the integral of an edited pdf is not 1
    class Doubled:
        what = "edited"

        def eval(self, dirs):
            rgb, p, t = side.eval(dirs)
            return rgb, p * np.float32(2.0), t

    _refused(_check_pdf_integral, Doubled(), name)
    _check_histogram(texel_, name, "unedited")
    _refused(_check_histogram, moved[rnd], name, "picked index + 1 on 1 % of the picks")


# ---- the device ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_gpu_tables(gpu_ctx_factory, name):
    side = _DeviceSide(gpu_ctx_factory(16, 16), name)
    _check_tables(side.tables(), name, "device")
    if name == "B":
        assert _plateaus(side.tables()[1])[40, 104:].sum() >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_gpu_picks_directions_and_pdf(gpu_ctx_factory, name):
    _check_side(_DeviceSide(gpu_ctx_factory(16, 16), name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_gpu_histogram(gpu_ctx_factory, name):
    side = _DeviceSide(gpu_ctx_factory(16, 16), name)
    _d, _pdf, texel = side.sample(np.stack([_random_values(N_RANDOM, 61), _random_values(N_RANDOM, 62)], axis=1))
    _check_histogram(texel, name, "device, map %s" % name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_gpu_pdf_integrates_to_one(gpu_ctx_factory, name):
    _check_pdf_integral(_DeviceSide(gpu_ctx_factory(16, 16), name), name)


@pytest.mark.gpu
def test_gpu_near_the_poles(gpu_ctx_factory):
    _check_near_poles(_DeviceSide(gpu_ctx_factory(16, 16), "A"))


# ---- transport: the estimator against quadrature ----------------------------------------------------------------------------------
#
# One 16 x 16 Lambertian quad under map A, seen by a 64 x 40 pinhole camera that sees nothing else; pathLength 3.  Every ray that
# leaves the quad misses, and a miss is accounted before the roulette: whichever estimator runs — BSDF sampling alone, MIS with the
# environment found by BSDF-sampled misses only, MIS with the environment as a light of the NEE — the expectation of every pixel is
# albedo x irradiance(map, n) / pi.  With a small emitter hidden below the quad (facing away: the Lambertian eval rejects it, the
# quad blocks it) the NEE chooses among two lights and every light-selection factor is in play, under LIGHTS_UNIFORM and LIGHTS_POWER.

ALBEDO = np.array([0.3, 0.5, 0.7])
TW, TH = 64, 40
assert BP.BLOCK == 8  # the blocks of test_bsdf_pins._BlockEstimate
ESTIMATORS = {"bsdf": (False, False), "mis, sampler off": (True, False), "mis, sampler on": (True, True)}


def _normal(tilt):
    M = np.asarray(capi.mat4_from_trs((0, 0, 0), (0, 0, tilt), (1, 1, 1)), np.float64).reshape(4, 4)
    n = M[:3, :3] @ np.array([0.0, 1.0, 0.0])
    return M, n / np.linalg.norm(n)


def _quad_scene(tilt, use_mis, env_sampling, emitter=False, light_mode=pod.LIGHTS_UNIFORM):
    M, n = _normal(tilt)
    xf = capi.mat4_from_trs((0, 0, 0), (0, 0, tilt), (1, 1, 1))
    meshes = [scenegen.quad((-8, 0, -8), (-8, 0, 8), (8, 0, 8), (8, 0, -8))]
    mats = [pod.make_material(pod.MAT_DIFFUSE, albedo=tuple(ALBEDO))]
    placements = [(0, 0, xf)]
    if emitter:  # 0.5 below the quad, facing away from it
        meshes.append(scenegen.quad((-0.25, -0.5, -0.25), (0.25, -0.5, -0.25), (0.25, -0.5, 0.25), (-0.25, -0.5, 0.25)))
        mats.append(pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), emissive=(1.0, 0.8, 0.6), intensity=20.0))
        placements.append((1, 1, xf))
    eye = M[:3, :3] @ np.array([1.5, 5.0, 1.0])
    cam = capi.camera_init(tuple(eye), tuple(-eye / np.linalg.norm(eye)), 20.0, TW, TH, 5.0, 0.0)
    sc = SH.BuiltScene(meshes, placements, materials=np.array(mats, dtype=pod.MAT_DT), camera=cam,
                       settings=workloads.make_settings(use_mis=use_mis, path_length=3, background=(1, 1, 1), background_intensity=1.0), hdr_map=_map("A"))
    sc.env_sampling = env_sampling
    sc.light_sampling = light_mode
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    assert len(sc.lights) == (1 if emitter else 0)
    # every pixel of every block sees the quad, from the side its normal points to: the four corners of every pixel
    pos = cam["position"].astype(np.float64)
    jj, ii = np.mgrid[0:TH + 1, 0:TW + 1]
    d = cam["lowerLeftCorner"].astype(np.float64) + cam["viewportX"].astype(np.float64) * (ii.reshape(-1, 1) / TW) + cam["viewportY"].astype(np.float64) * (jj.reshape(-1, 1) / TH) - pos
    assert pos @ n > 1.0 and np.all(d @ n < 0)
    p = (pos + d * (-(pos @ n) / (d @ n))[:, None]) @ M[:3, :3]  # back into the quad's own frame (M is a rotation)
    assert np.all(np.abs(p[:, 0]) < 7.5) and np.all(np.abs(p[:, 2]) < 7.5) and np.all(np.abs(p[:, 1]) < 1e-9)
    return sc


def _expectation(tilt):
    def make():
        irr, residue = E.irradiance(_map("A"), _normal(tilt)[1], sub=16)
        print("irradiance of map A on the normal tilted %g degrees: %s, quadrature residue %.3g" % (tilt, irr, residue))
        assert residue < 2e-5
        return ALBEDO * irr / np.pi

    return _cached(("expectation", tilt), make)


def _oracle_estimate8(scene, frames):
    return PP._oracle_estimate(scene, TW, TH, frames, estimate=BP._BlockEstimate)  # (8 x 8 pixel blocks)


def _gpu_estimate8(ctx, scene, frames):
    return PP._gpu_estimate(ctx, scene, TW, TH, frames, estimate=BP._BlockEstimate)


def _check_transport(estimate, tilt, frames, rel_se_floor, refused_scale, light_modes):
    want = _expectation(tilt)[None, :]
    est = {}
    for label, (use_mis, sampling) in ESTIMATORS.items():
        e = est[label] = estimate(_quad_scene(tilt, use_mis, sampling), frames)
        print("tilt %g, %s: mean %s, median relative standard error %.4f" % (tilt, label, e.mean.mean(axis=0), np.median(e.se / want)))
        _assert_agree(_z(e.mean, e.se, want, 0.0, systematic=1e-3), "quad under map A, tilt %g, %s, against quadrature" % (tilt, label))
    on = est["mis, sampler on"]
    assert np.median(on.se / want) <= rel_se_floor, "the estimate is too noisy for its pass to mean anything"
    assert np.median(on.se) < np.median(est["mis, sampler off"].se) and np.median(on.se) < np.median(est["bsdf"].se)
    with pytest.raises(AssertionError):
        _assert_agree(_z(on.mean, on.se, want * refused_scale, 0.0, systematic=1e-3), "the expectation x %g must be refused" % refused_scale)
    for mode in light_modes:  # two lights to choose among: the environment and an emitter that never contributes
        e = estimate(_quad_scene(tilt, True, True, emitter=True, light_mode=mode), frames)
        print("tilt %g, hidden emitter, light sampling %d: mean %s, median relative standard error %.4f" % (tilt, mode, e.mean.mean(axis=0), np.median(e.se / want)))
        assert np.median(e.se / want) <= rel_se_floor, "the estimate is too noisy for its pass to mean anything"
        _assert_agree(_z(e.mean, e.se, want, 0.0, systematic=1e-3), "quad under map A with a hidden emitter, tilt %g, light sampling %d" % (tilt, mode))
        with pytest.raises(AssertionError):
            _assert_agree(_z(e.mean, e.se, want * refused_scale, 0.0, systematic=1e-3), "the expectation x %g must be refused" % refused_scale)


@pytest.mark.parametrize("tilt", [0.0, 50.0])
def test_oracle_transport_under_the_map(tilt):
    _check_transport(_oracle_estimate8, tilt, 256, 0.02, 1.10, (pod.LIGHTS_UNIFORM,))


@pytest.mark.gpu
@pytest.mark.parametrize("tilt", [0.0, 50.0])
def test_gpu_transport_under_the_map(gpu_ctx_factory, tilt):
    _check_transport(lambda scene, frames: _gpu_estimate8(gpu_ctx_factory(TW, TH), scene, frames), tilt, 4096, 0.005, 1.03, (pod.LIGHTS_UNIFORM, pod.LIGHTS_POWER))


# ---- the glossy floor: the miss weight where BSDF sampling carries most of the energy -----------------------------------------------
#
# The rough conductor floor of tests/test_bsdf_pins.py (conductor r0.3, the extended conductor BSDF, paths of two vertices) under map
# A instead of its rectangular emitter: the expectation of that test's estimator structure, with the environment as the light — the
# sphere's quadrature nodes, L from the bilinear lookup, p_light = env_reference.pdf / (number of lights = 1).  A BSDF-sampled ray
# that finds this light LEAVES the scene: no roulette, and a p_light the validity rule (> 1e-4) rejects leaves it unweighted.  With
# the sampler off (no light at all) the same function's BSDF-sampling expectation holds.

WINDOW_COLUMNS, WINDOW_ROWS = (0.125, 0.875), (0.25, 0.5)  # u < 0.125 or u >= 0.875, 0.25 <= v < 0.5: texels 28 .. 3 of rows 4 .. 7


def _environment_nodes(name, fine, coarse=4, miss_pdf_scale=None):
    """a map as the light of test_bsdf_pins._floor_expectation: midpoints of `coarse`^2 cells per texel, of `fine`^2 inside the window of
    the map the floor mirrors towards the camera (the camera looks along -x from 15 degrees above the floor: the mirror direction lies
    at the map's seam, 5 .. 25 degrees above the horizon).  At that incidence the lobe is 2 alpha cos(theta_i) = 2 degrees wide across
    the plane of incidence: 8 cells per texel (1.4 degrees) put the expectation 3 % too high, 16 0.6 %, 32 0.13 % (measured).
    p_light = env_reference.pdf / nLights, nLights = 1.  miss_pdf_scale (the checker's own test): the pdf in the weight of a miss
    scaled by it, as a wrong light count there would."""
    img = _map(name)
    H, W = img.shape[:2]
    parts = []
    for sub, inside in ((coarse, False), (fine, True)):
        d, u, v, dw = E.sphere_grid(W, H, sub)
        window = ((u < WINDOW_COLUMNS[0]) | (u >= WINDOW_COLUMNS[1])) & (v >= WINDOW_ROWS[0]) & (v < WINDOW_ROWS[1])
        keep = (d[:, 1] > 0.0) & (window == inside)  # (up only: a conductor's Sample drops what it reflects below the floor, ConductorBSDF.cuh:41-42)
        parts.append((np.stack([d[:, 0], d[:, 2], d[:, 1]], axis=1)[keep],  # the floor's frame: (x, z, y)
                      dw[keep], G.texture(img, u, v)[keep], (E.pdf(_dist(name)["p"], d) / 1.0)[keep]))
    nodes = tuple(np.concatenate([part[k] for part in parts]) for k in range(4))
    assert abs(nodes[1].sum() / (2.0 * np.pi) - 1.0) < 1e-3
    if miss_pdf_scale is not None:
        nodes = nodes + (nodes[3] * miss_pdf_scale,)
    return lambda p: nodes


def _glossy_scene(W, H, name, sampling):
    sc = BP._floor_scene(W, H, BP.MATS["conductor r0.3"], True, sky=1.0)
    sc.hdr_map = _map(name)
    sc.env_sampling = sampling
    assert len(sc.lights) == 0
    return sc


def _glossy_expectation_at(W, H, name, pixels, fine, miss_pdf_scale=None):
    return BP._floor_expectation(BP.MATS["conductor r0.3"], _glossy_scene(W, H, name, True), W, H, light=_environment_nodes(name, fine, miss_pdf_scale=miss_pdf_scale),
                                 light_is_hit=False, pixels=pixels)[0:2]


def _glossy_expectation(W, H, name, pixels):
    """(sampler off, sampler on, sampler on at 16 cells) per block: the midpoint rule's h^2 removed by Richardson's rule from 16 and 32
    cells per texel; the correction itself — the finer grid's own error, |fine - coarse| / 3 — must stay under a quarter of the 1 % allowed"""
    want = {fine: _glossy_expectation_at(W, H, name, pixels, fine) for fine in (16, 32)}
    off, on = ((4.0 * want[32][k] - want[16][k]) / 3.0 for k in (0, 1))
    assert np.max(np.abs(want[32][1] - want[16][1]) / 3.0 / on) < 2.5e-3
    return off, on, want[16][1]


def _check_glossy_floor_under_the_map(estimate, name, frames, rel_se_bar):
    est = {on: estimate(lambda W, H: _glossy_scene(W, H, name, on), frames) for on in (False, True)}
    e = est[True]
    jj, ii = np.mgrid[0:e.H, 0:e.W]
    # the expectation at four pixel centres per 8 x 8 block, placed symmetrically about its centre (it varies slowly: the light is at infinity)
    pixels = (np.isin(jj % BP.BLOCK, (2, 5)) & np.isin(ii % BP.BLOCK, (2, 5))).reshape(-1)
    want_off, want_on, on_16 = _glossy_expectation(e.W, e.H, name, pixels)
    lit = want_off.max(1) > 0.05 * want_off.max()
    assert lit.mean() > 0.3
    print("conductor floor under map %s: expectation %s .. %s; median relative standard error: sampler off %.4f, on %.4f" % (
        name, np.round(want_on[lit].min(0), 5), np.round(want_on[lit].max(0), 5), np.median(est[False].se[lit] / want_off[lit]), np.median(e.se[lit] / want_on[lit])))
    assert np.median(e.se[lit] / want_on[lit]) < rel_se_bar, "the estimate is too noisy for its pass to mean anything"
    # (1 %, as tests/test_bsdf_pins.py: pixel-centre evaluation of the expectation inside a block, the quadrature, the offset of the shadow rays' origins)
    _assert_agree(_z(est[False].mean, est[False].se, want_off, 0.0, systematic=1e-2)[lit], "conductor floor under map %s, sampler off, against the formulas" % name)
    _assert_agree(_z(e.mean, e.se, want_on, 0.0, systematic=1e-2)[lit], "conductor floor under map %s, sampler on (NEE + MIS-weighted misses), against the formulas" % name)
    if name == "S":
        # Under map A the floor mirrors the dim sky only: the light pdf there is small against the lobe's, a miss's weight is 1 whatever
        # the light count in it, and the check above pins the SUM of the two techniques.  With the sun in the mirror the two pdfs are
        # of one size, and the same data must refuse the expectation of an estimator whose miss weight carries the light pdf halved or
        # doubled (a light count off by one in that one place: the weights then no longer sum to one).
        for scale in (0.5, 2.0):
            # (the shift from the 16-cell quadrature alone: a difference of two sums over the same nodes, which their common h^2 error leaves)
            wrong = want_on + (_glossy_expectation_at(e.W, e.H, name, pixels, 16, miss_pdf_scale=scale)[1] - on_16)
            print("miss weight with the light pdf x %g: the expectation moves by %+.3f .. %+.3f" % (scale, ((wrong - want_on) / want_on)[lit].min(), ((wrong - want_on) / want_on)[lit].max()))
            with pytest.raises(AssertionError):
                _assert_agree(_z(e.mean, e.se, wrong, 0.0, systematic=1e-2)[lit], "the light pdf x %g in the miss weight must be refused" % scale)


@pytest.mark.parametrize("name", ["A", "S"])
def test_oracle_glossy_floor_under_the_map(name):
    _check_glossy_floor_under_the_map(BP._oracle_estimator(32, 32), name, 768, 0.06)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "S"])
def test_gpu_glossy_floor_under_the_map(gpu_ctx_factory, name):
    _check_glossy_floor_under_the_map(BP._gpu_estimator(gpu_ctx_factory, 32, 32), name, 8192, 0.02)


# ---- an emitter that contributes, beside the environment: the factors on the MESH lights' pdf ------------------------------------------
#
# The hidden emitter above never contributes, so lightCount / nLights on a mesh light's pdf under LIGHTS_POWER — in the NEE and in
# the weight of a BSDF-sampled hit on an emitter — is not reached by it.  Here it is: test_physics_pins' rectangular emitter over a
# diffuse floor (closed-form form factor F), under a map of ONE colour c with the sampler on.  The emitter covers F of the floor
# point's cosine-weighted hemisphere and is black underneath, the map the rest: radiance = rho (L F + c (1 - F)), whatever the
# split between the two lights and the BSDF samples.  The systematic allowance, 2e-3, is the one test_physics_pins._check_quad_light
# gives this very scene and this very closed form (F evaluated at 4 x 4 positions per pixel, the shadow rays' origin offset); the
# map's term adds nothing to it: c is one colour, exact under the bilinear filter, and 1 - F carries F's own error.

FLAT_SKY = (60, 90, 140)


def _emitter_and_sky_scene(W, H, mode):
    sc = PP._quad_light_scene(W, H, True)
    sky = np.zeros((4, 8, 4), np.uint8)
    sky[...] = FLAT_SKY + (255,)
    sc.hdr_map = sky
    sc.env_sampling = True
    sc.light_sampling = mode
    return sc


def _check_emitter_and_sky(estimate, W, H, frames, rel_se_bar, refused_scale, modes):
    emitter = PP._quad_light_expectation(_emitter_and_sky_scene(W, H, modes[0]), W, H)  # rho L F per 16 x 16 block
    F = emitter / (PP.FLOOR_RHO * PP.LIGHT_LE)
    want = emitter + PP.FLOOR_RHO * G.srgb_decode(np.array(FLAT_SKY))[None, :] * (1.0 - F)
    share = emitter / want
    assert (share > 0.3).mean() > 0.5 and (1.0 - share).max() > 0.3  # the emitter carries most blocks, the map a good part of some
    for mode in modes:
        e = estimate(_emitter_and_sky_scene(W, H, mode), frames)
        print("emitter under a one-colour map, light sampling %d: emitter's share of the radiance %.2f .. %.2f, median relative standard error %.4f" % (
            mode, (emitter / want).min(), (emitter / want).max(), np.median(e.se / want)))
        assert np.median(e.se / want) < rel_se_bar, "the estimate is too noisy for its pass to mean anything"
        _assert_agree(_z(e.mean, e.se, want, 0.0, systematic=2e-3), "emitter and one-colour map against the form factor, light sampling %d" % mode)
        with pytest.raises(AssertionError):
            _assert_agree(_z(e.mean, e.se, want * refused_scale, 0.0, systematic=2e-3), "the expectation x %g must be refused" % refused_scale)
        # ... and so must the expectation with the emitter's part counted as if the environment were no light (nLights = lightCount)
        with pytest.raises(AssertionError):
            _assert_agree(_z(e.mean, e.se, want + 0.25 * emitter, 0.0, systematic=2e-3), "the emitter's part x 1.25 must be refused")


def test_oracle_emitter_and_environment_share_the_light_sample():
    # (64 x 64: 16 blocks — at 32 x 32 the four blocks' twelve comparisons are too few, and too correlated, for the mean of z^2 to mean anything)
    _check_emitter_and_sky(lambda sc, frames: PP._oracle_estimate(sc, 64, 64, frames), 64, 64, 128, 0.08, 1.10, (pod.LIGHTS_UNIFORM,))


@pytest.mark.gpu
def test_gpu_emitter_and_environment_share_the_light_sample(gpu_ctx_factory):
    _check_emitter_and_sky(lambda sc, frames: PP._gpu_estimate(gpu_ctx_factory(64, 64), sc, 64, 64, frames), 64, 64, 4096, 0.02, 1.03, (pod.LIGHTS_UNIFORM, pod.LIGHTS_POWER))
