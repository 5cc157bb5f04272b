"""Float environment maps on the device (nxhip_upload_env_float): storage, the lookup, the device-built sampler tables, the transport
under a sun 10^6 times the sky, the project's invariants, replacement and refusals — each against float64 numpy
(tests/env_float_reference.py), none against the oracle, which has no float path.

Maps (float32, H x W x 3):
  one      1 x 1
  odd      7 x 5: odd sizes, fewer texels than guide buckets; values 1e-3 .. 10 with one texel of 6e4
  wave     130 x 3: a row that is no multiple of a wave; 6e4 beside 1e-3
  long     1025 x 2: a row longer than one workgroup of the scan (256): the carry from chunk to chunk, four times and a single texel
  zero     64 x 32, all zero: the 1e-6 floor only
  sun      32 x 16: sky (0.02, 0.03, 0.06), one texel of (6e4, 5e4, 3.5e4) at (9, 4), three black rows at the bottom — the transport's map
  seam     32 x 16: the sun at (31, 5): its footprint wraps across the u seam
  top      128 x 64: the sun at (37, 0): its footprint wraps over the top row into the (black) bottom row, as the lookup's addressing does
  top_dim  128 x 64: the same with the sun at 1 / 32 (still 3e4 times the sky): 15 % of the draws in row 0 and 2.4 % in row 63, so the pdf
           check's share of unclear draws is 0.5 % and the pdf across the v wrap is asserted
  plateau  128 x 64: sky of 0.5 .. 1.5, rows 39 .. 41 with 104 texels of 1 followed by 24 of 0: the tail's weight is the floor, 1e-8 of the
           row's sum, which the binary32 cdf does not resolve (plateaus, asserted)
  noise    32 x 16 of 0 .. 4: the histogram's first map (plateau is the second)
  lookup   32 x 16, log-uniform 1e-3 .. 6e4 with 6e4 beside 1e-3: the lookup's map (a power of two on both axes)

Bounds.  Derived or conditions:
  stored texels   bit-equal to the upload
  cdf             |cdf32 - cdf64| <= 2^-23, non-decreasing, the last entry exactly 1
  picks, guides   exact against searchsorted / the host's rule on the tables read back; no plateau entry picked
  lookup, exact weights   (u, v) multiples of 2^-10 on power-of-two maps: |device - float64| <= 6 x 2^-24 x the largest of the four taps
                  (three roundings per lerp, two lerps deep)
  transport       |z| < 4.5, mean z^2 < 1.6 per 8 x 8 block and channel against albedo x irradiance / pi from float64 quadrature of the
                  float lookup, systematic 1e-3; sampler on: median relative standard error <= 1 % at 1024 frames (the numpy estimator
                  of tests/test_env_float.py predicts 1.06 / sqrt(64 x 1024) = 0.41 %; the factor 2.4 covers MIS and the later
                  bounces); the same data must refuse the expectation x 1.05
  directions, round trip, pdf   the checks of tests/test_env_pins.py with its bounds, imported: they are table-driven
Measured x 4 (MEASURED below is the device's worst figure on exactly these inputs, an MI355X; the bound is 4 x that and must stay
under the condition beside it):
                                         measured    bound      condition
  density, relative                      5.91e-8     2.4e-7     < 1e-5    (map `long`; one binary32 rounding of a binary64 value: 2^-24 = 6e-8)
  lookup at random (u, v) / largest tap  7.67e-6     3.1e-5     < 1e-4    (map `wave`; u W - 1/2 in binary32: 2^-24 x W of a texel in the weight;
                                                                            `lookup` 5.1e-7, `odd` 6.4e-7)
For the record (device): cdfs within 3.0e-8 of float64; lookups with exact weights within 1.4e-7 of the largest tap (bound 3.6e-7);
histogram z 0.08 (noise), 0.39 (plateau); 18 plateau entries in `plateau`; the pdf integrates to 1 + 5e-9 (sun), 1 - 1.3e-7 (odd).

Transport as measured on the device, 1024 frames, tilt 0 / 50 degrees: with the sampler on max |z| 1.84 / 1.77, mean z^2 0.63 / 0.67,
median relative standard error 0.40 % / 0.45 %; the expectation x 1.05 refused.  With the sampler OFF the two estimators (the same
frames: without a light the MIS estimator IS the BSDF estimator) find the sun by BSDF samples alone — one texel of 512, hit by one
sample in a hundred, worth 6e4 each: median relative standard error 3.3 % / 5.6 % at the same 1024 frames, ten times the sampler's;
max |z| 3.1, mean z^2 1.02 / 0.64.  They are asserted all the same, at that frame count: a block's mean is then the sum of
about 650 hits among 65 536 samples, enough for its standard error to mean what the z-test takes it to mean, and the test says what
it can at that noise: no bias above 5 % x 4.5.
"""
import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import env_float_reference as F
from tests import env_reference as E
from tests import geometry_reference as G
from tests import test_bsdf_pins as BP
from tests import test_env_pins as TP
from tests import test_physics_pins as PP
from tests.test_physics_pins import _assert_agree, _z

pytestmark = pytest.mark.gpu

MEASURED = dict(density=5.91e-8, lookup=7.67e-6)
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
CDF_BOUND = 2.0 ** -23
GUIDE = 64
SUN = np.array(F.SUN, np.float32)


# ---- the maps ------------------------------------------------------------------------------------------------------------------------

def _make(name):
    rng = np.random.RandomState({"odd": 2, "wave": 3, "long": 4, "noise": 5, "lookup": 6, "plateau": 7}.get(name, 0))
    if name == "one":
        return SUN.reshape(1, 1, 3).copy()
    if name == "odd":
        img = (10.0 ** rng.uniform(-3, 1, (5, 7, 3))).astype(np.float32)
        img[1, 4] = SUN
        return img
    if name == "wave":
        img = (10.0 ** rng.uniform(-3, 1, (3, 130, 3))).astype(np.float32)
        img[1, 64] = SUN
        img[1, 65] = 1e-3
        img[0, 129] = SUN  # the last texel of a row: its footprint wraps to column 0
        return img
    if name == "long":
        return rng.uniform(0.0, 2.0, (2, 1025, 3)).astype(np.float32)
    if name == "zero":
        return np.zeros((32, 64, 3), np.float32)
    if name == "sun":
        return F.sun_map()
    if name == "seam":
        return F.sun_map(32, 16, (31, 5))
    if name == "top":
        return F.sun_map(128, 64, (37, 0))
    if name == "top_dim":
        img = F.sun_map(128, 64, (37, 0))
        img[0, 37] *= np.float32(1.0 / 32.0)
        return img
    if name == "plateau":
        img = rng.uniform(0.5, 1.5, (64, 128, 3)).astype(np.float32)
        img[39:42, :104] = 1.0
        img[39:42, 104:] = 0.0
        return img
    if name == "noise":
        return rng.uniform(0.0, 4.0, (16, 32, 3)).astype(np.float32)
    assert name == "lookup"
    img = (10.0 ** rng.uniform(-3, np.log10(6e4), (16, 32, 3))).astype(np.float32)
    img[5, 9] = 6e4
    img[5, 10] = 1e-3
    img[6, 9] = 1e-3
    img[0, 0] = 6e4    # the corner: both wraps
    img[15, 31] = 1e-3
    return img


ALL = ["one", "odd", "wave", "long", "zero", "sun", "seam", "top", "top_dim", "plateau"]


def _map(name):
    """the map — also under test_env_pins' cache, whose imported checks look a map and its float64 distribution up by name.

    This writes into test_env_pins._CACHE, a private dictionary of a module this file must not edit, under keys no 8-bit map has
    ("float:<name>"): the imported checks (_check_pdf, _check_histogram, _check_pdf_integral) take a map's NAME and fetch its float64
    distribution through test_env_pins._dist(name), which is _cached(("dist", name), ...), so a filled cache entry is the one way to
    hand them a distribution of ours without copying them.  It depends on that key layout: _keys_are_where_the_checks_look() below
    fails loudly, before any check runs, should test_env_pins ever keep its cache otherwise."""
    key = "float:" + name
    if ("map", key) not in TP._CACHE:
        img = _make(name)
        assert img.dtype == np.float32 and np.all(np.isfinite(img)) and np.all(img >= 0)
        TP._CACHE[("map", key)] = img
        TP._CACHE[("dist", key)] = F.distribution(img)
        _keys_are_where_the_checks_look(key)
    return TP._CACHE[("map", key)]


def _keys_are_where_the_checks_look(key):
    assert TP._map(key) is TP._CACHE[("map", key)] and TP._dist(key) is TP._CACHE[("dist", key)], "test_env_pins no longer caches under (kind, name)"


def _dist(name):
    _map(name)
    return TP._CACHE[("dist", "float:" + name)]


class _Side:
    """the three calls of test_env_pins._DeviceSide on a float map"""
    what = "device, float map"

    def __init__(self, ctx, name, sampling=True):
        ctx.clear_textures()
        ctx.upload_env_float(_map(name))
        if sampling:
            ctx.set_env_sampling(True)
        self.ctx, self.name = ctx, name

    def tables(self):
        return self.ctx.read_env_tables()

    def sample(self, r):
        return self.ctx.env_sample_batch(r)

    def eval(self, d):
        return self.ctx.env_eval_batch(d)


# ---- storage, tables, guides ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL + ["lookup"])
def test_stored_texels_are_the_upload_bit_for_bit(gpu_ctx_factory, name):
    side = _Side(gpu_ctx_factory(16, 16), name, sampling=False)
    got = side.ctx.read_env_float()
    assert got.shape == _map(name).shape and np.array_equal(got.view(np.uint32), _map(name).view(np.uint32))


def _host_guide(cdf):
    """nxhip_scene.hip make_guide: the first index whose cdf exceeds b / 64, clamped to n - 1"""
    bounds = (np.arange(GUIDE + 1) / float(GUIDE)).astype(np.float32)
    return np.minimum(np.searchsorted(np.asarray(cdf, np.float64), bounds.astype(np.float64), side="right"), len(cdf) - 1).astype(np.uint32)


@pytest.mark.parametrize("name", ALL)
def test_tables_against_float64(gpu_ctx_factory, name):
    side = _Side(gpu_ctx_factory(16, 16), name)
    marginal, row, density = side.tables()
    img, want = _map(name), _dist(name)
    H, W = img.shape[:2]
    assert marginal.shape == (H,) and row.shape == (H, W) and density.shape == (H, W)
    assert marginal.dtype == np.float32 and row.dtype == np.float32 and density.dtype == np.float32
    assert np.all(np.diff(marginal) >= 0) and np.all(np.diff(row, axis=1) >= 0)
    assert marginal[-1] == np.float32(1.0) and np.all(row[:, -1] == np.float32(1.0))
    em = float(np.max(np.abs(marginal.astype(np.float64) - want["marginal"])))
    er = float(np.max(np.abs(row.astype(np.float64) - want["row"])))
    ed = float(np.max(np.abs(density.astype(np.float64) - want["density"]) / want["density"]))
    plateaus = int(TP._plateaus(row).sum() + TP._plateaus(marginal).sum())
    print("float map %s (%d x %d): marginal cdf %.3g, row cdfs %.3g (bound %.3g); density %.3g relative (bound %.3g); %d plateau entries" % (
        name, W, H, em, er, CDF_BOUND, ed, BOUND["density"], plateaus))
    assert em <= CDF_BOUND and er <= CDF_BOUND
    assert np.all(density > 0) and np.all(np.isfinite(density))
    assert 0.0 < BOUND["density"] < 1e-5 and ed <= BOUND["density"]
    if name == "plateau":
        assert TP._plateaus(row)[40, 106:127].sum() >= 1, "the row's zero tail must not resolve in binary32"
    if name == "zero":  # the floor alone: every texel alike
        assert np.max(np.abs(density.astype(np.float64) * (2.0 * np.pi ** 2) - 1.0)) < 1e-6
    # the guides: the host's rule applied to the tables as read back
    mg, rg = side.ctx.read_env_guides()
    assert np.array_equal(mg, _host_guide(marginal))
    for y in range(H):
        assert np.array_equal(rg[y], _host_guide(row[y])), "row %d" % y


def test_the_weight_is_the_footprint_not_the_texels_own_luminance(gpu_ctx_factory):
    """the sun's eight neighbours carry the bled luminance: against the own-luminance rule their density is off by orders of magnitude"""
    side = _Side(gpu_ctx_factory(16, 16), "sun")
    _m, _r, density = side.tables()
    own = F.distribution(_map("sun"), F.own_weight(_map("sun")))["density"]
    foot = _dist("sun")["density"]
    assert abs(float(density[4, 10]) / foot[4, 10] - 1.0) < 1e-6
    assert float(density[4, 10]) / own[4, 10] > 1e4 and float(density[3, 8]) / own[3, 8] > 1e3


# ---- picks, directions, round trip, pdf: the checks of test_env_pins on the float tables --------------------------------------------------

@pytest.mark.parametrize("name", ["one", "odd", "wave", "long", "sun", "seam", "top_dim", "plateau"])
def test_picks_directions_round_trip_and_pdf(gpu_ctx_factory, name):
    TP._check_side(_Side(gpu_ctx_factory(16, 16), name), "float:" + name)


def test_picks_directions_and_round_trip_with_the_sun_in_the_polar_row(gpu_ctx_factory):
    """Map `top` puts 58 % of the draws into row 0 of 64, inside the polar caps, where u is ill-conditioned: 1.8 % of them lie within the
    pdf check's margin of a texel edge, above the 1 % that check allows before it means anything.  So here: the picks, the directions
    and the round trip (all table-driven).  The pdf across the v wrap is asserted on `top_dim` above: the same map and footprint with
    the sun at 1 / 32, which leaves 0.5 % of the draws unclear (both shares from the float64 distribution, before any device ran)."""
    side, name = _Side(gpu_ctx_factory(16, 16), "top"), "float:top"
    tables, r, d, pdf, texel, back = TP._draws(side, name)
    TP._check_picks(r, texel, tables, name)
    rnd = slice(len(r) - TP.N_RANDOM, len(r))
    TP._check_directions(r[rnd], d[rnd], texel[rnd], tables, name)
    TP._check_round_trip(back[rnd], texel[rnd], name)
    assert np.all(np.isfinite(pdf)) and np.all(pdf > 0)


@pytest.mark.parametrize("name", ["noise", "plateau"])
def test_histogram_against_p64(gpu_ctx_factory, name):
    side = _Side(gpu_ctx_factory(16, 16), name)
    _d, _pdf, texel = side.sample(np.stack([TP._random_values(TP.N_RANDOM, 61), TP._random_values(TP.N_RANDOM, 62)], axis=1))
    TP._check_histogram(texel, "float:" + name, "device, float map %s" % name)


@pytest.mark.parametrize("name", ["sun", "odd"])
def test_pdf_integrates_to_one(gpu_ctx_factory, name):
    TP._check_pdf_integral(_Side(gpu_ctx_factory(16, 16), name), "float:" + name)


# ---- the lookup ----------------------------------------------------------------------------------------------------------------------

def _lookup_error(ctx, name, uv):
    img = _map(name)
    got = ctx.tex2d_batch("hdr", 0, uv)
    assert np.all(got[:, 3] == np.float32(1.0)), "alpha 1"
    want = F.texture(img, uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64))
    tap = F.taps(img, uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64)).max(axis=1, keepdims=True)
    err = np.abs(got[:, 0:3].astype(np.float64) - want)
    assert np.all(err[np.broadcast_to(tap == 0.0, err.shape)] == 0.0), "four black taps give black"
    return err / np.where(tap > 0.0, tap, 1.0)


@pytest.mark.parametrize("name", ["lookup", "sun", "top"])
def test_lookup_with_exact_weights(gpu_ctx_factory, name):
    """(u, v) multiples of 2^-10 (from a little outside [0, 1]: the wraps): u W - 1/2 and the weights are exact in binary32"""
    side = _Side(gpu_ctx_factory(16, 16), name, sampling=False)
    g = (np.arange(-64, 1024 + 65, dtype=np.float64) / 1024.0)
    rng = np.random.RandomState(8)
    uv = np.stack([g[rng.randint(0, len(g), 60000)], g[rng.randint(0, len(g), 60000)]], axis=1).astype(np.float32)
    # ... and every grid point of the rows / columns through the 6e4 texels
    uv = np.concatenate([uv, np.stack([g, np.full(len(g), 5.5 / 16.0)], axis=1).astype(np.float32), np.stack([np.full(len(g), 9.5 / 32.0), g], axis=1).astype(np.float32)])
    err = _lookup_error(side.ctx, name, uv)
    print("float map %s, %d lookups at multiples of 2^-10: worst error %.3g of the largest tap (bound %.3g)" % (name, len(uv), err.max(), 6 * 2.0 ** -24))
    assert err.max() <= 6 * 2.0 ** -24
    # the same lookup is what a miss sees
    d = E.direction(np.array([9, 10, 31]), np.array([4, 5, 0]), 0.25, 0.75, 32, 16).astype(np.float32)
    if name != "top":
        rgb, _p, _t = side.ctx.env_eval_batch(d, with_pdf=False)
        u, v = G.latlong(d)
        want = F.texture(_map(name), u, v)
        tap = F.taps(_map(name), u, v).max(axis=1, keepdims=True)
        assert np.max(np.abs(rgb.astype(np.float64) - want) / tap) <= BOUND["lookup"]


@pytest.mark.parametrize("name", ["lookup", "odd", "wave"])
def test_lookup_at_random_coordinates(gpu_ctx_factory, name):
    side = _Side(gpu_ctx_factory(16, 16), name, sampling=False)
    uv = np.random.RandomState(9).uniform(-0.25, 1.25, (100000, 2)).astype(np.float32)
    err = _lookup_error(side.ctx, name, uv)
    print("float map %s, %d random lookups: worst error %.3g of the largest tap (bound %.3g)" % (name, len(uv), err.max(), BOUND["lookup"]))
    assert 0.0 < BOUND["lookup"] < 1e-4 and err.max() <= BOUND["lookup"]


# ---- transport ---------------------------------------------------------------------------------------------------------------------------

FRAMES = 1024


def _float_quad_scene(tilt, use_mis, sampling):
    sc = TP._quad_scene(tilt, use_mis, sampling)
    sc.hdr_map = _map("sun")
    return sc


def _expectation(tilt):
    def make():
        irr, residue = F.irradiance(_map("sun"), TP._normal(tilt)[1], sub=16)
        print("irradiance of the float sun map on the normal tilted %g degrees: %s, quadrature residue %.3g" % (tilt, irr, residue))
        assert residue < 2e-5
        return TP.ALBEDO * irr / np.pi

    return TP._cached(("float expectation", tilt), make)


@pytest.mark.parametrize("tilt", [0.0, 50.0])
def test_transport_under_the_float_sun(gpu_ctx_factory, tilt):
    want = _expectation(tilt)[None, :]
    est = {}
    for label, (use_mis, sampling) in TP.ESTIMATORS.items():
        e = est[label] = TP._gpu_estimate8(gpu_ctx_factory(TP.TW, TP.TH), _float_quad_scene(tilt, use_mis, sampling), FRAMES)
        print("tilt %g, %s: mean %s, median relative standard error %.4f" % (tilt, label, e.mean.mean(axis=0), np.median(e.se / want)))
        _assert_agree(_z(e.mean, e.se, want, 0.0, systematic=1e-3), "quad under the float sun map, tilt %g, %s, against quadrature" % (tilt, label))
    on = est["mis, sampler on"]
    assert np.median(on.se / want) <= 0.01, "the sampler's noise floor: 0.41 % predicted for the light sample alone, 1 % allowed"
    assert np.median(on.se) < 0.5 * np.median(est["mis, sampler off"].se) and np.median(on.se) < 0.5 * np.median(est["bsdf"].se)
    with pytest.raises(AssertionError):
        _assert_agree(_z(on.mean, on.se, want * 1.05, 0.0, systematic=1e-3), "the expectation x 1.05 must be refused")


# ---- the project's invariants: the same bits however the frames are rendered -------------------------------------------------------------

IW, IH, IFRAMES = 64, 40, 12


def _invariant_scene():
    return TP._cached(("float invariant scene",), lambda: _float_quad_scene(50.0, True, True))


def _accumulated(factory, compact=pod.COMPACT_FAST, tail=0, per_pass=1, in_flight=1, order=pod.ORDER_ROWS, scene=None, prepare=None):
    ctx = factory(IW, IH)
    (scene or _invariant_scene()).upload(ctx)
    if prepare:
        prepare(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, compact, pod.CONDUCTOR_REFERENCE)
    ctx.set_pixel_order(order)
    ctx.set_tail_bounce(tail)
    ctx.set_frames_per_pass(per_pass)
    ctx.set_passes_in_flight(in_flight)
    ctx.reset_frame_number()
    for _ in range(IFRAMES // per_pass // in_flight):
        for _ in range(in_flight):
            ctx.render_frame()
        ctx.accumulate()
    ctx.sync()
    assert ctx.frame_number() == IFRAMES
    acc = ctx.read_accumulation()
    if order == pod.ORDER_TILES:  # back to rows
        rows = np.zeros_like(acc)
        rows[capi.tile_pixel_map(IW, IH, 1, 0, 1, tiled=True)] = acc
        acc = rows
    ctx.set_passes_in_flight(1)
    ctx.set_pixel_order(pod.ORDER_ROWS)
    return acc


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def base(gpu_ctx_factory):
    acc = _accumulated(gpu_ctx_factory)
    assert np.all(np.isfinite(acc)) and acc.max() > 1.0, "the sun must be in the picture"
    return acc


@pytest.mark.parametrize("how", [dict(per_pass=4), dict(in_flight=3), dict(compact=pod.COMPACT_ORDERED), dict(tail=3), dict(order=pod.ORDER_TILES),
                                 dict(per_pass=4, in_flight=3, tail=3, order=pod.ORDER_TILES)],
                         ids=["4 frames per pass", "3 passes in flight", "classic pipeline", "tail kernel from bounce 3", "tiles", "all of them"])
def test_accumulation_does_not_depend_on_how_the_frames_are_rendered(gpu_ctx_factory, base, how):
    assert _same(base, _accumulated(gpu_ctx_factory, **how))


# ---- replacement ---------------------------------------------------------------------------------------------------------------------------

def _eight_bit_scene():
    sc = TP._quad_scene(50.0, True, True)  # (under test_env_pins' 8-bit map A)
    return sc


def test_an_eight_bit_upload_replaces_a_float_map_and_the_other_way_round(gpu_ctx_factory, base):
    fresh8 = _accumulated(gpu_ctx_factory, scene=_eight_bit_scene())
    assert not _same(fresh8, base)

    def float_then_eight(ctx):
        ctx.upload_env_float(_map("top"))
        ctx.upload_texture("hdr", TP._map("A"))  # (the sampler is on: the new map gets new tables)

    def eight_then_float(ctx):
        ctx.upload_texture("hdr", TP._map("B"))
        ctx.upload_env_float(_map("sun"))
        assert np.array_equal(ctx.read_env_float().view(np.uint32), _map("sun").view(np.uint32))

    assert _same(fresh8, _accumulated(gpu_ctx_factory, scene=_eight_bit_scene(), prepare=float_then_eight))
    assert _same(base, _accumulated(gpu_ctx_factory, prepare=eight_then_float))
    # ... and with the sampler switched on only afterwards (nxhip_set_env_sampling(1) on a float map builds the tables)
    late = _float_quad_scene(50.0, True, False)
    assert _same(base, _accumulated(gpu_ctx_factory, scene=late, prepare=lambda ctx: ctx.set_env_sampling(True)))


def test_clear_textures_gives_the_flat_background(gpu_ctx_factory, base):
    flat = TP._quad_scene(50.0, True, False)
    flat.hdr_map = None
    want = _accumulated(gpu_ctx_factory, scene=flat)
    assert not _same(want, base)

    def clear(ctx):
        ctx.clear_textures()
        with pytest.raises(capi.NexusError):
            ctx.read_env_float()

    assert _same(want, _accumulated(gpu_ctx_factory, prepare=clear))


# ---- refusals: on the host, before anything is allocated or launched ----------------------------------------------------------------------

def test_bad_maps_are_refused_and_change_nothing(gpu_ctx_factory):
    import ctypes as C

    ctx = gpu_ctx_factory(IW, IH)
    _invariant_scene().upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)

    def frame():
        ctx.reset_frame_number()
        ctx.render_frame()
        return ctx.read_radiance().copy()

    before = frame()
    tables = ctx.read_env_tables()
    good = _map("seam")
    L = ctx.L
    for what, value in (("NaN", np.nan), ("a negative component", -1.0), ("inf", np.inf), ("-inf", -np.inf), ("-0.0 is fine, -1e-30 is not", -1e-30)):
        img = good.copy()
        img[7, 13, 1] = value
        with pytest.raises(capi.NexusError):
            ctx.upload_env_float(img)
        assert L.nxhip_upload_env_float(ctx.h, img.ctypes.data_as(C.c_void_p), 32, 16) == 1, what  # NXHIP_ERR_INVALID
        assert _same(before, frame()), what
    for what, args in (("NULL", (None, 32, 16)), ("zero width", (good.ctypes.data_as(C.c_void_p), 0, 16)), ("zero height", (good.ctypes.data_as(C.c_void_p), 32, 0)),
                       ("too wide", (good.ctypes.data_as(C.c_void_p), 32769, 1)), ("too many texels", (good.ctypes.data_as(C.c_void_p), 32768, 8192))):
        assert L.nxhip_upload_env_float(ctx.h, *args) == 1, what  # (sizes are refused before the array is read)
        assert _same(before, frame()), what
    after = ctx.read_env_tables()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(tables, after))
    assert np.array_equal(ctx.read_env_float().view(np.uint32), _map("sun").view(np.uint32))
    # a valid map is still taken afterwards
    ctx.upload_env_float(good)
    assert not _same(before, frame())
