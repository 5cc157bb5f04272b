"""Sun and sky on the device (nxhip_set_sky): the generated map and the hook against the float64 model (tests/sky_reference.py), the baked
sun disc, the installation as a float environment map, the project's invariants, replacement and refusals.

Maps, all with the default steps 64 x 16: 1 x 1 (the smallest), 7 x 5 (odd sizes), 130 x 3 (a row that is no multiple of a wave), 64 x 32
(the main map, under every parameter set of SETS).

The error of a texel or direction is max over channels |device - float64| / max(largest channel of that texel, 1e-6 x the map's largest
value).  The bound is 4 x MEASURED, the device's worst figure on exactly these inputs (an MI355X), and must stay below the condition 1e-3:
a kernel that forms heights as |p| - Rg in binary32 (half a metre at 6.4e6 m) cannot meet it.
                         measured    bound      condition
  map                    1.22e-5     4.9e-5     < 1e-3    (set "g0.9", 64 x 32, texel (39, 13) beside the sun: the peaked phase function
                                                           magnifies the direction's binary32 rounding; the next are "el5" 8.0e-6 and
                                                           "el-4" 7.3e-6; the small maps 2.7e-7 .. 9.8e-7)
  hook, 256 directions   6.06e-7     2.4e-6     < 1e-3    (altitude 3000 m; no direction is within 1e-4 rad of the switch: none left out)
  disc, map minus sky    5.66e-8     2.3e-7     < 1e-3    (256 x 128, across the seam: one binary32 rounding of the sum sky + disc)
For the record (device): the disc's energy is within 6e-8 of Lsun x the cap's solid angle on all four maps (bound 1e-5).
"""
import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import scene_helpers as SH
from tests import sky_reference as R
from tests.test_sky import REFUSALS, direction

pytestmark = pytest.mark.gpu

# the device's worst figures on the inputs below (where: the table above)
MEASURED = dict(map=1.22e-5, hook=6.06e-7, disc=5.66e-8)
CONDITION = 1e-3


def _bound(kind):
    bound = 4.0 * MEASURED[kind]
    assert bound < CONDITION
    return bound


def _sky(azimuth=40.0, elevation=30.0, **fields):
    fields.setdefault("width", 64)
    fields.setdefault("height", 32)
    return pod.Sky(sunDirection=direction(azimuth, elevation), **fields)


SETS = {
    "el60": _sky(elevation=60.0),
    "el5": _sky(elevation=5.0),
    "el0": _sky(elevation=0.0),
    "el-4": _sky(elevation=-4.0),
    "alt3000": _sky(altitude=3000.0),
    "alt3000 el-1": _sky(elevation=-1.0, altitude=3000.0),
    "mie0": _sky(mieScale=0.0),
    "mie5": _sky(mieScale=5.0),
    "rayleigh0": _sky(rayleighScale=0.0),
    "g-0.5": _sky(mieG=-0.5),
    "g0.9": _sky(mieG=0.9, elevation=10.0),
    "seam": _sky(azimuth=180.0, elevation=20.0),
    "steps 1 x 1": _sky(viewSteps=1, lightSteps=1),
    "steps 65 x 3": _sky(viewSteps=65, lightSteps=3),
    "coloured": _sky(sunIrradiance=(20.0, 10.0, 0.5), groundAlbedo=(0.0, 1.0, 0.4), elevation=15.0),
    "1 x 1": _sky(width=1, height=1),
    "7 x 5": _sky(width=7, height=5),
    "130 x 3": _sky(width=130, height=3),
}


def _error(got, want):
    """the module's measure, per texel: (n, 3) against (n, 3)"""
    got, want = np.asarray(got, np.float64).reshape(-1, 3), np.asarray(want, np.float64).reshape(-1, 3)
    scale = np.maximum(np.max(want, axis=1), 1e-6 * np.max(want))
    return np.max(np.abs(got - want), axis=1) / scale


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(16, 16)


@pytest.fixture(scope="module")
def reference_maps():
    return {}


def _reference(cache, name):
    if name not in cache:
        sky = SETS[name]
        W, H = int(sky["width"]), int(sky["height"])
        cache[name] = R.radiance(R.Params(sky), R.map_directions(W, H).reshape(-1, 3)).reshape(H, W, 3)
    return cache[name]


# ---- the map and the hook against float64 ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SETS))
def test_map_against_float64(ctx, reference_maps, name):
    sky = SETS[name]
    ctx.set_sky(sky)
    got = ctx.read_env_float()
    want = _reference(reference_maps, name)
    assert got.shape == want.shape and got.dtype == np.float32 and np.all(np.isfinite(got)) and np.all(got >= 0)
    assert np.max(want) > 0
    err = _error(got, want)
    worst = int(np.argmax(err))
    print("sky map %-13s %3d x %-3d: worst %.3g at texel (%d, %d); largest value %.4g" % (name, want.shape[1], want.shape[0], err[worst], worst % want.shape[1],
                                                                                          worst // want.shape[1], np.max(want)))
    assert err[worst] <= _bound("map")


def _hook_directions():
    """256 unit directions for the observer at 3000 m: the special ones first, then random ones over the sphere"""
    P = R.Params(SETS["alt3000"])
    dip = np.degrees(np.arccos(R.RG / (R.RG + 3000.0)))
    special = [direction(0.0, 0.0), direction(123.0, 0.0), P.sun, direction(0.0, -90.0), direction(0.0, 90.0),
               direction(40.0, -dip + 0.01), direction(40.0, -dip - 0.01), direction(250.0, -dip + 0.01), direction(250.0, -dip - 0.01)]
    rng = np.random.RandomState(11)
    rest = rng.normal(size=(256 - len(special), 3))
    rest /= np.linalg.norm(rest, axis=1, keepdims=True)
    d = np.concatenate([np.array(special), rest]).astype(np.float32)
    d[0] = (1.0, 0.0, 0.0)  # exactly horizontal
    return d


def test_hook_against_float64(ctx):
    sky = SETS["alt3000"]
    P = R.Params(sky)
    d = _hook_directions()
    assert d.shape == (256, 3)
    keep = R.horizon_switch_distance(P, d) > 1e-4  # (the reference alone decides what is left out)
    assert np.count_nonzero(~keep) <= 2
    want = R.radiance(P, d)
    below = d[:, 1].astype(np.float64) < -np.sin(np.arccos(R.RG / (R.RG + 3000.0)))
    assert np.count_nonzero(below) > 60 and np.count_nonzero(~below) > 60 and below[6] and not below[5]  # both branches, and the pair at the switch
    got = ctx.sky_radiance(sky, d)
    err = _error(got[keep], want[keep])
    print("sky hook, 256 directions at 3000 m (%d left out): worst %.3g" % (np.count_nonzero(~keep), err.max()))
    assert err.max() <= _bound("hook")
    # the map kernel calls the same function: the hook on the texel centres' directions gives the map, to the rounding of the directions
    ctx.set_sky(sky)
    centres = R.map_directions(64, 32).reshape(-1, 3).astype(np.float32)
    assert _error(ctx.sky_radiance(sky, centres), ctx.read_env_float()).max() < 1e-4
    assert ctx.sky_radiance(sky, np.zeros((0, 3), np.float32)).shape == (0, 3)


# ---- the disc --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size,alpha", [((64, 32), 0.1), ((256, 128), 0.03)], ids=["64 x 32", "256 x 128"])
@pytest.mark.parametrize("where", ["seam", "zenith"])
def test_disc_against_float64(ctx, size, alpha, where):
    W, H = size
    sun = direction(180.0, 20.0) if where == "seam" else np.array([0.0, 1.0, 0.0])
    sky = pod.Sky(sunDirection=sun, sunAngularRadius=alpha, sunDisc=1, width=W, height=H, sunIrradiance=(3.0, 2.0, 1.0))
    P = R.Params(sky)
    want = R.disc_term(P, W, H)
    lit = np.max(want, axis=2) > 0
    if where == "seam":
        assert lit[:, 0].any() and lit[:, -1].any() and not lit[:, W // 2].any()  # the box crosses the u seam
    else:
        assert lit[0].all() and not lit[H // 2].any()  # the box covers row 0, every column of it
    ctx.set_sky(sky)
    with_disc = ctx.read_env_float().astype(np.float64)
    plain = sky.copy()
    plain["sunDisc"] = 0
    ctx.set_sky(plain)
    without = ctx.read_env_float().astype(np.float64)
    got = with_disc - without
    assert np.all(got[~lit] == 0)  # nothing outside the cap is touched
    scale = np.maximum(np.max(with_disc, axis=2), 1e-6 * np.max(with_disc))
    err = np.max(np.abs(got - want), axis=2) / scale
    omega = R.texel_solid_angles(W, H)[:, None, None]
    l_sun = P.irradiance * R.sun_transmittance(P, P.nl) / (np.pi * np.sin(P.alpha) ** 2)
    energy = np.sum(got * omega, axis=(0, 1)) / (l_sun * R.cap_solid_angle(P.alpha))
    print("sky disc %d x %d, %s: worst %.3g; energy / (Lsun x cap) - 1 = %s" % (W, H, where, err.max(), energy - 1.0))
    assert err.max() <= _bound("disc")
    assert np.all(np.abs(energy - 1.0) < 1e-5)


# ---- installation: a sky is a float map ----------------------------------------------------------------------------------------------------

IW = IH = 32
FRAMES = 4


def _cornell(ctx):
    SH.cornell_scene(IW, IH, path_length=4).upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)


def _frames(ctx):
    ctx.reset_frame_number()
    for _ in range(FRAMES):
        ctx.render_frame()
        ctx.accumulate()
    return ctx.read_accumulation().copy()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _tables(ctx):
    return list(ctx.read_env_tables()) + list(ctx.read_env_guides())


def _tables_equal(a, b):
    return len(a) == len(b) == 5 and all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


INSTALLED = _sky(elevation=25.0, sunDisc=1, sunAngularRadius=0.1, sunIrradiance=(20.0, 20.0, 20.0))


@pytest.fixture(scope="module")
def installed(gpu_ctx_factory):
    """a Cornell box under a sky set while the sampler is on: (context, texels, tables, frames, flavor)"""
    c = gpu_ctx_factory(IW, IH)
    _cornell(c)
    c.upload_env_float(np.full((2, 4, 3), 0.5, np.float32))
    c.set_env_sampling(True)
    c.set_sky(INSTALLED)  # (a new map under an enabled sampler gets new tables)
    texels = c.read_env_float()
    tables = _tables(c)
    frames = _frames(c)
    return c, texels, tables, frames, c.debug_pass_flavor()


def test_a_sky_is_installed_as_the_float_map_of_its_texels(gpu_ctx_factory, installed):
    _c, texels, tables, frames, flavor = installed
    assert texels.shape == (32, 64, 3) and texels.max() > 100.0 * np.median(texels)  # the disc is in it
    other = gpu_ctx_factory(IW, IH)
    _cornell(other)
    other.upload_env_float(texels)
    other.set_env_sampling(True)
    assert _tables_equal(tables, _tables(other))
    assert _same(frames, _frames(other))
    assert flavor == other.debug_pass_flavor()  # the float map's word
    # the sampler switched on only after the sky: nxhip_set_env_sampling(1) builds the tables
    other.clear_textures()
    other.set_sky(INSTALLED)
    with pytest.raises(capi.NexusError):
        other.read_env_tables()
    other.set_env_sampling(True)
    assert _same(other.read_env_float(), texels) and _tables_equal(tables, _tables(other))
    assert _same(frames, _frames(other))


def test_clear_textures_after_a_sky_is_a_context_that_never_had_one(gpu_ctx_factory, installed):
    fresh = gpu_ctx_factory(IW, IH)
    _cornell(fresh)
    want = _frames(fresh)
    assert not _same(want, installed[3])  # the sky lights the box
    fresh.set_sky(INSTALLED)
    fresh.set_env_sampling(True)
    assert _same(installed[3], _frames(fresh))
    fresh.clear_textures()
    with pytest.raises(capi.NexusError):
        fresh.read_env_float()
    assert _same(want, _frames(fresh))


def test_an_eight_bit_map_replaces_a_sky_and_a_sky_replaces_it(gpu_ctx_factory, installed):
    eight = SH.checker_texture(16, 8, 3)
    c = gpu_ctx_factory(IW, IH)
    _cornell(c)
    c.upload_texture("hdr", eight)
    c.set_env_sampling(True)
    want8 = _frames(c)
    assert not _same(want8, installed[3])
    c.set_sky(INSTALLED)  # a sky replaces an RGBA8 map
    assert _same(c.read_env_float(), installed[1]) and _tables_equal(installed[2], _tables(c))
    assert _same(installed[3], _frames(c))
    c.upload_texture("hdr", eight)  # ... and an RGBA8 upload replaces a sky
    with pytest.raises(capi.NexusError):
        c.read_env_float()
    assert _same(want8, _frames(c))
    c.set_sky(INSTALLED)
    c.upload_env_float(np.full((2, 4, 3), 0.5, np.float32))  # ... as a float upload does
    assert c.read_env_float().shape == (2, 4, 3)


# ---- refusals: on the host, through a live context, the previous map and tables left in place -----------------------------------------------

def _between_sub_positions():
    """a 7 x 5 map whose disc of 0.004675 rad is centred on a corner shared by four sub-cells (tests/test_sky.py)"""
    u, v = (3 * 8 + 4) / 56.0, (2 * 8 + 4) / 40.0
    phi, theta = np.pi / 2 - np.pi * v, 2 * np.pi * u - np.pi
    return pod.Sky(sunDirection=(np.cos(phi) * np.cos(theta), np.sin(phi), np.cos(phi) * np.sin(theta)), sunDisc=1, width=7, height=5)


def test_bad_skies_are_refused_and_change_nothing(installed):
    c, texels, tables, frames, _flavor = installed
    L = c.L
    assert L.nxhip_set_sky(c.h, None) == 1 and b"NULL" in L.nxhip_last_error()
    for what, fields in REFUSALS:
        sky = np.ascontiguousarray(pod.Sky(**fields)).reshape(1)
        assert L.nxhip_set_sky(c.h, capi._ptr(sky)) == 1 and b"nxhip_set_sky" in L.nxhip_last_error(), what  # NXHIP_ERR_INVALID
        out = np.zeros((1, 3), np.float32)
        assert L.nxhip_sky_radiance_batch(c.h, capi._ptr(sky), capi._ptr(np.array([[0, 1, 0]], np.float32)), 1, capi._ptr(out)) == 1, what
    with pytest.raises(capi.NexusError, match="larger map or a larger sunAngularRadius"):
        c.set_sky(_between_sub_positions())
    good = np.ascontiguousarray(INSTALLED).reshape(1)
    rgb = np.zeros((1, 3), np.float32)
    assert L.nxhip_sky_radiance_batch(c.h, capi._ptr(good), None, 1, capi._ptr(rgb)) == 1
    assert L.nxhip_sky_radiance_batch(c.h, capi._ptr(good), capi._ptr(np.array([[0, np.nan, 0]], np.float32)), 1, capi._ptr(rgb)) == 1
    assert L.nxhip_set_sky(None, capi._ptr(good)) != 0 and b"null context" in L.nxhip_last_error()
    assert _same(c.read_env_float(), texels) and _tables_equal(tables, _tables(c))
    assert _same(frames, _frames(c))
