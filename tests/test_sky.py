"""Sun and sky on the CPU: the entry points of nxhip_set_sky that need no device (nxhip_sky_defaults, nxhip_sky_sun_light and the
validator it shares with nxhip_set_sky), the Python wrappers, and the float64 reference of tests/test_gpu_sky.py (tests/sky_reference.py)
checked for sense, so that the yardstick is not nonsense."""
import ctypes as C

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import sky_reference as R


def direction(azimuth_deg, elevation_deg):
    a, e = np.radians(azimuth_deg), np.radians(elevation_deg)
    return np.array([np.cos(e) * np.cos(a), np.sin(e), np.cos(e) * np.sin(a)])


def test_defaults_are_the_documented_values():
    s = capi.sky_defaults()
    assert np.allclose(s["sunDirection"], [np.sqrt(0.5), np.sqrt(0.5), 0.0], rtol=0, atol=1e-7)  # 45 degrees of elevation along +x
    assert s["sunAngularRadius"] == np.float32(0.004675) and np.all(s["sunIrradiance"] == 1.0) and s["altitude"] == 1.0
    assert s["rayleighScale"] == 1.0 and s["mieScale"] == 1.0 and s["mieG"] == np.float32(0.8) and np.all(s["groundAlbedo"] == np.float32(0.3))
    assert (s["width"], s["height"], s["viewSteps"], s["lightSteps"], s["sunDisc"]) == (2048, 1024, 64, 16, 0)
    assert s.tobytes() == pod.Sky().tobytes()  # the Python mirror of the defaults is the library's, byte for byte
    assert capi.lib().nxhip_sky_defaults(None) == 1 and b"NULL" in capi.lib().nxhip_last_error()


def test_the_struct_crosses_the_boundary_as_the_header_lays_it_out():
    assert pod.SKY_DT.itemsize == 76 and pod.SKY_DT.fields["width"][1] == 56 and pod.SKY_DT.fields["sunDisc"][1] == 72
    assert capi.lib().nxhip_abi_stamp() == capi.abi_stamp()  # (the stamp hashes sizeof(nx_sky) and its offsets)
    assert {"nxhip_set_sky", "nxhip_sky_defaults", "nxhip_sky_sun_light", "nxhip_sky_radiance_batch"} <= set(capi.HIP_SYMBOLS)
    assert capi.SIGNATURES["nxhip_sky_radiance_batch"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p])
    # every field, through the wrapper and back out of the record the library wrote
    sky = pod.Sky(sunDirection=(0.0, 0.0, -3.0), sunAngularRadius=0.02, sunIrradiance=(3.0, 2.0, 1.0), altitude=1234.0)
    light = capi.sky_sun_light(sky)
    assert light["type"] == pod.ALIGHT_DIRECTIONAL and light["angularRadius"] == np.float32(0.02) and light["intensity"] == 1.0
    assert np.array_equal(light["direction"], np.array([0.0, 0.0, 1.0], np.float32))  # normalised and negated
    with pytest.raises(ValueError):
        pod.Sky(noSuchField=1)


@pytest.mark.parametrize("altitude", [1.0, 3000.0])
@pytest.mark.parametrize("elevation", [90.0, 30.0, 2.0, 0.1, -1.0])
def test_sun_light_against_the_reference_transmittance(elevation, altitude):
    """colour x intensity = sunIrradiance x T_sun(observer) with 256 segments, relative 1e-6: one binary32 rounding of a binary64 value
    (6e-8) with room for the two sides' different arithmetic"""
    irradiance = np.array([1.5, 1.0, 0.25])
    sky = pod.Sky(sunDirection=7.0 * direction(130.0, elevation), altitude=altitude, sunIrradiance=irradiance, sunAngularRadius=0.01)
    light = capi.sky_sun_light(sky)
    P = R.Params(sky)
    want = P.irradiance * R.sun_transmittance(P, 256)
    got = light["colour"].astype(np.float64) * float(light["intensity"])
    if elevation < 0 and altitude == 1.0:
        assert np.all(want == 0) and np.all(got == 0)  # below the geometric horizon (the dip at 1 m is 0.03 degrees)
    else:
        assert np.all(want > 0)  # (-1 degree from 3000 m is above that horizon's 1.76-degree dip)
        assert np.max(np.abs(got - want) / want) < 1e-6
    assert np.max(np.abs(light["direction"].astype(np.float64) + P.sun)) < 1e-7
    assert light["angularRadius"] == np.float32(0.01) and light["type"] == pod.ALIGHT_DIRECTIONAL and not np.any(light["position"])


REFUSALS = [
    ("a NaN direction", dict(sunDirection=(np.nan, 1.0, 0.0))),
    ("an infinite irradiance", dict(sunIrradiance=(np.inf, 1.0, 1.0))),
    ("a NaN altitude", dict(altitude=np.nan)),
    ("a NaN angular radius", dict(sunAngularRadius=np.nan)),
    ("a NaN scale", dict(mieScale=np.nan)),
    ("an infinite g", dict(mieG=-np.inf)),
    ("a NaN albedo", dict(groundAlbedo=(0.1, np.nan, 0.1))),
    ("a zero direction", dict(sunDirection=(0.0, 0.0, 0.0))),
    ("a negative irradiance", dict(sunIrradiance=(1.0, -0.5, 1.0))),
    ("a negative albedo", dict(groundAlbedo=(-0.1, 0.3, 0.3))),
    ("an albedo above 1", dict(groundAlbedo=(0.3, 0.3, 1.5))),
    ("a negative Rayleigh scale", dict(rayleighScale=-1.0)),
    ("a negative Mie scale", dict(mieScale=-1.0)),
    ("g = 1", dict(mieG=1.0)),
    ("g = -1", dict(mieG=-1.0)),
    ("an altitude below 1", dict(altitude=0.5)),
    ("an altitude above 50000", dict(altitude=50001.0)),
    ("a negative angular radius", dict(sunAngularRadius=-0.001)),
    ("an angular radius of pi/2", dict(sunAngularRadius=np.float32(np.pi / 2) + np.float32(1e-6))),
    ("a zero width", dict(width=0)),
    ("a zero height", dict(height=0)),
    ("a width above 32768", dict(width=32769, height=1)),
    ("a height above 32768", dict(width=1, height=32769)),
    ("more than 2^27 texels", dict(width=32768, height=4097)),
    ("no view steps", dict(viewSteps=0)),
    ("too many view steps", dict(viewSteps=1025)),
    ("no light steps", dict(lightSteps=0)),
    ("too many light steps", dict(lightSteps=1025)),
    ("sunDisc above 1", dict(sunDisc=2)),
    ("a disc without a radius", dict(sunDisc=1, sunAngularRadius=0.0)),
]


@pytest.mark.parametrize("what,fields", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_sun_light_refuses_what_the_validator_refuses(what, fields):
    L = capi.lib()
    sky = np.ascontiguousarray(pod.Sky(**fields)).reshape(1)
    out = np.frombuffer(bytes([7]) * 64, dtype=pod.ALIGHT_DT).copy()
    before = out.tobytes()
    assert L.nxhip_sky_sun_light(capi._ptr(sky), capi._ptr(out)) == 1, what  # NXHIP_ERR_INVALID
    assert b"nxhip_sky_sun_light" in L.nxhip_last_error() and out.tobytes() == before, what
    with pytest.raises(capi.NexusError):
        capi.sky_sun_light(sky)


def test_sun_light_refuses_null_and_accepts_the_edges():
    L = capi.lib()
    sky = np.ascontiguousarray(pod.Sky()).reshape(1)
    out = np.zeros(1, dtype=pod.ALIGHT_DT)
    assert L.nxhip_sky_sun_light(None, capi._ptr(out)) == 1 and L.nxhip_sky_sun_light(capi._ptr(sky), None) == 1
    for fields in (dict(altitude=1.0), dict(altitude=50000.0), dict(sunAngularRadius=0.0), dict(mieG=0.99), dict(mieG=-0.99), dict(groundAlbedo=(0.0, 1.0, 0.5)),
                   dict(width=32768, height=4096), dict(viewSteps=1024, lightSteps=1), dict(rayleighScale=0.0, mieScale=0.0), dict(sunDisc=1)):
        capi.sky_sun_light(pod.Sky(**fields))
    assert np.all(capi.sky_sun_light(pod.Sky(rayleighScale=0.0, mieScale=0.0))["colour"] == 1.0)  # no atmosphere: T = 1


# ---- the reference itself ---------------------------------------------------------------------------------

def test_reference_zenith_is_blue_and_a_setting_sun_is_red():
    zenith = R.radiance(R.Params(pod.Sky(sunDirection=direction(0.0, 60.0))), [direction(0.0, 90.0)])[0]
    assert zenith[2] > 2.0 * zenith[0] and zenith[2] > zenith[1] > zenith[0]
    horizon = R.radiance(R.Params(pod.Sky(sunDirection=direction(0.0, 0.0))), [direction(0.0, 0.5)])[0]
    assert horizon[0] > 2.0 * horizon[2] and horizon[0] > horizon[1] > horizon[2]


def test_reference_without_an_atmosphere_is_the_lit_ground():
    """both scales 0: the sky is black, and the planet is a Lambertian sphere under the unattenuated sun"""
    sky = pod.Sky(sunDirection=direction(0.0, 30.0), rayleighScale=0.0, mieScale=0.0, groundAlbedo=(0.5, 0.25, 1.0), sunIrradiance=(2.0, 2.0, 2.0))
    got = R.radiance(R.Params(sky), [direction(40.0, 20.0), direction(0.0, -90.0)])
    assert np.all(got[0] == 0)
    assert np.allclose(got[1], np.array([0.5, 0.25, 1.0]) / np.pi * 2.0 * np.sin(np.radians(30.0)), rtol=1e-12)  # the nadir's normal is +y


def test_reference_default_quadrature_is_within_one_percent_of_a_fine_one():
    """64 x 16 steps against 1024 x 128 at altitude 1 m, |difference| / the view's largest channel, over the zenith, 2 and 0.2 degrees above
    the horizon towards the sun and two oblique views, for sun elevations 60, 30, 5, 0 and -4 degrees.
    MEASURED with this reference: 0.72 % (the oblique view at azimuth 200, elevation 10 under the -4-degree sun, whose ray crosses the
    planet's shadow: a step in the integrand); 0.40 % (0.2 degrees above the horizon, sun at 0) over the four other views.  1024 x 128
    itself is within 0.05 % of 2048 x 256."""
    views = [direction(0.0, 90.0), direction(0.0, 2.0), direction(0.0, 0.2), direction(70.0, 35.0), direction(200.0, 10.0)]
    worst = 0.0
    for elevation in (60.0, 30.0, 5.0, 0.0, -4.0):
        P = R.Params(pod.Sky(sunDirection=direction(0.0, elevation)))
        coarse, fine = R.radiance(P, views), R.radiance(P, views, nv=1024, nl=128)
        assert np.all(fine > 0)
        worst = max(worst, float(np.max(np.abs(coarse - fine) / np.max(fine, axis=1, keepdims=True))))
    print("default quadrature against 1024 x 128: worst %.4f %%" % (100.0 * worst))
    assert worst < 0.01


@pytest.mark.parametrize("size,alpha,sun", [((64, 32), 0.1, direction(30.0, 25.0)), ((256, 128), 0.03, direction(180.0, 40.0)), ((64, 32), 0.1, direction(0.0, 90.0)),
                                            ((130, 3), 0.3, direction(-90.0, -10.0)), ((512, 256), 0.004675, direction(12.0, 45.0))])
def test_reference_disc_carries_the_caps_solid_angle(size, alpha, sun):
    W, H = size
    P = R.Params(pod.Sky(sunDirection=sun, sunAngularRadius=alpha, sunDisc=1))
    c, k = R.disc_scale(P, W, H)
    omega = R.texel_solid_angles(W, H)
    assert abs(np.sum(omega) * W - 4.0 * np.pi) < 1e-12 and np.all((c >= 0) & (c <= 1)) and np.any(c > 0)
    alpha = P.alpha  # (the record's binary32 value)
    cap = R.cap_solid_angle(alpha)  # 2 pi (1 - cos alpha) as 4 pi sin^2(alpha / 2): the difference itself cancels to 1e-11 at 0.0047
    assert abs(cap - 2.0 * np.pi * (1.0 - np.cos(alpha))) <= 1e-10 * cap
    assert abs(np.sum(c * k * omega[:, None]) - cap) <= 1e-12 * cap
    assert 0.5 < k < 2.0  # 64 sub-positions per texel resolve the cap: the factor corrects, it does not invent


def test_reference_refuses_a_disc_between_the_sub_positions():
    """a 7 x 5 map's sub-positions are 0.11 rad apart in longitude and 0.079 in latitude: a disc of 0.004675 rad centred between four of them holds none"""
    W, H = 7, 5
    u, v = (3 * 8 + 4) / (W * 8.0), (2 * 8 + 4) / (H * 8.0)  # the corner shared by four sub-cells
    phi, theta = np.pi / 2 - np.pi * v, 2 * np.pi * u - np.pi
    sun = np.array([np.cos(phi) * np.cos(theta), np.sin(phi), np.cos(phi) * np.sin(theta)])
    with pytest.raises(ValueError, match="larger map or a larger sunAngularRadius"):
        R.disc_term(R.Params(pod.Sky(sunDirection=sun, sunDisc=1)), W, H)
    assert np.any(R.disc_term(R.Params(pod.Sky(sunDirection=sun, sunDisc=1, sunAngularRadius=0.1)), W, H) > 0)
