"""The float64 restatement of the detail maps' rule (tests/detail_reference.py) against what the contract says in words: the sign
conventions of glTF's tangent space, mirrored texture coordinates, a mirroring instance transform, every fallback condition, and the
linear lookup.  No device: these pin the reference the GPU tests compare with."""
import numpy as np

from nexus_amd import pod
from tests import detail_reference as R

EYE4 = np.eye(4)
DOWN = np.array([[0.0, 0.0, -1.0]])  # the view looks straight down on a +z surface


def _tri(uvs, pos=((0, 0, 0), (1, 0, 0), (0, 1, 0)), normal=(0, 0, 1)):
    return pod.make_triangles(np.asarray([pos], np.float32), uvs=np.asarray([uvs], np.float32), normals=np.asarray([[normal] * 3], np.float32))


def _const(r, g, b, w=4, h=4):
    img = np.zeros((h, w, 4), np.uint8)
    img[...] = (r, g, b, 255)
    return img


# u runs towards +x, v runs DOWN the image, i.e. towards -y; the normal is +z
UV = ((0, 1), (1, 1), (0, 0))
UV_MIRRORED = ((1, 1), (0, 1), (1, 0))  # u -> 1 - u
HIT = np.array([[0.25, 0.25]], np.float32)


def _ns(uvs, img, transform=EYE4, d=DOWN, **kw):
    return R.shading_frame(_tri(uvs, **kw), HIT, d, transform, np.linalg.inv(transform), R.MAT_DIFFUSE, normal_map=img)


def test_flat_texel_gives_the_interpolated_normal_and_no_fallback():
    f = _ns(UV, _const(255, 255, 255))  # m = (1, 1, 1): tilted both ways, to have something to compare with
    g = _ns(UV, _const(128, 128, 255))
    assert not g["fell_back"][0] and not f["fell_back"][0]
    assert np.allclose(g["ns"][0], _unit((1 / 255, 1 / 255, 1.0)), atol=1e-15)
    assert np.allclose(f["ns"][0], _unit((1, 1, 1)), atol=1e-15)


def _unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


def test_red_tilts_towards_plus_x_and_green_towards_plus_y():
    red = _ns(UV, _const(255, 128, 255))["ns"][0]
    green = _ns(UV, _const(128, 255, 255))["ns"][0]
    assert red[0] > 0.7 and abs(red[1]) < 0.01 and red[2] > 0
    assert green[1] > 0.7 and abs(green[0]) < 0.01 and green[2] > 0
    low = _ns(UV, _const(0, 128, 255))["ns"][0]
    assert low[0] < -0.7


def test_normal_scale_multiplies_x_and_y_only():
    img = _const(192, 64, 230)
    c = np.array([192, 64, 230]) / 255.0
    for s in (0.8, 1.0, 2.0):
        got = R.shading_frame(_tri(UV), HIT, DOWN, EYE4, EYE4, R.MAT_PLASTIC, normal_map=img, normal_scale=s)["ns"][0]
        assert np.allclose(got, _unit(((2 * c[0] - 1) * s, (2 * c[1] - 1) * s, 2 * c[2] - 1)), atol=1e-15)


def test_mirroring_u_flips_the_red_tilt_only():
    img = _const(220, 200, 240)
    a, b = _ns(UV, img), _ns(UV_MIRRORED, img)
    assert not a["fell_back"][0] and not b["fell_back"][0]
    assert np.allclose(b["ns"][0], a["ns"][0] * (-1, 1, 1), atol=1e-15)


def test_a_mirroring_instance_mirrors_the_shading_normal():
    img = _const(220, 200, 240)
    M = np.diag([-1.0, 1.0, 1.0, 1.0])
    a, b = _ns(UV, img), _ns(UV, img, transform=M)
    assert np.allclose(b["N"][0], (0, 0, 1)) and not b["fell_back"][0]
    assert np.allclose(b["ns"][0], a["ns"][0] * (-1, 1, 1), atol=1e-15)
    # ... and a rotation with a non-uniform scale carries the tangent with the geometry: u still runs along the image of +x
    c, s = np.cos(0.7), np.sin(0.7)
    Rz = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]) @ np.diag([2.0, 0.5, 1.5, 1.0])
    r = _ns(UV, _const(255, 128, 255), transform=Rz)["ns"][0]
    g = 1.0 / 255.0  # (byte 128 is a 255th above the middle) ... and green along the image of +y
    assert np.allclose(r, _unit((c - s * g, s + c * g, 1.0)), atol=1e-12)


def test_the_flip_negates_ns_with_the_normals_except_for_a_dielectric():
    img = _const(220, 200, 240)
    up = np.array([[0.0, 0.0, 1.0]])  # arriving from below: a back-face hit
    front = _ns(UV, img)
    back = R.shading_frame(_tri(UV), HIT, up, EYE4, EYE4, R.MAT_DIFFUSE, normal_map=img)
    glass = R.shading_frame(_tri(UV), HIT, up, EYE4, EYE4, R.MAT_DIELECTRIC, normal_map=img)
    assert np.allclose(back["ns"][0], -front["ns"][0]) and np.allclose(back["N"][0], (0, 0, -1)) and not back["fell_back"][0]
    assert np.allclose(glass["ns"][0], front["ns"][0]) and np.allclose(glass["N"][0], (0, 0, 1)) and not glass["fell_back"][0]


def test_every_fallback_condition_returns_the_interpolated_normal():
    img = _const(255, 128, 255)
    # det = 0: the three texture coordinates on one line
    f = _ns(((0, 0), (1, 1), (2, 2)), img)
    assert f["fell_back"][0] and np.allclose(f["ns"][0], (0, 0, 1))
    # the projected tangent has length 0: the vertex normals lie along the tangent itself
    d = _unit((-1, 0, -1))[None]
    f = _ns(UV, img, d=d, normal=(1, 0, 0))
    assert f["fell_back"][0] and np.allclose(f["ns"][0], (1, 0, 0))
    # ns has length 0: m = (0, 0, 0) half way between a texel of 0s and a texel of 255s
    two = np.zeros((1, 2, 4), np.uint8)
    two[0, 1] = 255
    t = _tri(((0.5, 1), (0.5 + 1e-3, 1), (0.5, 0)))
    f = R.shading_frame(t, np.zeros((1, 2), np.float32), DOWN, EYE4, EYE4, R.MAT_DIFFUSE, normal_map=two)
    assert np.array_equal(R.tex2d_linear(two, np.float32(0.5), np.float32(0.3))[:3], (0.5, 0.5, 0.5))
    assert f["fell_back"][0] and np.allclose(f["ns"][0], (0, 0, 1))
    # ns is not finite
    f = R.shading_frame(_tri(UV), HIT, DOWN, EYE4, EYE4, R.MAT_DIFFUSE, normal_map=img, normal_scale=np.inf)
    assert f["fell_back"][0] and np.allclose(f["ns"][0], (0, 0, 1))
    # the view is below the mapped horizon: ns leans 45 degrees towards +x, the view comes in at 20 degrees above the surface from -x
    graze = np.array([[np.cos(np.radians(20)), 0.0, -np.sin(np.radians(20))]])
    f = _ns(UV, img, d=graze)
    assert f["ns_dot_v"][0] < 0 < f["n_dot_v"][0]
    assert f["fell_back"][0] and np.allclose(f["ns"][0], (0, 0, 1))
    # ... and from +x the same view is above it
    f = _ns(UV, img, d=graze * (-1, 1, 1))
    assert not f["fell_back"][0] and f["ns"][0][0] > 0.7
    # no normal map: never a fallback
    f = R.shading_frame(_tri(UV), HIT, DOWN, EYE4, EYE4, R.MAT_DIFFUSE)
    assert not f["fell_back"][0] and np.allclose(f["ns"][0], (0, 0, 1))


def test_roughness_is_scaled_by_the_green_channel():
    img = _const(10, 51, 200)
    f = R.shading_frame(_tri(UV), HIT, DOWN, EYE4, EYE4, R.MAT_PLASTIC, roughness=0.5, roughness_map=img)
    assert f["roughness"][0] == 0.5 * (51 / 255.0)
    assert R.shading_frame(_tri(UV), HIT, DOWN, EYE4, EYE4, R.MAT_PLASTIC, roughness=0.5)["roughness"][0] == 0.5


def test_tex2d_linear_of_a_constant_map_is_exact_and_a_ramp_interpolates():
    rng = np.random.RandomState(5)
    uv = rng.uniform(-2, 3, (4096, 2)).astype(np.float32)
    for byte in (0, 1, 127, 128, 254, 255):
        got = R.tex2d_linear(_const(byte, byte, byte, 5, 3), uv[:, 0], uv[:, 1])
        assert np.all(got[:, :3] == byte / 255.0) and np.all(got[:, 3] == 1.0)
    ramp = np.zeros((1, 4, 4), np.uint8)
    ramp[0, :, 0] = (0, 85, 170, 255)
    # texel centres at (i + 1/2) / 4: exact there, linear in between, wrapping from the last to the first
    assert np.allclose(R.tex2d_linear(ramp, np.float32([0.125, 0.375, 0.625, 0.875]), np.float32([0.5] * 4))[:, 0], (0, 1 / 3, 2 / 3, 1))
    assert np.isclose(R.tex2d_linear(ramp, np.float32(0.25), np.float32(0.5))[0], 1 / 6)
    assert np.isclose(R.tex2d_linear(ramp, np.float32(1.0), np.float32(0.5))[0], 0.5)
    # the weights move in steps of 1/256
    got = R.tex2d_linear(ramp, np.float32(0.125 + 0.25 * np.arange(257) / 256.0), np.float32([0.5] * 257))[:, 0]
    assert np.allclose(got, (np.arange(257) / 256.0) / 3.0, atol=1e-12)
