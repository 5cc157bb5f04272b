"""Float environment maps on the CPU: the .hdr decoders that keep the range, the float64 checker of tests/test_gpu_env_float.py
tested on itself, and the new entry points' symbols.

Decoders.  IMGLoader::LoadHDRFloat (C++) and loaders.decode_hdr_float (Python) read the RGBE records the 8-bit decoders read and
return component = mantissa x 2^(e - 136), e = 0 giving 0, in binary32: both are compared bit for bit with that formula applied to the
records the test wrote (flat and run-length encoded files, written to tmp_path by tests/env_float_reference.write_hdr), the files
the 8-bit decoder refuses are refused, and the 8-bit decode of the same file (Scene::AddHDRMap's) is still pow(c, 1 / 2.2) x 255.

The checker tested on itself.  The 32 x 16 sun map (sky (0.02, 0.03, 0.06), one texel of (6e4, 5e4, 3.5e4) at (9, 4), three black rows
at the bottom), a Lambertian plane of normal +y, the one-sample light estimator L cos / (pi pdf): float64 quadrature gives 356.48 for
the red channel.  400 000 draws in 64 batches with the FOOTPRINT weight agree with it (mean 356.82 here; relative standard deviation
of one sample 1.07, largest sample 19.6 x the mean); the same draws with the texel's OWN luminance as weight give 202.09 — 43 % low,
every batch alike, because the halo the bilinear lookup spreads around the sun is a tail of value / pdf = sun / sky that 400 000
draws have not met — and are refused.  (Other seeds meet the halo once and then report 760 or 800 with a standard error of 590: an
estimator whose error estimate is itself meaningless.  The seed is fixed; the statement is about these draws.)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from nexus_amd import capi, loaders
from tests import env_float_reference as F
from tests.test_physics_pins import _assert_agree, _z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_HIP = ["nxhip_upload_env_float", "nxhip_read_env_float", "nxhip_read_env_guides"]
NEW_HOST = ["nxs_scene_set_hdr_map_float", "nxs_scene_add_hdr_map_file_float", "nxh_decode_hdr_float"]


# ---- the decoders ----------------------------------------------------------------------------------------------------------------

def _records(w, h, seed):
    rng = np.random.RandomState(seed)
    rgbe = rng.randint(0, 256, size=(h, w, 4)).astype(np.uint8)
    rgbe[..., 3] = rng.randint(100, 150, size=(h, w))
    rgbe[0, 0] = (200, 100, 50, 0)          # e = 0: black whatever the mantissas say
    rgbe[h - 1, w - 1] = (255, 255, 255, 144)  # 255 x 2^8: nothing is clamped
    rgbe[h // 2, :] = rgbe[h // 2, 0]          # a row of equal records: runs in every component
    return rgbe


CASES = [(7, 5, False), (40, 9, True), (9, 3, True), (130, 4, True), (32, 16, False)]


@pytest.mark.parametrize("w,h,rle", CASES)
def test_float_decoders_are_bit_equal_to_the_formula(tmp_path, w, h, rle):
    rgbe = _records(w, h, 11 + w)
    data = F.write_hdr(rgbe, rle)
    path = tmp_path / "map.hdr"
    path.write_bytes(data)
    want = F.rgbe_to_float(rgbe)
    assert want.dtype == np.float32 and want.shape == (h, w, 3)
    assert np.all(want[0, 0] == 0.0) and np.all(want[h - 1, w - 1] == np.float32(255.0 * 256.0))
    # the formula once more, in float64 (exact: an 8-bit mantissa times a power of two)
    e = rgbe[..., 3].astype(np.int64)
    assert np.array_equal(want.astype(np.float64), np.where(e[..., None] != 0, rgbe[..., 0:3] * np.ldexp(1.0, e - 136)[..., None], 0.0))
    got_py = loaders.decode_hdr_float(path.read_bytes())
    got_cpp = capi.decode_hdr_float(path.read_bytes())
    for got, who in ((got_py, "Python"), (got_cpp, "C++")):
        assert got.dtype == np.float32 and got.shape == (h, w, 3), who
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), who + ": not the formula bit for bit"


@pytest.mark.parametrize("w,h,rle", CASES[:2])
def test_the_eight_bit_decode_of_the_same_file_is_what_it_was(w, h, rle):
    """Scene::AddHDRMap's decode (IMGLoader::LoadIMG) and its Python twin: clamp(pow(c, 1 / 2.2) x 255 + 0.5), alpha 255"""
    rgbe = _records(w, h, 11 + w)
    data = F.write_hdr(rgbe, rle)
    f = F.rgbe_to_float(rgbe)
    z = np.power(f.astype(np.float64), np.float64(np.float32(1.0) / np.float32(2.2))).astype(np.float32) * np.float32(255.0) + np.float32(0.5)
    want = np.full((h, w, 4), 255, np.uint8)
    want[..., 0:3] = np.clip(z, 0.0, 255.0).astype(np.int32).astype(np.uint8)
    got_cpp, channels = capi.decode_image(data)
    assert channels == 3 and np.array_equal(got_cpp, want)
    got_py, channels = loaders.decode_hdr(data)
    assert channels == 3 and np.array_equal(got_py, want)


def test_what_the_eight_bit_decoder_refuses_the_float_decoder_refuses(tmp_path):
    from tests.test_image_decoders import hdr_cases

    def refused(decode, data):
        try:
            decode(data)
            return False
        except (capi.NexusError, ValueError, IndexError):
            return True

    good = F.write_hdr(_records(40, 9, 3), True)
    bad = {
        "not a Radiance file": b"#?RADIANCF\n" + good[11:],
        "no FORMAT line": good.replace(b"FORMAT=32-bit_rle_rgbe\n", b"FORMAT=32-bit_rle_xyze\n"),
        "another orientation": good.replace(b"-Y 9 +X 40", b"+Y 9 +X 40"),
        "a zero size": good.replace(b"-Y 9 +X 40", b"-Y 0 +X 40"),
        "too large": good.replace(b"-Y 9 +X 40", b"-Y 9 +X 40000"),
        "ends early": good[:len(good) - 40],
        "header not terminated": b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n",
        "a run past the end of the line": good[:good.index(b"+X 40\n") + 6] + bytes([2, 2, 0, 40, 128 + 41, 7]) + good[good.index(b"+X 40\n") + 12:],
    }
    for what, data in bad.items():
        assert refused(capi.decode_image, data), what + ": the 8-bit decoder takes it"
        assert refused(capi.decode_hdr_float, data), what
    # random damage (the files of tests/test_image_decoders.py): the two C++ decodes share one reader, and so do the two Python ones
    rng = np.random.RandomState(9)
    both = neither = 0
    for _name, data in hdr_cases(np.random.RandomState(7)):
        for trial in range(30):
            b = bytearray(data)
            if trial % 3 == 0:
                b[rng.randint(len(b))] = rng.randint(256)
            elif trial % 3 == 1:
                del b[rng.randint(max(1, len(b) // 2), len(b)):]
            else:
                at = rng.randint(len(b))
                b[at:at] = bytes(rng.randint(0, 256, rng.randint(1, 5)).astype(np.uint8))
            b = bytes(b)
            r8 = refused(capi.decode_image, b)
            assert refused(capi.decode_hdr_float, b) == r8
            assert refused(loaders.decode_hdr_float, b) == refused(loaders.decode_hdr, b)
            both += r8
            neither += not r8
    assert both > 10 and neither > 10


def test_facade_scene_takes_a_float_map(tmp_path):
    """Scene::AddHDRMapFloat through the flat C API: the array and the file (no device needed: the scene is host state)"""
    img = F.sun_map()
    sc = capi.Scene(64, 40)
    sc.set_hdr_map_float(img)
    path = tmp_path / "sun.hdr"
    path.write_bytes(F.write_hdr(F.float_to_rgbe(img), True))
    sc.add_hdr_map_file_float(str(tmp_path) + os.sep, "sun.hdr")
    with pytest.raises(capi.NexusError):
        sc.add_hdr_map_file_float(str(tmp_path) + os.sep, "missing.hdr")
    sc.close()


# ---- the checker tested on itself ---------------------------------------------------------------------------------------------------

DRAWS, BATCHES = 400_000, 64


def _batches(samples):
    b = samples.reshape(BATCHES, -1, 3)
    return b.mean(axis=1), b.std(axis=1, ddof=1) / np.sqrt(b.shape[1])


def test_footprint_weights_agree_with_quadrature_and_own_luminance_weights_are_refused():
    img = F.sun_map()
    n = np.array([0.0, 1.0, 0.0])
    irr, residue = F.irradiance(img, n, sub=16)
    want = irr / np.pi
    print("quadrature: %s, residue %.3g" % (want, residue))
    assert residue < 2e-5 and abs(want[0] - 356.48) < 0.01
    good = F.sample_estimator(img, F.distribution(img), n, DRAWS, 1)
    mean, se = _batches(good)
    print("footprint weight: mean %s, relative standard deviation of one sample %.3f, largest sample %.1f x the mean" % (
        good.mean(axis=0), good[:, 0].std() / good[:, 0].mean(), good[:, 0].max() / good[:, 0].mean()))
    _assert_agree(_z(mean, se, want[None, :], 0.0, systematic=1e-3), "footprint weights against quadrature")
    assert good[:, 0].std() / good[:, 0].mean() < 1.2 and good[:, 0].max() / good[:, 0].mean() < 25.0
    bad = F.sample_estimator(img, F.distribution(img, F.own_weight(img)), n, DRAWS, 1)
    mean, se = _batches(bad)
    print("own-luminance weight: mean %s" % bad.mean(axis=0))
    assert bad[:, 0].mean() < 0.6 * want[0], "these draws have not met the halo: 43 % low"
    with pytest.raises(AssertionError):
        _assert_agree(_z(mean, se, want[None, :], 0.0, systematic=1e-3), "own-luminance weights must be refused")


def test_footprint_kernel_is_the_integral_of_the_bilinear_filter():
    """the weight's kernel against brute force: the mean of the filtered luminance over 64 x 64 points of every texel's footprint"""
    rng = np.random.RandomState(5)
    img = rng.random_sample((5, 7, 3)) * np.array([1.0, 10.0, 100.0])
    img[2, 3] = (6e4, 5e4, 3.5e4)
    H, W = img.shape[:2]
    sub = 64
    u = (np.arange(W * sub) + 0.5) / (W * sub)
    v = (np.arange(H * sub) + 0.5) / (H * sub)
    vv, uu = np.meshgrid(v, u, indexing="ij")
    lum = F.luminance(F.texture(img, uu.ravel(), vv.ravel())).reshape(H, sub, W, sub).mean(axis=(1, 3))
    want = lum * np.sin(np.pi * (np.arange(H) + 0.5) / H)[:, None] + F.FLOOR
    # (the midpoint rule is exact for the piecewise-linear filter once no cell straddles a texel centre: sub is even)
    assert np.max(np.abs(F.footprint_weight(img) - want) / want) < 1e-12
    assert abs(F.KERNEL.sum() - 1.0) == 0.0 and 9 / 16 + 4 * 3 / 32 + 4 / 64 == 1.0


def test_reference_lookup_matches_the_eight_bit_reference_on_decoded_texels():
    """the float lookup is tests/geometry_reference.texture without the sRGB decode: the same (u, v), wrap and weights"""
    from tests import geometry_reference as G

    rng = np.random.RandomState(3)
    img8 = rng.randint(0, 256, (5, 7, 4)).astype(np.uint8)
    u, v = rng.random_sample(1000) * 3 - 1, rng.random_sample(1000) * 3 - 1
    assert np.max(np.abs(F.texture(G.srgb_decode(img8[..., 0:3]), u, v) - G.texture(img8, u, v))) < 1e-15


# ---- symbols ------------------------------------------------------------------------------------------------------------------------

def test_default_build_exports_the_new_entry_points():
    lib = capi.lib()
    for name in NEW_HIP + NEW_HOST:
        assert hasattr(lib, name), "libnexus_amd.so does not export %s" % name
    assert set(NEW_HIP) <= set(capi.HIP_SYMBOLS) and set(NEW_HOST) <= set(capi.HOST_SYMBOLS)
    assert capi.API_VERSION == 8, "entry points were only added"


def test_release_build_exports_the_new_entry_points():
    # (no skip where the compiler is missing: the library under test cannot be built without it, and a test that quietly does not run
    #  says nothing about the release build)
    out = os.path.join(ROOT, "nexus_amd", "lib", "release", "libnexus_amd.so")
    subprocess.run(["make", "-C", ROOT, "-j", "8", "release"], check=True, capture_output=True, timeout=900)
    L = C.CDLL(out)
    for name in NEW_HIP + NEW_HOST:
        assert hasattr(L, name), "the release library does not export %s" % name
    # not test hooks of the debug kind: a release library answers them (a null context is refused as everywhere)
    L.nxhip_last_error.restype = C.c_char_p
    assert L.nxhip_upload_env_float(None, None, 0, 0) != 0 and b"null context" in L.nxhip_last_error()
