"""Image files without stb: the PNG / OpenEXR writers (C++ nexus::WritePNG / WriteEXR and their Python twins), the Radiance
.hdr reader behind IMGLoader, and the headless Renderer facade (Renderer.cpp:41-77, 183-215)."""
import os

import numpy as np
import pytest

from nexus_amd import capi, imageio, loaders, pod
from tests import oracle_lib as O
from tests import scene_helpers as SH


def test_exr_and_png_writers_cpp_equals_python_and_round_trip(tmp_path):
    rng = np.random.RandomState(1)
    for (W, H) in ((1, 1), (37, 21), (128, 3)):
        rgb = rng.uniform(-2, 50, (W * H, 3)).astype(np.float32)
        rgb[0] = (np.inf, 0.0, 1e-30)
        a, b = str(tmp_path / "a.exr"), str(tmp_path / "b.exr")
        capi.write_exr(a, rgb, W, H, True)
        imageio.write_exr(b, rgb, W, H, True)
        assert open(a, "rb").read() == open(b, "rb").read()
        img, w, h = imageio.read_exr(a)
        assert (w, h) == (W, H) and np.array_equal(img[::-1].reshape(-1, 3).view(np.uint32), rgb.view(np.uint32))  # top row first in the file
        capi.write_exr(a, rgb, W, H, False)
        assert np.array_equal(imageio.read_exr(a)[0].reshape(-1, 3).view(np.uint32), rgb.view(np.uint32))
        px = rng.randint(0, 2 ** 32, W * H, dtype=np.uint64).astype(np.uint32)
        pa, pb = str(tmp_path / "a.png"), str(tmp_path / "b.png")
        capi.write_png(pa, px, W, H, True)
        imageio.write_png(pb, px, W, H, True)
        da, _ = loaders.decode_png(open(pa, "rb").read())
        db, _ = capi.decode_png(open(pb, "rb").read())
        want = px.view(np.uint8).reshape(H, W, 4)[::-1]
        assert np.array_equal(da, want) and np.array_equal(db, want)
    with pytest.raises(capi.NexusError):
        capi.write_exr(str(tmp_path / "no_such_dir" / "x.exr"), rgb, W, H)


def _hdr_file(w, h, rng, rle):
    rgbe = rng.randint(0, 256, size=(h, w, 4)).astype(np.uint8)
    rgbe[..., 3] = rng.randint(118, 140, size=(h, w))
    rgbe[0, 0, 3] = 0  # zero exponent: black
    if rle:  # long runs so that both run and literal packets appear
        rgbe[:, : w // 2, 0] = 200
        rgbe[:, :, 3] = 130
    out = b"#?RADIANCE\nEXPOSURE=1.0\nFORMAT=32-bit_rle_rgbe\n\n" + b"-Y %d +X %d\n" % (h, w)
    for y in range(h):
        if not rle:
            out += rgbe[y].tobytes()
            continue
        out += bytes([2, 2, w >> 8, w & 255])
        for c in range(4):
            row = rgbe[y, :, c]
            x = 0
            while x < w:
                run = 1
                while x + run < w and run < 127 and row[x + run] == row[x]:
                    run += 1
                if run >= 3:
                    out += bytes([128 + run, int(row[x])])
                    x += run
                else:
                    lit = 1
                    while x + lit < w and lit < 128 and not (x + lit + 2 < w and row[x + lit] == row[x + lit + 1] == row[x + lit + 2]):
                        lit += 1
                    out += bytes([lit]) + row[x: x + lit].tobytes()
                    x += lit
    return out, rgbe


@pytest.mark.parametrize("rle", [False, True])
def test_radiance_hdr_reader_cpp_equals_python(rle, tmp_path):
    rng = np.random.RandomState(4)
    data, rgbe = _hdr_file(40, 6, rng, rle)
    py, ch = loaders.decode_hdr(data)
    cpp, ch2 = capi.decode_png(data)  # nxh_decode_png is IMGLoader::LoadIMG: the file type is told from the signature
    assert ch == ch2 == 3 and py.shape == (6, 40, 4)
    assert np.array_equal(py, cpp)
    assert (rle or tuple(py[0, 0]) == (0, 0, 0, 255)) and py[..., :3].max() == 255 and 0 < py[..., :3].mean() < 255
    # a value by hand: mantissa 128, exponent 128 -> 0.5 -> pow(0.5, 1 / 2.2) * 255 + 0.5 = 186.6 -> 186
    one = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 1\n" + bytes([128, 64, 0, 128])
    assert tuple(capi.decode_png(one)[0][0, 0]) == (186, 136, 0, 255)
    # Scene::AddHDRMap(path, file) takes the same route
    p = tmp_path / "sky.hdr"
    p.write_bytes(data)
    sc = capi.Scene(16, 16)

    assert sc.L.nxs_scene_add_hdr_map_file(sc.h, (str(tmp_path) + os.sep).encode(), b"sky.hdr") == 0
    assert sc.L.nxs_scene_add_hdr_map_file(sc.h, (str(tmp_path) + os.sep).encode(), b"missing.hdr") != 0


@pytest.mark.gpu
def test_renderer_facade_drives_the_reference_loop_and_saves_images(tmp_path):
    W = H = 64
    sc = capi.Scene(W, H)
    sc.load_file(SH.GOLDEN + os.sep, "cornell_box.glb")
    sc.set_camera((0.0, 1.0, 3.9), (0.0, 0.0, -1.0), 40.0, 5.0, 0.0)
    sc.set_render_settings(O.make_settings(use_mis=True, path_length=3))
    r = capi.Renderer(W, H, sc)
    r.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    for _ in range(3):
        r.render(sc, 0.004)  # the scene is invalid at first: Update + frame number reset, as Renderer.cpp:52-56
    assert r.frame_number() == 3
    assert abs(r.megasamples_per_second() - W * H * 3 / 0.012 / 1e6) < 1e-6
    # the same frames through Scene + PathTracer directly
    sc2 = capi.Scene(W, H)
    sc2.load_file(SH.GOLDEN + os.sep, "cornell_box.glb")
    sc2.set_camera((0.0, 1.0, 3.9), (0.0, 0.0, -1.0), 40.0, 5.0, 0.0)
    sc2.set_render_settings(O.make_settings(use_mis=True, path_length=3))
    sc2.update()
    pt = capi.PathTracer(W, H)
    pt.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    pt.update_device_scene(sc2)
    for _ in range(3):
        pt.render(sc2)
    assert np.array_equal(r.read_pixels(), pt.read_pixels())
    shot, exr = str(tmp_path / "shot"), str(tmp_path / "acc.exr")
    r.save_screenshot(shot)  # ".png" is appended (Renderer.cpp:199-204)
    img, _ = loaders.decode_png(open(shot + ".png", "rb").read())
    assert np.array_equal(img[::-1].reshape(-1, 4), r.read_pixels().view(np.uint8).reshape(-1, 4))
    r.save_exr(exr)
    acc, w, h = imageio.read_exr(exr)
    assert np.array_equal(acc[::-1].reshape(-1, 3).view(np.uint32), r.read_accumulation().view(np.uint32))
    # moving an instance invalidates the scene: the next Render updates it and restarts the accumulation
    sc.set_instance_transform(5, (0.3, 0.0, 0.2), (90.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    r.render(sc, 0.004)
    assert r.frame_number() == 1
    r.close()
    pt.close()
