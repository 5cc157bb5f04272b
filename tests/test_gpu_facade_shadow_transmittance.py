"""PathTracer::SetShadowTransmittance through the C view (nxs_pathtracer_set_shadow_transmittance): the Cornell box with the two boxes'
baseColorFactor[3] set to 0.5 — a file this test writes — read by the C++ loader and rendered in NXHIP_SHADOWS_TRANSMIT gives the RGBA8
image and the accumulation of the bare C-ABI path in the same mode, and not those of the default."""
import json
import os
import struct

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import oracle_lib as O
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

W = H = 64
FRAMES = 3
NAME = "cornell_box_see_through.glb"


def _write_glb(directory):
    """tests/golden/cornell_box.glb with every material whose name ends in "Box" at alpha 0.5 (glTF: baseColorFactor[3], which the
    loaders map to `opacity`); the binary chunk is copied as it is"""
    data = open(os.path.join(SH.GOLDEN, "cornell_box.glb"), "rb").read()
    magic, version, _length = struct.unpack("<III", data[:12])
    json_len, json_type = struct.unpack("<II", data[12:20])
    doc = json.loads(data[20:20 + json_len])
    rest = data[20 + json_len:]
    changed = 0
    for m in doc["materials"]:
        if m.get("name", "").endswith("Box"):
            m["pbrMetallicRoughness"]["baseColorFactor"][3] = 0.5
            changed += 1
    assert changed >= 1, [m.get("name") for m in doc["materials"]]
    text = json.dumps(doc, separators=(",", ":")).encode()
    text += b" " * (-len(text) % 4)
    out = struct.pack("<III", magic, version, 12 + 8 + len(text) + len(rest)) + struct.pack("<II", len(text), json_type) + text + rest
    path = os.path.join(directory, NAME)
    with open(path, "wb") as f:
        f.write(out)
    return path


def _direct(gpu_ctx_factory, path, mode):
    scene = SH.glb_scene(path, W, H, path_length=4)
    assert (scene.materials["opacity"] == np.float32(0.5)).sum() >= 1
    scene.shadow_transmittance = mode
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.reset_frame_number()
    for _ in range(FRAMES):
        ctx.render_frame()
        ctx.accumulate()
    out = ctx.read_rgba8(), ctx.read_accumulation(), ctx.debug_pass_flavor()
    ctx.close()
    return out


def test_set_shadow_transmittance_through_the_facade_equals_the_capi_path(gpu_ctx_factory, tmp_path):
    path = _write_glb(str(tmp_path))
    sc = capi.Scene(W, H)
    sc.load_file(str(tmp_path) + os.sep, NAME)
    sc.set_camera((0.0, 1.0, 3.9), (0.0, 0.0, -1.0), 40.0, 5.0, 0.0)
    sc.set_render_settings(O.make_settings(use_mis=True, path_length=4))
    sc.update()
    pt = capi.PathTracer(W, H)
    pt.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    with pytest.raises(capi.NexusError, match="unknown mode"):
        pt.set_shadow_transmittance(2)
    pt.set_shadow_transmittance(pod.SHADOWS_TRANSMIT)
    pt.update_device_scene(sc)
    for _ in range(FRAMES):
        pt.render(sc)
    assert pt.frame_number() == FRAMES
    px, acc, flavor = _direct(gpu_ctx_factory, path, pod.SHADOWS_TRANSMIT)
    assert flavor & capi.FLAVOR_TRANSMIT
    assert np.array_equal(pt.read_pixels(), px)
    assert np.array_equal(pt.read_accumulation().view(np.uint32), acc.view(np.uint32))
    # the default gives other frames (the boxes' shadows are solid), and switching back restores them
    px0, acc0, flavor0 = _direct(gpu_ctx_factory, path, pod.SHADOWS_OPAQUE)
    assert not flavor0 & capi.FLAVOR_TRANSMIT and not np.array_equal(acc0, acc) and np.all(acc >= acc0)
    pt.set_shadow_transmittance(pod.SHADOWS_OPAQUE)
    pt.reset_frame_number()
    for _ in range(FRAMES):
        pt.render(sc)
    assert np.array_equal(pt.read_accumulation().view(np.uint32), acc0.view(np.uint32))
    pt.close()
    sc.close()
