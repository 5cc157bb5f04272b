"""Writes tests/golden/alpha_cutout.glb: a floor, an area light above it, two layered quads that carry an 8 x 8 RGBA8 map whose alpha is 0 or
255 in blocks of 2 x 2 texels with alphaMode MASK (the upper one with the default alphaCutoff, the lower one with 0.25), and one quad that
reuses the map with alphaMode OPAQUE.  The floor says nothing about its alpha (glTF's default: OPAQUE) and the light says BLEND.
Run from the repository root:
    python tools/make_alpha_cutout_glb.py
tests/test_alpha_mode_loader.py reads the file with and without the loaders' option and builds variants through build_glb(mutate)."""
import json
import os
import struct
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cutout_map():
    """8 x 8 RGBA8, row 0 = the top row: a checkerboard of 2 x 2-texel blocks, alpha 255 where (bx + by) is even and 0 elsewhere; a leaf green
    that varies a little from block to block, so that the colour is seen to come from the map"""
    img = np.zeros((8, 8, 4), np.uint8)
    for by in range(4):
        for bx in range(4):
            img[2 * by: 2 * by + 2, 2 * bx: 2 * bx + 2] = (40 + 10 * bx, 140 + 20 * by, 30, 255 if (bx + by) % 2 == 0 else 0)
    return img


def png_bytes(img):
    from nexus_amd import imageio

    h, w = img.shape[:2]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.png")
        imageio.write_png(path, np.ascontiguousarray(img).view(np.uint32).reshape(-1), w, h, flip_y=False)
        return open(path, "rb").read()


def build_glb(mutate=None):
    """the file's bytes; mutate(doc) may change the JSON document before it is written"""
    quad_i = np.array([0, 1, 2, 0, 2, 3], np.uint16)
    up = np.tile(np.array([(0, 1, 0)], np.float32), (4, 1))
    down = -up
    unit_uv = np.array([(0, 0), (0, 1), (1, 1), (1, 0)], np.float32)

    def square(half, y):
        return np.array([(-half, y, -half), (-half, y, half), (half, y, half), (half, y, -half)], np.float32)

    chunks, views, accessors = [], [], []

    def add_view(data, target=None):
        offset = sum(len(x) for x in chunks)
        chunks.append(data + b"\0" * (-len(data) % 4))
        views.append({"buffer": 0, "byteOffset": offset, "byteLength": len(data)})
        if target:
            views[-1]["target"] = target
        return len(views) - 1

    def add(arr, target, kind, ctype):
        acc = {"bufferView": add_view(arr.tobytes(), target), "componentType": ctype, "count": len(arr), "type": kind}
        if kind == "VEC3" and target == 34962:
            acc["min"], acc["max"] = [float(v) for v in arr.min(0)], [float(v) for v in arr.max(0)]
        accessors.append(acc)
        return len(accessors) - 1

    def prim(pos, nrm, uv, mat):
        attributes = {"POSITION": add(pos, 34962, "VEC3", 5126), "NORMAL": add(nrm, 34962, "VEC3", 5126)}
        if uv is not None:
            attributes["TEXCOORD_0"] = add(uv, 34962, "VEC2", 5126)
        return {"attributes": attributes, "indices": add(quad_i, 34963, "SCALAR", 5123), "material": mat}

    meshes = [
        {"name": "floor", "primitives": [prim(square(3.0, 0.0), up, None, 0)]},
        {"name": "leaves_upper", "primitives": [prim(square(1.0, 0.0), up, unit_uv * 2.0, 1)]},  # (the map repeated twice each way)
        {"name": "leaves_lower", "primitives": [prim(square(1.0, 0.0), up, unit_uv * 2.0, 2)]},
        {"name": "decal", "primitives": [prim(square(0.5, 0.0), up, unit_uv, 3)]},
        {"name": "lamp", "primitives": [prim(square(0.5, 0.0)[::-1].copy(), down, None, 4)]},  # (wound the other way: it faces the floor)
    ]
    base = {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 1.0}
    doc = {
        "asset": {"version": "2.0", "generator": "tools/make_alpha_cutout_glb.py"},
        "scene": 0,
        "scenes": [{"nodes": [0, 1, 2, 3, 4]}],
        "nodes": [
            {"name": "floor", "mesh": 0},
            {"name": "leaves_upper", "mesh": 1, "translation": [0.0, 1.4, 0.0]},
            {"name": "leaves_lower", "mesh": 2, "translation": [0.15, 1.0, 0.1]},
            {"name": "decal", "mesh": 3, "translation": [-1.6, 0.02, 0.8]},
            {"name": "lamp", "mesh": 4, "translation": [0.0, 2.6, 0.0]},
        ],
        "meshes": meshes,
        "materials": [
            {"name": "floor", "pbrMetallicRoughness": {"baseColorFactor": [0.6, 0.6, 0.6, 1.0], "metallicFactor": 0.0, "roughnessFactor": 1.0}},
            {"name": "leaves_upper", "pbrMetallicRoughness": dict(base), "alphaMode": "MASK"},
            {"name": "leaves_lower", "pbrMetallicRoughness": dict(base), "alphaMode": "MASK", "alphaCutoff": 0.25},
            {"name": "decal", "pbrMetallicRoughness": dict(base), "alphaMode": "OPAQUE"},
            {"name": "lamp", "pbrMetallicRoughness": {"baseColorFactor": [0.0, 0.0, 0.0, 1.0]}, "emissiveFactor": [1.0, 1.0, 1.0], "alphaMode": "BLEND",
             "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 30.0}}},
        ],
        "extensionsUsed": ["KHR_materials_emissive_strength"],
        "textures": [{"source": 0, "sampler": 0}],
        "samplers": [{"wrapS": 10497, "wrapT": 10497, "magFilter": 9729, "minFilter": 9729}],
        "images": [{"bufferView": add_view(png_bytes(cutout_map())), "mimeType": "image/png", "name": "cutout"}],
    }
    doc["buffers"] = [{"byteLength": sum(len(x) for x in chunks)}]
    doc["bufferViews"] = views
    doc["accessors"] = accessors
    if mutate is not None:
        mutate(doc)
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * (-len(js) % 4)
    binary = b"".join(chunks)
    total = 12 + 8 + len(js) + 8 + len(binary)
    return struct.pack("<III", 0x46546C67, 2, total) + struct.pack("<II", len(js), 0x4E4F534A) + js + struct.pack("<II", len(binary), 0x004E4942) + binary


def main():
    data = build_glb()
    with open(os.path.join(ROOT, "tests", "golden", "alpha_cutout.glb"), "wb") as f:
        f.write(data)
    print("wrote tests/golden/alpha_cutout.glb, %d bytes" % len(data))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
