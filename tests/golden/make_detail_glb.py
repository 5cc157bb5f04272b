"""Writes tests/golden/detail_maps.glb: a floor, a box on a node that is rotated and non-uniformly scaled, and a plinth, with a 4 x 4 normal
map (scale 0.8) and an 8 x 2 metallic-roughness map embedded as PNGs.  The floor names both maps, the box the metallic-roughness map
only, the plinth neither.  Run from the repository root:
    python tests/golden/make_detail_glb.py
The numbers the loaders must produce from it are worked out by hand in tests/test_detail_maps_loader.py, which also builds variants of
the document through build_glb(mutate)."""
import json
import os
import struct
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def quat(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = np.radians(degrees) / 2.0
    return [float(x) for x in (a * np.sin(h))] + [float(np.cos(h))]


def normal_map():
    """4 x 4 RGBA8, row 0 = the top row: texel (x, y) = (128 + 24 (x - 1.5), 128 - 20 (y - 1.5), 255 - 4 (x + y), 255)"""
    img = np.zeros((4, 4, 4), np.uint8)
    for y in range(4):
        for x in range(4):
            img[y, x] = (128 + 24 * (x - 1.5), 128 - 20 * (y - 1.5), 255 - 4 * (x + y), 255)
    return img


def roughness_map():
    """8 x 2 RGBA8 in glTF's channel assignment: G = roughness 40 + 30 x in the top row and 250 - 30 x in the bottom one, B = metalness 255
    (unused), R = 0"""
    img = np.zeros((2, 8, 4), np.uint8)
    for x in range(8):
        img[0, x] = (0, 40 + 30 * x, 255, 255)
        img[1, x] = (0, 250 - 30 * x, 255, 255)
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
    floor = np.array([(-3, 0, -3), (-3, 0, 3), (3, 0, 3), (3, 0, -3)], np.float32)
    floor_n = np.tile(np.array([(0, 1, 0)], np.float32), (4, 1))
    floor_uv = np.array([(0, 0), (0, 6), (6, 6), (6, 0)], np.float32)  # u along +x, v (down the image) along +z, the maps repeated six times
    quad_i = np.array([0, 1, 2, 0, 2, 3], np.uint16)
    c = np.array([(x, y, z) for x in (-0.3, 0.3) for y in (0.0, 0.6) for z in (-0.3, 0.3)], np.float32)
    faces = [((0, 1, 3, 2), (-1, 0, 0)), ((4, 6, 7, 5), (1, 0, 0)), ((0, 4, 5, 1), (0, -1, 0)), ((2, 3, 7, 6), (0, 1, 0)), ((0, 2, 6, 4), (0, 0, -1)), ((1, 5, 7, 3), (0, 0, 1))]
    box = np.concatenate([c[list(q)] for q, _ in faces]).astype(np.float32)
    box_n = np.concatenate([np.tile(np.array([n], np.float32), (4, 1)) for _, n in faces])
    box_uv = np.tile(np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32), (6, 1))
    box_i = np.concatenate([quad_i + 4 * k for k in range(6)])
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

    prims = []
    for pos, nrm, uv, idx, mat in ((floor, floor_n, floor_uv, quad_i, 0), (box, box_n, box_uv, box_i, 1), (box, box_n, box_uv, box_i, 2)):
        prims.append({"attributes": {"POSITION": add(pos, 34962, "VEC3", 5126), "NORMAL": add(nrm, 34962, "VEC3", 5126), "TEXCOORD_0": add(uv, 34962, "VEC2", 5126)},
                      "indices": add(idx, 34963, "SCALAR", 5123), "material": mat})
    images = [{"bufferView": add_view(png_bytes(normal_map())), "mimeType": "image/png", "name": "normal"},
              {"bufferView": add_view(png_bytes(roughness_map())), "mimeType": "image/png", "name": "metallicRoughness"}]
    doc = {
        "asset": {"version": "2.0", "generator": "tests/golden/make_detail_glb.py"},
        "scene": 0,
        "scenes": [{"nodes": [0, 1, 2, 3]}],
        "nodes": [
            {"name": "floor", "mesh": 0},
            {"name": "box", "mesh": 1, "translation": [0.8, 0.0, -0.4], "rotation": quat((0, 1, 0), 25.0), "scale": [1.5, 0.75, 1.0]},
            {"name": "plinth", "mesh": 2, "translation": [-1.0, 0.0, 0.3]},
            {"name": "lamp", "mesh": 3, "translation": [0.0, 2.4, 0.0]},
        ],
        "meshes": [{"name": "floor", "primitives": [prims[0]]}, {"name": "box", "primitives": [prims[1]]}, {"name": "plinth", "primitives": [prims[2]]}],
        "materials": [
            {"name": "floor", "pbrMetallicRoughness": {"baseColorFactor": [0.6, 0.6, 0.6, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.5,
                                                       "metallicRoughnessTexture": {"index": 1}},
             "normalTexture": {"index": 0, "scale": 0.8}},
            {"name": "box", "pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.3, 0.2, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.25,
                                                     "metallicRoughnessTexture": {"index": 1}}},
            {"name": "plinth", "pbrMetallicRoughness": {"baseColorFactor": [0.2, 0.5, 0.8, 1.0], "metallicFactor": 0.0, "roughnessFactor": 1.0}},
            {"name": "lamp", "pbrMetallicRoughness": {"baseColorFactor": [0.0, 0.0, 0.0, 1.0]}, "emissiveFactor": [1.0, 1.0, 1.0],
             "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 25.0}}},
        ],
        "extensionsUsed": ["KHR_materials_emissive_strength"],
        "textures": [{"source": 0, "sampler": 0}, {"source": 1, "sampler": 0}],
        "samplers": [{"wrapS": 10497, "wrapT": 10497}],
        "images": images,
    }
    # the lamp: a small quad facing down, so that the file lights itself
    lamp = np.array([(-0.4, 0, -0.4), (0.4, 0, -0.4), (0.4, 0, 0.4), (-0.4, 0, 0.4)], np.float32)
    lamp_n = np.tile(np.array([(0, -1, 0)], np.float32), (4, 1))
    doc["meshes"].append({"name": "lamp", "primitives": [{"attributes": {"POSITION": add(lamp, 34962, "VEC3", 5126), "NORMAL": add(lamp_n, 34962, "VEC3", 5126)},
                                                         "indices": add(quad_i, 34963, "SCALAR", 5123), "material": 3}]})
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
    with open(os.path.join(HERE, "detail_maps.glb"), "wb") as f:
        f.write(data)
    print("wrote detail_maps.glb, %d bytes" % len(data))


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    main()
