"""Writes tests/golden/punctual_lights.glb: a floor and a small box under one KHR_lights_punctual light of each kind, every light on a
node that is rotated and translated (one of them under a parent, one given as a matrix).  Run from the repository root:
    python tests/golden/make_punctual_glb.py
The numbers the loaders must produce from it are worked out by hand in tests/test_punctual_lights_loader.py."""
import json
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def quat(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = np.radians(degrees) / 2.0
    return [float(x) for x in (a * np.sin(h))] + [float(np.cos(h))]


def main():
    # a floor of two triangles and a box of twelve, one buffer: positions, normals, indices
    floor = np.array([(-3, 0, -3), (-3, 0, 3), (3, 0, 3), (3, 0, -3)], np.float32)
    floor_n = np.tile(np.array([(0, 1, 0)], np.float32), (4, 1))
    floor_i = np.array([0, 1, 2, 0, 2, 3], np.uint16)
    c = np.array([(x, y, z) for x in (-0.3, 0.3) for y in (0.0, 0.6) for z in (-0.3, 0.3)], np.float32)
    faces = [((0, 1, 3, 2), (-1, 0, 0)), ((4, 6, 7, 5), (1, 0, 0)), ((0, 4, 5, 1), (0, -1, 0)), ((2, 3, 7, 6), (0, 1, 0)), ((0, 2, 6, 4), (0, 0, -1)), ((1, 5, 7, 3), (0, 0, 1))]
    box = np.concatenate([c[list(q)] for q, _ in faces]).astype(np.float32)
    box_n = np.concatenate([np.tile(np.array([n], np.float32), (4, 1)) for _, n in faces])
    box_i = np.concatenate([np.array([0, 1, 2, 0, 2, 3], np.uint16) + 4 * k for k in range(6)])
    chunks, views, accessors = [], [], []

    def add(arr, target, kind, ctype):
        data = arr.tobytes()
        offset = sum(len(x) for x in chunks)
        chunks.append(data + b"\0" * (-len(data) % 4))
        views.append({"buffer": 0, "byteOffset": offset, "byteLength": len(data), "target": target})
        acc = {"bufferView": len(views) - 1, "componentType": ctype, "count": len(arr), "type": kind}
        if kind == "VEC3" and target == 34962:
            acc["min"], acc["max"] = [float(v) for v in arr.min(0)], [float(v) for v in arr.max(0)]
        accessors.append(acc)
        return len(accessors) - 1

    prims = []
    for pos, nrm, idx, mat in ((floor, floor_n, floor_i, 0), (box, box_n, box_i, 1)):
        prims.append({"attributes": {"POSITION": add(pos, 34962, "VEC3", 5126), "NORMAL": add(nrm, 34962, "VEC3", 5126)}, "indices": add(idx, 34963, "SCALAR", 5123),
                      "material": mat})
    s, co = float(np.sin(np.radians(30))), float(np.cos(np.radians(30)))
    doc = {
        "asset": {"version": "2.0", "generator": "tests/golden/make_punctual_glb.py"},
        "extensionsUsed": ["KHR_lights_punctual"],
        "extensions": {"KHR_lights_punctual": {"lights": [
            {"type": "point", "color": [1.0, 0.8, 0.6], "intensity": 5.0, "range": 4.0, "name": "lamp"},
            {"type": "spot", "color": [0.4, 0.6, 1.0], "intensity": 9.0, "spot": {"innerConeAngle": 0.25, "outerConeAngle": 0.5}, "name": "spot"},
            {"type": "directional", "intensity": 2.5, "name": "sun"},
            {"type": "spot", "intensity": 3.0, "name": "spot with the default cone"},
        ]}},
        "scene": 0,
        "scenes": [{"nodes": [0, 1, 2, 4, 5]}],
        "nodes": [
            {"name": "floor", "mesh": 0},
            {"name": "box", "mesh": 1, "translation": [0.8, 0.0, -0.4], "rotation": quat((0, 1, 0), 25.0)},
            # the lamp: under a parent that is rotated 90 degrees about y and moved; its own translation turns with the parent
            {"name": "arm", "translation": [1.0, 2.0, 0.5], "rotation": quat((0, 1, 0), 90.0), "children": [3]},
            {"name": "lamp", "translation": [0.5, 0.25, 0.0], "extensions": {"KHR_lights_punctual": {"light": 0}}},
            # the spot: rotated -90 degrees about x, so that its -Z axis looks straight down; then 30 degrees about z on top of it
            {"name": "spot", "translation": [-1.0, 2.5, 0.25], "rotation": quat((1, 0, 0), -90.0), "children": [6], "extensions": {"KHR_lights_punctual": {"light": 1}}},
            # the sun: a column-major matrix — rotation by 30 degrees about x (its -Z axis dips below the horizon) and a translation that means nothing
            {"name": "sun", "matrix": [1, 0, 0, 0, 0, co, -s, 0, 0, s, co, 0, 7.0, 8.0, 9.0, 1], "extensions": {"KHR_lights_punctual": {"light": 2}}},
            {"name": "second spot", "translation": [0.0, 0.0, -1.0], "rotation": quat((0, 0, 1), 30.0), "extensions": {"KHR_lights_punctual": {"light": 3}}},
        ],
        "meshes": [{"name": "floor", "primitives": [prims[0]]}, {"name": "box", "primitives": [prims[1]]}],
        "materials": [{"name": "floor", "pbrMetallicRoughness": {"baseColorFactor": [0.6, 0.6, 0.6, 1.0], "metallicFactor": 0.0, "roughnessFactor": 1.0}},
                      {"name": "box", "pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.3, 0.2, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.5}}],
        "buffers": [{"byteLength": sum(len(x) for x in chunks)}],
        "bufferViews": views,
        "accessors": accessors,
    }
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * (-len(js) % 4)
    binary = b"".join(chunks)
    total = 12 + 8 + len(js) + 8 + len(binary)
    with open(os.path.join(HERE, "punctual_lights.glb"), "wb") as f:
        f.write(struct.pack("<III", 0x46546C67, 2, total))
        f.write(struct.pack("<II", len(js), 0x4E4F534A) + js)
        f.write(struct.pack("<II", len(binary), 0x004E4942) + binary)
    print("wrote punctual_lights.glb, %d bytes" % total)


if __name__ == "__main__":
    main()
