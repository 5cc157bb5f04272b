"""Writes tests/golden/skinned_bar.glb: a skinned bar in a small lit room.  Run from the repository root:
    python tests/golden/make_skinned_glb.py
The bar: 4 x 4 x 24 quads along +y (four sides of 4 x 24 quads and two 4 x 4 caps, 832 triangles) with normals and texture
coordinates, 0.25 wide and 1.5 long in mesh space, on a node that is translated and scaled — so the inverse(meshNodeWorld) factor of
the joint palette matters.  Two joints, `root` at the bar's foot and `elbow` at its middle; the elbow's weight rises linearly from 0
to 1 over the middle third of the bar.  Animation 0 (`bend`, 1 s, LINEAR, three keys) turns the elbow 0 -> 45 -> 90 degrees about z;
animation 1 (`shift`, STEP, three keys) moves the elbow's translation.  A floor, a back wall and an emissive panel complete the room.
Every transform of the file is exactly representable in binary32, so the rest pose's palette is the identity to binary64 rounding.
The numbers the loaders and the pose evaluation must produce from it are restated in tests/test_skin_loader.py and
tests/test_animation.py, which also build variants of the document through build_glb(mutate)."""
import json
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

WIDTH, LENGTH, ACROSS, ALONG = 0.25, 1.5, 4, 24
BLEND_LO, BLEND_HI = LENGTH / 3.0, 2.0 * LENGTH / 3.0  # the middle third: the elbow's weight goes 0 -> 1 across it
MESH_TRANSLATION, MESH_SCALE = (0.5, 0.25, -0.75), 1.25
ELBOW_AT = LENGTH / 2.0  # mesh space; the elbow node's local translation is this times MESH_SCALE (0.9375)
BEND_TIMES, BEND_DEGREES = (0.0, 0.5, 1.0), (0.0, 45.0, 90.0)
SHIFT_TIMES = (0.0, 0.5, 1.0)
SHIFT_VALUES = ((0.0, ELBOW_AT * MESH_SCALE, 0.0), (0.25, ELBOW_AT * MESH_SCALE, 0.0), (0.25, ELBOW_AT * MESH_SCALE, 0.25))


def quat_z(degrees):
    h = np.radians(degrees) / 2.0
    return (0.0, 0.0, float(np.sin(h)), float(np.cos(h)))


def grid_face(origin, du, dv, nu, nv, normal, first):
    """(nu + 1) x (nv + 1) vertices origin + i du + j dv with one normal, uv = (i / nu, j / nv), and the 2 nu nv triangles"""
    i, j = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing="ij")
    pos = np.asarray(origin, np.float64) + i[..., None] * np.asarray(du, np.float64) + j[..., None] * np.asarray(dv, np.float64)
    uv = np.stack([i / nu, j / nv], -1)
    idx = []
    for a in range(nu):
        for b in range(nv):
            v00, v10, v11, v01 = a * (nv + 1) + b, (a + 1) * (nv + 1) + b, (a + 1) * (nv + 1) + b + 1, a * (nv + 1) + b + 1
            idx += [v00, v10, v11, v00, v11, v01]
    n = np.tile(np.asarray(normal, np.float64), ((nu + 1) * (nv + 1), 1))
    return pos.reshape(-1, 3), n, uv.reshape(-1, 2), np.asarray(idx) + first


def bar():
    """positions, normals, uvs (float32), indices (uint16), joints (uint16 x 4) and weights (float32 x 4) of the bar"""
    h, s, t = WIDTH / 2.0, WIDTH / ACROSS, LENGTH / ALONG
    faces = [  # origin, du (across), dv, nu, nv, outward normal: counter-clockwise seen from outside
        ((-h, 0, h), (s, 0, 0), (0, t, 0), ACROSS, ALONG, (0, 0, 1)), ((h, 0, -h), (-s, 0, 0), (0, t, 0), ACROSS, ALONG, (0, 0, -1)),
        ((h, 0, h), (0, 0, -s), (0, t, 0), ACROSS, ALONG, (1, 0, 0)), ((-h, 0, -h), (0, 0, s), (0, t, 0), ACROSS, ALONG, (-1, 0, 0)),
        ((-h, LENGTH, h), (s, 0, 0), (0, 0, -s), ACROSS, ACROSS, (0, 1, 0)), ((-h, 0, -h), (s, 0, 0), (0, 0, s), ACROSS, ACROSS, (0, -1, 0))]
    P, N, U, I = [], [], [], []
    first = 0
    for f in faces:
        p, n, u, i = grid_face(*f, first)
        first += len(p)
        P.append(p), N.append(n), U.append(u), I.append(i)
    pos = np.concatenate(P).astype(np.float32)
    w1 = np.clip((pos[:, 1].astype(np.float64) - BLEND_LO) / (BLEND_HI - BLEND_LO), 0.0, 1.0).astype(np.float32)
    weights = np.zeros((len(pos), 4), np.float32)
    weights[:, 0], weights[:, 1] = np.float32(1.0) - w1, w1
    joints = np.zeros((len(pos), 4), np.uint16)
    joints[:, 1] = np.where(w1 > 0, 1, 0)
    return pos, np.concatenate(N).astype(np.float32), np.concatenate(U).astype(np.float32), np.concatenate(I).astype(np.uint16), joints, weights


def column_major(m):
    return np.asarray(m, np.float32).T.reshape(16)


def translate(t):
    m = np.eye(4)
    m[:3, 3] = t
    return m


def build_glb(mutate=None):
    """the file's bytes; mutate(doc, add) may change the JSON document before it is written (add(array, target, type, componentType)
    appends an accessor and returns its index)"""
    chunks, views, accessors = [], [], []

    def add_view(data, target=None):
        offset = sum(len(x) for x in chunks)
        chunks.append(data + b"\0" * (-len(data) % 4))
        views.append({"buffer": 0, "byteOffset": offset, "byteLength": len(data)})
        if target:
            views[-1]["target"] = target
        return len(views) - 1

    def add(arr, target, kind, ctype):
        arr = np.ascontiguousarray(arr)
        acc = {"bufferView": add_view(arr.tobytes(), target), "componentType": ctype, "count": len(arr), "type": kind}
        if (kind == "VEC3" and target == 34962) or (kind == "SCALAR" and ctype == 5126):
            lo, hi = np.atleast_1d(arr.min(0)), np.atleast_1d(arr.max(0))
            acc["min"], acc["max"] = [float(v) for v in lo], [float(v) for v in hi]
        accessors.append(acc)
        return len(accessors) - 1

    pos, nrm, uv, idx, joints, weights = bar()
    bar_prim = {"attributes": {"POSITION": add(pos, 34962, "VEC3", 5126), "NORMAL": add(nrm, 34962, "VEC3", 5126), "TEXCOORD_0": add(uv, 34962, "VEC2", 5126),
                               "JOINTS_0": add(joints, 34962, "VEC4", 5123), "WEIGHTS_0": add(weights, 34962, "VEC4", 5126)},
                "indices": add(idx, 34963, "SCALAR", 5123), "material": 0}
    quad_i = np.array([0, 1, 2, 0, 2, 3], np.uint16)

    def quad(corners, normal, material):
        c = np.array(corners, np.float32)
        return {"attributes": {"POSITION": add(c, 34962, "VEC3", 5126), "NORMAL": add(np.tile(np.array([normal], np.float32), (4, 1)), 34962, "VEC3", 5126)},
                "indices": add(quad_i, 34963, "SCALAR", 5123), "material": material}

    floor = quad([(-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2)], (0, 1, 0), 1)
    wall = quad([(-2, 0, -2), (2, 0, -2), (2, 3, -2), (-2, 3, -2)], (0, 0, 1), 2)
    panel = quad([(-0.6, 0, -0.6), (0.6, 0, -0.6), (0.6, 0, 0.6), (-0.6, 0, 0.6)], (0, -1, 0), 3)
    # inverseBind[j] = inverse(jointWorld at bind) x meshNodeWorld
    mesh_world = translate(MESH_TRANSLATION) @ np.diag([MESH_SCALE, MESH_SCALE, MESH_SCALE, 1.0])
    root_world = translate(MESH_TRANSLATION)
    elbow_local = translate((0.0, ELBOW_AT * MESH_SCALE, 0.0))
    ibm = np.stack([column_major(np.linalg.inv(root_world) @ mesh_world), column_major(np.linalg.inv(root_world @ elbow_local) @ mesh_world)])
    bend_in = add(np.array(BEND_TIMES, np.float32), None, "SCALAR", 5126)
    bend_out = add(np.array([quat_z(d) for d in BEND_DEGREES], np.float32), None, "VEC4", 5126)
    shift_in = add(np.array(SHIFT_TIMES, np.float32), None, "SCALAR", 5126)
    shift_out = add(np.array(SHIFT_VALUES, np.float32), None, "VEC3", 5126)
    doc = {
        "asset": {"version": "2.0", "generator": "tests/golden/make_skinned_glb.py"},
        "scene": 0,
        "scenes": [{"nodes": [0, 1, 3, 4, 5]}],
        "nodes": [
            {"name": "bar", "mesh": 0, "skin": 0, "translation": list(MESH_TRANSLATION), "scale": [MESH_SCALE] * 3},
            {"name": "root", "translation": list(MESH_TRANSLATION), "children": [2]},
            {"name": "elbow", "translation": [0.0, ELBOW_AT * MESH_SCALE, 0.0]},
            {"name": "floor", "mesh": 1},
            {"name": "wall", "mesh": 2},
            {"name": "panel", "mesh": 3, "translation": [0.0, 2.9, 0.5]},
        ],
        "meshes": [{"name": "bar", "primitives": [bar_prim]}, {"name": "floor", "primitives": [floor]}, {"name": "wall", "primitives": [wall]},
                   {"name": "panel", "primitives": [panel]}],
        "skins": [{"name": "arm", "joints": [1, 2], "skeleton": 1, "inverseBindMatrices": add(ibm, None, "MAT4", 5126)}],
        "animations": [
            {"name": "bend", "samplers": [{"input": bend_in, "output": bend_out, "interpolation": "LINEAR"}],
             "channels": [{"sampler": 0, "target": {"node": 2, "path": "rotation"}}]},
            {"name": "shift", "samplers": [{"input": shift_in, "output": shift_out, "interpolation": "STEP"}],
             "channels": [{"sampler": 0, "target": {"node": 2, "path": "translation"}}]},
        ],
        "materials": [
            {"name": "bar", "pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.45, 0.2, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.6}},
            {"name": "floor", "pbrMetallicRoughness": {"baseColorFactor": [0.6, 0.6, 0.6, 1.0], "metallicFactor": 0.0, "roughnessFactor": 1.0}},
            {"name": "wall", "pbrMetallicRoughness": {"baseColorFactor": [0.3, 0.45, 0.7, 1.0], "metallicFactor": 0.0, "roughnessFactor": 1.0}},
            {"name": "panel", "pbrMetallicRoughness": {"baseColorFactor": [0.0, 0.0, 0.0, 1.0]}, "emissiveFactor": [1.0, 1.0, 1.0],
             "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 20.0}}},
        ],
        "extensionsUsed": ["KHR_materials_emissive_strength"],
    }
    doc["buffers"] = [{"byteLength": 0}]
    doc["bufferViews"] = views
    doc["accessors"] = accessors
    if mutate is not None:
        mutate(doc, add)
    doc["buffers"] = [{"byteLength": sum(len(x) for x in chunks)}]
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * (-len(js) % 4)
    binary = b"".join(chunks)
    total = 12 + 8 + len(js) + 8 + len(binary)
    return struct.pack("<III", 0x46546C67, 2, total) + struct.pack("<II", len(js), 0x4E4F534A) + js + struct.pack("<II", len(binary), 0x004E4942) + binary


def main():
    data = build_glb()
    with open(os.path.join(HERE, "skinned_bar.glb"), "wb") as f:
        f.write(data)
    print("wrote skinned_bar.glb, %d bytes" % len(data))


if __name__ == "__main__":
    main()
