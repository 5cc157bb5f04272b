"""Writes tests/golden/morph_bar.glb: the skinned bar's room and rig (make_skinned_glb.py, whose helpers build it) with three morph
targets on the bar.  Run from the repository root:
    python tests/golden/make_morph_glb.py
  * `bulge`  POSITION and NORMAL: the four sides swell outward, most at mid length, and their normals tilt along the bar;
  * `twist`  POSITION only: the bar turns about its axis, up to 0.6 rad at its tip;
  * `dent`   POSITION as a SPARSE accessor over zeros: the few vertices of the +z side around 3/4 of the length move inward.
The mesh carries the default weights [0, 0.25, 0] and the target names in extras.targetNames; a third animation (`morph`, LINEAR, three
keys) drives the bar node's weights.  The numbers the loaders must produce from it are restated in tests/test_morph_loader.py and
tests/test_morph_animation.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_skinned_glb as G  # noqa: E402

TARGET_NAMES = ["bulge", "twist", "dent"]
MESH_WEIGHTS = [0.0, 0.25, 0.0]
MORPH_TIMES = (0.0, 0.5, 1.0)
MORPH_VALUES = ((0.0, 0.0, 0.0), (1.0, 0.5, 0.0), (0.25, 0.0, 1.0))  # one row of three weights per key
BULGE, TILT, TWIST, DENT = 0.06, 0.25, 0.6, 0.05


def targets():
    """per vertex of G.bar(): bulge (dP, dN), twist dP, and the dent as (vertex indices, dP of those vertices); float32"""
    pos, nrm, _uv, _idx, _joints, _weights = G.bar()
    p, n = pos.astype(np.float64), nrm.astype(np.float64)
    y = p[:, 1] / G.LENGTH
    side = n[:, 1] == 0  # (the caps keep their normals)
    radial = np.stack([p[:, 0], np.zeros(len(p)), p[:, 2]], -1) / (G.WIDTH / 2.0)
    bulge_p = BULGE * np.sin(np.pi * y)[:, None] * radial
    bulge_n = np.zeros_like(p)
    bulge_n[side, 1] = -TILT * np.cos(np.pi * y[side])
    a = TWIST * y
    twist_p = np.stack([np.cos(a) * p[:, 0] + np.sin(a) * p[:, 2], p[:, 1], -np.sin(a) * p[:, 0] + np.cos(a) * p[:, 2]], -1) - p
    dented = np.flatnonzero((n[:, 2] == 1) & (np.abs(y - 0.75) < 0.05))
    dent_p = np.tile(np.array([0.0, 0.0, -DENT]), (len(dented), 1))
    return bulge_p.astype(np.float32), bulge_n.astype(np.float32), twist_p.astype(np.float32), dented.astype(np.uint16), dent_p.astype(np.float32)


def dense_dent():
    """the dent expanded: (vertices, 3) float32"""
    pos = G.bar()[0]
    _bp, _bn, _tp, dented, dent_p = targets()
    out = np.zeros_like(pos)
    out[dented] = dent_p
    return out


def add_morph(doc, add):
    bulge_p, bulge_n, twist_p, dented, dent_p = targets()
    assert 0 < len(dented) < 64 and np.all(np.diff(dented.astype(np.int64)) > 0)
    count = len(bulge_p)
    # a sparse accessor without a bufferView: zeros, except where its index list says otherwise
    indices_view = doc["accessors"][add(dented, None, "SCALAR", 5123)]["bufferView"]
    values_view = doc["accessors"][add(dent_p, None, "VEC3", 5126)]["bufferView"]
    doc["accessors"].append({"componentType": 5126, "count": count, "type": "VEC3", "min": [0.0, 0.0, -DENT], "max": [0.0, 0.0, 0.0],
                             "sparse": {"count": len(dented), "indices": {"bufferView": indices_view, "componentType": 5123}, "values": {"bufferView": values_view}}})
    dent = len(doc["accessors"]) - 1
    prim = doc["meshes"][0]["primitives"][0]
    prim["targets"] = [{"POSITION": add(bulge_p, 34962, "VEC3", 5126), "NORMAL": add(bulge_n, 34962, "VEC3", 5126)},
                       {"POSITION": add(twist_p, 34962, "VEC3", 5126)}, {"POSITION": dent}]
    doc["meshes"][0]["weights"] = list(MESH_WEIGHTS)
    doc["meshes"][0]["extras"] = {"targetNames": list(TARGET_NAMES)}
    times = add(np.array(MORPH_TIMES, np.float32), None, "SCALAR", 5126)
    values = add(np.array(MORPH_VALUES, np.float32).reshape(-1), None, "SCALAR", 5126)
    doc["animations"].append({"name": "morph", "samplers": [{"input": times, "output": values, "interpolation": "LINEAR"}],
                              "channels": [{"sampler": 0, "target": {"node": 0, "path": "weights"}}]})
    doc["asset"]["generator"] = "tests/golden/make_morph_glb.py"


def build_glb(mutate=None):
    """the file's bytes; mutate(doc, add), as in make_skinned_glb.build_glb, runs after the morph has been added"""
    def both(doc, add):
        add_morph(doc, add)
        if mutate is not None:
            mutate(doc, add)

    return G.build_glb(both)


def main():
    data = build_glb()
    with open(os.path.join(HERE, "morph_bar.glb"), "wb") as f:
        f.write(data)
    print("wrote morph_bar.glb, %d bytes" % len(data))


if __name__ == "__main__":
    main()
