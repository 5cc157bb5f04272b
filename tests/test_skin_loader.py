"""glTF skins through the Python reader (loaders.load_glb(skins=True)) and the host-side half of nxhip_set_blas_skin's rules
(pod.make_skin_corners, pod.normalise_skin_corners).  The fixture is tests/golden/skinned_bar.glb; what it must yield is restated here
from the generator's own arrays (tests/golden/make_skinned_glb.py)."""
import os
import sys

import numpy as np
import pytest

from nexus_amd import loaders, pod

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, GOLDEN)
import make_skinned_glb as G  # noqa: E402

PATH = os.path.join(GOLDEN, "skinned_bar.glb")


def test_the_committed_fixture_is_what_the_generator_writes():
    data = open(PATH, "rb").read()
    assert data == G.build_glb()
    assert len(data) < 100 * 1024


def test_corner_arrays_equal_what_the_generator_wrote():
    ls = loaders.load_glb(PATH, skins=True)
    assert ls.warnings == []
    assert len(ls.skins) == 1 and len(ls.animations) == 2 and len(ls.nodes) == 6
    skin = ls.skins[0]
    pos, nrm, uv, idx, joints, weights = G.bar()
    assert len(idx) == 3 * 832 and skin["mesh"] == 0 and len(ls.meshes[0]) == 832
    corners = skin["corners"]
    assert corners.dtype == pod.SKIN_CORNER_DT and len(corners) == 3 * 832
    assert np.array_equal(corners["joint"], joints[idx]) and corners["weight"].tobytes() == weights[idx].tobytes()
    # de-indexed with the same index array as the positions: corner 3 i + v is vertex v of triangle i
    tri = ls.meshes[0]
    assert np.stack([tri["pos0"], tri["pos1"], tri["pos2"]], 1).reshape(-1, 3).tobytes() == pos[idx].tobytes()
    # the weights blend linearly over the middle third
    y = pos[idx][:, 1].astype(np.float64)
    assert np.all(corners["weight"][y <= 0.5, 1] == 0) and np.all(corners["weight"][y >= 1.0, 1] == 1)
    mid = (y > 0.5) & (y < 1.0)
    assert mid.sum() > 0 and np.allclose(corners["weight"][mid, 1], (y[mid] - 0.5) / 0.5, atol=1e-7)
    assert skin["joints"] == [1, 2] and skin["mesh_node"] == 0
    want = np.tile(np.diag([1.25, 1.25, 1.25, 1.0]), (2, 1, 1))
    want[1, 1, 3] = -0.9375
    assert np.array_equal(skin["inverse_bind"], want)
    # nodes: parents and rest TRS
    assert [n["parent"] for n in ls.nodes] == [-1, -1, 1, -1, -1, -1]
    assert [n["name"] for n in ls.nodes[:3]] == ["bar", "root", "elbow"]
    assert np.array_equal(ls.nodes[0]["translation"], [0.5, 0.25, -0.75]) and np.array_equal(ls.nodes[0]["scale"], [1.25] * 3)
    assert np.array_equal(ls.nodes[2]["translation"], [0, 0.9375, 0]) and np.array_equal(ls.nodes[2]["rotation"], [0, 0, 0, 1])
    # animations as channels
    bend, shift = ls.animations
    assert bend["name"] == "bend" and len(bend["channels"]) == 1
    ch = bend["channels"][0]
    assert (ch["node"], ch["path"], ch["interpolation"]) == (2, "rotation", "LINEAR")
    assert np.array_equal(ch["times"], [0.0, 0.5, 1.0])
    assert np.array_equal(ch["values"], np.array([G.quat_z(d) for d in G.BEND_DEGREES], np.float32).astype(np.float64))
    ch = shift["channels"][0]
    assert (ch["node"], ch["path"], ch["interpolation"]) == (2, "translation", "STEP")
    assert np.array_equal(ch["values"], np.array(G.SHIFT_VALUES, np.float32).astype(np.float64))


def test_without_skins_the_scene_loads_as_before():
    plain, skinned = loaders.load_glb(PATH), loaders.load_glb(PATH, skins=True)
    assert plain.skins == [] and plain.animations == [] and plain.nodes == [] and plain.warnings == []
    for name, value in vars(plain).items():
        if name in ("skins", "animations", "nodes"):
            continue
        other = getattr(skinned, name)
        if name == "meshes":
            assert [m.tobytes() for m in value] == [m.tobytes() for m in other]
        elif name == "instances":
            assert len(value) == len(other) == 4
            for a, b in zip(value, other):
                assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
        elif isinstance(value, np.ndarray):
            assert value.tobytes() == other.tobytes(), name
        else:
            assert value == other, name
    # the bar is placed by its node's own transform: the palette carries inverse(meshNodeWorld), the instance puts it back
    assert np.array_equal(plain.instances[0]["position"], [0.5, 0.25, -0.75]) and np.array_equal(plain.instances[0]["scale"], [1.25] * 3)
    # ... and a file without skins gives empty lists with the flag on
    cornell = loaders.load_glb(os.path.join(GOLDEN, "cornell_box.glb"), skins=True)
    assert cornell.skins == [] and cornell.animations == [] and len(cornell.nodes) > 0 and cornell.warnings == []


def _variant(tmp_path, mutate):
    path = str(tmp_path / "variant.glb")
    with open(path, "wb") as f:
        f.write(G.build_glb(mutate))
    return path


def test_joints_1_a_morph_target_and_a_cubic_spline_load_with_their_warnings(tmp_path):
    pos, _nrm, _uv, _idx, joints, weights = G.bar()

    def more_influences(doc, add):
        a = doc["meshes"][0]["primitives"][0]["attributes"]
        a["JOINTS_1"] = add(joints, 34962, "VEC4", 5123)
        a["WEIGHTS_1"] = add(np.zeros_like(weights), 34962, "VEC4", 5126)

    def morph(doc, add):
        doc["meshes"][0]["primitives"][0]["targets"] = [{"POSITION": add(np.zeros_like(pos), 34962, "VEC3", 5126)}]
        doc["meshes"][0]["weights"] = [0.0]

    def cubic(doc, add):
        keys = np.array([G.quat_z(d) for d in G.BEND_DEGREES], np.float32)
        triples = np.zeros((3, 3, 4), np.float32)  # (in-tangent, value, out-tangent) per key
        triples[:, 0], triples[:, 1], triples[:, 2] = 7.0, keys, -7.0
        s = doc["animations"][0]["samplers"][0]
        s["interpolation"], s["output"] = "CUBICSPLINE", add(triples.reshape(9, 4), None, "VEC4", 5126)

    base = loaders.load_glb(PATH, skins=True)
    for mutate, word in ((more_influences, "JOINTS_1"), (morph, "morph targets"), (cubic, "CUBICSPLINE")):
        path = _variant(tmp_path, mutate)
        ls = loaders.load_glb(path, skins=True)
        assert len(ls.warnings) == 1 and word in ls.warnings[0], (word, ls.warnings)
        assert loaders.load_glb(path).warnings == []  # (off: as before, not a word)
        assert ls.skins[0]["corners"].tobytes() == base.skins[0]["corners"].tobytes()
        ch = ls.animations[0]["channels"][0]
        assert ch["interpolation"] == "LINEAR" and np.array_equal(ch["values"], base.animations[0]["channels"][0]["values"]), word


def test_weights_stored_as_normalised_integers_are_read(tmp_path):
    _pos, _nrm, _uv, idx, _joints, weights = G.bar()

    def as_bytes(doc, add):
        doc["meshes"][0]["primitives"][0]["attributes"]["WEIGHTS_0"] = add(np.round(weights.astype(np.float64) * 255).astype(np.uint8), 34962, "VEC4", 5121)
        doc["accessors"][-1]["normalized"] = True

    ls = loaders.load_glb(_variant(tmp_path, as_bytes), skins=True)
    want = (np.round(weights.astype(np.float64) * 255) / 255).astype(np.float32)[idx]
    assert ls.skins[0]["corners"]["weight"].tobytes() == want.tobytes()


# ---- the host half of nxhip_set_blas_skin ----------------------------------------------------------------------------------------------

def test_corner_records_and_renormalisation():
    c = pod.make_skin_corners([[3, 1, 0, 0], [0, 1, 2, 3]], [[0.2, 0.2, 0, 0], [1, 1, 1, 1]])
    assert c.dtype.itemsize == 24 and c.dtype.fields["weight"][1] == 8
    assert c.tobytes()[:8] == np.array([3, 1, 0, 0], "<u2").tobytes()
    n = pod.normalise_skin_corners(c, 4)
    assert np.array_equal(n["weight"], np.array([[0.5, 0.5, 0, 0], [0.25] * 4], np.float32))
    assert np.array_equal(n["joint"], [[3, 1, 0, 0], [0, 1, 2, 3]])
    # binary64 sum, one rounding
    w = np.array([[0.1, 0.2, 0.3, 0.7]], np.float32)
    n = pod.normalise_skin_corners(pod.make_skin_corners([[0, 1, 2, 3]], w), 4)
    assert np.array_equal(n["weight"], (w.astype(np.float64) / w.astype(np.float64).sum()).astype(np.float32))
    # the joint of a zero weight is rewritten to 0, whatever it named
    n = pod.normalise_skin_corners(pod.make_skin_corners([[1, 900, 2, 65535]], [[1, 0, 3, 0]]), 3)
    assert np.array_equal(n["joint"], [[1, 0, 2, 0]]) and np.array_equal(n["weight"], np.array([[0.25, 0, 0.75, 0]], np.float32))
    assert np.array_equal(c["weight"][0], np.array([0.2, 0.2, 0, 0], np.float32)), "the input is left alone"


@pytest.mark.parametrize("joints,weights,count,word", [
    ([[0, 0, 0, 0]], [[0, 0, 0, 0]], 2, "sum to 0"),
    ([[0, 2, 0, 0]], [[0.5, 0.5, 0, 0]], 2, "joint index"),
    ([[0, 1, 0, 0]], [[0.5, -0.5, 0, 0]], 2, "negative"),
    ([[0, 1, 0, 0]], [[0.5, np.nan, 0, 0]], 2, "not finite"),
    ([[0, 1, 0, 0]], [[0.5, np.inf, 0, 0]], 2, "not finite"),
    ([[0, 0, 0, 0]], [[1, 0, 0, 0]], 0, "joint count"),
    ([[0, 0, 0, 0]], [[1, 0, 0, 0]], 65537, "joint count"),
])
def test_what_the_call_refuses_is_refused_on_the_host(joints, weights, count, word):
    with pytest.raises(ValueError, match=word):
        pod.normalise_skin_corners(pod.make_skin_corners(joints, weights), count)


def test_corner_arrays_of_the_wrong_shape_are_refused():
    with pytest.raises(ValueError):
        pod.make_skin_corners([[0, 1, 2]], [[1, 0, 0]])
    with pytest.raises(ValueError):
        pod.make_skin_corners([[0, 1, 2, 70000]], [[1, 0, 0, 0]])
    assert pod.normalise_skin_corners(pod.make_skin_corners([[0, 0, 0, 0]], [[2, 0, 0, 0]]), 65536)["weight"][0, 0] == 1.0


# ---- the C++ reader (nexus::OBJLoader, LoadOptions::skins) ------------------------------------------------------------------------------

def test_the_cpp_reader_finds_the_same_skin(tmp_path):
    from nexus_amd import capi

    ls = loaders.load_glb(PATH, skins=True)
    corners, joints, animations, warnings = capi.load_scene_skins(PATH)
    assert joints == [2, 0, 0, 0] and animations == 2 and warnings == []
    assert corners[0].tobytes() == ls.skins[0]["corners"].tobytes() and corners[1:] == [None, None, None]
    assert capi.load_scene_skins(PATH, skins=False) == ([None] * 4, [0] * 4, 0, [])
    # the meshes are what they are without the flag
    plain, _m, _i = capi.load_scene_file(PATH)
    assert [m.tobytes() for m in plain] == [m.tobytes() for m in ls.meshes]


def test_the_cpp_reader_warns_like_the_python_reader(tmp_path):
    from nexus_amd import capi

    pos, _nrm, _uv, _idx, joints, weights = G.bar()

    def more_influences(doc, add):
        doc["meshes"][0]["primitives"][0]["attributes"]["JOINTS_1"] = add(joints, 34962, "VEC4", 5123)

    def morph(doc, add):
        doc["meshes"][0]["primitives"][0]["targets"] = [{"POSITION": add(np.zeros_like(pos), 34962, "VEC3", 5126)}]

    def cubic(doc, add):
        triples = np.zeros((3, 3, 4), np.float32)
        triples[:, 1] = np.array([G.quat_z(d) for d in G.BEND_DEGREES], np.float32)
        s = doc["animations"][0]["samplers"][0]
        s["interpolation"], s["output"] = "CUBICSPLINE", add(triples.reshape(9, 4), None, "VEC4", 5126)

    base = capi.load_scene_skins(PATH)[0][0]
    for mutate, word in ((more_influences, "JOINTS_1"), (morph, "morph targets"), (cubic, "CUBICSPLINE")):
        path = _variant(tmp_path, mutate)
        corners, joints_of, animations, warnings = capi.load_scene_skins(path)
        assert len(warnings) == 1 and word in warnings[0], (word, warnings)
        assert warnings == loaders.load_glb(path, skins=True).warnings, "the two readers say the same"
        assert capi.load_scene_skins(path, skins=False)[3] == []
        assert corners[0].tobytes() == base.tobytes() and joints_of[0] == 2 and animations == 2
