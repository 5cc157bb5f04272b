"""glTF morph targets through the Python reader (loaders.load_glb(morphs=True)), the C++ reader (LoadOptions::morphs) and the host-side
half of the binding (pod.make_morph_corners).  The fixture is tests/golden/morph_bar.glb; what it must yield is restated here from the
generator's own arrays (tests/golden/make_morph_glb.py)."""
import os
import sys

import numpy as np
import pytest

from nexus_amd import capi, loaders, pod

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, GOLDEN)
import make_morph_glb as G  # noqa: E402
import make_skinned_glb as S  # noqa: E402

PATH = os.path.join(GOLDEN, "morph_bar.glb")


def _variant(tmp_path, mutate):
    path = str(tmp_path / "variant.glb")
    with open(path, "wb") as f:
        f.write(G.build_glb(mutate))
    return path


def test_the_committed_fixture_is_what_the_generator_writes():
    data = open(PATH, "rb").read()
    assert data == G.build_glb()
    assert len(data) < 100 * 1024


def test_deltas_equal_what_the_generator_wrote_de_indexed():
    ls = loaders.load_glb(PATH, morphs=True)
    assert ls.warnings == []
    assert len(ls.morphs) == 1 and ls.skins == [] and len(ls.nodes) == 6 and len(ls.animations) == 3
    m = ls.morphs[0]
    idx = S.bar()[3]
    bulge_p, bulge_n, twist_p, dented, _dent_p = G.targets()
    d = m["deltas"]
    assert d.dtype == pod.MORPH_CORNER_DT and d.shape == (3, 3 * 832) and m["mesh"] == 0 and m["mesh_node"] == 0
    assert d["dPosition"][0].tobytes() == bulge_p[idx].tobytes() and d["dNormal"][0].tobytes() == bulge_n[idx].tobytes()
    assert d["dPosition"][1].tobytes() == twist_p[idx].tobytes()
    assert not d["dNormal"][1].any() and not d["dNormal"][2].any(), "a target without NORMAL has zero normal deltas"
    # the sparse accessor expanded over zeros
    dense = G.dense_dent()
    assert d["dPosition"][2].tobytes() == dense[idx].tobytes()
    assert 0 < np.count_nonzero(np.any(dense != 0, axis=1)) == len(dented) < 64
    assert np.any(d["dPosition"][0] != 0) and np.any(d["dNormal"][0] != 0) and np.any(d["dPosition"][1] != 0)
    # defaults, names, the weights channel
    assert m["weights"].dtype == np.float32 and np.array_equal(m["weights"], [0.0, 0.25, 0.0]) and m["names"] == ["bulge", "twist", "dent"]
    ch = ls.animations[2]["channels"]
    assert ls.animations[2]["name"] == "morph" and len(ch) == 1
    assert (ch[0]["node"], ch[0]["path"], ch[0]["interpolation"]) == (0, "weights", "LINEAR")
    assert ch[0]["values"].shape == (3, 3) and np.array_equal(ch[0]["values"], np.array(G.MORPH_VALUES)) and np.array_equal(ch[0]["times"], G.MORPH_TIMES)
    # the triangles are those of a run without the option
    assert [t.tobytes() for t in ls.meshes] == [t.tobytes() for t in loaders.load_glb(PATH).meshes]


def test_skins_alone_load_as_before_with_the_old_warning():
    skinned = loaders.load_glb(PATH, skins=True)
    assert skinned.warnings == ["mesh 0 primitive 0: morph targets are ignored"]
    assert skinned.morphs == [] and len(skinned.animations) == 3 and skinned.animations[2]["channels"] == []
    both = loaders.load_glb(PATH, skins=True, morphs=True)
    assert both.warnings == [] and len(both.skins) == len(skinned.skins) == 1
    for a, b in zip(skinned.skins, both.skins):
        assert a["corners"].tobytes() == b["corners"].tobytes() and a["joints"] == b["joints"] and a["mesh_node"] == b["mesh_node"]
        assert np.array_equal(a["inverse_bind"], b["inverse_bind"])
    for a, b in zip(skinned.animations[:2], both.animations[:2]):
        assert len(a["channels"]) == len(b["channels"]) == 1
        for x, y in zip(a["channels"], b["channels"]):
            assert (x["node"], x["path"], x["interpolation"]) == (y["node"], y["path"], y["interpolation"])
            assert np.array_equal(x["times"], y["times"]) and np.array_equal(x["values"], y["values"])
    plain = loaders.load_glb(PATH)
    assert plain.warnings == [] and plain.morphs == [] and plain.nodes == [] and plain.animations == []
    # the skinned fixture, which has no targets, yields none with the option on
    bar = loaders.load_glb(os.path.join(GOLDEN, "skinned_bar.glb"), skins=True, morphs=True)
    assert bar.morphs == [] and bar.warnings == [] and len(bar.skins) == 1


def test_node_weights_win_over_mesh_weights_and_no_weights_are_zeros(tmp_path):
    def on_node(doc, add):
        doc["nodes"][0]["weights"] = [0.5, 0.0, 1.0]

    def none(doc, add):
        del doc["meshes"][0]["weights"], doc["meshes"][0]["extras"]

    for mutate, want, names in ((on_node, [0.5, 0.0, 1.0], ["bulge", "twist", "dent"]), (none, [0.0, 0.0, 0.0], [])):
        path = _variant(tmp_path, mutate)
        m = loaders.load_glb(path, morphs=True).morphs[0]
        assert np.array_equal(m["weights"], want) and m["names"] == names
        _d, w, _a, warnings = capi.load_scene_morphs(path)
        assert np.array_equal(w[0], want) and warnings == []


def test_a_sparse_accessor_over_a_buffer_view_is_read(tmp_path):
    bulge_p, _bn, _tp, dented, dent_p = G.targets()
    idx = S.bar()[3]

    def over_bulge(doc, add):
        acc = doc["accessors"][doc["meshes"][0]["primitives"][0]["targets"][2]["POSITION"]]
        acc["bufferView"] = doc["accessors"][add(bulge_p, 34962, "VEC3", 5126)]["bufferView"]

    path = _variant(tmp_path, over_bulge)
    want = bulge_p.copy()
    want[dented] = dent_p
    assert loaders.load_glb(path, morphs=True).morphs[0]["deltas"]["dPosition"][2].tobytes() == want[idx].tobytes()
    assert capi.load_scene_morphs(path)[0][0]["dPosition"][2].tobytes() == want[idx].tobytes()


def test_what_the_readers_refuse(tmp_path):
    pos = S.bar()[0]

    def second_primitive_without_targets(doc, add):
        prim = dict(doc["meshes"][0]["primitives"][0])
        del prim["targets"]
        doc["meshes"][0]["primitives"].append(prim)

    def integer_target(doc, add):
        doc["meshes"][0]["primitives"][0]["targets"][1]["POSITION"] = add(np.zeros((len(pos), 3), np.int16), 34962, "VEC3", 5122)

    for mutate, word in ((second_primitive_without_targets, "different numbers of morph targets"), (integer_target, "float VEC3")):
        path = _variant(tmp_path, mutate)
        with pytest.raises(ValueError, match=word):
            loaders.load_glb(path, morphs=True)
        with pytest.raises(capi.NexusError, match=word):
            capi.load_scene_morphs(path)
        assert loaders.load_glb(path).warnings == []  # (off: as before, not a word)


def test_the_cpp_reader_returns_the_same_bytes_and_warnings(tmp_path):
    ls = loaders.load_glb(PATH, skins=True, morphs=True)
    deltas, weights, animations, warnings = capi.load_scene_morphs(PATH, skins=True)
    assert animations == 3 and warnings == ls.warnings == []
    assert deltas[0].shape == (3, 3 * 832) and deltas[0].tobytes() == ls.morphs[0]["deltas"].tobytes() and deltas[1:] == [None, None, None]
    assert weights[0].tobytes() == ls.morphs[0]["weights"].tobytes() and weights[1:] == [None, None, None]
    assert capi.load_scene_morphs(PATH, morphs=False) == ([None] * 4, [None] * 4, 0, [])
    # without the new flag the C++ reader says what it said, like the Python reader
    assert capi.load_scene_skins(PATH)[3] == loaders.load_glb(PATH, skins=True).warnings == ["mesh 0 primitive 0: morph targets are ignored"]
    corners = capi.load_scene_skins(PATH)[0][0]
    assert corners.tobytes() == ls.skins[0]["corners"].tobytes()

    def cubic(doc, add):  # a CUBICSPLINE weights sampler: (in-tangent, value, out-tangent) rows of three weights per key
        rows = np.zeros((3, 3, 3), np.float32)
        rows[:, 0], rows[:, 1], rows[:, 2] = 7.0, np.array(G.MORPH_VALUES, np.float32), -7.0
        s = doc["animations"][2]["samplers"][0]
        s["interpolation"], s["output"] = "CUBICSPLINE", add(rows.reshape(-1), None, "SCALAR", 5126)

    path = _variant(tmp_path, cubic)
    py = loaders.load_glb(path, morphs=True)
    assert len(py.warnings) == 1 and "CUBICSPLINE" in py.warnings[0] and capi.load_scene_morphs(path)[3] == py.warnings
    ch = py.animations[2]["channels"][0]
    assert ch["interpolation"] == "LINEAR" and np.array_equal(ch["values"], np.array(G.MORPH_VALUES))


# ---- the host half of the binding -------------------------------------------------------------------------------------------------------

def test_morph_corner_records():
    dp = np.arange(2 * 6 * 3, dtype=np.float32).reshape(2, 6, 3)
    c = pod.make_morph_corners(dp)
    assert c.dtype == pod.MORPH_CORNER_DT and c.dtype.itemsize == 24 and c.dtype.fields["dNormal"][1] == 12 and c.shape == (2, 6)
    assert np.array_equal(c["dPosition"], dp) and not c["dNormal"].any()
    assert c.tobytes()[:12] == dp[0, 0].tobytes()
    c = pod.make_morph_corners(dp[0], -dp[0])  # one target given as (3 n, 3)
    assert c.shape == (1, 6) and np.array_equal(c["dNormal"][0], -dp[0])
    assert pod.MORPH_MAX_TARGETS == 1024
    for bad in (np.zeros((2, 5, 3)), np.zeros((2, 6, 2)), np.zeros(6)):
        with pytest.raises(ValueError):
            pod.make_morph_corners(bad)
    with pytest.raises(ValueError):
        pod.make_morph_corners(dp, np.zeros((2, 3, 3)))
