"""KHR_lights_punctual in both .glb readers (host/OBJLoader.cpp through the C-ABI, nexus_amd/loaders.py), and the Scene's analytic-light list
through nxs_*.  The fixture tests/golden/punctual_lights.glb is written by tests/golden/make_punctual_glb.py; what the readers must make of
it is worked out by hand below.  No GPU."""
import os

import numpy as np
import pytest

from nexus_amd import capi, loaders, pod
from tests import scene_helpers as SH

GLB = os.path.join(SH.GOLDEN, "punctual_lights.glb")
S30, C30 = 0.5, np.sqrt(3.0) / 2.0

# In the order the node walk meets them (scene roots 0, 1, 2 -> 3, 4 -> 6, 5):
#   lamp         child of "arm" (at (1, 2, 0.5), turned 90 degrees about y).  Ry(90) takes (x, y, z) to (z, y, -x): the child's translation
#                (0.5, 0.25, 0) becomes (0, 0.25, -0.5); world position (1, 2.25, 0).  -Z: -Ry(90)(0, 0, 1) = -(1, 0, 0).
#   spot         at (-1, 2.5, 0.25), turned -90 degrees about x.  Rx(-90) takes (x, y, z) to (x, z, -y): +Z goes to (0, 1, 0), so -Z looks
#                straight down.  Cone angles as written: 0.25, 0.5.
#   second spot  child of the spot: its translation (0, 0, -1) becomes Rx(-90)(0, 0, -1) = (0, -1, 0): world (-1, 1.5, 0.25).  Its own
#                rotation is about z and leaves -Z alone: straight down as well.  No `spot` object: the defaults 0 and pi / 4.
#   sun          a column-major matrix, Rx(30) and a translation: +Z goes to the third column (0, sin 30, cos 30), -Z to (0, -0.5, -0.866).
#                The position is the node's translation, whatever it means for a sun.
WANT = [
    dict(type=pod.ALIGHT_POINT, position=(1.0, 2.25, 0.0), direction=(-1.0, 0.0, 0.0), colour=(1.0, 0.8, 0.6), intensity=5.0, inner=0.0, outer=0.0),
    dict(type=pod.ALIGHT_SPOT, position=(-1.0, 2.5, 0.25), direction=(0.0, -1.0, 0.0), colour=(0.4, 0.6, 1.0), intensity=9.0, inner=0.25, outer=0.5),
    dict(type=pod.ALIGHT_SPOT, position=(-1.0, 1.5, 0.25), direction=(0.0, -1.0, 0.0), colour=(1.0, 1.0, 1.0), intensity=3.0, inner=0.0, outer=np.pi / 4),
    dict(type=pod.ALIGHT_DIRECTIONAL, position=(7.0, 8.0, 9.0), direction=(0.0, -S30, -C30), colour=(1.0, 1.0, 1.0), intensity=2.5, inner=0.0, outer=0.0),
]


def _check(lights, who):
    assert len(lights) == len(WANT), who
    for got, want in zip(lights, WANT):
        assert int(got["type"]) == want["type"], who
        assert np.allclose(got["position"], want["position"], atol=1e-6), (who, got["position"])
        assert np.allclose(got["direction"], want["direction"], atol=1e-6), (who, got["direction"])
        assert np.allclose(got["colour"], np.float32(want["colour"]), rtol=0, atol=0) and got["intensity"] == np.float32(want["intensity"])
        assert got["innerConeAngle"] == np.float32(want["inner"]) and got["outerConeAngle"] == np.float32(want["outer"]), who
        assert got["radius"] == 0.0 and got["angularRadius"] == 0.0  # (glTF's lights are points and delta suns; `range` is ignored)


def test_both_readers_make_the_same_records_of_the_fixture():
    py = loaders.load_glb(GLB).analytic_lights
    cc = capi.load_scene_analytic_lights(GLB)
    _check(py, "nexus_amd/loaders.py")
    _check(cc, "host/OBJLoader.cpp")
    for name in pod.ALIGHT_DT.names:
        assert np.allclose(py[name], cc[name], rtol=0, atol=1e-6), name
    # the meshes beside the lights are read as before
    meshes, mats, insts = capi.load_scene_file(GLB)
    assert [len(m) for m in meshes] == [2, 12] and len(insts) == 2


def test_a_file_without_the_extension_has_no_lights():
    assert len(capi.load_scene_analytic_lights(os.path.join(SH.GOLDEN, "cornell_box.glb"))) == 0
    assert len(loaders.load_glb(os.path.join(SH.GOLDEN, "cornell_box.glb")).analytic_lights) == 0


def test_the_fixture_is_what_its_generator_writes(tmp_path):
    import importlib.util
    import shutil

    spec = importlib.util.spec_from_file_location("make_punctual_glb", os.path.join(SH.GOLDEN, "make_punctual_glb.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.HERE = str(tmp_path)
    mod.main()
    assert open(os.path.join(str(tmp_path), "punctual_lights.glb"), "rb").read() == open(GLB, "rb").read()
    assert os.path.getsize(GLB) < 8192
    shutil.rmtree(str(tmp_path), ignore_errors=True)


def test_scene_round_trip_through_the_c_view():
    sc = capi.Scene(32, 32)
    assert len(sc.analytic_lights()) == 0
    a = pod.make_analytic_light(pod.ALIGHT_POINT, position=(1, 2, 3), colour=(0.5, 0.25, 1.0), intensity=4.0, radius=0.125)
    b = pod.make_analytic_light(pod.ALIGHT_DIRECTIONAL, direction=(0.0, -1.0, 0.5), intensity=2.0, angular_radius=0.01)
    assert sc.add_analytic_light(a) == 0 and sc.add_analytic_light(b) == 1
    got = sc.analytic_lights()
    assert got.tobytes() == np.array([a, b], dtype=pod.ALIGHT_DT).tobytes()
    sc.load_file(SH.GOLDEN + os.sep, "punctual_lights.glb")  # a file's lights join the list
    assert len(sc.analytic_lights()) == 2 + len(WANT) and sc.instance_count() == 2
    _check(sc.analytic_lights()[2:], "Scene::CreateMeshInstanceFromFile")
    sc.remove_analytic_light(0)
    assert sc.analytic_lights()[0].tobytes() == np.array(b, dtype=pod.ALIGHT_DT).tobytes() and len(sc.analytic_lights()) == 1 + len(WANT)
    with pytest.raises(capi.NexusError):
        sc.remove_analytic_light(99)
    assert sc.light_count() == 0  # (the mesh-light list is another list)
    sc.close()
