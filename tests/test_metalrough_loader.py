"""tests/golden/metal_rough.glb through both .glb readers — nexus_amd.loaders (Python) and nexus::OBJLoader (C++, through the C-ABI) — with
the metallic-roughness option on and off: the same tables from both, the values worked out by hand with the option on, the parent's
tables byte for byte with it off (tests/golden/metal_rough_parent_tables.npz: written by the readers as they were before the option
existed, for this file and for cornell_box.glb).  No GPU."""
import os

import numpy as np

from nexus_amd import capi, loaders, pod
from tests.golden import make_metal_rough_glb as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILE = os.path.join(GOLDEN, "metal_rough.glb")


def _bytes(mats):
    return np.frombuffer(np.ascontiguousarray(mats, dtype=pod.MAT_DT).tobytes(), np.uint8).reshape(len(mats), 60)


def test_the_committed_file_is_what_the_generator_writes():
    assert open(FILE, "rb").read() == G.build_glb()
    assert os.path.getsize(FILE) < 16384


def test_option_off_gives_the_parents_tables():
    parent = np.load(os.path.join(GOLDEN, "metal_rough_parent_tables.npz"))
    for name in ("metal_rough", "cornell_box"):
        path = os.path.join(GOLDEN, name + ".glb")
        py = _bytes(loaders.load_glb(path).materials)
        assert np.array_equal(py, _bytes(loaders.load_glb(path, metal_rough=False).materials))
        cpp = _bytes(capi.load_scene_file(path)[1])
        assert np.array_equal(py, parent[name]) and np.array_equal(cpp, parent[name]), name
        assert not np.any(py[:, 56] == pod.MAT_METALROUGH)


def test_option_on_gives_the_files_own_model_from_both_readers():
    ls = loaders.load_glb(FILE, metal_rough=True)
    meshes, mats, insts = capi.load_scene_file(FILE, metal_rough=True)
    assert np.array_equal(_bytes(ls.materials), _bytes(mats)), "the two readers agree byte for byte"
    f = np.float32
    # name: type, albedo, roughness, ior, metallic, emissive, intensity, opacity — by hand from the generator's document
    want = [
        (pod.MAT_METALROUGH, (0.5, 0.5, 0.5), 0.5, 1.5, 0.0, (0, 0, 0), 1.0, 1.0),            # floor
        (pod.MAT_METALROUGH, (1.0, 1.0, 1.0), 0.15, 1.5, 0.0, (0, 0, 0), 1.0, 1.0),           # metallicFactor 0
        (pod.MAT_METALROUGH, (1.0, 0.77, 0.34), 0.15, 1.5, 1.0, (0, 0, 0), 1.0, 1.0),         # metallicFactor 1
        (pod.MAT_METALROUGH, (1.0, 0.77, 0.34), 0.5, 1.33, 1.0, (0, 0, 0), 1.0, 1.0),         # metallicFactor absent: glTF's default 1; KHR_materials_ior
        None,                                                                                  # transmissive: stays what it was
        (pod.MAT_METALROUGH, (0.9, 0.6, 0.3), 0.8, 1.5, 0.75, (0, 0, 0), 1.0, 0.75),          # the textured panel; opacity = baseColorFactor[3]
        (pod.MAT_METALROUGH, (0.0, 0.0, 0.0), 1.0, 1.5, 1.0, (1.0, 0.9, 0.8), 25.0, 1.0),     # the lamp: both factors absent
    ]
    parent = np.load(os.path.join(GOLDEN, "metal_rough_parent_tables.npz"))["metal_rough"]
    assert len(mats) == len(want) == 7
    for i, w in enumerate(want):
        m = mats[i]
        if w is None:
            assert int(m["type"]) == pod.MAT_DIELECTRIC and np.array_equal(_bytes(mats[i:i + 1])[0], parent[i]), "a transmissive material is the DIELECTRIC of the option-off table"
            assert float(m["u"][4]) == float(f(1.5))
            continue
        t, albedo, rough, ior, metallic, emissive, intensity, opacity = w
        assert int(m["type"]) == t, i
        assert np.array_equal(m["u"][0:3], np.array(albedo, f)) and m["u"][3] == f(rough) and m["u"][4] == f(ior) and m["u"][5] == f(metallic) and m["u"][6] == 0.0, (i, m["u"])
        assert np.array_equal(m["emissive"], np.array(emissive, f)) and m["intensity"] == f(intensity) and m["opacity"] == f(opacity), i
        assert int(m["diffuseMapId"]) == -1 and int(m["emissiveMapId"]) == -1
    # the detail table: the option does not touch it — the panel names the one metallic-roughness image, nobody a normal map
    assert ls.material_roughness_texture == [-1, -1, -1, -1, -1, 0, -1] and ls.material_normal_texture == [-1] * 7
    texs, normal_of, rough_of, scale_of, warnings = capi.load_scene_detail(FILE)
    assert list(rough_of) == ls.material_roughness_texture and list(normal_of) == ls.material_normal_texture and not warnings
    assert len(texs) == 1 and texs[0][0] == "roughness" and np.array_equal(texs[0][1], G.checker_map()) and np.array_equal(ls.detail_textures[0][1], G.checker_map())
    img = G.checker_map()
    assert set(np.unique(img[..., 2])) == {0, 255} and img[0, 0, 2] == 255 and img[0, 1, 2] == 0 and len(np.unique(img[..., 1])) == 16
    # geometry and placement do not depend on the option
    off = capi.load_scene_file(FILE)
    assert len(meshes) == len(off[0]) == 7 and all(np.array_equal(a, b) for a, b in zip(meshes, off[0])) and np.array_equal(insts, off[2])
