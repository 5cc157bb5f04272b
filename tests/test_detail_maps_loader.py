"""glTF normalTexture and metallicRoughnessTexture in both .glb readers: the Python reader (nexus_amd.loaders.load_glb) and the C++ one
(OBJLoader through the C-ABI) give the same detail fields for tests/golden/detail_maps.glb, and those are the numbers worked out here
by hand from what tests/golden/make_detail_glb.py writes.  Files without such maps give empty detail fields and no warnings."""
import importlib.util
import os

import numpy as np
import pytest

from nexus_amd import capi, loaders
from tests import scene_helpers as SH

GLB = os.path.join(SH.GOLDEN, "detail_maps.glb")


def _generator():
    spec = importlib.util.spec_from_file_location("make_detail_glb", os.path.join(SH.GOLDEN, "make_detail_glb.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _expected_textures():
    # 4 x 4 normal map, row 0 = top: (R, G, B) = (128 + 24 (x - 1.5), 128 - 20 (y - 1.5), 255 - 4 (x + y))
    normal = np.zeros((4, 4, 4), np.uint8)
    normal[..., 0] = np.array([92, 116, 140, 164])[None, :]
    normal[..., 1] = np.array([158, 138, 118, 98])[:, None]
    normal[..., 2] = np.array([[255, 251, 247, 243], [251, 247, 243, 239], [247, 243, 239, 235], [243, 239, 235, 231]])
    normal[..., 3] = 255
    # 8 x 2 metallic-roughness map: G climbs 40 .. 250 along the top row and falls 250 .. 40 along the bottom one, B = 255, R = 0
    rough = np.zeros((2, 8, 4), np.uint8)
    rough[0, :, 1] = [40, 70, 100, 130, 160, 190, 220, 250]
    rough[1, :, 1] = [250, 220, 190, 160, 130, 100, 70, 40]
    rough[..., 2] = 255
    rough[..., 3] = 255
    return normal, rough


def test_the_committed_file_is_what_the_generator_writes():
    assert open(GLB, "rb").read() == _generator().build_glb()
    assert os.path.getsize(GLB) < 8192


def test_both_readers_give_the_detail_fields_worked_out_by_hand():
    normal, rough = _expected_textures()
    py = loaders.load_glb(GLB)
    c_tex, c_normal, c_rough, c_scale, c_warn = capi.load_scene_detail(GLB)
    for textures in (py.detail_textures, c_tex):
        assert [k for k, _ in textures] == ["normal", "roughness"]
        assert np.array_equal(textures[0][1], normal) and np.array_equal(textures[1][1], rough)
    # floor: both maps, scale 0.8; box: the metallic-roughness map only; plinth and lamp: neither
    assert py.material_normal_texture == c_normal == [0, -1, -1, -1]
    assert py.material_roughness_texture == c_rough == [1, 1, -1, -1]
    assert np.array_equal(np.float32(py.material_normal_scale), np.float32([0.8, 1.0, 1.0, 1.0])) and np.array_equal(np.float32(c_scale), np.float32([0.8, 1.0, 1.0, 1.0]))
    assert py.warnings == [] and c_warn == []
    # the list of base-colour and emissive images is untouched: this file has none
    assert py.textures == [] and capi.load_scene_textures(GLB)[0] == []
    # the box's node is rotated 25 degrees about y and scaled (1.5, 0.75, 1)
    box = py.instances[1]
    assert np.allclose(box["scale"], (1.5, 0.75, 1.0), atol=1e-6) and np.allclose(box["rotation"], (0.0, 25.0, 0.0), atol=1e-4)
    # roughnessFactor 0.5 / 0.25 / 1 reach the materials as before; the G channel multiplies them on the device
    meshes, mats, insts = capi.load_scene_file(GLB)
    assert len(meshes) == 4 and np.array_equal(mats["u"][:, 3], py.materials["u"][:, 3])
    # the floor's texture coordinates: 0 .. 6 both ways, v flipped as every reader flips it
    uv = np.concatenate([py.meshes[0]["texCoord%d" % k] for k in range(3)])
    assert uv[:, 0].min() == 0 and uv[:, 0].max() == 6 and uv[:, 1].min() == -5 and uv[:, 1].max() == 1
    for k in range(3):
        assert np.array_equal(py.meshes[0]["texCoord%d" % k], meshes[0]["texCoord%d" % k])


@pytest.mark.parametrize("name", ["cornell_box.glb", "punctual_lights.glb"])
def test_files_without_detail_maps_give_empty_fields_and_no_warnings(name):
    path = os.path.join(SH.GOLDEN, name)
    py = loaders.load_glb(path)
    c_tex, c_normal, c_rough, c_scale, c_warn = capi.load_scene_detail(path)
    n = len(py.materials)
    assert py.detail_textures == [] and c_tex == []
    assert py.material_normal_texture == c_normal == [-1] * n and py.material_roughness_texture == c_rough == [-1] * n
    assert py.material_normal_scale == c_scale == [1.0] * n
    assert py.warnings == [] and c_warn == []


def test_texcoord_sets_and_texture_transforms_are_warned_about(tmp_path):
    def mutate(doc):
        doc["materials"][0]["normalTexture"]["texCoord"] = 1
        doc["materials"][1]["pbrMetallicRoughness"]["metallicRoughnessTexture"]["extensions"] = {"KHR_texture_transform": {"scale": [2, 2]}}

    path = tmp_path / "variant.glb"
    path.write_bytes(_generator().build_glb(mutate))
    py = loaders.load_glb(str(path))
    c_warn = capi.load_scene_detail(str(path))[4]
    for warnings in (py.warnings, c_warn):
        assert len(warnings) == 2
        assert "material 0" in warnings[0] and "normalTexture" in warnings[0] and "texCoord 1" in warnings[0]
        assert "material 1" in warnings[1] and "metallicRoughnessTexture" in warnings[1] and "KHR_texture_transform" in warnings[1]
    # the maps are used all the same, with set 0 as it is
    assert py.material_normal_texture == [0, -1, -1, -1] and py.material_roughness_texture == [1, 1, -1, -1]
    assert py.warnings == c_warn


def test_an_obj_has_no_detail_fields(tmp_path):
    path = tmp_path / "one.obj"
    path.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    py = loaders.load_obj(str(path))
    assert py.detail_textures == [] and py.material_normal_texture == [-1] and py.material_roughness_texture == [-1] and py.material_normal_scale == [1.0]
    assert capi.load_scene_detail(str(path))[:4] == ([], [-1], [-1], [1.0])
