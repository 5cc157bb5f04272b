"""glTF alphaMode / alphaCutoff in the loaders: tests/golden/alpha_cutout.glb (tools/make_alpha_cutout_glb.py) read with and without the
option, by the Python reader and by the C++ reader through its C-API.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

from nexus_amd import capi, loaders, pod
from tests import scene_helpers as SH

PATH = os.path.join(SH.GOLDEN, "alpha_cutout.glb")

# floor (the file says nothing: glTF's default), leaves_upper (MASK, default cutoff), leaves_lower (MASK 0.25), decal (OPAQUE), lamp (BLEND)
WANT = [(pod.ALPHA_OPAQUE, 0.5), (pod.ALPHA_MASK, 0.5), (pod.ALPHA_MASK, 0.25), (pod.ALPHA_OPAQUE, 0.5), (pod.ALPHA_BLEND, 0.5)]


def _generator():
    spec = importlib.util.spec_from_file_location("make_alpha_cutout_glb", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "make_alpha_cutout_glb.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _as_pairs(table):
    return [(int(a["mode"]), float(a["cutoff"])) for a in table]


def test_the_committed_file_is_what_the_generator_writes():
    assert open(PATH, "rb").read() == _generator().build_glb()
    assert os.path.getsize(PATH) < 16 * 1024


def test_python_reader_with_and_without_the_option():
    plain = loaders.load_glb(PATH)
    assert plain.material_alpha is None, "off by default: every existing scene renders as before"
    ls = loaders.load_glb(PATH, alpha_modes=True)
    assert ls.material_alpha.dtype == pod.ALPHA_DT and _as_pairs(ls.material_alpha) == [(m, pytest.approx(c)) for m, c in WANT]
    # nothing else moves
    assert np.array_equal(plain.materials, ls.materials) and len(plain.meshes) == len(ls.meshes) == 5
    assert ls.material_names == ["floor", "leaves_upper", "leaves_lower", "decal", "lamp"]
    # the map: one texture shared by three materials, alpha 0 or 255 in 2 x 2-texel blocks
    assert ls.material_diffuse_texture == [-1, 0, 0, 0, -1] and len(ls.textures) == 1
    px = ls.textures[0][1]
    assert px.shape == (8, 8, 4) and set(np.unique(px[..., 3])) == {0, 255}
    blocks = px[..., 3].reshape(4, 2, 4, 2)
    assert np.all(blocks == blocks[:, :1, :, :1]) and px[0, 0, 3] == 255 and px[0, 2, 3] == 0


def test_cpp_reader_with_and_without_the_option():
    assert len(capi.load_scene_material_alpha(PATH, alpha_modes=False)) == 0
    got = capi.load_scene_material_alpha(PATH)
    assert _as_pairs(got) == [(m, pytest.approx(c)) for m, c in WANT]
    # ... and agrees with the Python reader record for record
    assert np.array_equal(got, loaders.load_glb(PATH, alpha_modes=True).material_alpha)
    # the option changes nothing else the reader returns
    meshes, mats, insts = capi.load_scene_file(PATH)
    assert len(meshes) == 5 and len(mats) == 5 and len(insts) == 5


def test_an_unknown_mode_is_an_error_in_both_readers(tmp_path):
    def mutate(doc):
        doc["materials"][1]["alphaMode"] = "DITHER"
    bad = tmp_path / "bad.glb"
    bad.write_bytes(_generator().build_glb(mutate))
    with pytest.raises(ValueError, match="alphaMode"):
        loaders.load_glb(str(bad), alpha_modes=True)
    with pytest.raises(capi.NexusError, match="alphaMode"):
        capi.load_scene_material_alpha(str(bad))
    # (not asked, not looked at)
    assert loaders.load_glb(str(bad)).material_alpha is None
    assert len(capi.load_scene_material_alpha(str(bad), alpha_modes=False)) == 0


@pytest.mark.parametrize("cutoff", [1.5, -0.1])
def test_a_mask_cutoff_outside_the_unit_interval_is_refused_by_the_readers_with_the_materials_number(tmp_path, cutoff):
    def mutate(doc):
        doc["materials"][2]["alphaCutoff"] = cutoff
        doc["materials"][3]["alphaCutoff"] = 4.0  # (OPAQUE: the number means nothing and is carried as it stands)
    bad = tmp_path / "cutoff.glb"
    bad.write_bytes(_generator().build_glb(mutate))
    with pytest.raises(ValueError, match="material 2 .*alphaCutoff"):
        loaders.load_glb(str(bad), alpha_modes=True)
    with pytest.raises(capi.NexusError, match="material 2 .*alphaCutoff"):
        capi.load_scene_material_alpha(str(bad))
    assert loaders.load_glb(str(bad)).material_alpha is None
    # the ends of the interval are fine
    def ends(doc):
        doc["materials"][1]["alphaCutoff"] = 0.0
        doc["materials"][2]["alphaCutoff"] = 1.0
    ok = tmp_path / "ends.glb"
    ok.write_bytes(_generator().build_glb(ends))
    assert [float(a["cutoff"]) for a in capi.load_scene_material_alpha(str(ok))][1:3] == [0.0, 1.0]
    assert np.array_equal(capi.load_scene_material_alpha(str(ok)), loaders.load_glb(str(ok), alpha_modes=True).material_alpha)


def test_the_scene_facade_carries_the_modes_only_when_asked():
    sc = capi.Scene(32, 32)
    sc.load_file(SH.GOLDEN + os.sep, "alpha_cutout.glb")
    assert len(sc.material_alphas()) == 0
    sc.close()
    sc = capi.Scene(32, 32)
    sc.set_material_alpha_modes(True)
    sc.load_file(SH.GOLDEN + os.sep, "alpha_cutout.glb")
    assert _as_pairs(sc.material_alphas()) == [(m, pytest.approx(c)) for m, c in WANT]
    sc.close()
