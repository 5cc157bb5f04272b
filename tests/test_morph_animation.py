"""Morph weights on the host (nexus_amd.animation.morph_weights and its C++ twin nexus::Scene::MorphWeights through capi.Scene): the
fixture's defaults, and its weights channel at, between and outside the keys, STEP and LINEAR."""
import copy
import os
import sys

import numpy as np
import pytest

from nexus_amd import animation, capi, loaders

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, GOLDEN)
import make_morph_glb as G  # noqa: E402

PATH = os.path.join(GOLDEN, "morph_bar.glb")
_SCENE = []
KEYS = np.array(G.MORPH_VALUES, np.float64)
TIMES = [None, -2.0, 0.0, 0.125, 0.3, 0.5, 0.77, 1.0, 9.0]


def scene():
    if not _SCENE:
        _SCENE.append(loaders.load_glb(PATH, skins=True, morphs=True))
    return _SCENE[0]


def test_the_defaults_without_an_animation_or_without_a_weights_channel():
    s = scene()
    for w in (animation.morph_weights(s, 0), animation.morph_weights(s, s.morphs[0], None, 0.7), animation.morph_weights(s, 0, 0, 0.5), animation.morph_weights(s, 0, 1, 0.5)):
        assert w.dtype == np.float32 and w.shape == (3,) and np.array_equal(w, [0.0, 0.25, 0.0])
    w = animation.morph_weights(s, 0)
    w[0] = 5.0
    assert s.morphs[0]["weights"][0] == 0.0, "a copy: the scene's defaults are left alone"


def test_linear_at_between_and_outside_the_keys():
    s = scene()
    for t, want in ((0.0, KEYS[0]), (0.5, KEYS[1]), (1.0, KEYS[2]), (-1.0, KEYS[0]), (3.0, KEYS[2]),
                    (0.25, 0.5 * KEYS[0] + 0.5 * KEYS[1]), (0.75, 0.5 * KEYS[1] + 0.5 * KEYS[2]), (0.6, 0.8 * KEYS[1] + 0.2 * KEYS[2])):
        got = animation.morph_weights(s, 0, 2, t)
        assert got.dtype == np.float32 and np.allclose(got, want, rtol=0, atol=2.0 ** -23), (t, got, want)
    # binary64, rounded once
    t = 0.3
    u = (t - 0.0) / (0.5 - 0.0)
    assert np.array_equal(animation.morph_weights(s, 0, 2, t), ((1.0 - u) * KEYS[0] + u * KEYS[1]).astype(np.float32))
    # the bones do not see the weights channel, and the weights do not see the bones'
    assert np.array_equal(animation.joint_palette(s, 0, 2, 0.3), animation.joint_palette(s, 0, None, 0.0))


def test_step_holds_until_the_next_key():
    s = scene()
    step = copy.deepcopy(s.animations[2])
    step["channels"][0]["interpolation"] = "STEP"
    for t, k in ((-1.0, 0), (0.0, 0), (0.25, 0), (0.4999, 0), (0.5, 1), (0.9, 1), (1.0, 2), (4.0, 2)):
        assert np.array_equal(animation.morph_weights(s, 0, step, t), KEYS[k].astype(np.float32)), t


def test_a_channel_of_another_width_is_refused():
    s = scene()
    wrong = copy.deepcopy(s.animations[2])
    wrong["channels"][0]["values"] = wrong["channels"][0]["values"][:, :2]
    with pytest.raises(ValueError):
        animation.morph_weights(s, 0, wrong, 0.3)


@pytest.mark.parametrize("animation_idx", [None, 0, 2])
def test_the_cpp_scene_evaluates_the_same_weights_to_the_bit(animation_idx):
    sc = capi.Scene(32, 32)
    try:
        sc.set_skins(True)
        sc.set_morphs(True)
        sc.load_file(os.path.dirname(PATH) + os.sep, os.path.basename(PATH))
        assert sc.mesh_count() == 4 and sc.animation_count() == 3
        assert [sc.mesh_target_count(m) for m in range(4)] == [3, 0, 0, 0] and [sc.mesh_joint_count(m) for m in range(4)] == [2, 0, 0, 0]
        for t in TIMES[1:]:
            got = sc.morph_weights(0, animation_idx, t)
            want = animation.morph_weights(scene(), 0, animation_idx, t)
            assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (animation_idx, t, got, want)
        with pytest.raises(capi.NexusError):
            sc.morph_weights(1, None, 0.0)  # the floor has no targets
        with pytest.raises(capi.NexusError):
            sc.morph_weights(0, 3, 0.0)  # no such animation
        # the joint palette is what it is without the weights channel in the scene
        assert sc.joint_palette(0, 2, 0.3).tobytes() == sc.joint_palette(0, None, 0.0).tobytes()
    finally:
        sc.close()


def test_a_scene_loaded_without_morphs_has_none():
    sc = capi.Scene(32, 32)
    try:
        sc.set_skins(True)
        sc.load_file(os.path.dirname(PATH) + os.sep, os.path.basename(PATH))
        assert [sc.mesh_target_count(m) for m in range(4)] == [0] * 4 and sc.animation_count() == 3
        with pytest.raises(capi.NexusError):
            sc.morph_weights(0, None, 0.0)
    finally:
        sc.close()
