"""Pose evaluation on the host (nexus_amd/animation.py joint_palette) against closed forms written here in float64, on
tests/golden/skinned_bar.glb: the elbow turns about z at the pivot (0, 0.75, 0) of the bar's mesh space — the file's node transforms
are exactly representable, and the uniform scale of the mesh node commutes with the rotation — and the root joint never moves.

Tolerance: both sides are binary64 results rounded once to binary32, so each entry may differ by one binary32 ulp, taken at the larger
of |entry| and the largest magnitude of its row (the row's entries come out of sums of that size)."""
import os

import numpy as np
import pytest

from nexus_amd import animation, loaders

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skinned_bar.glb")
PIVOT = np.array([0.0, 0.75, 0.0])
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
_SCENE = []


def scene():
    if not _SCENE:
        _SCENE.append(loaders.load_glb(PATH, skins=True))
    return _SCENE[0]


def ulps_apart(got, want, ulps=1):
    """entries of two (joints, 12) palettes within `ulps` binary32 ulp at max(|entry|, row maximum)"""
    got, want = np.asarray(got, np.float32).reshape(-1, 3, 4), np.asarray(want, np.float64).astype(np.float32).reshape(-1, 3, 4)
    scale = np.maximum(np.abs(want), np.max(np.abs(want), axis=2, keepdims=True)).astype(np.float32)
    tol = ulps * np.spacing(scale).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return bool(np.all(err <= tol)), float(np.max(err / tol))


def turn_about_pivot(degrees):
    """rotate by `degrees` about z at PIVOT: p' = R (p - c) + c"""
    a = np.radians(degrees)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return np.concatenate([R, (PIVOT - R @ PIVOT)[:, None]], 1)


def test_the_rest_pose_is_the_identity():
    pal = animation.joint_palette(scene(), 0, None, 0.0)
    assert pal.shape == (2, 12) and pal.dtype == np.float32
    assert ulps_apart(pal, [IDENTITY, IDENTITY])[0]
    assert ulps_apart(animation.joint_palette(scene(), scene().skins[0]), [IDENTITY, IDENTITY])[0]  # (the skin itself; rest pose by default)


@pytest.mark.parametrize("t,degrees", [(0.5, 45.0), (0.0, 0.0), (1.0, 90.0), (0.25, 22.5), (0.8, 72.0)])
def test_the_elbow_palette_is_the_turn_about_its_pivot(t, degrees):
    pal = animation.joint_palette(scene(), 0, 0, t)
    ok, worst = ulps_apart(pal, [IDENTITY, turn_about_pivot(degrees)])
    print("t = %g: worst entry %.3f of the tolerance" % (t, worst))
    assert ok, worst
    assert ulps_apart(pal[:1], [IDENTITY])[0], "the root joint is not animated"


def test_times_outside_the_keys_clamp():
    s = scene()
    assert np.array_equal(animation.joint_palette(s, 0, 0, -3.0), animation.joint_palette(s, 0, 0, 0.0))
    assert np.array_equal(animation.joint_palette(s, 0, 0, 17.0), animation.joint_palette(s, 0, 0, 1.0))
    assert ulps_apart(animation.joint_palette(s, 0, 0, 17.0), [IDENTITY, turn_about_pivot(90.0)])[0]
    assert np.array_equal(animation.joint_palette(s, 0, 1, -1.0), animation.joint_palette(s, 0, None, 0.0))


def test_a_step_channel_holds_its_value_until_the_next_key():
    s = scene()

    def shifted(dx, dz):  # the elbow moved by (dx, 0, dz) in world units = that / 1.25 in the bar's mesh space
        m = IDENTITY.copy()
        m[:, 3] = (dx / 1.25, 0.0, dz / 1.25)
        return m

    for t, want in ((0.0, shifted(0, 0)), (0.25, shifted(0, 0)), (0.4999, shifted(0, 0)), (0.5, shifted(0.25, 0)), (0.75, shifted(0.25, 0)),
                    (0.9999, shifted(0.25, 0)), (1.0, shifted(0.25, 0.25)), (2.0, shifted(0.25, 0.25))):
        assert ulps_apart(animation.joint_palette(s, 0, 1, t), [IDENTITY, want])[0], t
    # the same keys read LINEAR move at once
    import copy

    linear = copy.deepcopy(s.animations[1])
    linear["channels"][0]["interpolation"] = "LINEAR"
    assert ulps_apart(animation.joint_palette(s, 0, linear, 0.25), [IDENTITY, shifted(0.125, 0)])[0]


def test_slerp_takes_the_shorter_arc_and_survives_equal_keys():
    q0 = np.array([0.0, 0.0, 0.0, 1.0])
    half = np.radians(100.0) / 2
    q1 = np.array([0.0, 0.0, np.sin(half), np.cos(half)])
    mid = animation.slerp(q0, -q1, 0.5)  # -q1 is the same rotation: the interpolation must not go the long way round
    quarter = np.radians(50.0) / 2
    assert np.allclose(mid, [0, 0, np.sin(quarter), np.cos(quarter)], atol=1e-15)
    assert np.allclose(animation.slerp(q1, q1, 0.3), q1, atol=1e-15)  # 1 - |q0 . q1| < 1e-9: normalised lerp, no division by sin(0)
    near = q1 + np.array([0, 0, 1e-12, 0])
    near /= np.linalg.norm(near)
    assert np.all(np.isfinite(animation.slerp(q1, near, 0.5)))


def test_parents_compose_down_the_tree():
    """the elbow is a child of the root joint: a turn of the ROOT carries the elbow with it"""
    import copy

    s = scene()
    anim = copy.deepcopy(s.animations[0])
    anim["channels"][0]["node"] = 1  # the same keys on the root joint, whose pivot is the bar's foot
    pal = animation.joint_palette(s, 0, anim, 0.5)
    a = np.radians(45.0)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    turned = np.concatenate([R, np.zeros((3, 1))], 1)  # about the mesh-space origin
    assert ulps_apart(pal, [turned, turned])[0]
    world = animation.node_world_matrices(s, anim, 0.5)
    assert np.allclose(world[2][:3, 3], np.array([0.5, 0.25, -0.75]) + R @ np.array([0.0, 0.9375, 0.0]), atol=1e-15)


@pytest.mark.parametrize("animation_idx,t", [(None, 0.0), (0, 0.0), (0, 0.3), (0, 0.5), (0, 0.77), (0, 1.0), (1, 0.25), (1, 0.5), (0, -1.0), (1, 9.0)])
def test_the_cpp_scene_evaluates_the_same_palette(animation_idx, t):
    """nexus::Scene::JointPalette (through capi.Scene) against animation.joint_palette: two independent binary64 evaluations, each
    rounded once, so two binary32 ulp"""
    from nexus_amd import capi

    sc = capi.Scene(32, 32)
    try:
        sc.set_skins(True)
        sc.load_file(os.path.dirname(PATH) + os.sep, os.path.basename(PATH))
        assert sc.mesh_count() == 4 and sc.animation_count() == 2
        assert [sc.mesh_joint_count(m) for m in range(4)] == [2, 0, 0, 0]
        got = sc.joint_palette(0, animation_idx, t)
        want = animation.joint_palette(scene(), 0, animation_idx, t)
        ok, worst = ulps_apart(got, want.astype(np.float64), ulps=2)
        assert got.shape == want.shape == (2, 12) and ok, worst
        with pytest.raises(capi.NexusError):
            sc.joint_palette(1, None, 0.0)  # the floor has no skin
        with pytest.raises(capi.NexusError):
            sc.joint_palette(0, 2, 0.0)  # no such animation
    finally:
        sc.close()


def test_a_scene_loaded_without_skins_has_none():
    from nexus_amd import capi

    sc = capi.Scene(32, 32)
    try:
        sc.load_file(os.path.dirname(PATH) + os.sep, os.path.basename(PATH))
        assert sc.mesh_count() == 4 and sc.animation_count() == 0 and [sc.mesh_joint_count(m) for m in range(4)] == [0] * 4
        with pytest.raises(capi.NexusError):
            sc.joint_palette(0, None, 0.0)
    finally:
        sc.close()
