"""The light table of NXHIP_LIGHTS_POWER on the device (nx_lights.hip) against the numpy restatement (tests/light_reference.py): layout,
cumulative probabilities, the pick and its probability; rebuilt after instances move and meshes deform; the entry points' refusals.

Bound on a probability: |P - p64| <= 2^-23 + 1e-5 p64 against the float64 shares.  The first term: P is the difference of two
binary32 roundings of values <= 1, 2^-25 each, with a factor-2 margin; the second: the areas are computed in binary32 from the
transformed corners."""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen
from tests import light_reference as LR
from tests import light_scenes as LS

pytestmark = pytest.mark.gpu

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _power_ctx(gpu_ctx_factory, scene):
    ctx = gpu_ctx_factory(64, 48)
    scene.upload(ctx)
    ctx.set_light_sampling(pod.LIGHTS_POWER)
    return ctx


def _check_table(ctx, w, entry_light, base, what):
    cdf, light, got_base = ctx.read_light_table(len(base) - 1)
    assert np.array_equal(got_base, base), what
    assert len(cdf) == len(w) and np.array_equal(light, entry_light), what
    assert np.all(np.diff(cdf) >= 0) and cdf[-1] == np.float32(1.0), what
    P = LR.probabilities(cdf)
    p64 = LR.shares(w)
    err = np.abs(P.astype(np.float64) - p64) - 1e-5 * p64
    print("%s: %d entries, max (|P - p64| - 1e-5 p64) = %.3g (bound %.3g), max relative error of the large entries %.3g" % (
        what, len(w), err.max(), 2.0 ** -23, (np.abs(P - p64) / np.maximum(p64, 1e-30))[p64 >= np.median(p64)].max()))
    assert err.max() <= 2.0 ** -23, what
    assert np.all(P[w == 0.0] == 0.0), what
    return cdf


def _pick_values(cdf, n_random, seed=11):
    rng = np.random.RandomState(seed)
    u = np.concatenate([np.array([0.0, 1.0 - 2.0 ** -23], np.float32), cdf, np.nextafter(cdf, np.float32(0)), np.nextafter(cdf, np.float32(2)),
                        (rng.randint(0, 1 << 23, n_random) / float(1 << 23)).astype(np.float32)])
    return u[(u >= 0) & (u < 1)]


def _check_picks(ctx, cdf, n_random=100000):
    u = _pick_values(cdf, n_random)
    assert len(u) >= 100000
    entry, prob = ctx.light_pick_batch(u)
    want = LR.pick(cdf, u)
    assert np.array_equal(entry, want)
    assert np.array_equal(prob, LR.probabilities(cdf)[want])
    assert np.all(prob > 0)
    _, steps = LR.guided_pick(cdf, LR.guide(cdf), u[-n_random:])
    print("%d entries: %d picks equal searchsorted; the walk on the random ones: mean %.3f steps, max %d" % (len(cdf), len(u), steps.mean(), steps.max()))


def test_table_of_the_emitter_scene(gpu_ctx_factory):
    scene = _cached("emitters", LS.emitter_scene)
    w, entry_light, base = LR.scene_weights(scene)
    assert base.tolist() == [0, 2, 4, 4 + 192, 198] and np.all(w > 0)
    ctx = _power_ctx(gpu_ctx_factory, scene)
    cdf = _check_table(ctx, w, entry_light, base, "emitter scene")
    _check_picks(ctx, cdf)


def test_picks_on_a_70000_triangle_light(gpu_ctx_factory):
    """the scan spans several workgroups, the guide has 131 072 entries"""
    scene = _cached("torus70k", lambda: LS.one_light_scene(scenegen.displaced_torus(175, 200, seed=2, major=1.0, minor=0.45)))
    w, entry_light, base = LR.scene_weights(scene)
    assert len(w) == 70000 and LR.guide_size(len(w)) == 131072
    ctx = _power_ctx(gpu_ctx_factory, scene)
    cdf = _check_table(ctx, w, entry_light, base, "70 000-triangle torus")
    _check_picks(ctx, cdf)


def test_picks_on_one_large_triangle_and_4000_slivers(gpu_ctx_factory):
    """long walks, and most guide slots landing on one entry"""
    scene = _cached("slivers", lambda: LS.one_light_scene(LS.slivers_and_a_slab(4000)))
    w, entry_light, base = LR.scene_weights(scene)
    ctx = _power_ctx(gpu_ctx_factory, scene)
    cdf = _check_table(ctx, w, entry_light, base, "slab and slivers")
    gd = LR.guide(cdf)
    assert np.bincount(gd).max() > 2000, "many guide slots on the large entry"
    _check_picks(ctx, cdf)


def test_table_follows_moved_instances_and_deformed_meshes(gpu_ctx_factory):
    scene = _cached("emitters", LS.emitter_scene)
    ctx = _power_ctx(gpu_ctx_factory, scene)
    w0, entry_light, base = LR.scene_weights(scene)
    _check_table(ctx, w0, entry_light, base, "before")
    # the large panel twice as large again
    moved = capi.mat4_from_trs((1.0, 2.75, -0.5), (0, 0, 0), (6, 6, 6))
    ctx.set_instance_transforms([LS.PANEL_BIG_INSTANCE], [moved])
    instances = scene.instances.copy()
    instances["transform"][LS.PANEL_BIG_INSTANCE] = moved
    w1, _, _ = LR.weights(scene.meshes, instances, scene.materials, scene.lights, scene.emissive_maps)
    assert np.allclose(w1[2:4], 4.0 * w0[2:4]) and np.array_equal(w1[4:], w0[4:])
    _check_table(ctx, w1, entry_light, base, "after nxhip_set_instance_transforms")
    # ... and the torus light deformed (BLAS ids are upload order: the torus is mesh 2)
    bent = LS.light_torus(seed=9, amp=0.2)
    ctx.update_blas(2, bent)
    meshes = list(scene.meshes)
    meshes[2] = bent
    w2, _, _ = LR.weights(meshes, instances, scene.materials, scene.lights, scene.emissive_maps)
    assert not np.allclose(w2[4:196], w1[4:196], rtol=1e-3) and np.array_equal(w2[:4], w1[:4])
    cdf = _check_table(ctx, w2, entry_light, base, "after nxhip_update_blas")
    _check_picks(ctx, cdf)


def test_refusals(gpu_ctx_factory):
    scene = _cached("emitters", LS.emitter_scene)
    ctx = gpu_ctx_factory(64, 48)
    scene.upload(ctx)
    with pytest.raises(capi.NexusError, match="unknown mode"):
        ctx.set_light_sampling(2)
    with pytest.raises(capi.NexusError, match="NXHIP_LIGHTS_POWER"):
        ctx.read_light_table(len(scene.lights))  # (the default mode has no table)
    ctx.set_light_sampling(pod.LIGHTS_POWER)
    for bad in (1.0, np.nan, -0.25, np.inf):
        with pytest.raises(capi.NexusError, match=r"\[0, 1\)"):
            ctx.light_pick_batch(np.array([0.5, bad], np.float32))
    # one instance named twice: refused by the render, accepted again by the default mode
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    twice = np.concatenate([scene.lights, scene.lights[1:2]])
    ctx.set_lights(twice)
    with pytest.raises(capi.NexusError, match="twice"):
        ctx.render_frame()
    ctx.set_light_sampling(pod.LIGHTS_UNIFORM)
    ctx.render_frame()
    ctx.sync()


@pytest.mark.parametrize("case", ["no lights", "lights that emit nothing"])
def test_power_mode_without_anything_to_sample_renders_without_light_samples(gpu_ctx_factory, case):
    scene = LS.emitter_scene()
    if case == "no lights":
        scene.lights = np.zeros(0, pod.LIGHT_DT)
    else:  # the light list stays, the materials stop emitting (the textured one through a zero intensity)
        scene.materials["intensity"] = 0.0
    ctx = gpu_ctx_factory(64, 48)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.set_light_sampling(pod.LIGHTS_POWER)
    ctx.reset_frame_number()
    for _ in range(2):
        ctx.render_frame()
        ctx.accumulate()
    assert np.all(np.isfinite(ctx.read_radiance())) and np.all(np.isfinite(ctx.read_accumulation()))
    assert not np.any(ctx.read_queue_sizes()["traceShadowSize"]), "no light sample, no shadow ray"
    with pytest.raises(capi.NexusError, match="empty" if case == "no lights" else "invalid"):
        ctx.light_pick_batch(np.array([0.5], np.float32))  # (nothing can be picked, and the hook says so)
    if case == "no lights":  # the emitters are still seen by the paths that hit them
        assert ctx.read_accumulation().max() > 0
