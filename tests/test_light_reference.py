"""The numpy restatement of the light table (tests/light_reference.py) checked against its own definition: the guided walk is
searchsorted, the probabilities sum to one, an entry without weight is never picked."""
import numpy as np

from tests import light_reference as LR


def _small_table():
    # 11 entries: zeros at the front, in the middle and at the end, a dominant entry, a sliver
    w = np.array([0.0, 3.0, 0.0, 0.0, 1e-3, 40.0, 2.5, 0.0, 7.0, 1.25, 0.0])
    return w, LR.table(w)


def test_guided_walk_is_searchsorted_on_every_random_number_of_a_small_table():
    w, cdf = _small_table()
    gd = LR.guide(cdf)
    assert len(gd) == 16
    u = (np.arange(1 << 23, dtype=np.float64) / (1 << 23)).astype(np.float32)  # every value rng_next can return
    got, steps = LR.guided_pick(cdf, gd, u)
    want = LR.pick(cdf, u)
    assert np.array_equal(got, want)
    assert not np.any(w[got] == 0.0), "an entry without weight was picked"
    print("small table: mean steps %.3f, max %d" % (steps.mean(), steps.max()))
    # every entry with weight is reached, with the frequency its binary32 probability says (u is an exact grid: counts are exact)
    P = LR.probabilities(cdf)
    counts = np.bincount(got, minlength=len(cdf))
    assert np.array_equal(counts > 0, P > 0)
    assert np.abs(counts / float(1 << 23) - P.astype(np.float64)).max() <= 2.0 ** -23


def test_guided_walk_is_searchsorted_on_a_70000_entry_table():
    rng = np.random.RandomState(5)
    w = rng.lognormal(0.0, 2.0, 70000)
    w[rng.rand(70000) < 0.1] = 0.0
    cdf = LR.table(w)
    gd = LR.guide(cdf)
    assert len(gd) == 131072
    u = np.concatenate([rng.rand(200000).astype(np.float32), cdf[:-1], np.nextafter(cdf[:-1], np.float32(0)), np.nextafter(cdf[:-1], np.float32(2)),
                        np.array([0.0, 1.0 - 2.0 ** -23], np.float32)])
    u = u[(u >= 0) & (u < 1)]
    got, steps = LR.guided_pick(cdf, gd, u)
    assert np.array_equal(got, LR.pick(cdf, u))
    assert not np.any(w[got] == 0.0)
    assert steps[:200000].mean() <= 2.0, "expected steps of the cut-point method"
    print("70 000 entries: mean steps %.3f, max %d" % (steps[:200000].mean(), steps.max()))


def test_probabilities_sum_to_one_and_follow_the_weights():
    for w in (_small_table()[0], np.random.RandomState(2).rand(5000) ** 8):
        cdf = LR.table(w)
        P = LR.probabilities(cdf)
        assert np.all(np.diff(cdf) >= 0) and cdf[-1] == np.float32(1.0)
        assert abs(P.astype(np.float64).sum() - 1.0) <= len(w) * 2.0 ** -24
        assert np.all(P[w == 0.0] == 0.0)
        p64 = LR.shares(w)
        assert np.all(np.abs(P - p64) <= 2.0 ** -23 + 1e-5 * p64)


def test_a_table_without_weight_is_invalid():
    assert LR.table(np.zeros(7)) is None
    assert LR.table(np.array([1.0, np.inf])) is None


def test_weights_of_a_scaled_instance():
    from nexus_amd import capi, pod, scenegen
    from tests import scene_helpers as SH

    quad = scenegen.quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1))
    mats = np.array([pod.make_material(pod.MAT_DIFFUSE, emissive=(1.0, 0.5, 0.25), intensity=2.0),
                     pod.make_material(pod.MAT_DIFFUSE, emissive=(0.0, 1.0, 0.0), intensity=-1.0)], dtype=pod.MAT_DT)
    sc = SH.BuiltScene([quad], [(0, 0, capi.mat4_from_trs((0, 1, 0), (0, 0, 0), (3, 3, 3))), (0, 1, SH.IDENTITY)], materials=mats)
    sc.lights = np.zeros(2, pod.LIGHT_DT)
    sc.lights["type"] = pod.LIGHT_MESH
    sc.lights["meshId"] = [0, 1]
    w, light, base = LR.scene_weights(sc)
    Y = 2.0 * (0.2126 + 0.7152 * 0.5 + 0.0722 * 0.25)
    assert np.allclose(w[:2], 18.0 * Y, rtol=1e-6) and np.all(w[2:] == 0.0)  # (a negative weight counts as 0)
    assert light.tolist() == [0, 0, 1, 1] and base.tolist() == [0, 2, 4]
