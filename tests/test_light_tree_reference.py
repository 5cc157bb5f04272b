"""The light tree's numpy restatement (tests/light_tree_reference.py) proves itself, and the library carries the entry points of
nxhip_set_light_importance: no GPU needed.

What the GPU tests take from here: WORST_REL_PROB32_VS_PMF64, the largest relative difference between the binary32 probability lookup
and the float64 probabilities that this file prints (and bounds), is the yardstick of the device tolerance in tests/test_gpu_light_tree.py."""
import ctypes

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import light_reference as LR
from tests import light_scenes as LS
from tests import light_tree_reference as LT

# Printed by test_reference_proves_itself below: 7.0e-7 (slivers) and 1.32e-5 (clusters, at the points inside a cluster).
# The bound asserted here is reasoned, not measured: a leaf's probability is a product of `depth` factors a / (a + b); each factor
# carries the roundings of two importances (about twelve operations each, 2^-24 apiece) and of one addition and one division,
# (2 x 12 + 2) x 2^-24 per level, 12 levels at G = 4 096: 312 x 2^-24 = 1.9e-5.  On top of that comes the cancellation in d = p - c where
# a point lies near a box centre: coordinates up to 64 and distances down to about 0.25 amplify the rounding of c by up to 256, twice
# in d2: 512 x 2^-24 = 3.1e-5 for each of the (at most two) levels whose boxes are that near.  Together below 1e-4.
WORST_REL_PROB32_VS_PMF64 = 1.32e-5
REASONED_REL_BOUND = 1e-4


def test_library_exports_the_entry_points():
    L = capi.lib()
    for name in ("nxhip_set_light_importance", "nxhip_read_light_tree", "nxhip_light_tree_pick_batch", "nxhip_light_tree_prob_batch", "nxhip_light_tree_leaves_for",
                 "nxs_pathtracer_set_light_importance"):
        assert hasattr(L, name) and name in capi.SIGNATURES, name
    assert capi.SIGNATURES["nxhip_light_tree_leaves_for"][0] is ctypes.c_uint32
    assert (pod.LIGHT_IMPORTANCE_POWER, pod.LIGHT_IMPORTANCE_POSITION) == (0, 1)
    for method in ("set_light_importance", "read_light_tree", "light_tree_pick_batch", "light_tree_prob_batch"):
        assert callable(getattr(capi.Context, method)), method


def test_leaves_for():
    L = capi.lib()
    asked = [0, 1, 2, 3, 4001, 1 << 23, (1 << 23) + 1]
    want = [0, 1, 2, 4, 4096, 1 << 23, 0]
    assert [int(L.nxhip_light_tree_leaves_for(n)) for n in asked] == want
    assert [LT.leaves_for(n) for n in asked] == want


def _slivers():
    scene = LS.one_light_scene(LS.slivers_and_a_slab(4000))
    w, _, _ = LR.scene_weights(scene)
    corners = LT.corners64(scene.meshes, scene.instances, scene.lights)
    assert len(w) == 4001 and len(corners) == 4001
    inside = np.array([(6.0, 0.5, 1.0), (1.0, 0.25, 1.0), (7.5, 0.0, 3.0)])
    return corners, w, inside


def _clusters():
    corners, w, centres = LT.five_clusters()
    assert len(w) == 1500
    return corners, w, centres + np.array([(0.3, -0.2, 0.1)])


def _points(tree, inside):
    mid = 0.5 * (tree.lo[tree.G].astype(np.float64) + tree.hi[tree.G].astype(np.float64))  # a leaf's centre: d2 = 0 there
    return [("inside %d" % i, p) for i, p in enumerate(inside)] + [("on a leaf's centre", mid), ("at 1e3", np.array((1e3, -1e3, 1e3))), ("at 1e20", np.array((1e20, 1e20, -1e20)))]


@pytest.mark.parametrize("name", ["slivers and a slab", "five clusters"])
def test_reference_proves_itself(name):
    corners, w, inside = _slivers() if name == "slivers and a slab" else _clusters()
    order = LT.morton_order(corners)
    assert np.array_equal(np.sort(order), np.arange(len(w)))
    tree = LT.tree_from(order, LT.boxes64(corners), w)
    N, G = len(w), tree.G
    assert G == LT.leaves_for(N) and np.all(tree.w[G + N:] == 0) and np.all(np.isinf(tree.lo[G + N:]))
    assert np.all(tree.lo[1] == tree.lo[G:G + N].min(axis=0)) and np.all(tree.hi[1] == tree.hi[G:G + N].max(axis=0)) and tree.w[1] == 1
    assert abs(tree.W[1] - w.sum()) <= 1e-12 * w.sum()
    slots = np.arange(N)
    rng = np.random.RandomState(5)
    worst = 0.0
    for what, p in _points(tree, inside):
        p32 = np.asarray(p, np.float32)
        pmf = LT.pmf64(tree, p32)
        u = np.concatenate([(rng.randint(0, 1 << 23, 2498) / float(1 << 23)).astype(np.float32), np.array([0.0, LT.U_MAX], np.float32)])
        entry, P = LT.replay32(tree, p32, u)
        if what == "at 1e20":  # d2 overflows: every importance is 0, no sample, every probability 0
            assert np.all(pmf == 0) and np.all(entry == LT.NO_ENTRY) and np.all(P == 0)
            assert np.all(LT.prob32(tree, p32, slots) == 0)
            continue
        assert abs(pmf.sum() - 1.0) <= 1e-12, what
        assert np.all(entry != LT.NO_ENTRY) and np.all(P > 0), what
        slot = LT.slot_of(tree, N)[entry]
        assert np.array_equal(LT.prob32(tree, p32, slot).view(np.uint32), P.view(np.uint32)), what  # bit for bit
        assert np.all(w[entry] > 0), what
        P_all = LT.prob32(tree, p32, slots).astype(np.float64)
        assert abs(P_all.sum() - 1.0) <= 5e-8 * 4, what  # (binary32 products: 5e-8 in the prototype, a factor 4 of margin)
        rel = np.abs(P_all - pmf[:N])[pmf[:N] > 0] / pmf[:N][pmf[:N] > 0]
        worst = max(worst, rel.max())
        # the descent lands where u says: the picked slot's cumulative range in the float64 pmf holds u, up to the roundings
        cum = np.cumsum(pmf)
        assert np.all(np.abs(np.clip(u.astype(np.float64), cum[slot] - pmf[slot], cum[slot]) - u) <= 1e-4), what
        print("%s, %s: sum of prob32 - 1 = %.2g, worst relative |prob32 - pmf64| = %.3g" % (name, what, P_all.sum() - 1.0, rel.max()))
    print("%s: WORST relative |prob32 - pmf64| over the points = %.3g (in the file: %.3g; reasoned bound %.3g)" % (name, worst, WORST_REL_PROB32_VS_PMF64, REASONED_REL_BOUND))
    assert worst <= REASONED_REL_BOUND


def test_u_extremes_reach_the_first_and_the_last_reachable_slot():
    corners, w, inside = _clusters()
    w = w.copy()
    w[::7] = 0.0  # zero-weight entries are never picked
    tree = LT.tree_from(LT.morton_order(corners), LT.boxes64(corners), w)
    p = np.asarray(inside[2], np.float32)
    u = np.concatenate([np.array([0.0, LT.U_MAX], np.float32), np.linspace(0, 1, 4001, dtype=np.float32)[:-1]])
    entry, P = LT.replay32(tree, p, u)
    assert np.all(w[entry] > 0) and np.all(P > 0)
    pmf = LT.pmf64(tree, p)
    reachable = np.flatnonzero(pmf > 0)
    slot = LT.slot_of(tree, len(w))[entry]
    assert slot[0] == reachable[0] and slot[1] == reachable[-1]
    assert np.all(np.diff(slot[2:]) >= 0), "the descent is monotone in u"
