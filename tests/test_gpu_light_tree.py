"""The light tree of NXHIP_LIGHT_IMPORTANCE_POSITION on the device (nx_lights.hip, nx_lights.h) against the numpy restatement
(tests/light_tree_reference.py): the tree read back, the descent and the probability lookup bit for bit, the probabilities against
float64, a histogram of picks, the entry points' refusals, and the tree after instances move and meshes deform.

Tolerance of a device probability against the float64 pmf on the same (read-back) nodes: 4 x the worst relative difference the CPU
test of the restatement prints (tests/test_light_tree_reference.py WORST_REL_PROB32_VS_PMF64 = 1.32e-5), i.e. 5.3e-5."""
import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import light_reference as LR
from tests import light_scenes as LS
from tests import light_tree_reference as LT
from tests import light_tree_scenes as LTS
from tests.test_light_tree_reference import WORST_REL_PROB32_VS_PMF64

pytestmark = pytest.mark.gpu

PROB_REL_TOL = 4 * WORST_REL_PROB32_VS_PMF64  # (the figure comes from the CPU test's print, see the docstring)
assert PROB_REL_TOL == 4 * 1.32e-5
PICKS_PER_POINT = 2000


def _dark_light_scene():
    """the emitter scene with the torus light's material emitting nothing: 192 zero-weight leaves"""
    sc = LS.emitter_scene()
    sc.materials["intensity"][3] = 0.0
    return sc


SCENES = {
    "N = 1": lambda: LS.one_light_scene(LTS.tiny_light(1)),
    "N = 2": lambda: LS.one_light_scene(LTS.tiny_light(2)),
    "N = 3": lambda: LS.one_light_scene(LTS.tiny_light(3)),
    "emitter scene": LS.emitter_scene,
    "slivers and a slab": lambda: LS.one_light_scene(LS.slivers_and_a_slab(4000)),
    "a light that emits nothing": _dark_light_scene,
    "clustered panels": LTS.clustered_panels,
}
_CACHE = {}


def _scene(name):
    if name not in _CACHE:
        _CACHE[name] = SCENES[name]()
    return _CACHE[name]


def _tree_ctx(gpu_ctx_factory, scene):
    ctx = gpu_ctx_factory(64, 48)
    scene.upload(ctx)
    ctx.set_light_sampling(pod.LIGHTS_POWER)
    ctx.set_light_importance(pod.LIGHT_IMPORTANCE_POSITION)
    return ctx


def _ulps(a, b):
    """distance in units of the last place of b (binary32)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(b), np.float32(1e-30))).astype(np.float64)


def _read(ctx, meshes, instances, materials, lights, emissive_maps):
    w, _, _ = LR.weights(meshes, instances, materials, lights, emissive_maps)
    corners = LT.corners64(meshes, instances, lights)
    nodes8, order = ctx.read_light_tree()
    return LT.tree_of_nodes8(nodes8), order, w, corners


def _issue_figures(t, order, w, corners):
    """the three figures the feature's issue set bars on: leaf shares against float64 (relative), leaf boxes against the binary32 of the
    float64-transformed corners (ulp), inner w against binary32((Wl + Wr) / Wroot) from the float64 weights (ulp)"""
    N, G = len(w), t.G
    share = LR.shares(w)[order]
    got = t.w[G:G + N].astype(np.float64)
    rel = np.abs(got - share)[share > 0] / share[share > 0]
    lo64, hi64 = LT.boxes64(corners)
    box_ulps = max(_ulps(t.lo[G:G + N], lo64[order].astype(np.float32)).max(), _ulps(t.hi[G:G + N], hi64[order].astype(np.float32)).max())
    ref = LT.tree_from(order, (lo64, hi64), w)
    inner_ulps = _ulps(t.w[1:G], ref.w[1:G]).max() if G > 1 else 0.0
    return (rel.max() if rel.size else 0.0), box_ulps, inner_ulps


def _check_tree(ctx, meshes, instances, materials, lights, emissive_maps, what):
    """every check on the tree read back; returns (Tree of the device's nodes, w float64[N], corners float64[N, 3, 3]).
    Bars against float64 geometry: a leaf's share 4e-7 relative, a leaf's box 2 ulp, an inner w 1 ulp (and, against its children's stored
    values, 1.5 ulp: its own rounding and half an ulp of each child, whose ulps are no larger than its own); inner boxes exactly."""
    t, order, w, corners = _read(ctx, meshes, instances, materials, lights, emissive_maps)
    N, G = len(w), t.G
    assert G == LT.leaves_for(N) and len(order) == N, what
    assert np.array_equal(np.sort(order), np.arange(N)), "%s: order is a permutation" % what
    assert np.array_equal(t.entry[G:G + N], order) and np.all(t.entry[1:G] == 0), what
    # padded slots are empty
    assert np.all(t.w[G + N:] == 0) and np.all(t.lo[G + N:] == np.inf) and np.all(t.hi[G + N:] == -np.inf) and np.all(t.entry[G + N:] == LT.NO_ENTRY), what
    rel, box_ulps, inner_ulps = _issue_figures(t, order, w, corners)
    print("%s: N = %d, G = %d; leaf shares: max relative error %.3g; leaf boxes: %.2f ulp; inner w: %.2f ulp" % (what, N, G, rel, box_ulps, inner_ulps))
    share = LR.shares(w)[order]
    assert np.all(t.w[G:G + N][share == 0] == 0), what
    assert rel <= 4e-7 and box_ulps <= 2 and inner_ulps <= 1, what
    if G > 1:
        k = np.arange(1, G)
        assert np.array_equal(t.lo[k], np.minimum(t.lo[2 * k], t.lo[2 * k + 1])) and np.array_equal(t.hi[k], np.maximum(t.hi[2 * k], t.hi[2 * k + 1])), "%s: inner boxes exactly" % what
        kids = t.w[2 * k].astype(np.float64) + t.w[2 * k + 1].astype(np.float64)
        assert np.all(np.abs(t.w[k].astype(np.float64) - kids) <= 1.5 * np.spacing(t.w[k])), "%s: an inner w against its children's" % what
    assert t.w[1] == 1, what
    return t, w, corners


def _points(t, corners, seed):
    """a point near a light, a leaf's centre (d2 = 0), one at 1e3, one at 1e20, and 64 seeded points in the scene's bounds"""
    rng = np.random.RandomState(seed)
    lo, hi = corners.reshape(-1, 3).min(axis=0) - 1.0, corners.reshape(-1, 3).max(axis=0) + 1.0
    near = corners[0].mean(axis=0) + (0.3, -0.4, 0.2)
    mid = 0.5 * (t.lo[t.G].astype(np.float64) + t.hi[t.G].astype(np.float64))
    named = np.array([near, mid, (1e3, -1e3, 1e3), (1e20, 1e20, -1e20)])
    return np.concatenate([named, rng.uniform(lo, hi, (64, 3))]).astype(np.float32)


def _check_picks(ctx, t, w, corners, what, seed=3):
    N = len(w)
    pts = _points(t, corners, seed)
    rng = np.random.RandomState(seed + 1)
    u = np.concatenate([(rng.randint(0, 1 << 23, (len(pts), PICKS_PER_POINT - 2)) / float(1 << 23)).astype(np.float32),
                        np.zeros((len(pts), 1), np.float32), np.full((len(pts), 1), LT.U_MAX, np.float32)], axis=1)
    P = np.repeat(pts, PICKS_PER_POINT, axis=0)
    entry, prob = ctx.light_tree_pick_batch(P, u.reshape(-1))
    want_entry, want_prob = LT.replay32(t, P, u.reshape(-1))
    assert np.array_equal(entry, want_entry), "%s: entries against the replay" % what
    assert np.array_equal(prob.view(np.uint32), want_prob.view(np.uint32)), "%s: probabilities against the replay, bit for bit" % what
    far = np.repeat(np.arange(len(pts)) == 3, PICKS_PER_POINT)
    if t.G == 1:  # the rule's own exception: the root is the leaf, nothing is descended, P = 1 wherever the point is (the density then fails pdf_valid)
        assert np.all(entry == 0) and np.all(prob == 1)
        far[:] = False
    assert np.all(entry[far] == LT.NO_ENTRY) and np.all(prob[far] == 0), "%s: the point at 1e20 has no sample" % what
    assert np.all(entry[~far] != LT.NO_ENTRY) and np.all(w[entry[~far]] > 0) and np.all(prob[~far] > 0), "%s: a zero-weight entry is never picked" % what
    again = ctx.light_tree_prob_batch(P[~far], entry[~far])
    assert np.array_equal(again.view(np.uint32), prob[~far].view(np.uint32)), "%s: the lookup equals the pick's probability bit for bit" % what
    # all entries at 8 points
    worst_rel, worst_sum = 0.0, 0.0
    for p in np.concatenate([pts[:3], pts[4:9]]):
        got = ctx.light_tree_prob_batch(np.repeat(p[None], N, axis=0), np.arange(N, dtype=np.uint32)).astype(np.float64)
        pmf = LT.pmf64(t, p)[LT.slot_of(t, N)]
        assert np.all(got[w == 0] == 0), "%s: a zero-weight entry has probability 0" % what
        worst_rel = max(worst_rel, (np.abs(got - pmf)[pmf > 0] / pmf[pmf > 0]).max())
        assert np.all(got[pmf == 0] == 0), what
        worst_sum = max(worst_sum, abs(got.sum() - 1.0))
    print("%s: %d picks equal the replay; over all entries at 8 points: worst relative |P - pmf64| %.3g (bar %.3g), worst |sum - 1| %.3g (bar 1e-6)" % (
        what, len(entry), worst_rel, PROB_REL_TOL, worst_sum))
    assert worst_rel <= PROB_REL_TOL, what
    assert worst_sum <= 1e-6, what


@pytest.mark.parametrize("name", list(SCENES))
def test_tree_and_picks(gpu_ctx_factory, name):
    scene = _scene(name)
    ctx = _tree_ctx(gpu_ctx_factory, scene)
    t, w, corners = _check_tree(ctx, scene.meshes, scene.instances, scene.materials, scene.lights, scene.emissive_maps, name)
    if name == "a light that emits nothing":
        assert (w == 0).sum() == 192
    if name == "clustered panels":
        slot = LT.slot_of(t, len(w)).reshape(LTS.GROUPS, -1)
        for g in range(LTS.GROUPS):
            assert slot[g].max() - slot[g].min() == slot.shape[1] - 1, "group %d occupies one contiguous range of slots" % g
    _check_picks(ctx, t, w, corners, name)


@pytest.mark.parametrize("name", list(SCENES))
def test_tree_values_at_the_bars_the_issue_set(gpu_ctx_factory, name):
    """The three bars on values that pass through geometry, against float64: every leaf's share within 4e-7 relative (binary32 rounding of
    a share, with margin), leaf boxes within 2 ulp of the binary32 of the float64-transformed corners, every inner w within 1 ulp of
    binary32((Wl + Wr) / Wroot) from the float64 weights.  The build meets them because it forms corners, areas and luminances in
    binary64 from the binary32 inputs (nx_lights.hip light_tree_leaf_kernel); a build from the light sample's binary32 mat_point and
    tri_area values measured 8.3e-7 / 42 ulp / 6 ulp on the emitter scene (a rotated light) and 1.5e-5 / 240 ulp on the clustered panels."""
    scene = _scene(name)
    ctx = _tree_ctx(gpu_ctx_factory, scene)
    rel, box_ulps, inner_ulps = _issue_figures(*_read(ctx, scene.meshes, scene.instances, scene.materials, scene.lights, scene.emissive_maps))
    print("%s: leaf shares %.3g (bar 4e-7), leaf boxes %.2f ulp (bar 2), inner w %.2f ulp (bar 1)" % (name, rel, box_ulps, inner_ulps))
    assert rel <= 4e-7
    assert box_ulps <= 2
    assert inner_ulps <= 1


def test_two_contexts_hold_the_same_tree(gpu_ctx_factory):
    scene = _scene("slivers and a slab")
    a, b = (_tree_ctx(gpu_ctx_factory, scene).read_light_tree() for _ in range(2))
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def test_histogram_of_picks(gpu_ctx_factory):
    """200 000 picks at one point of the clustered panels against pmf64, cells of expectation >= 20: (chi2 - dof) / sqrt(2 dof) < 5"""
    scene = _scene("clustered panels")
    ctx = _tree_ctx(gpu_ctx_factory, scene)
    nodes8, order = ctx.read_light_tree()
    t = LT.tree_of_nodes8(nodes8)
    N, n = len(order), 200000
    p = np.array((2.0, 1.0, 1.0), np.float32)
    u = (np.random.RandomState(17).randint(0, 1 << 23, n) / float(1 << 23)).astype(np.float32)
    entry, _ = ctx.light_tree_pick_batch(np.repeat(p[None], n, axis=0), u)
    expect = LT.pmf64(t, p)[:N] * n  # by slot
    seen = np.bincount(LT.slot_of(t, N)[entry], minlength=N).astype(np.float64)
    cells_e, cells_s, e_acc, s_acc = [], [], 0.0, 0.0
    for e, s in zip(expect, seen):  # neighbouring slots merged until a cell expects 20
        e_acc += e
        s_acc += s
        if e_acc >= 20:
            cells_e.append(e_acc)
            cells_s.append(s_acc)
            e_acc = s_acc = 0.0
    if e_acc > 0:
        cells_e[-1] += e_acc
        cells_s[-1] += s_acc
    cells_e, cells_s = np.array(cells_e), np.array(cells_s)
    dof = len(cells_e) - 1
    chi2 = ((cells_s - cells_e) ** 2 / cells_e).sum()
    z = (chi2 - dof) / np.sqrt(2 * dof)
    print("histogram: %d cells, chi2 %.1f, (chi2 - dof) / sqrt(2 dof) = %.2f (bar 5); the nearest group's share %.4f" % (len(cells_e), chi2, z, expect.max() / n))
    assert dof >= 8 and z < 5


def test_refusals(gpu_ctx_factory):
    scene = _scene("emitter scene")
    ctx = gpu_ctx_factory(64, 48)
    scene.upload(ctx)
    with pytest.raises(capi.NexusError, match="unknown importance"):
        ctx.set_light_importance(2)
    p, u, e = np.zeros((1, 3), np.float32), np.array([0.5], np.float32), np.zeros(1, np.uint32)
    hooks = (lambda: ctx.read_light_tree(), lambda: ctx.light_tree_pick_batch(p, u), lambda: ctx.light_tree_prob_batch(p, e))
    for mode, importance in ((pod.LIGHTS_UNIFORM, pod.LIGHT_IMPORTANCE_POWER), (pod.LIGHTS_UNIFORM, pod.LIGHT_IMPORTANCE_POSITION), (pod.LIGHTS_POWER, pod.LIGHT_IMPORTANCE_POWER)):
        ctx.set_light_sampling(mode)
        ctx.set_light_importance(importance)
        for hook in hooks:
            with pytest.raises(capi.NexusError, match="NXHIP_LIGHT_IMPORTANCE_POSITION"):
                hook()
    ctx.set_light_importance(pod.LIGHT_IMPORTANCE_POSITION)
    _, order = ctx.read_light_tree()
    N = len(order)
    for bad in (np.nan, np.inf):
        with pytest.raises(capi.NexusError, match="not finite"):
            ctx.light_tree_pick_batch(np.array([(0, 0, 0), (0, bad, 0)], np.float32), np.array([0.5, 0.5], np.float32))
        with pytest.raises(capi.NexusError, match="not finite"):
            ctx.light_tree_prob_batch(np.array([(0, 0, 0), (0, bad, 0)], np.float32), np.zeros(2, np.uint32))
    for bad in (1.0, np.nan, -0.25):
        with pytest.raises(capi.NexusError, match=r"\[0, 1\)"):
            ctx.light_tree_pick_batch(np.zeros((2, 3), np.float32), np.array([0.5, bad], np.float32))
    with pytest.raises(capi.NexusError, match="no such entry"):
        ctx.light_tree_prob_batch(np.zeros((2, 3), np.float32), np.array([0, N], np.uint32))
    assert ctx.light_tree_prob_batch(np.zeros((1, 3), np.float32), np.array([N - 1], np.uint32))[0] > 0


@pytest.mark.parametrize("case", ["no lights", "lights that emit nothing"])
def test_nothing_to_sample(gpu_ctx_factory, case):
    scene = LS.emitter_scene()
    if case == "no lights":
        scene.lights = np.zeros(0, pod.LIGHT_DT)
    else:
        scene.materials["intensity"] = 0.0
    ctx = gpu_ctx_factory(64, 48)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.set_light_sampling(pod.LIGHTS_POWER)
    ctx.set_light_importance(pod.LIGHT_IMPORTANCE_POSITION)
    ctx.reset_frame_number()
    for _ in range(2):
        ctx.render_frame()
        ctx.accumulate()
    assert np.all(np.isfinite(ctx.read_radiance())) and np.all(np.isfinite(ctx.read_accumulation()))
    assert not np.any(ctx.read_queue_sizes()["traceShadowSize"]), "no light sample, no shadow ray"
    for hook in (lambda: ctx.light_tree_pick_batch(np.zeros((1, 3), np.float32), np.array([0.5], np.float32)),
                 lambda: ctx.light_tree_prob_batch(np.zeros((1, 3), np.float32), np.zeros(1, np.uint32))):
        with pytest.raises(capi.NexusError, match=("empty|no such entry") if case == "no lights" else "invalid"):
            hook()
    if case == "lights that emit nothing":
        nodes8, _ = ctx.read_light_tree()
        assert np.all(nodes8[:, 3] == 0), "every w is 0"


def test_tree_follows_moved_instances_and_deformed_meshes(gpu_ctx_factory):
    scene = _scene("emitter scene")
    ctx = _tree_ctx(gpu_ctx_factory, scene)
    _check_tree(ctx, scene.meshes, scene.instances, scene.materials, scene.lights, scene.emissive_maps, "before")
    moved = capi.mat4_from_trs((-2.0, 3.25, 1.5), (0, 0, 0), (6, 6, 6))  # the large panel moved, and twice as large again
    ctx.set_instance_transforms([LS.PANEL_BIG_INSTANCE], [moved])
    instances = scene.instances.copy()
    instances["transform"][LS.PANEL_BIG_INSTANCE] = moved
    _check_tree(ctx, scene.meshes, instances, scene.materials, scene.lights, scene.emissive_maps, "after nxhip_set_instance_transforms")
    bent = LS.light_torus(seed=9, amp=0.2)
    ctx.update_blas(2, bent)
    meshes = list(scene.meshes)
    meshes[2] = bent
    t, w, corners = _check_tree(ctx, meshes, instances, scene.materials, scene.lights, scene.emissive_maps, "after nxhip_update_blas")
    _check_picks(ctx, t, w, corners, "after nxhip_update_blas", seed=8)
