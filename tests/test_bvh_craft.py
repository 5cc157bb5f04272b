"""The hand-made trees of tests/bvh_craft.py, on the CPU: the encoder writes the boxes and ranges it was asked for, the oracle's
traversal of the chains finds what brute force finds, and every ray reaches exactly the stack depth the GPU tests
(tests/test_gpu_deep_stack.py) build on — the same scenes and the same rays."""
import numpy as np
import pytest

from nexus_amd import pod
from tests import bvh_craft as BC
from tests import oracle_lib as O
from tests.test_builder_parity import _decode_children
from tests.test_tlas_refit import _check_tlas_structure


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("D,per_level,deep,first,fine", [(1, 1, -1, 0, True), (2, 1, -1, 0, True), (10, 1, -1, 0, True), (10, 2, 1, 0, True), (33, 1, -1, 0, True),
                                                        (40, 3, -1, 0, True), (13, 1, 1, 200, False), (63, 1, -1, 0, True), (26, 1, -1, 229, False)])
def test_chain_blas_decodes_to_what_was_asked_for(D, per_level, deep, first, fine):
    nodes, tris, idx = BC.chain_blas(D, seed=D, per_level=per_level, deep=deep, first_level=first, fine=fine)
    assert len(nodes) == 2 * D - 1 and len(tris) == D * per_level and idx.tolist() == list(range(len(tris)))
    tmin = np.minimum(np.minimum(tris["pos0"], tris["pos1"]), tris["pos2"]).astype(np.float64)
    tmax = np.maximum(np.maximum(tris["pos0"], tris["pos1"]), tris["pos2"]).astype(np.float64)
    seen_nodes, seen_tris = set(), set()
    at = 0
    for i in range(D):
        assert at not in seen_nodes
        seen_nodes.add(at)
        kids = _decode_children(nodes[at])
        if i == D - 1:
            assert [(k[0], k[1], k[4], k[5]) for k in kids] == [(0, "leaf", i * per_level, per_level)]
            leaf_of = kids[0]
        else:
            assert [k[1] for k in kids] == ["inner", "inner"] and [k[0] for k in kids] == [0, 1]
            assert [k[4] for k in kids] == [2 * i + 1, 2 * i + 2], "inner children are consecutive and follow their parent"
            stub, rest = (kids[0], kids[1]) if deep < 0 else (kids[1], kids[0])
            assert np.array_equal(stub[2], [-1, -1, (first + i) / 32]) and np.array_equal(stub[3], [1, 1, (first + i + 1) / 32])
            assert np.array_equal(rest[2], [-1, -1, (first + i + 1) / 32]) and np.array_equal(rest[3], [1, 1, (first + D) / 32])
            seen_nodes.add(stub[4])
            (leaf_of,) = _decode_children(nodes[stub[4]])
            at = rest[4]
        s, kind, lo, hi, first_prim, count = leaf_of
        assert (s, kind, first_prim, count) == (0, "leaf", i * per_level, per_level)
        assert np.array_equal(lo, [-1, -1, (first + i) / 32]) and np.array_equal(hi, [1, 1, (first + i + 1) / 32])
        for k in range(first_prim, first_prim + count):
            seen_tris.add(k)
            assert np.all(lo <= tmin[idx[k]]) and np.all(tmax[idx[k]] <= hi), "triangle %d inside its slab" % k
    assert len(seen_nodes) == len(nodes) and len(seen_tris) == len(tris)


def test_encoder_quantises_outwards_and_refuses_what_does_not_fit():
    n = BC.encode_node((0.0, 0.0, 0.0), (124, 124, 124), [None, ("leaf", 2, 3, (0.13, 0.26, 0.0), (1.01, 1.0, 31.875)), None, ("inner", (0.0, 0.0, 0.0), (0.125, 0.25, 0.5))],
                       child_base=7, prim_base=40)
    kids = _decode_children(n)
    assert [(k[0], k[1], k[4], k[5]) for k in kids] == [(1, "leaf", 42, 3), (3, "inner", 7, 1)]
    assert np.array_equal(kids[0][2], [0.125, 0.25, 0.0]) and np.array_equal(kids[0][3], [1.125, 1.0, 31.875])
    assert np.array_equal(kids[1][2], [0, 0, 0]) and np.array_equal(kids[1][3], [0.125, 0.25, 0.5])
    assert int(n["imask"]) == 8 and n["meta"].tolist() == [0, 0xE2, 0, 0x20 | 27, 0, 0, 0, 0]
    with pytest.raises(AssertionError):
        BC.encode_node((0.0, 0.0, 0.0), (124, 124, 124), [("inner", (0, 0, 0), (1, 1, 32.0))])
    with pytest.raises(AssertionError):
        BC.encode_node((0.0, 0.0, 0.0), (124, 124, 124), [("leaf", 22, 3, (0, 0, 0), (1, 1, 1))])


@pytest.mark.parametrize("name", list(BC.TOWERS))
@pytest.mark.parametrize("mixed", [False, True])
def test_chain_tlas_is_a_valid_tree_over_its_instances(name, mixed):
    scene, _rays = BC.tower_case(name, mixed)
    T, last, _D = BC.TOWERS[name]
    assert len(scene.tlas_nodes) == 2 * T - 1 and len(scene.instances) == T - 1 + last
    _check_tlas_structure(scene.tlas_nodes, scene.tlas_idx, scene.instances, built=False)
    identity = [np.array_equal(np.asarray(i["invTransform"]).reshape(4, 4), np.eye(4, dtype=np.float32)) for i in scene.instances]
    assert all(identity) if not mixed else (any(identity) and not all(identity))


def _classes(scene, rays):
    """(going down, going up, beside the scene) of BC.mixed_rays"""
    beside = rays["origin"][:, 0] > scene.instances["boundsMax"][:, 0].max() + 1.0
    down = (rays["direction"][:, 2] < 0) & ~beside
    return down, ~down & ~beside, beside


@pytest.mark.parametrize("D", (4,) + BC.CHAIN_LEVELS + (31,) + BC.LIMIT_LEVELS)
def test_every_ray_of_a_chain_reaches_exactly_the_named_depth(D):
    """the table of measured depths: D levels -> maxStack D - 1 for every ray that goes down, 1 going up, 0 beside the scene"""
    scene, rays = BC.limit_case(D) if D in BC.LIMIT_LEVELS else BC.chain_case(D)
    orc = scene.oracle()
    depth = BC.per_ray_stack(orc, rays)
    down, up, beside = _classes(scene, rays)
    print("D = %d: maxStack of the rays going down %s, going up %s, beside %s" % (D, np.unique(depth[down]).tolist(), np.unique(depth[up]).tolist(), np.unique(depth[beside]).tolist()))
    assert down.mean() >= 0.45 and up.mean() >= 0.25 and beside.mean() >= 0.15
    assert np.all(depth[down] == D - 1) and np.all(depth[up] == (1 if D > 1 else 0)) and np.all(depth[beside] == 0)
    st = O.TraceStats()
    want = orc.trace_closest(rays, st)
    assert st.maxStack == D - 1
    bf = orc.brute_closest(rays)
    assert np.array_equal(_bits(want["hitDistance"]), _bits(bf["hitDistance"])), "oracle traversal against brute force"
    assert np.array_equal(want["triIdx"], bf["triIdx"]), "every level's triangle is its own: no ties"
    assert (want["hitDistance"][down] < 1e29).mean() > 0.9 and np.all(want["hitDistance"][beside] > 1e29)
    # the triangle a deep ray ends on tells which popped entry was read: level i's stub is the entry at stack position i
    popped_far = down & (want["triIdx"] >= 8) & (want["triIdx"] < D - 1)
    if D >= 10:
        assert popped_far.sum() >= 0.25 * down.sum()
    # any hit: a limit at the hit culls the boxes behind it; a limit beyond the scene leaves the depth as it is (the first triangle
    # is tested at the bottom of the chain)
    tmax = BC.shadow_tmax(want, seed=D)
    sub = slice(0, 4000)
    any_depth = BC.per_ray_stack(orc, rays[sub], tmax[sub])
    far = down[sub] & (tmax[sub] == 10.0)
    assert far.sum() > 500 and np.all(any_depth[far] == D - 1) and np.all(any_depth <= D - 1)
    assert np.array_equal(orc.trace_any(rays, tmax), orc.brute_any(rays, tmax))


def test_twin_triangles_and_the_other_slot_order():
    """coincident copies (what sends the thin kernel's search to its in-order replay): same distances as brute force, same depths;
    deep = +1: the rays going UP are the deep ones"""
    scene, rays = BC.chain_case(20, per_level=2)
    orc = scene.oracle()
    down, up, _ = _classes(scene, rays)
    depth = BC.per_ray_stack(orc, rays)
    assert np.all(depth[down] == 19) and np.all(depth[up] == 1)
    want, bf = orc.trace_closest(rays), orc.brute_closest(rays)
    assert np.array_equal(_bits(want["hitDistance"]), _bits(bf["hitDistance"]))
    assert np.array_equal(want["triIdx"] // 2, bf["triIdx"] // 2)
    flipped = BC.chain_scene(20, seed=3, deep=+1)
    rays = BC.mixed_rays(flipped, 4000, seed=9)
    down, up, _ = _classes(flipped, rays)
    depth = BC.per_ray_stack(flipped.oracle(), rays)
    assert np.all(depth[up] == 19) and np.all(depth[down] == 1)
    assert np.array_equal(_bits(flipped.oracle().trace_closest(rays)["hitDistance"]), _bits(flipped.oracle().brute_closest(rays)["hitDistance"]))


@pytest.mark.parametrize("name", list(BC.TOWERS))
@pytest.mark.parametrize("mixed", [False, True])
def test_towers_take_the_rays_going_down_to_31_and_32_entries(name, mixed):
    scene, rays = BC.tower_case(name, mixed)
    orc = scene.oracle()
    depth = BC.per_ray_stack(orc, rays)
    down, up, beside = _classes(scene, rays)
    print("%s, mixed %s: maxStack histogram of the rays going down %s" % (name, mixed, np.bincount(depth[down]).tolist()))
    assert depth.max() == 32 and (depth == 32).mean() >= 0.45 and np.all(depth[down] >= 31)
    assert np.all(depth[up] <= 2) and np.all(depth[beside] == 0) and (depth <= 2).mean() >= 0.45
    want, bf = orc.trace_closest(rays), orc.brute_closest(rays)
    assert np.array_equal(_bits(want["hitDistance"]), _bits(bf["hitDistance"]))
    hit = want["triIdx"] != 0xffffffff
    assert len(np.unique(want["instanceIdx"][hit])) == len(scene.instances), "every instance is somebody's closest hit"
    tmax = BC.shadow_tmax(want, seed=1)
    assert np.array_equal(orc.trace_any(rays, tmax), orc.brute_any(rays, tmax))


def test_without_levels_removes_the_stubs_from_the_named_level_on_only():
    scene, rays = BC.limit_case(40)
    cut = BC.without_levels(scene, 32)
    want, got = scene.oracle().trace_closest(rays), cut.oracle().trace_closest(rays)
    assert not np.any((got["triIdx"] >= 32) & (got["triIdx"] < 39))
    gone = (want["triIdx"] >= 32) & (want["triIdx"] < 39)
    assert gone.sum() > 1000 and np.array_equal(got[~gone], want[~gone])
    assert np.array_equal(scene.blas[0][1], BC.limit_case(40)[0].blas[0][1]), "the cached scene is left as it was"


@pytest.mark.parametrize("mixed", [False, True])
def test_frame_scene_reaches_the_limit_with_primary_and_shadow_rays(mixed):
    W, H = 64, 48
    scene = BC.frame_scene(W, H, mixed)
    w = O.Wavefront(scene.oracle(), W * H, None, pod.RNG_PIXEL_KEYED, pod.CONDUCTOR_REFERENCE)
    w.render(1, threads=4)
    closest, shadow = w.trace_stats()
    q = w.queue_sizes()
    print("closest-hit maxStack %d over %d rays, any-hit maxStack %d over %d rays" % (closest["maxStack"], closest["rays"], shadow["maxStack"], shadow["rays"]))
    assert 24 <= closest["maxStack"] <= 32 and 9 <= shadow["maxStack"] <= 32
    assert q["traceSize"][1] > 1000 and q["traceSize"][2] > 100 and shadow["rays"] > 100
    assert float(w.radiance().mean()) > 0.05
    w.close()
