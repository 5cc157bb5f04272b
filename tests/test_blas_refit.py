"""BLAS refit on the host (nxh_bvh8_refit = nexus::BVH8::Refit = collapse::Refit over the triangles' vertex boxes), the byte
reference of nxhip_update_blas: with unchanged triangles it reproduces the builder's bytes; after the mesh deformed — up to 3.5 x the
amplitude, so that it leaves its old root box — every box on the way to a triangle still holds it, and rays through the refitted
tree find what brute force finds."""
import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import deform_meshes as D
from tests import scene_helpers as SH
from tests.test_builder_parity import _decode_children

_BUILT = {}


def _built(m):
    if m not in _BUILT:
        tris = D.base_grid(m)
        _BUILT[m] = (tris,) + capi.bvh8_build(tris, threads=4)
    return _BUILT[m]


@pytest.mark.parametrize("m", D.SIZES)
def test_refit_with_unchanged_triangles_is_the_builders_output(m):
    tris, nodes, idx = _built(m)
    assert len(tris) == 2 * m * m
    again = capi.bvh8_refit(nodes, idx, tris)
    assert again.tobytes() == np.ascontiguousarray(nodes).tobytes()


def _check_boxes_hold(nodes, idx, tris):
    """every vertex inside the dequantised box of its leaf slot and of every ancestor's child slot, in float64; returns the number
    of (slot, triangle) pairs checked"""
    p = np.stack([tris["pos0"], tris["pos1"], tris["pos2"]], axis=1).astype(np.float64)   # [tri, vertex, axis]
    tmin, tmax = p.min(axis=1), p.max(axis=1)
    order = np.asarray(idx, np.int64)
    checked = 0
    seen = np.zeros(len(tris), bool)

    def below(ni):
        """(lo, hi) of all triangles under node ni; asserts the slots' boxes on the way"""
        nonlocal checked
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        for _s, kind, blo, bhi, first, count in _decode_children(nodes[ni]):
            if kind == "inner":
                clo, chi = below(first)
            else:
                t = order[first:first + count]
                assert not seen[t].any()
                seen[t] = True
                clo, chi = tmin[t].min(axis=0), tmax[t].max(axis=0)
                checked += count
            assert np.all(blo <= clo) and np.all(bhi >= chi), (ni, _s, kind, blo - clo, bhi - chi)
            lo, hi = np.minimum(lo, clo), np.maximum(hi, chi)
        return lo, hi

    below(0)
    assert seen.all()
    return checked


@pytest.mark.parametrize("m", D.SIZES)
def test_refitted_boxes_hold_the_deformed_triangles(m):
    tris, nodes, idx = _built(m)
    for shape in range(len(D.SHAPES)):
        moved = D.deformed_grid(m, shape)
        refit = capi.bvh8_refit(nodes, idx, moved)
        for f in ("imask", "childBaseIdx", "triangleBaseIdx", "meta"):  # only frames and quantised boxes change
            assert np.array_equal(refit[f], nodes[f]), f
        assert refit.tobytes() != np.ascontiguousarray(nodes).tobytes()
        assert _check_boxes_hold(refit, idx, moved) == len(tris)
    # the largest deformation leaves the old root frame: the stale tree does NOT hold it (what a stale root copy would miss)
    with pytest.raises(AssertionError):
        _check_boxes_hold(nodes, idx, D.deformed_grid(m))


def test_oracle_through_the_refitted_tree_agrees_with_brute_force():
    m = 40
    tris, nodes, idx = _built(m)
    scene = SH.BuiltScene([tris], [(0, 0, capi.mat4_from_trs((0.1, -0.2, 0.05), (20, 35, 10), (1.2, 0.8, 1.1)))])
    assert scene.blas[0][0].tobytes() == nodes.tobytes()
    after = D.host_deformed(scene, {0: D.deformed_grid(m)})
    rays = D.rays_for(5000, 3)
    got = after.oracle().trace_closest(rays)
    want = after.oracle().brute_closest(rays)
    assert (want["hitDistance"] < pod.MISS_DISTANCE).mean() > 0.2
    assert np.array_equal(got["hitDistance"].view(np.uint32), want["hitDistance"].view(np.uint32))
    assert ((got["triIdx"] == want["triIdx"]).mean()) > 0.999  # (equidistant hits on a shared edge may resolve differently)
    # ... and the stale tree loses hits of the moved mesh
    stale = D.with_blas(scene, [(nodes, D.deformed_grid(m), idx)])
    lost = stale.oracle().trace_closest(rays)
    assert not np.array_equal(lost["hitDistance"].view(np.uint32), want["hitDistance"].view(np.uint32))


def test_refit_of_a_tree_whose_children_precede_their_parents():
    """the device builders need not number children after parents: the same tree renumbered deepest level first (the root stays
    node 0, runs of siblings stay consecutive and in order) gives the same bytes, node for node"""
    m = 40
    tris, nodes, idx = _built(m)
    depth = D.node_depths(nodes)
    assert depth.min() == 0 and depth.max() >= 2
    old_of_new = np.concatenate([[0], [k for d in range(depth.max(), 0, -1) for k in np.flatnonzero(depth == d)]])
    new_of_old = np.empty(len(nodes), np.int64)
    new_of_old[old_of_new] = np.arange(len(nodes))

    def renumbered(src):
        out = src[old_of_new].copy()
        inner = out["imask"] != 0
        out["childBaseIdx"][inner] = new_of_old[out["childBaseIdx"][inner]]
        return out

    shuffled = renumbered(nodes)
    inner = np.flatnonzero(shuffled["imask"] != 0)
    assert np.any(shuffled["childBaseIdx"][inner] < inner), "no child precedes its parent: the renumbering tests nothing"
    moved = D.deformed_grid(m)
    assert capi.bvh8_refit(shuffled, idx, moved).tobytes() == renumbered(capi.bvh8_refit(nodes, idx, moved)).tobytes()


def test_refit_rejects_malformed_input():
    tris, nodes, idx = _built(7)
    moved = D.deformed_grid(7)
    with pytest.raises(capi.NexusError):      # fewer triangles than the index list names
        capi.bvh8_refit(nodes, idx[:-1], moved[:-1])
    with pytest.raises(capi.NexusError):      # no triangles, no nodes
        capi.bvh8_refit(nodes, idx[:0], moved[:0])
    with pytest.raises(capi.NexusError):
        capi.bvh8_refit(nodes[:0], idx, moved)
    bad = idx.copy()
    bad[3] = len(tris)                          # an index out of range
    with pytest.raises(capi.NexusError):
        capi.bvh8_refit(nodes, bad, moved)
    broken = nodes.copy()
    if broken["imask"][0]:
        broken["childBaseIdx"][0] = len(nodes)  # children outside the array
        with pytest.raises(capi.NexusError):
            capi.bvh8_refit(broken, idx, moved)
        broken["childBaseIdx"][0] = 0           # a node may not be its own descendant
        with pytest.raises(capi.NexusError):
            capi.bvh8_refit(broken, idx, moved)
    broken = nodes.copy()
    broken["triangleBaseIdx"][len(nodes) - 1] = len(tris)  # a leaf range past the index list
    with pytest.raises(capi.NexusError):
        capi.bvh8_refit(broken, idx, moved)
