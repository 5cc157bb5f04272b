"""The device builders' binary trees, cost table and collapse (nx_lbvh.hip) held to their algorithms: the tree a build otherwise frees is
read back (nxhip_debug_keep_binary_tree / nxhip_debug_read_binary_tree) and judged by tests/binary_tree_reference.py — (a) structure
with every box the exact union of its children's, the builder's own check ((b) radix tree from its definition, (c) clustering rounds,
(d) top-down SAH optimality in float64), (e) the cost table entry by entry in binary32 and against a float64 programme, (f) an exact
replay of the collapse against the wide nodes.  tests/test_binary_tree_reference.py judges those checks on the CPU.

Figures of the last run on an MI355X (printed by the tests; the bounds are binary_tree_reference.SAH_SLACK and dp_bound(height)),
maxima over the 40 builds, all checks active:
  SAH excess (cost of a split over the best candidate's, float64)   3.58e-08  (planar, builder -1; 0 everywhere else)   bound 9.54e-07
  DP deviation (a device cost against the float64 programme)        2.51e-06  (copies, clustering: a tree 307 levels deep, bound 3.71e-05);
                                                                    at most 0.113 of its bound; 1.8e-07 on the 20 000-triangle soup (bound 2.5e-06)
  cost of the wide tree against the programme's optimum             1.32e-09  (planar, clustering r = 16; <= 6e-15 on every other build)
The first run found one defect (fixed in nx_lbvh.hip): check (d) on `copies`, builder -1 — "node 98 (4 primitives, centroids
coincide): split 1 : 3, not in half".
"""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen
from nexus_amd.capi import NexusError
from tests import binary_tree_reference as R
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

MESHES = {
    "nine": lambda: scenegen.random_soup(9, seed=4),              # the smallest tree past the single-node path
    "ribbon64": lambda: R.ribbon(64),                             # one wave
    "ribbon65": lambda: R.ribbon(65),                             # one wave and a lane
    "soup1000": lambda: scenegen.random_soup(1000, seed=3),       # upper levels share a segment per workgroup, lower levels do not
    "torus1024": lambda: scenegen.displaced_torus(32, 16, seed=2),  # the regular grid of the workload: tied centroids
    "copies": lambda: R.copies_and_distinct(300, 100),            # equal Morton codes, nodes that nothing separates
    "planar": lambda: R.planar_grid(12),                          # a dead axis in the binning
    "soup20000": lambda: scenegen.random_soup(20000, seed=8),     # enough workgroups to span the XCDs: the fence-free publish
}
BUILDERS = (-1, 0, 3, 16)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(32, 32)
    c.debug_keep_binary_tree(True)
    yield c
    c.close()


def _report(what, figures):
    print("%s: height %d, %d wide nodes, SAH excess %.3g (bound %.3g), DP deviation %.3g (bound %.3g), collapse cost off the optimum by %.3g" % (
        what, figures["height"], figures["wide_nodes"], figures["sah_excess"], R.SAH_SLACK, figures["dp_deviation"], R.dp_bound(figures["height"]), figures["collapse_excess"]))


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", list(MESHES))
def test_blas_binary_tree_cost_table_and_collapse_are_the_algorithms(ctx, name, builder):
    tris = np.ascontiguousarray(MESHES[name](), dtype=pod.TRI_DT)
    plo, phi = R.boxes_of(tris)
    ctx.set_device_builder(builder)
    bid = ctx.build_blas(tris)
    nodes, idx = ctx.read_blas(bid, len(tris))
    T = ctx.debug_read_binary_tree()
    assert T["n"] == len(tris) and T["builder"] == builder and T["prim_cost"] == 0.75
    _report("%s, builder %d" % (name, builder), R.check_all(T, plo, phi, nodes, idx))


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n_inst", [9, 60])
def test_tlas_binary_tree_cost_table_and_collapse_are_the_algorithms(n_inst, builder):
    """nxhip_rebuild_tlas goes through the same build with an instance priced at 4.  Its primitives are the instance boxes the device
    tightened, which stay on the device: they are taken from the tree's own leaves (and must lie within the records' boxes), so the
    leaf half of (a) says nothing here; every other check stands as for a BLAS."""
    scene = SH.instanced_scene(seed=9, n_inst=n_inst)
    with capi.Context(32, 32) as ctx:
        scene.upload(ctx)
        ctx.set_device_builder(builder)
        ctx.debug_keep_binary_tree(True)
        nodes, idx = ctx.rebuild_tlas(scene.instances)
        T = ctx.debug_read_binary_tree()
    assert T["n"] == n_inst and T["builder"] == builder and T["prim_cost"] == 4.0
    order = T["leaf_order"].astype(np.int64)
    assert sorted(order.tolist()) == list(range(n_inst))
    plo, phi = np.zeros((n_inst, 3), np.float32), np.zeros((n_inst, 3), np.float32)
    plo[order], phi[order] = T["box"][n_inst - 1:, 0], T["box"][n_inst - 1:, 1]
    assert np.all(plo >= scene.instances["boundsMin"]) and np.all(phi <= scene.instances["boundsMax"]) and np.all(plo <= phi)
    _report("TLAS of %d, builder %d" % (n_inst, builder), R.check_all(T, plo, phi, nodes, idx))


def test_the_hook_changes_nothing_and_keeps_nothing_while_it_is_off():
    """Off (the default) a build stashes nothing; on or off, the wide nodes are the same: byte for byte where every collapse level is one
    wave of work items (their atomics come in lane order), and as the replay of the kept tree where node numbers depend on timing."""
    small = np.ascontiguousarray(R.ribbon(64), dtype=pod.TRI_DT)
    large = np.ascontiguousarray(scenegen.random_soup(1000, seed=3), dtype=pod.TRI_DT)
    for builder in BUILDERS:
        with capi.Context(32, 32) as off, capi.Context(32, 32) as on:
            off.set_device_builder(builder)
            on.set_device_builder(builder)
            on.debug_keep_binary_tree(True)
            a, b = off.read_blas(off.build_blas(small), len(small)), on.read_blas(on.build_blas(small), len(small))
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), builder
            with pytest.raises(NexusError, match="no binary tree is stashed"):
                off.debug_read_binary_tree()
            assert on.debug_read_binary_tree()["n"] == len(small)
            nodes_off, idx_off = off.read_blas(off.build_blas(large), len(large))
            nodes_on, idx_on = on.read_blas(on.build_blas(large), len(large))
            T = on.debug_read_binary_tree()
            assert len(nodes_off) == len(nodes_on)
            R.check_collapse(T, nodes_on, idx_on)
            R.check_collapse(T, nodes_off, idx_off)
            with pytest.raises(NexusError, match="no binary tree is stashed"):
                off.debug_read_binary_tree()
            # a single node has no binary tree; the batched build is not covered and leaves the stash alone; off drops it
            on.build_blas(small[:8])
            T = on.debug_read_binary_tree()
            assert T["n"] == 0 and len(T["left"]) == 0 and T["builder"] == builder and T["prim_cost"] == 0.75
            on.build_blas(large[:100])
            on.set_device_builder(-1)
            on.build_blas_batch([large[:50], large[50:90]])
            assert on.debug_read_binary_tree()["n"] == 100
            on.debug_keep_binary_tree(False)
            with pytest.raises(NexusError, match="no binary tree is stashed"):
                on.debug_read_binary_tree()
            on.build_blas(small)
            with pytest.raises(NexusError, match="no binary tree is stashed"):
                on.debug_read_binary_tree()
