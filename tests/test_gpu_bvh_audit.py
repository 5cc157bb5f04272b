"""Exact audit (tests/bvh_audit.py) of every device producer of 80-byte nodes — the three BLAS builders, the batched build, the
BLAS refit, the TLAS build and the TLAS refit — on the meshes of tests/bvh_audit_cases.py, and the rays that graze the far face of
a node on the 255 * 2^n boundary through the trace kernels, against the oracle's brute force.  Every test prints the worst
containment shortfall and the worst looseness it met."""
import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import bvh_audit as A
from tests import bvh_audit_cases as K
from tests import deform_meshes as D
from tests import oracle_lib as O
from tests import scene_helpers as SH
from tests.test_tlas_refit import _geometry_bounds

pytestmark = pytest.mark.gpu

BUILDERS = {0: "radix tree", 16: "clustering r=16", 3: "clustering r=3", -1: "top-down SAH"}


class _Worst:
    def __init__(self):
        self.rep = A.Report()

    def add(self, r):
        w = self.rep
        w.nodes, w.slots, w.wide_exponents = w.nodes + r.nodes, w.slots + r.slots, w.wide_exponents + r.wide_exponents
        w.rounded_frames, w.rounded_worst_steps = w.rounded_frames + r.rounded_frames, max(w.rounded_worst_steps, r.rounded_worst_steps)
        if r.short_steps > w.short_steps:
            w.short_steps, w.short_ulp, w.short_at = r.short_steps, r.short_ulp, r.short_at
        if r.loose_steps > w.loose_steps:
            w.loose_steps, w.loose_ulp, w.loose_at = r.loose_steps, r.loose_ulp, r.loose_at


def _audit(nodes, idx, tris, worst, what):
    rep = A.audit(nodes, idx, *A.triangle_boxes(tris), check=False)
    assert not rep.failures, (what, rep.failures[:6])
    worst.add(rep)


def _install_single(ctx, bid, root):
    inst = np.array([capi.instance_init(bid, 0, SH.IDENTITY, root)], dtype=pod.INST_DT)
    tn, ti = capi.tlas_build(inst)
    ctx.set_tlas(tn, ti, inst)
    return inst, tn, ti


def _sliver_check(ctx, nodes, idx, tris, inst, tn, ti, case):
    """trace_batch and trace_shadow_batch on the grazing rays against the oracle's brute force over the same triangles"""
    place, axis, n, k = case
    rays = K.sliver_rays(n, k, axis)
    oracle = O.OracleScene([(nodes, tris, idx)], inst, tn, ti)
    want = oracle.brute_closest(rays)
    hit = want["hitDistance"] < 1e29
    assert hit[1:].all(), case
    got = ctx.trace_batch(rays)
    assert np.array_equal(got["hitDistance"].view(np.uint32), want["hitDistance"].view(np.uint32)), (case, got["hitDistance"], want["hitDistance"])
    # shadow rays that end just beyond the hit (a step of 2^-20 of the distance): occluded wherever brute force hits
    tmax = np.where(hit, want["hitDistance"] * np.float32(1.0 + 2.0 ** -20), np.float32(4.0 * np.ldexp(255.0, n))).astype(np.float32)
    occ = ctx.trace_shadow_batch(rays, tmax)
    assert np.array_equal(occ, oracle.brute_any(rays, tmax)) and np.array_equal(occ.astype(bool), hit), (case, occ, hit)
    return len(rays)


@pytest.mark.parametrize("radius", list(BUILDERS))
def test_device_built_small_meshes_pass_the_audit(gpu_ctx_factory, radius):
    ctx = gpu_ctx_factory(32, 32)
    ctx.set_device_builder(radius)
    worst = _Worst()
    for name, make in K.SMALL.items():
        tris = np.ascontiguousarray(make(), dtype=pod.TRI_DT)
        ctx.clear_blas()
        bid = ctx.build_blas(tris)
        _audit(*ctx.read_blas(bid, len(tris)), tris, worst, (BUILDERS[radius], name))
    print(worst.rep.line("device build, %s, small meshes" % BUILDERS[radius]))


@pytest.mark.parametrize("place", K.BOUNDARY_PLACES)
@pytest.mark.parametrize("radius", list(BUILDERS))
def test_device_built_boundary_family_passes_the_audit_and_the_sliver_rays(gpu_ctx_factory, radius, place):
    ctx = gpu_ctx_factory(32, 32)
    ctx.set_device_builder(radius)
    worst, rays = _Worst(), 0
    for axis in range(3):
        for n in K.BOUNDARY_N:
            for k in K.BOUNDARY_K:
                case = (place, axis, n, k)
                tris = K.boundary_mesh(n, k, axis, place)
                ctx.clear_blas()
                bid = ctx.build_blas(tris)
                nodes, idx = ctx.read_blas(bid, len(tris))
                _audit(nodes, idx, tris, worst, (BUILDERS[radius], case))
                inst, tn, ti = _install_single(ctx, bid, nodes[0])
                A.audit(tn, ti, *A.instance_boxes(inst), tlas=True)
                rays += _sliver_check(ctx, nodes, idx, tris, inst, tn, ti, case)
    print(worst.rep.line("device build, %s, boundary family (%s), %d grazing rays bit-equal to brute force" % (BUILDERS[radius], place, rays)))


def test_batched_build_passes_the_audit(gpu_ctx_factory):
    meshes = [np.ascontiguousarray(make(), dtype=pod.TRI_DT) for make in K.SMALL.values()]
    meshes += [K.boundary_mesh(n, k, axis, place) for place in K.BOUNDARY_PLACES for axis in range(3) for n in K.BOUNDARY_N for k in K.BOUNDARY_K]
    ctx = gpu_ctx_factory(32, 32)
    ctx.clear_blas()
    ids = ctx.build_blas_batch(meshes)
    trees = ctx.read_blas_batch(ids[0], [len(m) for m in meshes])
    worst = _Worst()
    for k, ((nodes, idx), tris) in enumerate(zip(trees, meshes)):
        _audit(nodes, idx, tris, worst, ("batched build, mesh %d" % k))
    print(worst.rep.line("device batched build, %d meshes" % len(meshes)))


@pytest.mark.parametrize("tree", ["host", "device-sah", "device-radix"])
def test_device_refitted_blas_passes_the_audit(gpu_ctx_factory, tree):
    """nxhip_update_blas on a wavy grid and onto the boundary (the k = 12 tree refitted to the vertices of every other k): the
    audit, the host refit's bytes, and the grazing rays"""
    ctx = gpu_ctx_factory(32, 32)
    worst, rays = _Worst(), 0

    def start(tris):
        ctx.clear_blas()
        if tree == "host":
            nodes, idx = capi.bvh8_build(tris, threads=2)
            return ctx.upload_blas(nodes, tris, idx), nodes, idx
        ctx.set_device_builder(-1 if tree == "device-sah" else 0)
        bid = ctx.build_blas(tris)
        return (bid,) + ctx.read_blas(bid, len(tris))

    base = np.ascontiguousarray(D.base_grid(40), dtype=pod.TRI_DT)
    bid, nodes0, idx0 = start(base)
    for shape in range(len(D.SHAPES)):
        moved = np.ascontiguousarray(D.deformed_grid(40, shape), dtype=pod.TRI_DT)
        ctx.update_blas(bid, moved)
        got, got_idx = ctx.read_blas(bid, len(moved))
        assert np.array_equal(got_idx, idx0)
        _audit(got, got_idx, moved, worst, (tree, "wavy grid", shape))
        assert got.tobytes() == capi.bvh8_refit(nodes0, idx0, moved).tobytes()
    for place in K.BOUNDARY_PLACES:
        for axis, n in ((0, -20), (1, -8), (2, 3), (2, -20)):
            bid, nodes0, idx0 = start(K.boundary_mesh(n, 12, axis, place))
            for k in K.BOUNDARY_K:
                moved = K.boundary_mesh(n, k, axis, place)
                ctx.update_blas(bid, moved)
                got, got_idx = ctx.read_blas(bid, len(moved))
                _audit(got, got_idx, moved, worst, (tree, place, axis, n, k))
                assert got.tobytes() == capi.bvh8_refit(nodes0, idx0, moved).tobytes(), (tree, place, axis, n, k)
                inst, tn, ti = _install_single(ctx, bid, got[0])
                rays += _sliver_check(ctx, got, got_idx, moved, inst, tn, ti, (place, axis, n, k))
    print(worst.rep.line("device BLAS refit of a %s tree, %d grazing rays bit-equal to brute force" % (tree, rays)))


@pytest.mark.parametrize("n_inst", [1, 2, 9, 60])
def test_device_tlas_build_and_refit_pass_the_audit(gpu_ctx_factory, n_inst):
    scene = K.tlas_scene(n_inst)
    ctx = gpu_ctx_factory(32, 32)
    scene.upload(ctx)
    # a host-built tree refitted on the device: the records can be read back, so the audit is exact
    moved = K.moved_instances(scene, 77)
    ids = np.arange(1, n_inst, dtype=np.uint32)
    if len(ids):
        ctx.set_instance_transforms(ids, moved["transform"][1:])
    got_nodes, got_inst = ctx.read_tlas(len(scene.tlas_nodes), n_inst)
    assert got_inst.tobytes() == moved.tobytes()
    rep = A.audit(got_nodes, scene.tlas_idx, *A.instance_boxes(got_inst), tlas=True)
    print(rep.line("device TLAS refit of a host-built tree, %d instances" % n_inst))
    assert got_nodes.tobytes() == capi.tlas_refit(scene.tlas_nodes, scene.tlas_idx, moved).tobytes()
    # built on the device from tightened boxes: against the geometry, inner slots too, then moved once more
    for builder in BUILDERS:
        ctx.set_device_builder(builder)
        nodes, idx = ctx.rebuild_tlas(scene.instances)
        rep = A.audit_tlas_geometry(nodes, idx, *_geometry_bounds(scene, scene.instances))
        print(rep.line("device TLAS build (%s), %d instances, against geometry" % (BUILDERS[builder], n_inst)))
        if len(ids):
            ctx.set_instance_transforms(ids, moved["transform"][1:])
        refit, _ = ctx.read_tlas(len(nodes), n_inst)
        rep = A.audit_tlas_geometry(refit, idx, *_geometry_bounds(scene, moved))
        print(rep.line("device TLAS refit of that tree, against geometry"))
    ctx.set_device_builder(-1)
