"""Host data producers: the product's parallel BVH2 / BVH8 / TLAS builders (C++, through the flat C API) against the
oracle's serial restatement of the reference algorithm — byte for byte — plus structural invariants of the 80-byte nodes."""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen
from tests import bvh_audit
from tests import oracle_lib as O
from tests import scene_helpers as SH

MESHES = {
    "soup": lambda: scenegen.random_soup(3000, seed=1),
    "height_field": lambda: scenegen.height_field(48, seed=2),
    "torus": lambda: scenegen.displaced_torus(96, 48, seed=3),
    "planar_quad": lambda: scenegen.quad((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)),
    "single": lambda: scenegen.random_soup(1, seed=4),
    "duplicates": lambda: np.repeat(scenegen.random_soup(4, seed=5), 9),
    "degenerate_centroids": lambda: np.concatenate([scenegen.random_soup(40, seed=6), np.repeat(scenegen.random_soup(1, seed=7), 40)]),
}


@pytest.mark.parametrize("name", list(MESHES))
def test_bvh2_and_bvh8_bytes_equal_oracle(name):
    tris = MESHES[name]()
    on, oi = O.bvh2_build(tris)
    pn, pi = capi.bvh2_build(tris, threads=4)
    assert on.tobytes() == pn.tobytes() and np.array_equal(oi, pi)
    o8, oidx = O.bvh8_build(tris, clamp_qhi=1)
    p8, pidx = capi.bvh8_build(tris, threads=4)
    assert o8.tobytes() == p8.tobytes() and np.array_equal(oidx, pidx)


def test_build_is_independent_of_thread_count():
    tris = scenegen.displaced_torus(256, 128, seed=8)  # 65 536 triangles: above the task-spawn threshold
    a = capi.bvh8_build(tris, threads=1)
    b = capi.bvh8_build(tris, threads=8)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    o = O.bvh8_build(tris, clamp_qhi=1)
    assert o[0].tobytes() == a[0].tobytes() and np.array_equal(o[1], a[1])


def _decode_children(node):
    """(slot, kind, lo3, hi3, first, count) for every non-empty child, boxes dequantised to floats."""
    scale = np.array([np.array([int(e) << 23], np.uint32).view(np.float32)[0] for e in node["e"]], np.float64)
    p = node["p"].astype(np.float64)
    out = []
    inner_rank = 0
    for s in range(8):
        meta = int(node["meta"][s])
        if meta == 0:
            continue
        lo = p + scale * np.array([node["qlox"][s], node["qloy"][s], node["qloz"][s]], np.float64)
        hi = p + scale * np.array([node["qhix"][s], node["qhiy"][s], node["qhiz"][s]], np.float64)
        if node["imask"] & (1 << s):
            assert meta == (0x20 | (24 + s))
            out.append((s, "inner", lo, hi, int(node["childBaseIdx"]) + inner_rank, 1))
            inner_rank += 1
        else:
            cnt = bin(meta >> 5).count("1")
            assert (meta >> 5) == (1 << cnt) - 1 and 1 <= cnt <= 3
            out.append((s, "leaf", lo, hi, int(node["triangleBaseIdx"]) + (meta & 0x1F), cnt))
    return out


@pytest.mark.parametrize("name", ["soup", "torus", "planar_quad", "degenerate_centroids"])
def test_bvh8_structure_is_valid_and_conservative(name):
    """tests/bvh_audit.py: every triangle once, meta encodings, 1-3 primitives per leaf slot and at most 24 per node; every slot
    box, inner and leaf, contains the exact box of what lies under it and is less than a grid step wider; every frame's origin
    and exponent are the subtree's minimum and the smallest exponent that covers its extent"""
    tris = MESHES[name]()
    nodes, idx = capi.bvh8_build(tris, threads=4)
    rep = bvh_audit.audit(nodes, idx, *bvh_audit.triangle_boxes(tris))
    print(rep.line("host build, %s" % name))
    assert rep.nodes == len(nodes)


def test_mat4_instance_camera_equal_oracle():
    rng = np.random.RandomState(0)
    tris = scenegen.displaced_torus(24, 12, seed=2)
    nodes, _ = capi.bvh8_build(tris, threads=2)
    for _ in range(20):
        pos, rot, scl = rng.uniform(-3, 3, 3), rng.uniform(-180, 180, 3), rng.uniform(0.3, 2.0, 3)
        a, b = O.mat4_from_trs(pos, rot, scl), capi.mat4_from_trs(pos, rot, scl)
        assert a.tobytes() == b.tobytes()
        assert O.mat4_invert(a).tobytes() == capi.mat4_invert(b).tobytes()
        ia, ib = O.instance_init(3, 7, a, nodes[0]), capi.instance_init(3, 7, b, nodes[0])
        assert ia.tobytes() == ib.tobytes()
    for w, h, fov in [(512, 512, 40.0), (1920, 1080, 60.0), (96, 64, 50.0)]:
        ca = O.camera_init((0.1, 1.0, 3.9), (0.0, -0.2, -0.98), fov, w, h, 5.0, 1.5)
        cb = capi.camera_init((0.1, 1.0, 3.9), (0.0, -0.2, -0.98), fov, w, h, 5.0, 1.5)
        assert ca.tobytes() == cb.tobytes()
    # singular matrix inverts to identity (Mat4.h:185-193)
    assert np.array_equal(capi.mat4_invert(np.zeros(16, np.float32)), np.eye(4, dtype=np.float32).reshape(16))


@pytest.mark.parametrize("n_inst", [1, 2, 3, 9, 40])
def test_tlas_bytes_equal_oracle(n_inst):
    rng = np.random.RandomState(n_inst)
    tris = scenegen.displaced_torus(24, 12, seed=2)
    nodes, _ = capi.bvh8_build(tris, threads=2)
    insts = np.array([capi.instance_init(0, 0, capi.mat4_from_trs(rng.uniform(-4, 4, 3), rng.uniform(0, 360, 3), rng.uniform(0.5, 1.5, 3)), nodes[0])
                      for _ in range(n_inst)], dtype=pod.INST_DT)
    on, oi = O.tlas_build(insts)
    pn, pi = capi.tlas_build(insts)
    assert on.tobytes() == pn.tobytes() and np.array_equal(oi, pi)
    assert sorted(pi.tolist()) == list(range(n_inst))
