"""Shared inputs of the deforming-mesh tests (tests/test_blas_refit.py, test_gpu_blas_refit.py, test_host_facade_deform.py): a wavy
grid whose triangle i stays triangle i while amplitude and phase change, the host-side answer for a scene after some of its meshes
moved (nxh_bvh8_refit, BVHInstance::SetTransform bounds, nxh_tlas_refit), and the depth of a BVH8's nodes."""
import numpy as np

from nexus_amd import capi, pod, scenegen
from tests import scene_helpers as SH

SIZES = (1, 7, 40, 100)       # m: the grid has m x m x 2 triangles
BASE = dict(amp=0.08, phase=0.3)
# the deformations, mildest first; the last one is 3.5 x the base amplitude (the issue asks for at least 2.5 x): the mesh leaves its
# old root box, so a stale root copy in an instance record, stale instance bounds or a stale TLAS lose hits
SHAPES = (dict(amp=0.05, phase=1.1), dict(amp=0.17, phase=2.0), dict(amp=0.28, phase=4.4))


def wavy_grid(m, amp, phase, freq=2.3):
    """2 m^2 triangles over [-1, 1]^2, y = 0.11 + amp sin(freq x + phase) cos(1.3 freq z + 0.7 phase) (never exactly zero at a grid
    point with these constants, so no box corner is a zero whose sign fmin / fmax could pick either way); triangle order and
    texture coordinates depend on m only."""
    g = np.linspace(-1.0, 1.0, m + 1)
    xx, zz = np.meshgrid(g, g, indexing="ij")
    yy = 0.11 + amp * np.sin(freq * xx + phase) * np.cos(1.3 * freq * zz + 0.7 * phase)
    P = np.stack([xx, yy, zz], -1)
    du = np.gradient(P, axis=0)
    dv = np.gradient(P, axis=1)
    N = np.cross(dv, du)
    N /= np.maximum(np.linalg.norm(N, axis=-1, keepdims=True), 1e-30)
    uv = np.stack([(xx + 1) / 2, (zz + 1) / 2], -1).astype(np.float32)
    return scenegen._grid_surface_triangles(P.astype(np.float32), N.astype(np.float32), uv, False, False)


def base_grid(m):
    return wavy_grid(m, **BASE)


def deformed_grid(m, shape=-1):
    return wavy_grid(m, **SHAPES[shape])


def node_depths(nodes):
    """depth of every node, walking from the root (children need not follow their parents in the array); -1: not reached"""
    depth = np.full(len(nodes), -1, np.int64)
    depth[0] = 0
    todo = [0]
    while todo:
        i = todo.pop()
        for k in range(bin(int(nodes["imask"][i])).count("1")):
            c = int(nodes["childBaseIdx"][i]) + k
            assert depth[c] == -1
            depth[c] = depth[i] + 1
            todo.append(c)
    return depth


def with_blas(scene, blas, instances=None, tlas=None):
    """a copy of a BuiltScene with other BLAS tuples (and instances / (tlas_nodes, tlas_idx))"""
    out = SH.BuiltScene.__new__(SH.BuiltScene)
    out.__dict__.update(scene.__dict__)
    out.blas = list(blas)
    out.meshes = [b[1] for b in out.blas]
    if instances is not None:
        out.instances = instances
    if tlas is not None:
        out.tlas_nodes, out.tlas_idx = tlas
    return out


def host_deformed(scene, new_tris, blas=None, tlas=None):
    """What the host classes give for `scene` after the meshes in new_tris {blas id: triangles} moved: nxh_bvh8_refit of the nodes,
    BVHInstance::SetTransform bounds from the new roots for the instances of those meshes, nxh_tlas_refit.  `blas`: the (nodes,
    tris, idx) list the device holds when it is not scene.blas (device-built trees); `tlas`: likewise (nodes, idx)."""
    blas = list(blas if blas is not None else scene.blas)
    for b, tris in new_tris.items():
        nodes, _old, idx = blas[b]
        tris = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
        blas[b] = (capi.bvh8_refit(nodes, idx, tris), tris, idx)
    insts = scene.instances.copy()
    for i, old in enumerate(scene.instances):
        b = int(old["bvhIdx"])
        if b in new_tris:
            insts[i] = capi.instance_init(b, int(old["materialId"]), old["transform"], blas[b][0][0])
    tlas_nodes, tlas_idx = tlas if tlas is not None else (scene.tlas_nodes, scene.tlas_idx)
    return with_blas(scene, blas, insts, (capi.tlas_refit(tlas_nodes, tlas_idx, insts), tlas_idx))


def rays_for(n, seed, extent=1.2):
    a = scenegen.random_rays(n // 2, seed=seed, radius=3.0 * extent, target_extent=extent)
    b = scenegen.interior_rays(n - n // 2, seed=seed + 1, extent=extent)
    return np.concatenate([a, b])
