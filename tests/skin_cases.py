"""Shared inputs of the skinned-mesh tests (tests/test_gpu_pose_blas.py, tools/pose_bench.py): small bars, two-joint skins over any
mesh, joint palettes, and the float64 restatement of the blending rule of include/nexus_hip.h (nxhip_pose_blas) with the error bounds
the tests hold the device to."""
import numpy as np

from nexus_amd import pod

U = 2.0 ** -24  # unit roundoff of binary32


def gamma(n):
    return n * U / (1.0 - n * U)


def ribbon(count, zero_normals=False):
    """`count` triangles of a ribbon along +y (a bar one quad wide), slightly twisted so that no coordinate is exactly 0, with unit
    normals (or none: the loaders' (0, 0, 0)) and texture coordinates"""
    k = np.arange(count + 2, dtype=np.float64)
    side = np.where(k % 2 == 0, -1.0, 1.0)
    y = 0.05 + 0.11 * (k // 2) + 0.013 * side
    P = np.stack([0.2 * side + 0.03 * np.sin(0.7 * k + 0.4), y, 0.06 + 0.05 * np.cos(0.45 * k)], -1)
    N = np.stack([0.15 * np.sin(0.3 * k + 0.2), 0.1 * np.cos(0.2 * k), np.ones_like(k)], -1)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    UV = np.stack([(side + 1) / 2, k / (count + 1)], -1)
    tri = np.stack([np.arange(count), np.arange(count) + 1, np.arange(count) + 2], -1)
    tri[1::2] = tri[1::2][:, [1, 0, 2]]  # one winding throughout
    normals = np.zeros((count, 3, 3), np.float32) if zero_normals else N[tri].astype(np.float32)
    return pod.make_triangles(P[tri].astype(np.float32), normals=normals, uvs=UV[tri].astype(np.float32))


def corner_positions(tris):
    """(3 n, 3) float32: corner 3 i + v = vertex v of triangle i"""
    t = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
    return np.stack([t["pos0"], t["pos1"], t["pos2"]], 1).reshape(-1, 3)


def corner_normals(tris):
    t = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
    return np.stack([t["normal0"], t["normal1"], t["normal2"]], 1).reshape(-1, 3)


def two_joint_skin(tris, axis, joint_count, one_hot=False, seed=5):
    """nx_skin_corner records blending joint 0 into joint min(1, joint_count - 1) linearly across the mesh's extent on `axis`; every
    seventh corner carries two more small influences (all four slots in use), and the weights are NOT normalised — each corner's are
    scaled by a factor in [0.5, 1.5] — so that the call's re-normalisation is part of what is tested.  one_hot: each corner wholly on
    the nearer joint.  Joints beyond the second are present in the palette but unused."""
    p = corner_positions(tris)[:, axis].astype(np.float64)
    lo, hi = p.min(), p.max()
    w1 = (p - lo) / (hi - lo) if hi > lo else np.full(len(p), 0.5)
    last = min(1, joint_count - 1)
    joints = np.zeros((len(p), 4), np.int64)
    weights = np.zeros((len(p), 4), np.float64)
    if one_hot:
        joints[:, 0] = np.where(w1 >= 0.5, last, 0)
        weights[:, 0] = 1.0
        return pod.make_skin_corners(joints, weights)
    joints[:, 1] = last
    weights[:, 0], weights[:, 1] = 1.0 - w1, w1
    extra = np.arange(len(p)) % 7 == 3
    joints[extra, 2], joints[extra, 3] = last, 0
    weights[extra, 2], weights[extra, 3] = 0.125, 0.0625
    rng = np.random.RandomState(seed)
    weights *= rng.uniform(0.5, 1.5, (len(p), 1))
    # an unused slot may name any joint at all: the call rewrites it to 0
    joints[weights == 0] = 65535
    return pod.make_skin_corners(joints, weights)


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def palette(kind, joint_count, extent, seed=1):
    """(joint_count, 12) float32.  "ordinary": per joint a rotation of up to 50 degrees composed with per-axis scales in [0.5, 2] and a
    translation of up to the mesh's extent; "mirror": the same with x negated (det < 0 for every joint, so for every blend that keeps
    the sign); "outward": 3.5 x the extent outward along +y on top of a mild rotation — the mesh leaves its old root box; "identity"."""
    rng = np.random.RandomState(seed)
    out = np.zeros((joint_count, 3, 4))
    for j in range(joint_count):
        if kind == "identity":
            out[j, :, :3] = np.eye(3)
            continue
        R = _rotation(rng.normal(size=3), np.radians(rng.uniform(-50, 50) if kind != "outward" else rng.uniform(-15, 15)))
        s = rng.uniform(0.5, 2.0, 3) if kind != "outward" else np.ones(3)
        if kind == "mirror":
            s[0] = -s[0]
        out[j, :, :3] = R * s[None, :]
        out[j, :, 3] = rng.uniform(-extent, extent, 3) if kind != "outward" else np.array([0.1 * extent * rng.uniform(-1, 1), 3.5 * extent, 0.1 * extent * rng.uniform(-1, 1)])
    return out.reshape(joint_count, 12).astype(np.float32)


def reference(bind, corners, pal):
    """The blending rule in float64 over the values the device holds: `bind` triangles, `corners` as nxhip_set_blas_skin stores them
    (pod.normalise_skin_corners), `pal` (joints, 12) float32.  Returns a dict per corner (3 n rows): pos, the position bound's A, the
    unit normal (0 where the bind normal is 0), the normal's conditioning ||t|| / ||v|| and whether the bind normal is zero."""
    J = np.asarray(pal, np.float64).reshape(-1, 3, 4)
    w = corners["weight"].astype(np.float64)
    jt = corners["joint"].astype(np.int64)
    p = np.concatenate([corner_positions(bind).astype(np.float64), np.ones((len(w), 1))], 1)
    n = corner_normals(bind).astype(np.float64)
    M = np.einsum("ck,ckrs->crs", w, J[jt])
    pos = np.einsum("crs,cs->cr", M, p)
    A = np.einsum("ck,ckrs,cs->cr", w, np.abs(J[jt]), np.abs(p))

    def cof(m):
        c = np.empty(m.shape[:-2] + (3, 3))
        for r in range(3):
            for s in range(3):
                r1, r2, s1, s2 = (r + 1) % 3, (r + 2) % 3, (s + 1) % 3, (s + 2) % 3
                c[..., r, s] = m[..., r1, s1] * m[..., r2, s2] - m[..., r1, s2] * m[..., r2, s1]
        return c

    M3 = M[:, :, :3]
    v = np.einsum("crs,cs->cr", cof(M3), n)
    v[np.linalg.det(M3) < 0] *= -1.0
    a = np.abs(M3)
    abs_cof = np.empty_like(a)
    for r in range(3):
        for s in range(3):
            r1, r2, s1, s2 = (r + 1) % 3, (r + 2) % 3, (s + 1) % 3, (s + 2) % 3
            abs_cof[:, r, s] = a[:, r1, s1] * a[:, r2, s2] + a[:, r1, s2] * a[:, r2, s1]
    t = np.einsum("crs,cs->cr", abs_cof, np.abs(n))
    zero = np.all(n == 0, axis=1)
    vn = np.linalg.norm(v, axis=1)
    unit = np.where(zero[:, None], 0.0, v / np.where(vn > 0, vn, 1.0)[:, None])
    cond = np.where(zero, 0.0, np.linalg.norm(t, axis=1) / np.where(vn > 0, vn, 1.0))
    return dict(pos=pos, A=A, normal=unit, cond=cond, zero=zero)


def check_posed(got, bind, corners, pal, what=""):
    """the device's posed triangles against `reference`, by the bounds of the issue: positions |device - ref| <= gamma_8 A per
    component; normals ||n' - v / ||v|| ||_inf <= 2 gamma_16 ||t|| / ||v|| + 4 u, with ||t|| / ||v|| <= 8 asserted of the inputs first;
    zero bind normals stay zero; texture coordinates bit-equal.  Returns the worst ratios (error / bound)."""
    ref = reference(bind, corners, pal)
    assert float(ref["cond"].max()) <= 8.0, (what, "the test's own normals are ill-conditioned", float(ref["cond"].max()))
    gp = corner_positions(got).astype(np.float64)
    gn = corner_normals(got).astype(np.float64)
    bound_p = gamma(8) * ref["A"]
    err_p = np.abs(gp - ref["pos"])
    bound_n = 2.0 * gamma(16) * ref["cond"] + 4.0 * U
    err_n = np.max(np.abs(gn - ref["normal"]), axis=1)
    rp = float(np.max(err_p / np.maximum(bound_p, 1e-300)))
    live = ~ref["zero"]
    rn = float(np.max(err_n[live] / bound_n[live])) if live.any() else 0.0
    print("%s: %d corners, position error / bound %.3f, normal error / bound %.3f (worst conditioning %.2f), %d zero normals" % (
        what, len(gp), rp, rn, float(ref["cond"].max()), int(ref["zero"].sum())))
    assert np.all(err_p <= bound_p), (what, rp)
    assert np.all(err_n[live] <= bound_n[live]), (what, rn)
    assert np.all(gn[ref["zero"]] == 0.0), what
    g, b = np.ascontiguousarray(got, dtype=pod.TRI_DT), np.ascontiguousarray(bind, dtype=pod.TRI_DT)
    for k in range(3):
        assert g["texCoord%d" % k].tobytes() == b["texCoord%d" % k].tobytes(), what
    return rp, rn
