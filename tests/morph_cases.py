"""Shared inputs of the morph-target tests (tests/test_gpu_pose_morph.py, tools/morph_bench.py): deltas over any mesh, weight sets, and
the float64 restatement of the rule of include/nexus_hip.h (nxhip_pose_blas_morph) with the error bounds the tests hold the device to.

THE BOUNDS, derived (u = 2^-24, gamma_k = k u / (1 - k u); A = the number of active targets):

  positions   The device evaluates fl(... fl(fl(p + fl(w_1 d_1)) + fl(w_2 d_2)) ...) per component: A products, A additions, left to
              right.  p passes through A roundings, the product of target t through 1 + (A - t + 1) <= A + 1.  A fused multiply-add
              only removes roundings.  So  |err_c| <= gamma_{A+1} (|p_c| + sum_t |w_t| |dP_t,c|).
  normals     The same sum over the normal: the device holds v + e instead of v = n + sum_t w_t dN_t, with |e_c| <= gamma_{A+1} t_c,
              t_c = |n_c| + sum_t |w_t| |dN_t,c|.  For vectors a, b:  || a / ||a|| - b / ||b|| || <= 2 ||a - b|| / ||b||, so normalising
              v + e instead of v moves the unit vector by at most 2 gamma_{A+1} ||t|| / ||v||.  The normalisation itself — three squares,
              two additions, a root, a division — leaves each component (at most 1 in magnitude) within (3/2 + 1 + 1) u < 4 u.
              ||n' - v / ||v|| ||_inf <= 2 gamma_{A+1} ||t|| / ||v|| + 4 u  — skin_cases.check_posed's bound with the sum's gamma in place of
              the cofactor product's.  ||t|| / ||v|| <= 8 is asserted of the inputs first, as there.
  morph+skin  With (p', n') the exact morph of the corner and M = sum_k w_k J[j_k]:
              positions   the skin's own bound gamma_8 sum_k w_k sum_c |J_k[r][c]| |(p', 1)_c|, plus the morph's error bound_c carried
                          through the matrix, sum_c |M[r][c]| bound_c;
              normals     the skin's own 2 gamma_16 ||T|| / ||V|| + 4 u with V = +-cof(M3) n', T = |cof|(|M3|) |n'|, plus the morph's
                          normal error b (per component of the unit n') carried through the cofactor matrix and the normalisation:
                          2 || |cof|(|M3|) (b, b, b) || / ||V||.
"""
import numpy as np

from nexus_amd import pod
from tests import skin_cases as K

U, gamma = K.U, K.gamma


def deltas(tris, targets, seed=3, outward=None, plain=()):
    """(targets, 3 n) nx_morph_corner records over `tris`: smooth per-corner position deltas of up to 0.3 x the mesh's extent and normal
    deltas of up to 0.1 per component (the unnormalised normal keeps a length the bound's conditioning accepts for |w| summing to 3).
    outward: the index of a target that instead carries the whole mesh 3.5 x its extent along +y — a pose by it leaves the old root box;
    plain: indices of targets without NORMAL (zero normal deltas), which `outward` is too."""
    p = K.corner_positions(tris).astype(np.float64)
    ext = float(np.max(p.max(0) - p.min(0))) or 1.0
    rng = np.random.RandomState(seed)
    dp = np.zeros((targets, len(p), 3))
    dn = np.zeros((targets, len(p), 3))
    for t in range(targets):
        f, ph = rng.uniform(0.5, 3.0, (3, 3)), rng.uniform(0, 6.28, 3)
        dp[t] = 0.3 * ext * np.sin(p @ f.T / ext + ph) * rng.uniform(0.2, 1.0, (len(p), 1))
        dn[t] = 0.1 * np.cos(p @ f / ext + ph[::-1])
        if t == outward:
            dp[t] = 0.02 * dp[t] + np.array([0.0, 3.5 * ext, 0.0])
        if t == outward or t in plain:
            dn[t] = 0.0
    return pod.make_morph_corners(dp, dn)


def reference(bind, d, weights):
    """The rule in float64 over the values the device holds: `bind` triangles, `d` (T, 3 n) nx_morph_corner records, `weights` float32 (T,).
    Per corner: pos and its bound's magnitude B, the exact unnormalised normal v with t, the unit normal (0 where the bind normal is 0 or
    v is), the conditioning ||t|| / ||v||, which bind normals are zero, and the active count."""
    w = np.asarray(weights, np.float32).astype(np.float64)
    act = np.flatnonzero(w != 0)
    p = K.corner_positions(bind).astype(np.float64)
    n = K.corner_normals(bind).astype(np.float64)
    dP = d["dPosition"][act].astype(np.float64)
    dN = d["dNormal"][act].astype(np.float64)
    wa = w[act][:, None, None]
    pos = p + np.sum(wa * dP, 0)
    B = np.abs(p) + np.sum(np.abs(wa) * np.abs(dP), 0)
    v = n + np.sum(wa * dN, 0)
    t = np.abs(n) + np.sum(np.abs(wa) * np.abs(dN), 0)
    zero = np.all(n == 0, axis=1)
    vn = np.linalg.norm(v, axis=1)
    if len(act) == 0:  # the stage is absent: the bind normal as it is
        unit = n.copy()
    else:
        unit = np.where(zero[:, None], 0.0, v / np.where(vn > 0, vn, 1.0)[:, None])
    cond = np.where(zero, 0.0, np.linalg.norm(t, axis=1) / np.where(vn > 0, vn, 1.0))
    return dict(pos=pos, B=B, normal=unit, cond=cond, zero=zero, active=len(act))


def bounds(ref):
    """(per component position bound, per corner normal bound) of a `reference`"""
    g = gamma(ref["active"] + 1)
    return g * ref["B"], 2.0 * g * ref["cond"] + 4.0 * U


def _texcoords_equal(got, bind, what):
    g, b = np.ascontiguousarray(got, dtype=pod.TRI_DT), np.ascontiguousarray(bind, dtype=pod.TRI_DT)
    for k in range(3):
        assert g["texCoord%d" % k].tobytes() == b["texCoord%d" % k].tobytes(), what


def _hold(err_p, bound_p, err_n, bound_n, zero, gn, what, worst_cond):
    rp = float(np.max(err_p / np.maximum(bound_p, 1e-300)))
    live = ~zero
    rn = float(np.max(err_n[live] / bound_n[live])) if live.any() else 0.0
    print("%s: %d corners, position error / bound %.3f, normal error / bound %.3f (worst conditioning %.2f), %d zero normals" % (
        what, len(err_p), rp, rn, worst_cond, int(zero.sum())))
    assert np.all(err_p <= bound_p), (what, rp)
    assert np.all(err_n[live] <= bound_n[live]), (what, rn)
    assert np.all(gn[zero] == 0.0), what
    return rp, rn


def check_morphed(got, bind, d, weights, what=""):
    """the device's morphed triangles (no skin) against `reference` by the bounds above; zero bind normals stay zero; texture coordinates
    bit-equal.  Returns the worst ratios (error / bound)."""
    ref = reference(bind, d, weights)
    assert ref["active"] > 0, "with no active target the result is the bind copy, bit for bit: compare bytes"
    assert float(ref["cond"].max()) <= 8.0, (what, "the test's own normals are ill-conditioned", float(ref["cond"].max()))
    gp, gn = K.corner_positions(got).astype(np.float64), K.corner_normals(got).astype(np.float64)
    bound_p, bound_n = bounds(ref)
    _texcoords_equal(got, bind, what)
    return _hold(np.abs(gp - ref["pos"]), bound_p, np.max(np.abs(gn - ref["normal"]), axis=1), bound_n, ref["zero"], gn, what, float(ref["cond"].max()))


def _abs_cof(a):
    out = np.empty_like(a)
    for r in range(3):
        for s in range(3):
            r1, r2, s1, s2 = (r + 1) % 3, (r + 2) % 3, (s + 1) % 3, (s + 2) % 3
            out[:, r, s] = a[:, r1, s1] * a[:, r2, s2] + a[:, r1, s2] * a[:, r2, s1]
    return out


def _cof(m):
    c = np.empty_like(m)
    for r in range(3):
        for s in range(3):
            r1, r2, s1, s2 = (r + 1) % 3, (r + 2) % 3, (s + 1) % 3, (s + 2) % 3
            c[:, r, s] = m[:, r1, s1] * m[:, r2, s2] - m[:, r1, s2] * m[:, r2, s1]
    return c


def check_morphed_and_posed(got, bind, d, weights, corners, pal, what=""):
    """the device's triangles after morph + skin against float64: skin_cases.reference's rule (restated here because it has to start from
    the float64 (p', n'), which no 96-byte triangle holds) over the exact morph, by the morph+skin bounds above.  corners: as
    nxhip_set_blas_skin stores them (pod.normalise_skin_corners)."""
    ref = reference(bind, d, weights)
    assert ref["active"] > 0 and float(ref["cond"].max()) <= 8.0, (what, float(ref["cond"].max()))
    mb_p, mb_n = bounds(ref)
    J = np.asarray(pal, np.float64).reshape(-1, 3, 4)
    w = corners["weight"].astype(np.float64)
    jt = corners["joint"].astype(np.int64)
    p1 = np.concatenate([ref["pos"], np.ones((len(w), 1))], 1)
    M = np.einsum("ck,ckrs->crs", w, J[jt])
    pos = np.einsum("crs,cs->cr", M, p1)
    A = np.einsum("ck,ckrs,cs->cr", w, np.abs(J[jt]), np.abs(p1))
    M3 = M[:, :, :3]
    bound_p = gamma(8) * A + np.einsum("crs,cs->cr", np.abs(M3), mb_p)
    n1 = ref["normal"]
    V = np.einsum("crs,cs->cr", _cof(M3), n1)
    V[np.linalg.det(M3) < 0] *= -1.0
    ac = _abs_cof(np.abs(M3))
    T = np.einsum("crs,cs->cr", ac, np.abs(n1))
    zero = np.all(n1 == 0, axis=1)
    Vn = np.where(np.linalg.norm(V, axis=1) > 0, np.linalg.norm(V, axis=1), 1.0)
    unit = np.where(zero[:, None], 0.0, V / Vn[:, None])
    cond = np.where(zero, 0.0, np.linalg.norm(T, axis=1) / Vn)
    assert float(cond.max()) <= 8.0, (what, "the posed normals are ill-conditioned", float(cond.max()))
    carried = np.linalg.norm(np.einsum("crs,c->cr", ac, mb_n), axis=1) / Vn
    bound_n = 2.0 * gamma(16) * cond + 4.0 * U + 2.0 * carried
    gp, gn = K.corner_positions(got).astype(np.float64), K.corner_normals(got).astype(np.float64)
    _texcoords_equal(got, bind, what)
    return _hold(np.abs(gp - pos), bound_p, np.max(np.abs(gn - unit), axis=1), bound_n, zero, gn, what, float(cond.max()))
