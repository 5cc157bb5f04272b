"""Float64 brute force of the alpha-test rule (include/nexus_hip.h, nxhip_set_material_alpha), built on tests/transmittance_reference.py
(intersect, bilinear_alpha, clamp_opacity).  Reads no product code.

A ray (o, d, tmax) against a list of SURFACES — one per instance: world-space triangles with texture coordinates, an opacity, optionally
an RGBA8 map, and an alpha mode with its cutoff.  Moeller-Trumbore on every triangle; a triangle with 0 < t < tmax and u >= 0, v >= 0,
u + v <= 1 is a crossing, and s = o a as in the transmittance contract.  Then

    MASK    s < cutoff: the crossing does not exist, for any ray.  Otherwise it is solid.
    OPAQUE  the crossing is solid: alpha is not looked at.
    BLEND   the crossing is what it was: a hit for the closest-hit search, an occlusion for a plain shadow ray, a factor 1 - s for a
            shadow ray that carries a transmittance.

and the answers are: the closest surviving crossing (t, u, v, triangle, instance), occlusion (some surviving crossing), and T — 0 where
a solid crossing survives, else the product of 1 - s over the BLEND crossings.

A ray is `unclear`, and left out by the caller, when a binary32 implementation may decide a crossing the other way: a barycentric within
EDGE of an edge, t within EDGE (relative) of 0 or tmax (the conditions of the transmittance reference), |s - cutoff| < CUTOFF on a MASK
crossing, or a weight argument frac 256 + 0.5 within WEIGHT of an integer on a crossing whose alpha is read (not OPAQUE) and whose four
texels do not all hold one alpha — where they do, the weight multiplies an exact zero in every format and cannot matter."""
import numpy as np

from tests import transmittance_reference as R

BLEND, MASK, OPAQUE = 0, 1, 2
EDGE, WEIGHT = R.EDGE, R.WEIGHT
CUTOFF = 1e-4
MAX_LEFT_OUT = 1e-3  # the project's bar for such shares


class Surface(R.Surface):
    def __init__(self, positions, uvs, opacity=1.0, rgba8=None, mode=BLEND, cutoff=0.5):
        super().__init__(positions, uvs, opacity, rgba8)
        self.mode, self.cutoff = int(mode), float(cutoff)


def _footprint_uniform(rgba8, s, t, dtype):
    """do the four texels of the bilinear footprint at (s, t) hold one alpha?"""
    H, W = rgba8.shape[:2]
    x, y = np.asarray(s, dtype) * dtype(W) - dtype(0.5), np.asarray(t, dtype) * dtype(H) - dtype(0.5)
    fx, fy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    a = rgba8[..., 3]
    i0, i1, j0, j1 = np.mod(fx, W), np.mod(fx + 1, W), np.mod(fy, H), np.mod(fy + 1, H)
    return (a[j0, i0] == a[j0, i1]) & (a[j0, i0] == a[j1, i0]) & (a[j0, i0] == a[j1, i1])


def trace(o, d, tmax, surfaces, dtype=np.float64):
    """dict over the N rays: t, u, v (dtype; t = inf on a miss), tri, inst (int64, -1 on a miss) of the closest surviving crossing;
    occluded (bool); T (dtype); crossings / rejected (int64: geometric crossings, and those a MASK took away); unclear (bool)"""
    o, d = np.asarray(o, dtype), np.asarray(d, dtype)
    tmax = np.broadcast_to(np.asarray(tmax, dtype), (len(o),))
    N = len(o)
    one = dtype(1.0)
    best = {"t": np.full(N, np.inf, dtype), "u": np.zeros(N, dtype), "v": np.zeros(N, dtype), "tri": np.full(N, -1, np.int64), "inst": np.full(N, -1, np.int64)}
    occluded, unclear = np.zeros(N, bool), np.zeros(N, bool)
    T = np.ones(N, dtype)
    crossings, rejected = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for si, S in enumerate(surfaces):
        op = dtype(R.clamp_opacity(S.opacity))
        for ti, (P, UV) in enumerate(zip(S.positions, S.uvs)):
            t, u, v = R.intersect(o, d, P[0], P[1], P[2], dtype)
            with np.errstate(invalid="ignore"):
                hit = ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) & (t > 0) & (t < tmax)
                w = one - u - v
                finite = np.isfinite(tmax)
                lim = np.where(finite, tmax, dtype(0.0))
                band = (np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(w)) < EDGE) & (u > -EDGE) & (v > -EDGE) & (w > -EDGE) & (t > -EDGE * lim) & (~finite | (t < lim * (1 + EDGE)))
                ends = ((np.abs(t) < EDGE * np.where(finite, lim, np.abs(t) + 1)) | (finite & (np.abs(t - lim) < EDGE * lim))) & (u > -EDGE) & (v > -EDGE) & (w > -EDGE)
            unclear |= band | ends
            a = np.ones(N, dtype)
            if S.rgba8 is not None and S.mode != OPAQUE:
                UVd = np.asarray(UV, dtype)
                st = u[:, None] * UVd[1][None, :] + v[:, None] * UVd[2][None, :] + w[:, None] * UVd[0][None, :]
                safe = np.where(hit[:, None], st, dtype(0.0))
                a, ax, ay = R.bilinear_alpha(S.rgba8, safe[:, 0], safe[:, 1], dtype)
                near = (np.abs(ax - np.round(ax)) < WEIGHT) | (np.abs(ay - np.round(ay)) < WEIGHT)
                unclear |= hit & near & ~_footprint_uniform(S.rgba8, safe[:, 0], safe[:, 1], dtype)
            s = op * a
            survives = hit
            if S.mode == MASK:
                unclear |= hit & (np.abs(s - dtype(S.cutoff)) < CUTOFF)
                survives = hit & ~(s < dtype(S.cutoff))
                rejected += hit & ~survives
            crossings += hit
            occluded |= survives
            if S.mode == BLEND:
                T = np.where(survives, T * (one - s), T)
            else:
                T = np.where(survives, dtype(0.0), T)
            closer = survives & (t < best["t"])
            for k, val in (("t", t), ("u", u), ("v", v)):
                best[k] = np.where(closer, val, best[k])
            best["tri"] = np.where(closer, ti, best["tri"])
            best["inst"] = np.where(closer, si, best["inst"])
    out = dict(best)
    out.update(occluded=occluded, T=T, crossings=crossings, rejected=rejected, unclear=unclear)
    return out


def both(o, d, tmax, surfaces):
    """the rule in float64 and in binary32 on the same (binary32) inputs: (r64, r32)"""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    tmax = np.asarray(tmax, np.float32)
    return trace(o.astype(np.float64), d.astype(np.float64), tmax.astype(np.float64), surfaces), trace(o, d, tmax, surfaces, dtype=np.float32)


def kept(r64, r32=None):
    """the rays that count: neither run calls them unclear"""
    keep = ~r64["unclear"]
    return keep & ~r32["unclear"] if r32 is not None else keep


def record_deviation(r64, r32, keep):
    """worst |t|, |u|, |v| deviation of the binary32 run from the float64 run among the kept rays on which both name the same crossing"""
    same = keep & (r64["tri"] == r32["tri"]) & (r64["inst"] == r32["inst"]) & (r64["tri"] >= 0)
    return {k: float(np.abs(r32[k][same].astype(np.float64) - r64[k][same]).max()) if same.any() else 0.0 for k in ("t", "u", "v")}, same
