"""Float64 brute force of the shadow-ray transmittance contract (include/nexus_hip.h, nxhip_set_shadow_transmittance).  Reads no product code.

A ray (o, d, tmax) against a list of SURFACES — world-space triangles with texture coordinates, one opacity and, optionally, one RGBA8 map
per surface: Moeller-Trumbore on every triangle; a triangle with 0 < t < tmax and u >= 0, v >= 0, u + v <= 1 is a crossing;

    T = prod over the crossings of (1 - o a),   o = the opacity clamped to [0, 1] (not below 1, a NaN included: 1),
                                                a = 1 without a map, else the map's bilinear alpha at (1 - u - v) uv0 + u uv1 + v uv2.

The bilinear lookup, by its DEFINITION (normalised coordinates; texel centres at +0.5; wrap on both axes; row 0 first; fractional weights
rounded to 1/256): x = s W - 0.5, i = floor(x), w = floor((x - i) 256 + 0.5) / 256, likewise in t with H; the value is the two-step
lerp top = a[j, i] + w_x (a[j, i+1] - a[j, i]), bottom likewise in row j + 1, top + w_y (bottom - top), indices modulo W and H, alpha as
byte / 255.

Every function takes `dtype`: float64 is the reference; float32 runs the same rule in binary32, rounding after every operation, which is
what the tolerance of a binary32 implementation is derived from (deviation, below) — never from the implementation's own results."""
import numpy as np


class Surface:
    def __init__(self, positions, uvs, opacity=1.0, rgba8=None):
        """positions (n, 3, 3) world space, uvs (n, 3, 2), rgba8 (H, W, 4) uint8 or None"""
        self.positions = np.asarray(positions, np.float64)
        self.uvs = np.asarray(uvs, np.float64)
        self.opacity = float(opacity)
        self.rgba8 = None if rgba8 is None else np.ascontiguousarray(rgba8, np.uint8)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def intersect(o, d, p0, p1, p2, dtype=np.float64):
    """Moeller-Trumbore, rays (N, 3) against ONE triangle: t, u, v (N,) — u belongs to p1, v to p2"""
    o, d = np.asarray(o, dtype), np.asarray(d, dtype)
    p0, e0, e1 = np.asarray(p0, dtype), np.asarray(p1, dtype) - np.asarray(p0, dtype), np.asarray(p2, dtype) - np.asarray(p0, dtype)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = _cross(d, e1[None, :])
        inv = dtype(1.0) / _dot(e0[None, :], q)
        s = o - p0[None, :]
        u = inv * _dot(s, q)
        r = _cross(s, e0[None, :])
        v = inv * _dot(d, r)
        t = inv * _dot(e1[None, :], r)
    return t, u, v


def bilinear_alpha(rgba8, s, t, dtype=np.float64, channel=3):
    """the map's bilinear value of `channel` as byte / 255 at normalised (s, t); also the two weight arguments frac 256 + 0.5"""
    H, W = rgba8.shape[:2]
    s, t = np.asarray(s, dtype), np.asarray(t, dtype)
    a = rgba8[..., channel].astype(dtype) / dtype(255.0)
    x, y = s * dtype(W) - dtype(0.5), t * dtype(H) - dtype(0.5)
    fx, fy = np.floor(x), np.floor(y)
    argx, argy = (x - fx) * dtype(256.0) + dtype(0.5), (y - fy) * dtype(256.0) + dtype(0.5)
    wx, wy = np.floor(argx) * dtype(1.0 / 256.0), np.floor(argy) * dtype(1.0 / 256.0)
    i0, i1 = np.mod(fx.astype(np.int64), W), np.mod(fx.astype(np.int64) + 1, W)
    j0, j1 = np.mod(fy.astype(np.int64), H), np.mod(fy.astype(np.int64) + 1, H)
    top = a[j0, i0] + wx * (a[j0, i1] - a[j0, i0])
    bot = a[j1, i0] + wx * (a[j1, i1] - a[j1, i0])
    return top + wy * (bot - top), argx, argy


def clamp_opacity(o):
    return 1.0 if not (o < 1.0) else max(o, 0.0)


EDGE = 1e-5     # a barycentric this close to an edge, t this close (relative) to 0 or tmax: the crossing may go either way in binary32
WEIGHT = 1e-3   # a weight argument frac 256 + 0.5 this close to an integer: the 1/256 weight may round either way

# what a wrong implementation would do (tests/test_transmittance_reference.py: the checker refuses each)
VARIANTS = ("drop", "union", "mirror_v", "red")


def transmittance(o, d, tmax, surfaces, dtype=np.float64, variant=None):
    """dict: T (N,), crossed (N,) the number of crossings, unclear (N,) bool — see EDGE and WEIGHT"""
    o, d = np.asarray(o, dtype), np.asarray(d, dtype)
    tmax = np.asarray(tmax, dtype)
    N = len(o)
    T = np.ones(N, dtype)
    crossed = np.zeros(N, np.int64)
    unclear = np.zeros(N, bool)
    one = dtype(1.0)
    for S in surfaces:
        op = dtype(clamp_opacity(S.opacity))
        for P, UV in zip(S.positions, S.uvs):
            t, u, v = intersect(o, d, P[0], P[1], P[2], dtype)
            with np.errstate(invalid="ignore"):
                hit = ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) & (t > 0) & (t < tmax)
                # near misses and near hits alike: inside a band around the triangle's edges or the ray's ends
                w = one - u - v
                band = (np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(w)) < EDGE) & (u > -EDGE) & (v > -EDGE) & (w > -EDGE) & (t > -EDGE * tmax) & (t < tmax * (1 + EDGE))
                ends = ((np.abs(t) < EDGE * tmax) | (np.abs(t - tmax) < EDGE * tmax)) & (u > -EDGE) & (v > -EDGE) & (w > -EDGE)
            unclear |= band | ends
            a = np.ones(N, dtype)
            if S.rgba8 is not None:
                UVd = np.asarray(UV, dtype)
                st = u[:, None] * UVd[1][None, :] + v[:, None] * UVd[2][None, :] + (one - u - v)[:, None] * UVd[0][None, :]
                tt = one - st[:, 1] if variant == "mirror_v" else st[:, 1]  # (the map read upside down)
                with np.errstate(invalid="ignore"):
                    safe = np.where(hit[:, None], np.stack([st[:, 0], tt], 1), dtype(0.0))
                a, ax, ay = bilinear_alpha(S.rgba8, safe[:, 0], safe[:, 1], dtype, channel=0 if variant == "red" else 3)
                near = (np.abs(ax - np.round(ax)) < WEIGHT) | (np.abs(ay - np.round(ay)) < WEIGHT)
                unclear |= hit & near
            s = op + a - op * a if variant == "union" else op * a
            if variant == "drop":  # one crossing dropped on 1 % of the rays: the first one of every hundredth ray
                drop = hit & (crossed == 0) & (np.arange(N) % 100 == 7)
                crossed += drop  # (counted, not multiplied)
                hit = hit & ~drop
            T = np.where(hit, T * (one - s), T)
            crossed += hit
    return {"T": T, "crossed": crossed, "unclear": unclear}


def deviation(o, d, tmax, surfaces):
    """the same rule in binary32 against float64 on the same (binary32) inputs: |T32 - T64| per ray, and the float64 result; rays either
    side calls unclear are not counted by the caller"""
    o, d, tmax = np.asarray(o, np.float32), np.asarray(d, np.float32), np.asarray(tmax, np.float32)
    r64 = transmittance(o.astype(np.float64), d.astype(np.float64), tmax.astype(np.float64), surfaces)
    r32 = transmittance(o, d, tmax, surfaces, dtype=np.float32)
    return np.abs(r32["T"].astype(np.float64) - r64["T"]), r64, r32


def check(got, ref, tolerance, max_unclear=0.02, what="transmittance"):
    """Does `got` (N,) agree with the reference's dict?  Exactly 0.0 where the reference is exactly 0 (an opaque crossing, or o a = 1),
    exactly 1.0 where nothing was crossed, within `tolerance` elsewhere; unclear rays are left out, and may be at most `max_unclear` of
    all.  Returns (ok, text)."""
    got = np.asarray(got, np.float64)
    keep = ~ref["unclear"]
    share = 1.0 - keep.mean()
    zero, clear = keep & (ref["T"] == 0.0), keep & (ref["crossed"] == 0)
    rest = keep & ~zero & ~clear
    dev = np.abs(got - ref["T"])
    worst = dev[rest].max() if rest.any() else 0.0
    bad_zero, bad_one = int((got[zero] != 0.0).sum()), int((got[clear] != 1.0).sum())
    text = ("%s: %d rays, %.2f %% left out as unclear; %d must be exactly 0 (%d are not), %d exactly 1 (%d are not); %d others, worst deviation %.3g (tolerance %.3g)"
            % (what, len(got), 100.0 * share, zero.sum(), bad_zero, clear.sum(), bad_one, rest.sum(), worst, tolerance))
    ok = share <= max_unclear and bad_zero == 0 and bad_one == 0 and worst <= tolerance and bool(np.all(np.isfinite(got)))
    return ok, text
