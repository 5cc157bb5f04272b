"""Geometric ground truth in numpy float64 for tests/test_geometry_pins.py.

It shares no text with the kernels or the oracle: it imports neither tests.oracle_lib nor any product builder, walks no tree and
uses no inverse matrix for intersections.  Every instance's vertices go FORWARD through its `transform` (widened to float64), and
rays are intersected with those world-space triangles by brute force.

* World.closest: Moeller-Trumbore over all world triangles; per ray the winner's t, (instance, triangle), the runner-up's t and the
  affine weights w0, w1, w2 of the hit point with respect to the winner's WORLD vertices, solved from [P0 P1 P2; 1 1 1] w = [X; 1]
  (not taken from the intersection's own u, v: which weight belongs to which vertex is then independent of any intersection code).
* World.occluded: is there a triangle with 0 < t < tmax, and how close (relatively) any crossing comes to tmax.
* World.texcoord / World.normal: attributes at a hit from those weights; the normal goes through inv(M3)^T (float64 numpy inverse),
  negated when inv(M3)^T cross(p1 - p0, p2 - p0) looks along the ray.
* texture: wrap addressing, exact bilinear weights, texel centres at +0.5, RGB decoded by the IEC 61966-2-1 formula.
* latlong: direction -> (u, v) of the equirectangular map, u = (atan2(z, x) + pi) / (2 pi), v = 1 - (asin(y) + pi / 2) / pi.

Margins (a float32 rounding must not be able to flip an id or a hit into a miss): a ray is `unclear` if the runner-up lies within
MARGIN relative of the winner, or if it crosses the plane of any triangle at or in front of the winner (any triangle, for a miss) within
MARGIN of one of that triangle's edges in affine weight — this contains "a weight of the winner below MARGIN" and also covers the
near-misses; for the shadow test, if a crossing lies within MARGIN relative of tmax.
"""
import numpy as np

MARGIN = 1e-3
MISS = np.inf


def _f64(a):
    return np.asarray(a, np.float64)


class World:
    def __init__(self, meshes, mesh_of_instance, transforms):
        """meshes: triangle record arrays (pos0..2, normal0..2, texCoord0..2); transforms: (n, 16) row-major 4 x 4, translation in
        the last column"""
        self.meshes = meshes
        self.mesh_of_instance = np.asarray(mesh_of_instance, np.int64)
        self.M = _f64(transforms).reshape(-1, 4, 4)
        P, inst, tri = [], [], []
        for i, (b, M) in enumerate(zip(self.mesh_of_instance, self.M)):
            m = meshes[int(b)]
            obj = np.stack([_f64(m["pos0"]), _f64(m["pos1"]), _f64(m["pos2"])], axis=1)  # (T, 3 vertices, 3)
            P.append(obj @ M[:3, :3].T + M[:3, 3])
            inst.append(np.full(len(m), i, np.int64))
            tri.append(np.arange(len(m), dtype=np.int64))
        self.P = np.concatenate(P)
        self.inst = np.concatenate(inst)
        self.tri = np.concatenate(tri)

    def _crossings(self, rays, chunk=256):
        """per chunk of rays: (slice, t, u, v) each (rays, triangles), nan / inf where the ray is parallel to the plane"""
        P0 = self.P[:, 0]
        e1 = self.P[:, 1] - P0
        e2 = self.P[:, 2] - P0
        o_all, d_all = _f64(rays["origin"]), _f64(rays["direction"])
        for a in range(0, len(o_all), chunk):
            sl = slice(a, min(len(o_all), a + chunk))
            o, d = o_all[sl, None, :], d_all[sl, None, :]
            with np.errstate(divide="ignore", invalid="ignore"):
                pvec = np.cross(d, e2[None])
                inv = 1.0 / np.einsum("tk,rtk->rt", e1, pvec)
                s = o - P0[None]
                u = np.einsum("rtk,rtk->rt", s, pvec) * inv
                q = np.cross(s, e1[None])
                v = np.einsum("rtk,rtk->rt", np.broadcast_to(d, q.shape), q) * inv
                t = np.einsum("tk,rtk->rt", e2, q) * inv
            yield sl, t, u, v

    def closest(self, rays):
        n = len(rays)
        out = dict(t=np.full(n, MISS), t2=np.full(n, MISS), index=np.full(n, -1, np.int64), unclear=np.zeros(n, bool))
        for sl, t, u, v in self._crossings(rays):
            with np.errstate(invalid="ignore"):
                inside = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
                edge = np.minimum(np.minimum(u, v), 1.0 - u - v)
                th = np.where(inside, t, MISS)
                order = np.argsort(th, axis=1)[:, :2]
                rows = np.arange(th.shape[0])
                t1, t2 = th[rows, order[:, 0]], th[rows, order[:, 1]]
                near_edge = (np.abs(edge) < MARGIN) & (t > 0) & (t <= (t1 * (1.0 + MARGIN))[:, None])
            out["t"][sl], out["t2"][sl] = t1, t2
            out["index"][sl] = np.where(np.isfinite(t1), order[:, 0], -1)
            out["unclear"][sl] = near_edge.any(axis=1) | (np.isfinite(t1) & (t2 <= t1 * (1.0 + MARGIN)))
        hit = out["index"] >= 0
        k = np.where(hit, out["index"], 0)
        out["hit"] = hit
        out["inst"] = np.where(hit, self.inst[k], -1)
        out["tri"] = np.where(hit, self.tri[k], -1)
        # the affine weights of X = o + t d in the winner's world triangle: four equations, three unknowns, least squares
        X = _f64(rays["origin"]) + np.where(hit, out["t"], 0.0)[:, None] * _f64(rays["direction"])
        A = np.concatenate([np.swapaxes(self.P[k], 1, 2), np.ones((n, 1, 3))], axis=1)  # (n, 4, 3): columns are the vertices
        b = np.concatenate([X, np.ones((n, 1))], axis=1)
        w = np.einsum("nij,nj->ni", np.linalg.pinv(A), b)
        out["w"] = np.where(hit[:, None], w, 0.0)
        out["unclear"] |= hit & (out["w"].min(axis=1) < MARGIN)
        return out

    def occluded(self, rays, tmax):
        """(occluded, unclear): is some triangle crossed at 0 < t < tmax; unclear: a crossing within MARGIN relative of tmax, or a
        plane crossed before tmax within MARGIN of a triangle's edge"""
        tmax = _f64(tmax)
        occ = np.zeros(len(rays), bool)
        unclear = np.zeros(len(rays), bool)
        nearest = np.full(len(rays), np.inf)
        for sl, t, u, v in self._crossings(rays):
            tm = tmax[sl, None]
            with np.errstate(invalid="ignore"):
                inside = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
                edge = np.minimum(np.minimum(u, v), 1.0 - u - v)
                rel = np.where(inside, np.abs(t - tm) / tm, np.inf)
                near_edge = (np.abs(edge) < MARGIN) & (t > 0) & (t <= tm * (1.0 + MARGIN))
            occ[sl] = (inside & (t < tm)).any(axis=1)
            nearest[sl] = rel.min(axis=1)
            unclear[sl] = near_edge.any(axis=1) | (nearest[sl] < MARGIN)
        return occ, unclear, nearest

    def _attribute(self, res, name):
        k = np.where(res["hit"], res["index"], 0)
        out = 0.0
        for c in range(3):
            vals = np.concatenate([_f64(self.meshes[int(b)]["%s%d" % (name, c)]) for b in self.mesh_of_instance])[k]
            out = out + res["w"][:, c:c + 1] * vals
        return out

    def texcoord(self, res):
        return self._attribute(res, "texCoord")

    def normal(self, res, rays):
        """normalize(inv(M3)^T sum w_k normal_k), negated when inv(M3)^T cross(p1 - p0, p2 - p0) looks along the ray; 0 for a miss"""
        i = np.where(res["hit"], res["inst"], 0)
        NT = np.swapaxes(np.linalg.inv(self.M[:, :3, :3]), 1, 2)[i]  # inv(M3)^T per ray
        n = np.einsum("nij,nj->ni", NT, self._attribute(res, "normal"))
        k = np.where(res["hit"], res["index"], 0)
        pos = [np.concatenate([_f64(self.meshes[int(b)]["pos%d" % c]) for b in self.mesh_of_instance])[k] for c in range(3)]
        g = np.einsum("nij,nj->ni", NT, np.cross(pos[1] - pos[0], pos[2] - pos[0]))
        with np.errstate(invalid="ignore", divide="ignore"):
            n = n / np.linalg.norm(n, axis=1, keepdims=True)
        along = np.einsum("ni,ni->n", g, _f64(rays["direction"])) > 0
        n = np.where(along[:, None], -n, n)
        return np.where(res["hit"][:, None], n, 0.0)


def srgb_decode(c8):
    """IEC 61966-2-1: 8-bit code -> linear"""
    x = _f64(c8) / 255.0
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def texture(img, u, v):
    """img (H, W, 4) uint8 -> linear RGB (n, 3) at normalised (u, v): wrap, bilinear, texel centres at +0.5"""
    img = np.asarray(img)
    H, W = img.shape[:2]
    lin = srgb_decode(img[..., 0:3])
    x = _f64(u) * W - 0.5
    y = _f64(v) * H - 0.5
    i0 = np.floor(x)
    j0 = np.floor(y)
    ax = (x - i0)[:, None]
    ay = (y - j0)[:, None]
    i0 = i0.astype(np.int64)
    j0 = j0.astype(np.int64)
    ia, ib = i0 % W, (i0 + 1) % W
    ja, jb = j0 % H, (j0 + 1) % H
    top = lin[ja, ia] * (1.0 - ax) + lin[ja, ib] * ax
    bot = lin[jb, ia] * (1.0 - ax) + lin[jb, ib] * ax
    return top * (1.0 - ay) + bot * ay


def latlong(d):
    d = _f64(d)
    theta = np.arctan2(d[:, 2], d[:, 0])
    phi = np.arcsin(np.clip(d[:, 1], -1.0, 1.0))
    return (theta + np.pi) / (2.0 * np.pi), 1.0 - (phi + np.pi / 2.0) / np.pi
