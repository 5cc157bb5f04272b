"""Float64 restatement of the detail maps' shading rule (include/nexus_hip.h, nxhip_set_material_detail) and of tex2d_linear.

Written from the contract, not from the kernels.  Everything is binary64 except what the contract fixes in binary32 because it DECIDES
something discrete: the hit's texture coordinates (bary2 of the material kernels) and the lookup's addressing and 1/256 weights — a
coordinate a rounding away from a weight step would otherwise move the result by a 256th of a texel difference, which is no rounding
error.  The blend of the four taps, the frame and the normal are binary64."""
import numpy as np

MAT_DIFFUSE, MAT_DIELECTRIC, MAT_PLASTIC, MAT_CONDUCTOR = 0, 1, 2, 3

f32 = np.float32


def hit_texcoord(uv0, uv1, uv2, hu, hv):
    """the material kernels' bary2 in binary32, one rounding per operation: w = 1 - u - v; u t1 + v t2 + w t0 per component"""
    uv0, uv1, uv2 = (np.asarray(a, f32) for a in (uv0, uv1, uv2))
    hu, hv = np.asarray(hu, f32)[..., None], np.asarray(hv, f32)[..., None]
    w = (f32(1.0) - hu) - hv
    return ((hu * uv1) + (hv * uv2)) + (w * uv0)


def tex2d_linear(img, u, v):
    """img: H x W x 4 uint8; u, v: binary32 coordinates.  Wrap addressing, texel centres at +0.5, bilinear weights rounded to 1/256,
    every channel byte / 255: (..., 4) float64"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    xb, yb = u * f32(W) - f32(0.5), v * f32(H) - f32(0.5)
    fx, fy = np.floor(xb), np.floor(yb)
    ax = (np.floor((xb - fx) * f32(256.0) + f32(0.5)) * f32(1.0 / 256.0)).astype(np.float64)[..., None]
    ay = (np.floor((yb - fy) * f32(256.0) + f32(0.5)) * f32(1.0 / 256.0)).astype(np.float64)[..., None]
    i0, i1 = np.mod(fx.astype(np.int64), W), np.mod(fx.astype(np.int64) + 1, W)
    j0, j1 = np.mod(fy.astype(np.int64), H), np.mod(fy.astype(np.int64) + 1, H)
    t = img.astype(np.float64) / 255.0
    top = t[j0, i0] + ax * (t[j0, i1] - t[j0, i0])
    bot = t[j1, i0] + ax * (t[j1, i1] - t[j1, i0])
    return top + ay * (bot - top)


def _unit(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / np.sqrt((a * a).sum(-1))[..., None]


def _dot(a, b):
    return (a * b).sum(-1)


def shading_frame(tris, hit_uv, ray_dir, transform, inv_transform, mat_type, normal_map=None, normal_scale=1.0, roughness=0.0, roughness_map=None):
    """tris: records with pos0..2, normal0..2, texCoord0..2 (pod.TRI_DT rows, one per hit); hit_uv: (n, 2) barycentrics of the hit record;
    ray_dir: (n, 3); transform / inv_transform: 4 x 4 row-major, object to world and back.  Returns a dict:
      ns         world-space shading normal after fallback and flip          N        the interpolated normal after the flip
      fell_back  a normal map was named and the result went back to N        roughness  what the BSDF receives
    and what the tests' exclusions look at: det, tangent_sine (sine of the angle between the world tangent and N), ns_dot_v, n_dot_v
    (of the candidate ns and of N, before the flip; nan where there is no candidate)."""
    n = len(hit_uv)
    hu, hv = np.asarray(hit_uv, np.float64)[:, 0], np.asarray(hit_uv, np.float64)[:, 1]
    d = np.asarray(ray_dir, np.float64).reshape(n, 3)
    M = np.asarray(transform, np.float64).reshape(4, 4)[:3, :3]
    IT = np.asarray(inv_transform, np.float64).reshape(4, 4)[:3, :3]
    p0, p1, p2 = (np.asarray(tris["pos%d" % k], np.float64).reshape(n, 3) for k in range(3))
    n0, n1, n2 = (np.asarray(tris["normal%d" % k], np.float64).reshape(n, 3) for k in range(3))
    w = 1.0 - hu - hv
    N = _unit((n1 * hu[:, None] + n2 * hv[:, None] + n0 * w[:, None]) @ IT)  # (IT^T n as a row vector: n @ IT)
    g = _unit(np.cross(p1 - p0, p2 - p0) @ IT)
    uv0, uv1, uv2 = (np.asarray(tris["texCoord%d" % k], f32).reshape(n, 2) for k in range(3))
    tex = hit_texcoord(uv0, uv1, uv2, hu, hv)
    rough = np.full(n, float(roughness))
    if roughness_map is not None:
        rough = float(f32(roughness)) * tex2d_linear(roughness_map, tex[:, 0], tex[:, 1])[:, 1]
    out = {"det": np.full(n, np.nan), "tangent_sine": np.full(n, np.nan), "ns_dot_v": np.full(n, np.nan), "n_dot_v": -_dot(N, d)}
    ns = N.copy()
    fell = np.zeros(n, bool)
    if normal_map is not None:
        c = tex2d_linear(normal_map, tex[:, 0], tex[:, 1])
        s = float(normal_scale)
        m = np.stack([(2.0 * c[:, 0] - 1.0) * s, (2.0 * c[:, 1] - 1.0) * s, 2.0 * c[:, 2] - 1.0], 1)
        a0, a1, a2 = (a.astype(np.float64) for a in (uv0, uv1, uv2))
        du1, dv1, du2, dv2 = a1[:, 0] - a0[:, 0], a1[:, 1] - a0[:, 1], a2[:, 0] - a0[:, 0], a2[:, 1] - a0[:, 1]
        det = du1 * dv2 - du2 * dv1
        sg = np.where(det < 0, -1.0, 1.0)
        e1, e2 = p1 - p0, p2 - p0
        Tu = ((e1 * dv2[:, None] - e2 * dv1[:, None]) * sg[:, None]) @ M.T
        Tv = ((e2 * du1[:, None] - e1 * du2[:, None]) * sg[:, None]) @ M.T
        tp = Tu - N * _dot(N, Tu)[:, None]
        tl = np.sqrt(_dot(tp, tp))
        with np.errstate(invalid="ignore", divide="ignore"):
            t = tp / tl[:, None]
            b = np.cross(N, t)
            b = np.where((_dot(b, -Tv) >= 0)[:, None], b, -b)
            raw = t * m[:, 0:1] + b * m[:, 1:2] + N * m[:, 2:3]
            rl = np.sqrt(_dot(raw, raw))
            cand = raw / rl[:, None]
            ok = (np.abs(det) > 0) & np.isfinite(tl) & (tl > 0) & np.isfinite(rl) & (rl > 0) & np.isfinite(cand).all(1)
            horizon = _dot(cand, -d) * _dot(N, -d)
            ok &= horizon > 0
            out["tangent_sine"] = tl / np.sqrt(_dot(Tu, Tu))
        out["det"], out["ns_dot_v"] = det, _dot(cand, -d)
        ns = np.where(ok[:, None], cand, N)
        fell = ~ok
    flip = (_dot(g, d) > 0) & (mat_type != MAT_DIELECTRIC)
    sign = np.where(flip, -1.0, 1.0)[:, None]
    out.update(ns=ns * sign, N=N * sign, gNormal=g * sign, fell_back=fell, roughness=rough, texcoord=tex)
    return out
