"""References for the feature buffers (AOVs) and the edge-avoiding a-trous filter, shared by tests/test_aov.py (CPU) and the GPU tests.

* primary_rays: generate_kernel's ray of a pinhole or thin-lens camera, restated in numpy float32 in the kernel's order of operations
  (jitter and lens point from the oracle's orc_rng_init_pixel / orc_rand; an fmaf is a float64 product-sum rounded once to float32).
* primary_features: albedo + coverage and depth from the ORACLE's hit record of that ray (exact values: the device must give the same
  bits) and the shading normal recomputed from the hit record in a dtype of the caller's choice.
* atrous: the filter of include/nexus_hip.h (nxhip_denoise) in numpy — float64 as the definition is written, or float32 in the
  kernel's order of operations (what the tolerance of the device comparison is derived from).
"""
import ctypes as C

import numpy as np

from nexus_amd import pod
from tests import oracle_lib as O

f32 = np.float32
FLT_MAX = np.float32(3.402823466e38)


def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def primary_rays(cam, W, H, frame):
    """The rays generate_kernel makes for frame `frame`, row-major over the image: pinhole or thin lens (unit_disk's rejection loop on the
    oracle's random numbers, the lens offset right * rdx + up * rdy added to the origin and taken off the direction).  Both are held
    against the float64 camera of tests/camera_reference.py by tests/test_camera_reference.py."""
    L = O.lib()
    n = W * H
    lens_radius = f32(cam["lensRadius"])
    xs = np.empty(n, f32)
    ys = np.empty(n, f32)
    disk = np.zeros((n, 2), f32)
    for g in range(n):
        j, i = divmod(g, W)
        st = C.c_uint32(L.orc_rng_init_pixel(i, j, W, frame))
        xs[g] = L.orc_rand(C.byref(st))
        ys[g] = L.orc_rand(C.byref(st))
        while True:  # (unit_disk is drawn whatever the lens radius)
            a = f32(L.orc_rand(C.byref(st)))
            b = f32(L.orc_rand(C.byref(st)))
            px = f32(2.0) * (a - f32(0.5))
            py = f32(2.0) * (b - f32(0.5))
            if np.sqrt(px * px + py * py) < f32(1.0):
                break
        disk[g] = (px, py)
    g = np.arange(n)
    i = (g % W).astype(f32)
    j = (g // W).astype(f32)
    x = (i + xs) / f32(W)
    y = (j + ys) / f32(H)
    pos = np.asarray(cam["position"], f32).reshape(3)
    llc = np.asarray(cam["lowerLeftCorner"], f32).reshape(3)
    vx = np.asarray(cam["viewportX"], f32).reshape(3)
    vy = np.asarray(cam["viewportY"], f32).reshape(3)
    right = np.asarray(cam["right"], f32).reshape(3)
    up = np.asarray(cam["up"], f32).reshape(3)
    rdx = lens_radius * disk[:, 0]
    rdy = lens_radius * disk[:, 1]
    offset = right[None, :] * rdx[:, None] + up[None, :] * rdy[:, None]  # (a pinhole: +0 or -0, which changes no bit below)
    d = ((llc[None, :] + vx[None, :] * x[:, None]) + vy[None, :] * y[:, None]) - pos[None, :]
    d = d - offset
    dd = fma32(d[:, 2], d[:, 2], fma32(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))
    inv = f32(1.0) / np.sqrt(dd)
    d = d * inv[:, None]
    rays = np.zeros(n, pod.RAY_DT)
    rays["origin"] = pos[None, :] + offset
    rays["direction"] = d
    return rays


def material_albedo(materials):
    """What the albedo buffer holds for an untextured material: its albedo, (1, 1, 1) for a conductor"""
    base = np.array(materials["u"][:, 0:3], f32)
    base[materials["type"] == pod.MAT_CONDUCTOR] = 1.0
    return base


def _hit_triangles(sc, hits, hit):
    inst = np.where(hit, hits["instanceIdx"], 0).astype(np.int64)
    tri = np.where(hit, hits["triIdx"], 0).astype(np.int64)
    tris = np.zeros(len(hits), pod.TRI_DT)
    for b in np.unique(sc.instances["bvhIdx"][inst]):
        sel = sc.instances["bvhIdx"][inst] == b
        tris[sel] = sc.meshes[int(b)][tri[sel]]
    return inst, tris


def shading_normals(sc, hits, rays, dtype):
    """normalize(IT^T bary(normals)), negated where the geometric normal looks along the ray: shade_path's expression, evaluated in
    `dtype` (float32: with the kernel's fused operations; float64: plainly).  Rows of misses are 0."""
    hit = hits["hitDistance"] < pod.MISS_DISTANCE
    inst, tris = _hit_triangles(sc, hits, hit)
    single = dtype == np.float32
    T = dtype

    def fma(a, b, c):
        return fma32(a, b, c) if single else a * b + c

    def dot(a, b):
        return fma(a[:, 2], b[:, 2], fma(a[:, 1], b[:, 1], a[:, 0] * b[:, 0]))

    def cross(a, b):
        return np.stack([fma(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1])), fma(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2])), fma(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]))], axis=1)

    IT = np.asarray(sc.instances["invTransform"][inst], T).reshape(-1, 16)

    def transposed(v):
        return np.stack([fma(IT[:, 8 + k], v[:, 2], fma(IT[:, 4 + k], v[:, 1], IT[:, k] * v[:, 0])) for k in range(3)], axis=1)

    def normalize(v):
        return v * (T(1.0) / np.sqrt(dot(v, v)))[:, None]

    u = hits["u"].astype(T)[:, None]
    v = hits["v"].astype(T)[:, None]
    w = T(1.0) - u - v
    n0, n1, n2 = (np.asarray(tris[k], T) for k in ("normal0", "normal1", "normal2"))
    p0, p1, p2 = (np.asarray(tris[k], T) for k in ("pos0", "pos1", "pos2"))
    with np.errstate(invalid="ignore", divide="ignore"):
        normal = normalize(transposed((n1 * u + n2 * v) + n0 * w))
        g = normalize(transposed(cross(p1 - p0, p2 - p0)))
        flip = dot(g, np.asarray(rays["direction"], T)) > 0
    normal = np.where(flip[:, None], -normal, normal)
    return np.where(hit[:, None], normal, T(0.0)), flip


def primary_features(sc, W, H, frame):
    """(albedo4 float32, depth float32, hits, rays) of frame `frame`, row-major: albedo + coverage and depth exactly as the device must
    give them (the oracle's closest hit of the restated ray; texture colours through orc_tex2d)."""
    rays = primary_rays(sc.camera, W, H, frame)
    osc = sc.oracle()
    hits = osc.trace_closest(rays)
    hit = hits["hitDistance"] < pod.MISS_DISTANCE
    inst, tris = _hit_triangles(sc, hits, hit)
    mid = sc.instances["materialId"][inst]
    albedo = np.zeros((W * H, 4), f32)
    albedo[:, 0:3] = material_albedo(sc.materials)[mid]
    dmap = sc.materials["diffuseMapId"][mid]
    textured = np.flatnonzero(hit & (dmap >= 0))
    if len(textured):
        u, v = hits["u"], hits["v"]
        w = f32(1.0) - u - v
        t0, t1, t2 = tris["texCoord0"], tris["texCoord1"], tris["texCoord2"]
        tu = u * t1[:, 0] + v * t2[:, 0] + w * t0[:, 0]  # bary2, no fused operations (nx_math.h)
        tv = u * t1[:, 1] + v * t2[:, 1] + w * t0[:, 1]
        out = np.zeros(4, f32)
        for k in textured:
            img = np.ascontiguousarray(sc.diffuse_maps[int(dmap[k])], dtype=np.uint8)
            desc = O._TexDesc(img.shape[1], img.shape[0], O._ptr(img))
            O.lib().orc_tex2d(C.byref(desc), float(tu[k]), float(tv[k]), O._ptr(out))
            albedo[k, 0:3] = out[0:3]
    albedo[:, 3] = 1.0
    albedo[~hit] = 0.0
    depth = np.where(hit, hits["hitDistance"], f32(0.0)).astype(f32)
    return albedo, depth, hits, rays


def running_mean32(frames):
    """accumulate_kernel's update over a list of per-frame arrays (frame numbers 1 ..), float32"""
    a = None
    for k, r in enumerate(frames, start=1):
        r = np.asarray(r, f32)
        a = r.copy() if k == 1 else a + (r - a) / f32(k)
    return a


def same_bits(a, b):
    a = np.ascontiguousarray(a, f32)
    b = np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


# ---- the filter ------------------------------------------------------------------------------------------

H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
DEFAULTS = dict(iterations=5, sigma_color=2.5, sigma_normal=0.3, sigma_albedo=0.2, sigma_depth=0.025)  # nxhip_denoise_defaults


def atrous(colour, albedo4, normal_depth4, iterations, sigma_color, sigma_normal, sigma_albedo, sigma_depth, dtype=np.float64):
    """colour (H, W, 3), albedo4 / normal_depth4 (H, W, 4) -> C_iterations (H, W, 3).
    float64: the definition as written.  float32: the kernel's order — squared differences summed ((x^2 + y^2) + z^2), each term times
    a reciprocal 1 / sigma^2 formed once, terms added colour, normal, albedo, depth; taps dy-major, dx-minor."""
    T = dtype
    single = dtype == np.float32
    C0 = np.asarray(colour, T)
    A = np.asarray(albedo4, T)
    N = np.asarray(normal_depth4, T)[..., 0:3]
    Z = np.asarray(normal_depth4, T)[..., 3]
    Hh, Ww = Z.shape
    for i in range(iterations):
        s = 1 << i
        if single:
            sc = f32(sigma_color) * f32(2.0 ** -i)
            inv_c = min(f32(1.0) / (sc * sc), FLT_MAX)
            inv_n = min(f32(1.0) / (f32(sigma_normal) * f32(sigma_normal)), FLT_MAX)
            inv_a = min(f32(1.0) / (f32(sigma_albedo) * f32(sigma_albedo)), FLT_MAX)
            sz = f32(sigma_depth) * np.maximum(Z, f32(1e-6))
            with np.errstate(over="ignore", divide="ignore"):
                inv_z = np.minimum(f32(1.0) / (sz * sz), FLT_MAX)
        num = np.zeros_like(C0)
        den = np.zeros((Hh, Ww), T)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                # centre region whose tap lies inside the image
                y0, y1 = max(0, -oy), min(Hh, Hh - oy)
                x0, x1 = max(0, -ox), min(Ww, Ww - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                dc = C0[P] - C0[Q]
                dn = N[P] - N[Q]
                da = A[P] - A[Q]
                dz = Z[P] - Z[Q]
                d2c = (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]
                d2n = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                d2a = ((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]) + da[..., 3] * da[..., 3]
                with np.errstate(over="ignore", under="ignore"):
                    if single:
                        e = ((d2c * inv_c + d2n * inv_n) + d2a * inv_a) + (dz * dz) * inv_z[P]
                        w = (f32(H5[dx + 2]) * f32(H5[dy + 2])) * np.exp(-e).astype(f32)
                    else:
                        e = (d2c / (sigma_color * 2.0 ** -i) ** 2 + d2n / sigma_normal ** 2 + d2a / sigma_albedo ** 2
                             + dz * dz / (sigma_depth * np.maximum(Z[P], 1e-6)) ** 2)
                        w = H5[dx + 2] * H5[dy + 2] * np.exp(-e)
                num[P] += w[..., None] * C0[Q]
                den[P] += w
        C0 = num / den[..., None]
    return C0


# A constant image through one iteration: sum(w c) / sum(w) — 25 products, 24 additions in each sum, one division; every rounding is at
# most half a unit in the last place of a value no larger than the result, and iterations do not add up (each starts from a constant
# up to that bound).  Relative to the image's largest value, float32:
FIXED_POINT_BOUND = 5 * 27 * 2.0 ** -24


def synthetic_inputs(W, H, seed=7, noise=0.25):
    """Piecewise-constant colour under seeded noise, with step edges in normal, albedo and depth: (colour (H,W,3), albedo4, normalDepth4)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    region = (xx > W // 3).astype(int) + (yy > H // 2).astype(int) * 2 + (xx + yy > (W + H) * 0.7).astype(int) * 4
    palette = rng.uniform(0.1, 1.5, (8, 3))
    colour = palette[region] * rng.uniform(1.0 - noise, 1.0 + noise, (H, W, 3))
    albedo = np.zeros((H, W, 4))
    albedo[..., 0:3] = rng.uniform(0.2, 0.9, (8, 3))[region]
    albedo[..., 3] = 1.0
    normals = rng.normal(size=(8, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    nd = np.zeros((H, W, 4))
    nd[..., 0:3] = normals[region]
    nd[..., 3] = rng.uniform(1.0, 9.0, 8)[region] + 0.002 * xx
    sky = (yy < 6) & (xx > W - 40)  # a patch of misses: coverage 0, depth 0
    albedo[sky] = 0.0
    nd[sky] = 0.0
    return colour.astype(f32), albedo.astype(f32), nd.astype(f32)


def rel_dev(a, ref):
    """largest deviation relative to the reference image's largest value"""
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(ref, np.float64))) / np.max(np.abs(ref)))
