"""The environment map's importance sampler in numpy float64, for tests/test_env_pins.py.

It shares no text with the kernels or the oracle: it imports neither tests.oracle_lib nor the product, and takes from
tests/geometry_reference.py only the sRGB decoding, the bilinear lookup and the direction -> (u, v) mapping, which
tests/test_geometry_pins.py pins on their own.

The map is H x W texels, row 0 at the top (d.y = +1), u = (atan2(z, x) + pi) / (2 pi) along a row, v = 1 - (asin(y) + pi / 2) / pi
down the rows.  The sampler (include/nexus_hip.h, nxhip_read_env_tables) draws a texel with probability proportional to

    weight(x, y) = luminance(srgb_decode(texel)) * sin(pi (y + 1/2) / H) + 1e-6

(luminance = 0.2126 R + 0.7152 G + 0.0722 B; the additive 1e-6 is the documented floor that keeps a black map samplable — stated
here, not rediscovered), a point uniformly in (u, v) inside it, and the direction of that point.  A texel covers du dv = 1 / (W H)
of the unit square and d(omega) = 2 pi^2 cos(latitude) du dv, so the pdf per solid angle is p(texel) W H / (2 pi^2 cos(latitude)).

* distribution(img): p64, the marginal cdf over rows, the conditional cdfs along every row, the density p64 W H / (2 pi^2).
* pick(cdf32, r): the inversion on the float32 tables as read back: the first index whose cdf exceeds r.
* direction(...): the direction of a point of a texel, from float64 (u, v).
* pdf(p64, d): the pdf per solid angle at a direction.
* irradiance(img, n, sub): midpoint quadrature of the map as the renderer looks it up (bilinear, wrap) against a Lambertian normal.
"""
import numpy as np

from tests.geometry_reference import latlong, srgb_decode, texture

FLOOR = 1e-6
MIN_COS_LATITUDE = 1e-6  # the documented clamp of the pdf's 1 / cos(latitude)


def distribution(img):
    """img (H, W, 4) uint8 -> dict(p, marginal, row, density), all float64: p[y, x] sums to 1; marginal[y] = P(row <= y);
    row[y, x] = P(column <= x | row y); density = p W H / (2 pi^2).  Every cdf ends in exactly 1."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    lin = srgb_decode(img[..., 0:3])
    lum = 0.2126 * lin[..., 0] + 0.7152 * lin[..., 1] + 0.0722 * lin[..., 2]
    weight = lum * np.sin(np.pi * (np.arange(H) + 0.5) / H)[:, None] + FLOOR
    p = weight / weight.sum()
    row_sum = p.sum(axis=1)
    marginal = np.cumsum(row_sum)
    marginal[-1] = 1.0
    row = np.cumsum(p, axis=1) / row_sum[:, None]
    row[:, -1] = 1.0
    return dict(p=p, marginal=marginal, row=row, density=p * W * H / (2.0 * np.pi ** 2))


def pick(cdf32, r):
    """the first index whose cdf exceeds r (the last index when none does).  cdf32: (n,) — one index per r — or (rows, n) with `r` a
    pair (row index per sample, r per sample): the search then runs inside each sample's own row."""
    if isinstance(r, tuple):
        rows, rr = r
        cdf = np.asarray(cdf32, np.float64)
        n = cdf.shape[1]
        # rows laid end to end, row k lifted by 2 k: exact in float64 (binary32 values <= 1 plus a small even integer)
        flat = (cdf + 2.0 * np.arange(cdf.shape[0])[:, None]).ravel()
        idx = np.searchsorted(flat, np.asarray(rr, np.float64) + 2.0 * np.asarray(rows), side="right") - np.asarray(rows) * n
        return np.minimum(idx, n - 1)
    cdf = np.asarray(cdf32, np.float64)
    return np.minimum(np.searchsorted(cdf, np.asarray(r, np.float64), side="right"), len(cdf) - 1)


def fraction(cdf32, idx, r, rows=None):
    """where r lies inside entry idx of a cdf: (r - cdf[idx - 1]) / (cdf[idx] - cdf[idx - 1]) in float64, cdf[-1] = 0.  cdf32: (n,), or
    (rows, n) with `rows` the row of every sample"""
    cdf = np.asarray(cdf32, np.float64)
    if rows is not None:
        lo, hi = np.where(idx > 0, cdf[rows, np.maximum(idx - 1, 0)], 0.0), cdf[rows, idx]
    else:
        lo, hi = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], 0.0), cdf[idx]
    return (np.asarray(r, np.float64) - lo) / (hi - lo)


def direction(x, y, fx, fy, W, H):
    """the direction of the point (fx, fy) in [0, 1)^2 of texel (x, y)"""
    u = (np.asarray(x, np.float64) + fx) / W
    v = (np.asarray(y, np.float64) + fy) / H
    phi = (1.0 - v) * np.pi - np.pi / 2.0
    theta = u * 2.0 * np.pi - np.pi
    return np.stack([np.cos(phi) * np.cos(theta), np.sin(phi), np.cos(phi) * np.sin(theta)], axis=1)


def texel_of(d, W, H):
    """(x, y, distance of (u W, v H) to the nearest texel edge, in texels) of directions d"""
    u, v = latlong(d)
    fx, fy = u * W, v * H
    x = np.clip(np.floor(fx), 0, W - 1).astype(np.int64)
    y = np.clip(np.floor(fy), 0, H - 1).astype(np.int64)
    edge = np.minimum(np.minimum(fx - x, x + 1 - fx), np.minimum(fy - y, y + 1 - fy))
    return x, y, edge


def cos_latitude(d):
    d = np.asarray(d, np.float64)
    return np.maximum(np.sqrt(np.maximum(1.0 - d[:, 1] ** 2, 0.0)), MIN_COS_LATITUDE)


def pdf(p64, d):
    """pdf per solid angle of the sampler at the (unit) directions d: p64[texel] W H / (2 pi^2 cos(latitude))"""
    H, W = p64.shape
    x, y, _ = texel_of(d, W, H)
    return p64[y, x] * W * H / (2.0 * np.pi ** 2 * cos_latitude(d))


def sphere_grid(W, H, sub):
    """midpoints of sub x sub cells per texel: (directions (n, 3), u, v, solid angle of each cell)"""
    u = (np.arange(W * sub) + 0.5) / (W * sub)
    v = (np.arange(H * sub) + 0.5) / (H * sub)
    vv, uu = np.meshgrid(v, u, indexing="ij")
    uu, vv = uu.ravel(), vv.ravel()
    phi = (1.0 - vv) * np.pi - np.pi / 2.0
    theta = uu * 2.0 * np.pi - np.pi
    d = np.stack([np.cos(phi) * np.cos(theta), np.sin(phi), np.cos(phi) * np.sin(theta)], axis=1)
    return d, uu, vv, np.cos(phi) * (2.0 * np.pi / (W * sub)) * (np.pi / (H * sub))


def _irradiance_once(img, n, sub):
    H, W = np.asarray(img).shape[:2]
    d, u, v, dw = sphere_grid(W, H, sub)
    cos = np.maximum(d @ np.asarray(n, np.float64), 0.0)
    return (texture(img, u, v) * (cos * dw)[:, None]).sum(axis=0)


def irradiance(img, n, sub=16):
    """integral of texture(img, u, v) max(n . omega, 0) d(omega) per channel, and an estimate of what is left of the quadrature
    error, relative.  Midpoint rule over sub / 2, sub and 2 sub cells per texel and axis (all even: no cell straddles the bilinear
    filter's kinks at the texel centres), which converges as h^2; two neighbouring resolutions are combined by Richardson's rule,
    (4 fine - coarse) / 3.  Returned: the extrapolation from the finer pair, and how far the one from the coarser pair lies from
    it — the error of the COARSER extrapolation, so an upper estimate of what is left in the finer."""
    assert sub % 4 == 0
    a, b, c = (_irradiance_once(img, n, s) for s in (sub // 2, sub, 2 * sub))
    coarser, best = (4.0 * b - a) / 3.0, (4.0 * c - b) / 3.0
    return best, float(np.max(np.abs(best - coarser) / best))
