"""The float environment map (nxhip_upload_env_float) in numpy float64, for tests/test_env_float.py and tests/test_gpu_env_float.py.

Like tests/env_reference.py it shares no text with the kernels: it imports neither the product nor the oracle, and takes from
tests/env_reference.py and tests/geometry_reference.py what does not depend on the kind of map (the direction -> (u, v) mapping, the
cdf inversion, the sphere's quadrature nodes, the pdf of a direction).

The map is H x W x 3 of linear radiance, row 0 at the top (d.y = +1), with the 8-bit map's (u, v).

* texture(img, u, v): the lookup — bilinear, wrap on both axes, texel centres at +0.5, exact fractional weights.
* footprint_weight(img): the sampler's texel weight (include/nexus_hip.h, nxhip_upload_env_float):
      Lf(x, y) = sum over dy, dx in {-1, 0, 1} of k[dy] k[dx] lum(x + dx, y + dy),  k = (1/8, 3/4, 1/8), neighbours wrapping on both axes
      weight(x, y) = Lf(x, y) sin(pi (y + 1/2) / H) + 1e-6,  lum = 0.2126 R + 0.7152 G + 0.0722 B
  Lf is the integral of the bilinearly filtered luminance over the texel's footprint: along one axis the filtered value at offset t
  from the centre is (1 - |t|) own + |t| neighbour, whose integral over t in [-1/2, 1/2] is 3/4 own + 1/8 of each neighbour.
* own_weight(img): the 8-bit maps' rule applied to the float values (the texel's own luminance) — what must NOT be used: kept for
  the test that shows why.
* distribution(img, weight=None): p, marginal, row, density in the shape of env_reference.distribution.
* irradiance(img, n, sub): env_reference.irradiance with the float lookup.
"""
import numpy as np

from tests import env_reference as E

FLOOR = E.FLOOR
KERNEL = np.array([0.125, 0.75, 0.125])


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def texture(img, u, v):
    """img (H, W, 3) linear -> (n, 3) at normalised (u, v), float64"""
    lin = _f64(img)
    H, W = lin.shape[:2]
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


def taps(img, u, v):
    """the largest of the four texels a lookup at (u, v) reads, per sample and channel"""
    lin = _f64(img)
    H, W = lin.shape[:2]
    i0 = np.floor(_f64(u) * W - 0.5).astype(np.int64)
    j0 = np.floor(_f64(v) * H - 0.5).astype(np.int64)
    ia, ib = i0 % W, (i0 + 1) % W
    ja, jb = j0 % H, (j0 + 1) % H
    return np.maximum(np.maximum(lin[ja, ia], lin[ja, ib]), np.maximum(lin[jb, ia], lin[jb, ib]))


def luminance(img):
    lin = _f64(img)
    return 0.2126 * lin[..., 0] + 0.7152 * lin[..., 1] + 0.0722 * lin[..., 2]


def _sin_rows(H):
    return np.sin(np.pi * (np.arange(H) + 0.5) / H)[:, None]


def footprint_weight(img):
    lum = luminance(img)
    Lf = np.zeros_like(lum)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            # value at (x + dx, y + dy): roll by the negative offset
            Lf += KERNEL[dy + 1] * KERNEL[dx + 1] * np.roll(np.roll(lum, -dy, axis=0), -dx, axis=1)
    return Lf * _sin_rows(lum.shape[0]) + FLOOR


def own_weight(img):
    lum = luminance(img)
    return lum * _sin_rows(lum.shape[0]) + FLOOR


def distribution(img, weight=None):
    """img (H, W, 3) -> dict(p, marginal, row, density), all float64, in the shape of env_reference.distribution; `weight`: the
    texel weights instead of footprint_weight(img)"""
    weight = footprint_weight(img) if weight is None else _f64(weight)
    H, W = weight.shape
    p = weight / weight.sum()
    row_sum = p.sum(axis=1)
    marginal = np.cumsum(row_sum)
    marginal[-1] = 1.0
    row = np.cumsum(p, axis=1) / row_sum[:, None]
    row[:, -1] = 1.0
    return dict(p=p, marginal=marginal, row=row, density=p * W * H / (2.0 * np.pi ** 2))


def _irradiance_once(img, n, sub):
    H, W = np.asarray(img).shape[:2]
    d, u, v, dw = E.sphere_grid(W, H, sub)
    cos = np.maximum(d @ _f64(n), 0.0)
    return (texture(img, u, v) * (cos * dw)[:, None]).sum(axis=0)


def irradiance(img, n, sub=16):
    """integral of texture(img, u, v) max(n . omega, 0) d(omega) per channel and the relative quadrature residue: the midpoint rule
    at sub / 2, sub and 2 sub cells per texel and axis with Richardson's rule, as env_reference.irradiance"""
    assert sub % 4 == 0
    a, b, c = (_irradiance_once(img, n, s) for s in (sub // 2, sub, 2 * sub))
    coarser, best = (4.0 * b - a) / 3.0, (4.0 * c - b) / 3.0
    return best, float(np.max(np.abs(best - coarser) / best))


def sample_estimator(img, dist, n, draws, seed):
    """`draws` samples of the one-sample light estimator L cos / (pi pdf) for a Lambertian plane of normal n and albedo 1: a texel
    from dist["p"], a point uniformly inside it, L from the float lookup.  Returned: (draws, 3) float64."""
    lin = _f64(img)
    H, W = lin.shape[:2]
    rng = np.random.RandomState(seed)
    p = dist["p"].reshape(-1)
    texel = np.minimum(np.searchsorted(np.cumsum(p), rng.random_sample(draws), side="right"), W * H - 1)
    y, x = np.divmod(texel, W)
    fx, fy = rng.random_sample(draws), rng.random_sample(draws)
    d = E.direction(x, y, fx, fy, W, H)
    u, v = (x + fx) / W, (y + fy) / H
    cos_lat = np.maximum(np.sqrt(np.maximum(1.0 - d[:, 1] ** 2, 0.0)), E.MIN_COS_LATITUDE)
    pdf = p[texel] * W * H / (2.0 * np.pi ** 2 * cos_lat)
    cos = np.maximum(d @ _f64(n), 0.0)
    return texture(lin, u, v) * (cos / (np.pi * pdf))[:, None]


# ---- the maps the tests share --------------------------------------------------------------------------------------------------

SKY, SUN = (0.02, 0.03, 0.06), (6e4, 5e4, 3.5e4)


def sun_map(W=32, H=16, sun_xy=(9, 4), black_rows=3):
    """sky everywhere, a one-texel sun, the bottom rows black: H x W x 3 float32"""
    img = np.zeros((H, W, 3), np.float32)
    img[...] = SKY
    img[sun_xy[1], sun_xy[0]] = SUN
    if black_rows:
        img[H - black_rows:] = 0.0
    return img


# ---- a small Radiance .hdr writer (the tests write their files to tmp_path) -------------------------------------------------------

def float_to_rgbe(img):
    """H x W x 3 float -> H x W x 4 uint8 RGBE (shared exponent of the largest component, mantissas truncated)"""
    lin = _f64(img)
    m = lin.max(axis=2)
    e = np.zeros(m.shape, np.int64)
    nz = m > 1e-32
    e[nz] = np.floor(np.log2(m[nz])).astype(np.int64) + 1  # m < 2^e
    scale = np.where(nz, np.ldexp(1.0, 8 - e), 0.0)
    out = np.zeros(lin.shape[:2] + (4,), np.uint8)
    out[..., 0:3] = np.clip(np.floor(lin * scale[..., None]), 0, 255).astype(np.uint8)
    out[..., 3] = np.where(nz, e + 128, 0).astype(np.uint8)
    return out


def rgbe_to_float(rgbe):
    """the decoders' formula: component = mantissa x 2^(e - 136) in binary32, e = 0 gives 0"""
    rgbe = np.asarray(rgbe, np.uint8)
    e = rgbe[..., 3].astype(np.int32)
    scale = np.where(e != 0, np.ldexp(np.float32(1.0), e - 136), np.float32(0.0)).astype(np.float32)
    return (rgbe[..., 0:3].astype(np.float32) * scale[..., None]).astype(np.float32)


def write_hdr(rgbe, rle):
    """the bytes of a Radiance .hdr file of the records rgbe (H x W x 4 uint8), flat or run-length encoded (8 <= W < 32768)"""
    rgbe = np.asarray(rgbe, np.uint8)
    h, w = rgbe.shape[:2]
    body = b""
    for y in range(h):
        if not rle or w < 8 or w >= 32768:
            body += rgbe[y].tobytes()
            continue
        body += bytes([2, 2, w >> 8, w & 255])
        for ch in range(4):
            row = rgbe[y, :, ch]
            x = 0
            while x < w:
                run = 1
                while x + run < w and run < 127 and row[x + run] == row[x]:
                    run += 1
                if run >= 3:
                    body += bytes([128 + run, int(row[x])])
                    x += run
                else:
                    n = 1
                    while x + n < w and n < 128 and not (x + n + 2 < w and row[x + n] == row[x + n + 1] == row[x + n + 2]):
                        n += 1
                    body += bytes([n]) + row[x:x + n].tobytes()
                    x += n
    return b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w) + body
