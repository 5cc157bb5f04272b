"""The medium's rule (include/nexus_hip.h, nxhip_set_medium) restated in numpy: the segment of a ray inside the box, the free flight, the
Henyey-Greenstein pdf and its inversion, the continuation's direction, and the single-scattering integral of a point light by quadrature with
its variance under the rule's own estimator.  Every function takes the number format as `dt`: float64 is the reference, float32 the same
formulas in the device's precision (tests/test_medium_reference.py derives the hook's bars from the difference)."""
import numpy as np

INV_4PI = 0.07957747154594767


def segment(box_min, box_max, o, d, t_end, dt=np.float64):
    """(t0, L, crosses): the rule's t0 and L = t1 - t0 for rays (o[k], d[k]) that end at t_end[k] (inf: a miss); where L <= 0 or the segment
    is empty both are 0 and crosses is False, as the hook reports them"""
    o, d = np.asarray(o, dt).reshape(-1, 3), np.asarray(d, dt).reshape(-1, 3)
    lo = np.zeros(len(o), dt)
    hi = np.asarray(t_end, dt).reshape(-1).copy()
    empty = np.zeros(len(o), bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(3):
            bmin, bmax = dt(box_min[i]), dt(box_max[i])
            a, b = (bmin - o[:, i]) / d[:, i], (bmax - o[:, i]) / d[:, i]
            along = d[:, i] == 0
            lo = np.where(along, lo, np.maximum(lo, np.minimum(a, b)))
            hi = np.where(along, hi, np.minimum(hi, np.maximum(a, b)))
            empty |= along & ~((bmin <= o[:, i]) & (o[:, i] <= bmax))
        L = hi - lo
    crosses = ~empty & (L > 0)
    return np.where(crosses, lo, dt(0)), np.where(crosses, L, dt(0)), crosses


def flight(sigma_t, xi, dt=np.float64):
    """s = -log(1 - xi) / sigmaT"""
    return -np.log(dt(1) - np.asarray(xi, dt)) / dt(sigma_t)


def transmittance(sigma_t, L, dt=np.float64):
    return np.exp(-dt(sigma_t) * np.asarray(L, dt))


def hg_pdf(g, c, dt=np.float64):
    """p(c) = (1 - g^2) / (4 pi (1 + g^2 - 2 g c)^1.5), written as the rule writes it"""
    g = dt(g)
    g2 = g * g
    t = (dt(1) + g2) - (dt(2) * g) * np.asarray(c, dt)
    return ((dt(1) - g2) * dt(INV_4PI)) / (t * np.sqrt(t))


def hg_invert(g, xi1, dt=np.float64):
    """the cosine the rule draws from xi1"""
    g, xi1 = dt(g), np.asarray(xi1, dt)
    if abs(g) < 1e-3:
        return dt(1) - dt(2) * xi1
    g2 = g * g
    q = (dt(1) - g2) / ((dt(1) - g) + (dt(2) * g) * xi1)
    return np.clip(((dt(1) + g2) - q * q) / (dt(2) * g), dt(-1), dt(1))


def phase_sample(g, d, xi1, xi2, dt=np.float64):
    """(omega, pdf): the continuation about the direction of travel d[k], in the branch-free frame of Duff et al. 2017"""
    d = np.asarray(d, dt).reshape(-1, 3)
    c = hg_invert(g, xi1, dt)
    sin_t = np.sqrt(np.maximum(dt(0), dt(1) - c * c))
    phi = dt(6.28318531 if dt == np.float32 else 2.0 * np.pi) * np.asarray(xi2, dt)
    sg = np.copysign(dt(1), d[:, 2])
    k = dt(-1) / (sg + d[:, 2])
    b = d[:, 0] * d[:, 1] * k
    t0 = np.stack([dt(1) + sg * d[:, 0] * d[:, 0] * k, sg * b, -sg * d[:, 0]], 1)
    t1 = np.stack([b, sg + d[:, 1] * d[:, 1] * k, -d[:, 1]], 1)
    w = t0 * (np.cos(phi) * sin_t)[:, None] + t1 * (np.sin(phi) * sin_t)[:, None] + d * c[:, None]
    w = w / np.sqrt((w * w).sum(1))[:, None]
    return w, hg_pdf(g, c, dt)


def camera_rays(cam, W, H, sub):
    """origin and the unit directions of sub x sub positions in every pixel of a pinhole camera record: (3,), (sub^2, pixels, 3), float64"""
    pos = cam["position"].astype(np.float64)
    jj, ii = np.mgrid[0:H, 0:W]
    out = []
    for a in range(sub):
        for b in range(sub):
            x = ((ii + (a + 0.5) / sub) / W).reshape(-1, 1)
            y = ((jj + (b + 0.5) / sub) / H).reshape(-1, 1)
            d = cam["lowerLeftCorner"].astype(np.float64) + cam["viewportX"].astype(np.float64) * x + cam["viewportY"].astype(np.float64) * y - pos
            out.append(d / np.sqrt((d * d).sum(1))[:, None])
    return pos, np.stack(out)


def single_scatter(medium, light_pos, intensity, o, d, nodes=96):
    """Paths of two vertices in a medium without surfaces, lit by a point light INSIDE the box: per ray (o, d[k]) the expectation of the
    rule's estimator and its second moment, both per unit of radiant intensity.  The path scatters at t with density sigma exp(-sigma (t -
    t0)) on the segment and then carries f(t) = albedo p(c) exp(-sigma |P - x|) / |P - x|^2 x intensity; albedo is left to the caller (a
    factor per channel).  Gauss-Legendre on the segment."""
    sigma, g = float(medium["sigmaT"]), float(medium["g"])
    d = np.asarray(d, np.float64).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(o, np.float64), d.shape)
    t0, L, crosses = segment(medium["boxMin"].astype(np.float64), medium["boxMax"].astype(np.float64), o, d, np.full(len(d), np.inf))
    x, w = np.polynomial.legendre.leggauss(nodes)
    t = t0[:, None] + 0.5 * L[:, None] * (x[None, :] + 1.0)
    wt = 0.5 * L[:, None] * w[None, :]
    P = np.asarray(light_pos, np.float64)
    X = o[:, None, :] + d[:, None, :] * t[:, :, None]
    to = P - X
    dist = np.sqrt((to * to).sum(-1))
    c = (to * d[:, None, :]).sum(-1) / dist
    f = hg_pdf(g, c) * np.exp(-sigma * dist) / (dist * dist) * intensity
    dens = sigma * np.exp(-sigma * (t - t0[:, None]))
    mean = (dens * f * wt).sum(1)
    second = (dens * f * f * wt).sum(1)
    return np.where(crosses, mean, 0.0), np.where(crosses, second, 0.0)


def isotropic_limit(light_pos, intensity, o, d, t0, t1):
    """sigma -> 0, g = 0: integral of I / (4 pi |P - x|^2) dt over [t0, t1] = I / (4 pi h) x (atan((t1 - tc) / h) - atan((t0 - tc) / h)), h = the
    distance of the light from the ray, tc = the parameter of its foot"""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    rel = np.asarray(light_pos, np.float64) - np.asarray(o, np.float64)
    tc = d @ rel
    h = np.sqrt(np.maximum((rel * rel).sum() - tc * tc, 0.0))
    return intensity * INV_4PI / h * (np.arctan((t1 - tc) / h) - np.arctan((t0 - tc) / h))
