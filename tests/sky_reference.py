"""The sun-and-sky model of nxhip_set_sky (include/nexus_hip.h) in numpy float64, for tests/test_sky.py and tests/test_gpu_sky.py.

Written from the model's text and Nishita et al. 1993, in metres, with positions as vectors and the height of a point as |p| - Rg (in
float64 that difference is good to a nanometre; the device avoids it).  Vectorised over directions; the light ray's segments are an
array axis, the view ray's a Python loop.

* Params(sky): a pod.SKY_DT record read as float64 (the sun direction normalised here).
* map_directions(W, H): the texel centres' directions, (H, W, 3).
* radiance(P, dirs, nv=None, nl=None): the sky term, ground included, no disc: (n, 3).
* sun_transmittance(P, segments, origin=None): T_sun by the light-ray rule, (3,); 0 when the ray towards the sun hits the planet.
* disc_coverage(P, W, H), texel_solid_angles(W, H), disc_term(P, W, H): c (H, W), Omega (H,), and Lsun c k (H, W, 3) — ValueError when
  the disc fell between the sub-positions.
"""
import numpy as np

RG, RT = 6360000.0, 6420000.0
BETA_R = np.array([5.802e-6, 13.558e-6, 33.1e-6])
BETA_M, MIE_SSA = 3.996e-6, 0.9
HR, HM = 8000.0, 1200.0


class Params:
    def __init__(self, sky):
        f = lambda name: np.asarray(sky[name], dtype=np.float64)  # noqa: E731
        s = f("sunDirection")
        self.sun = s / np.sqrt(np.sum(s * s))
        self.alpha = float(f("sunAngularRadius"))
        self.irradiance = f("sunIrradiance")
        self.altitude = float(f("altitude"))
        self.beta_r = BETA_R * float(f("rayleighScale"))
        self.beta_m = BETA_M * float(f("mieScale"))
        self.beta_m_ext = self.beta_m / MIE_SSA
        self.g = float(f("mieG"))
        self.albedo = f("groundAlbedo")
        self.nv, self.nl = int(sky["viewSteps"]), int(sky["lightSteps"])
        self.observer = np.array([0.0, RG + self.altitude, 0.0])


def map_directions(W, H):
    u = (np.arange(W) + 0.5) / W
    v = (np.arange(H) + 0.5) / H
    phi = (np.pi / 2 - np.pi * v)[:, None]
    theta = (2 * np.pi * u - np.pi)[None, :]
    return np.stack([np.cos(phi) * np.cos(theta), np.sin(phi) * np.ones_like(theta), np.cos(phi) * np.sin(theta)], axis=-1)


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _exit_distance(p, d):
    """distance to the Rt sphere along p + t d from a point inside it"""
    b = _dot(p, d)
    return -b + np.sqrt(b * b - (_dot(p, p) - RT * RT))


def _ground_hit(p, d):
    """(hits, distance): the first hit of p + t d, t > 0, with the Rg sphere, from a point on or above it"""
    b = _dot(p, d)
    disc = b * b - (_dot(p, p) - RG * RG)
    hits = (b < 0) & (disc >= 0)
    return hits, np.where(hits, -b - np.sqrt(np.maximum(disc, 0.0)), 0.0)


def _segments(t_end, n):
    """quadratic edges t_i = t_end (i / n)^2: (midpoints, lengths), each (..., n)"""
    edges = t_end[..., None] * (np.arange(n + 1) / n) ** 2
    return 0.5 * (edges[..., 1:] + edges[..., :-1]), edges[..., 1:] - edges[..., :-1]


def _light_depths(p, sun, nl, occlusion=True):
    """the light-ray rule from the points p (..., 3): (visible, tauR, tauM) with nl segments to the Rt exit"""
    visible = ~_ground_hit(p, sun)[0] if occlusion else np.ones(p.shape[:-1], dtype=bool)
    mid, du = _segments(_exit_distance(p, sun), nl)
    pts = p[..., None, :] + mid[..., None] * sun
    h = np.sqrt(_dot(pts, pts)) - RG
    return visible, np.sum(np.exp(-h / HR) * du, axis=-1), np.sum(np.exp(-h / HM) * du, axis=-1)


def sun_transmittance(P, segments, origin=None):
    p = P.observer if origin is None else np.asarray(origin, dtype=np.float64)
    visible, tau_r, tau_m = _light_depths(p[None, :], P.sun, segments)
    return np.where(visible[0], np.exp(-(P.beta_r * tau_r[0] + P.beta_m_ext * tau_m[0])), 0.0)


def radiance(P, dirs, nv=None, nl=None):
    nv, nl = P.nv if nv is None else nv, P.nl if nl is None else nl
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    o = np.broadcast_to(P.observer, d.shape)
    ground, t_ground = _ground_hit(o, d)
    t_end = np.where(ground, t_ground, _exit_distance(o, d))
    mid, ds = _segments(t_end, nv)
    mu = _dot(d, P.sun)
    phase_r = 3.0 / (16.0 * np.pi) * (1.0 + mu * mu)
    g = P.g
    phase_m = 3.0 / (8.0 * np.pi) * (1.0 - g * g) * (1.0 + mu * mu) / ((2.0 + g * g) * (1.0 + g * g - 2.0 * g * mu) ** 1.5)
    tau_r, tau_m = np.zeros(len(d)), np.zeros(len(d))
    out = np.zeros((len(d), 3))
    for i in range(nv):
        p = o + mid[:, i, None] * d
        h = np.sqrt(_dot(p, p)) - RG
        rho_r, rho_m = np.exp(-h / HR), np.exp(-h / HM)
        view_r, view_m = tau_r + 0.5 * rho_r * ds[:, i], tau_m + 0.5 * rho_m * ds[:, i]
        visible, light_r, light_m = _light_depths(p, P.sun, nl)
        atten = np.exp(-(P.beta_r[None, :] * (view_r + light_r)[:, None] + P.beta_m_ext * (view_m + light_m)[:, None]))
        scatter = P.beta_r[None, :] * (rho_r * phase_r)[:, None] + P.beta_m * (rho_m * phase_m)[:, None]
        out += np.where(visible[:, None], scatter * ds[:, i, None] * atten, 0.0)
        tau_r += rho_r * ds[:, i]
        tau_m += rho_m * ds[:, i]
    out *= P.irradiance[None, :]
    if np.any(ground):
        pg = o + t_end[:, None] * d
        n = pg / np.sqrt(_dot(pg, pg))[:, None]
        cos_sun = _dot(n, P.sun)
        _, light_r, light_m = _light_depths(RG * n, P.sun, nl, occlusion=False)  # (below the point's horizon: the cosine is 0)
        t_view = np.exp(-(P.beta_r[None, :] * tau_r[:, None] + P.beta_m_ext * tau_m[:, None]))
        t_sun = np.exp(-(P.beta_r[None, :] * light_r[:, None] + P.beta_m_ext * light_m[:, None]))
        lit = t_view * P.albedo[None, :] / np.pi * P.irradiance[None, :] * t_sun * np.maximum(cos_sun, 0.0)[:, None]
        out += np.where((ground & (cos_sun > 0))[:, None], lit, 0.0)
    return out


def horizon_switch_distance(P, dirs):
    """how far (radians) each direction is from the cone where the view ray starts to hit the planet"""
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    dip = np.arccos(RG / (RG + P.altitude))  # the geometric horizon lies this far below the horizontal
    elevation = np.arcsin(np.clip(d[:, 1] / np.sqrt(_dot(d, d)), -1.0, 1.0))
    return np.abs(elevation + dip)


def texel_solid_angles(W, H):
    edges = np.pi / 2 - np.pi * np.arange(H + 1) / H
    return (2 * np.pi / W) * (np.sin(edges[:-1]) - np.sin(edges[1:]))


def disc_coverage(P, W, H):
    u = (np.arange(W * 8) + 0.5) / (W * 8)  # sub-position (i + 1/2) / 8 of texel x: (x + (i + 1/2) / 8) / W
    v = (np.arange(H * 8) + 0.5) / (H * 8)
    phi = (np.pi / 2 - np.pi * v)[:, None]
    theta = (2 * np.pi * u - np.pi)[None, :]
    d = np.stack([np.cos(phi) * np.cos(theta), np.sin(phi) * np.ones_like(theta), np.cos(phi) * np.sin(theta)], axis=-1)
    cross = np.cross(d, P.sun)
    angle = np.arctan2(np.sqrt(_dot(cross, cross)), _dot(d, P.sun))
    inside = (angle <= P.alpha).reshape(H, 8, W, 8)
    return inside.sum(axis=(1, 3)) / 64.0


def cap_solid_angle(alpha):
    return 2 * np.pi * 2 * np.sin(alpha / 2) ** 2  # 2 pi (1 - cos alpha), without the cancellation


def disc_scale(P, W, H):
    """(c, k): the coverage and the map's normalisation factor"""
    c = disc_coverage(P, W, H)
    total = np.sum(c * texel_solid_angles(W, H)[:, None])
    if total == 0:
        raise ValueError("the sun's disc fell between the sub-positions: use a larger map or a larger sunAngularRadius")
    return c, cap_solid_angle(P.alpha) / total


def disc_term(P, W, H):
    c, k = disc_scale(P, W, H)
    l_sun = P.irradiance * sun_transmittance(P, P.nl) / (np.pi * np.sin(P.alpha) ** 2)
    return c[:, :, None] * k * l_sun[None, None, :]
