"""The analytic lights' sampling rule (include/nexus_hip.h, "THE SAMPLING RULE") in numpy, written from the contract's text alone.

It shares no text with the kernels: the device is compared with THIS (tests/test_gpu_analytic_lights.py), and this is compared with
closed forms (tests/test_analytic_light_reference.py).  Everything takes a `dtype`: float64 is the reference; float32 is the same rule
in the device's number format, evaluated only to DERIVE the tolerance the device is held to (4 x the worst deviation between the two).

Lights are records of pod.ALIGHT_DT (or anything indexable by the same field names)."""
import numpy as np

POINT, SPOT, DIRECTIONAL = 0, 1, 2


def table(light, dtype=np.float64):
    """the derived constants of one light: computed in float64 from the record's float32 fields, rounded ONCE to `dtype`"""
    d = np.asarray(light["direction"], np.float64)
    n = np.sqrt((d * d).sum())
    kind = int(light["type"])
    axis = d / n if n > 0 else np.array([0.0, 0.0, -1.0])
    scale, offset = 0.0, 1.0
    if kind == SPOT:
        ci, co = np.cos(np.float64(light["innerConeAngle"])), np.cos(np.float64(light["outerConeAngle"]))
        scale = 1.0 / max(1e-3, ci - co)
        offset = -co * scale
    radius = 0.0 if kind == DIRECTIONAL else np.float64(light["radius"])
    t = dict(kind=kind, centre=np.asarray(light["position"], np.float64), radius=radius, radius2=radius * radius, axis=axis,
             power=np.asarray(light["colour"], np.float64) * np.float64(light["intensity"]), scale=scale, offset=offset,
             q=2.0 * np.sin(0.5 * np.float64(light["angularRadius"])) ** 2)
    return {k: (v if k == "kind" else np.asarray(v, np.float64).astype(dtype)) for k, v in t.items()}


def frame(a):
    """the two tangents of the contract's frame about the unit vectors a[n, 3] (Duff et al. 2017)"""
    one = a.dtype.type(1)
    sg = np.where(np.signbit(a[:, 2]), -one, one)
    k = -one / (sg + a[:, 2])
    b = a[:, 0] * a[:, 1] * k
    t0 = np.stack([one + sg * a[:, 0] * a[:, 0] * k, sg * b, -sg * a[:, 0]], 1)
    t1 = np.stack([b, sg + a[:, 1] * a[:, 1] * k, -a[:, 1]], 1)
    return t0, t1


def sample(light, origins, r, dtype=np.float64, naive_q=False):
    """The draw for `light` from origins[n, 3] (already offset) with r[n, 2].  Returns a dict: direction[n, 3], tmax[n], factor[n, 3],
    ok[n], and the intermediate q, d, cos_theta, att, unattenuated[n, 3] (= factor without att).  naive_q: the cancelling form
    1 - sqrt(1 - s^2) the contract forbids (a control)."""
    T = table(light, dtype)
    f = dtype
    o = np.asarray(origins, np.float64).astype(f)
    r1, r2 = np.asarray(r, np.float64)[:, 0].astype(f), np.asarray(r, np.float64)[:, 1].astype(f)
    n = len(o)
    one, two = f(1), f(2)
    if T["kind"] == DIRECTIONAL:
        a = np.repeat(-T["axis"][None, :], n, 0)
        d = np.ones(n, f)
        d2 = np.ones(n, f)
        q = np.full(n, T["q"], f)
        ok = np.ones(n, bool)
    else:
        to = T["centre"][None, :] - o
        d2 = (to * to).sum(1, dtype=f)
        d = np.sqrt(d2)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = to / d[:, None]
            s2 = T["radius2"] / d2
            ok = d > T["radius"]
            root = np.sqrt(np.maximum(one - s2, f(0)))
            q = (one - root) if naive_q else s2 / (one + root)
    rq = r1 * q
    cos_t = one - rq
    sin2 = rq * (two - rq)
    with np.errstate(invalid="ignore"):
        sin_t = np.sqrt(sin2)  # (an origin inside the sphere — ok false — has no cone: NaN there)
    phi = f(2 * np.pi) * r2
    t0, t1 = frame(a)
    direction = t0 * (np.cos(phi) * sin_t)[:, None] + t1 * (np.sin(phi) * sin_t)[:, None] + a * cos_t[:, None]
    if T["kind"] == DIRECTIONAL:
        tmax = np.full(n, 1e30, f)
    else:
        tmax = d * cos_t - np.sqrt(np.maximum(T["radius2"] - d2 * sin2, f(0)))
    cd = -(a * T["axis"][None, :]).sum(1, dtype=f)  # cosine between the axis and the direction from the centre to o
    att = np.clip(cd * T["scale"] + T["offset"], f(0), one) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        unatt = T["power"][None, :] * (two / (d2 * (two - q)))[:, None]
    return dict(direction=direction, tmax=tmax, factor=unatt * att[:, None], ok=ok, q=q, d=d, cos_theta=cos_t, att=att, unattenuated=unatt, axis=a)


def hits_light(light, origins, direction):
    """float64: does the ray (origin, direction) meet the light's sphere (POINT, SPOT) / point into its disc (DIRECTIONAL)?  And the
    angular distance to the rim, theta_max - theta (radians; negative: outside)."""
    T = table(light)
    o = np.asarray(origins, np.float64)
    w = np.asarray(direction, np.float64)
    w = w / np.sqrt((w * w).sum(1))[:, None]
    if T["kind"] == DIRECTIONAL:
        a = np.repeat(-T["axis"][None, :], len(o), 0)
        theta_max = np.full(len(o), 2.0 * np.arcsin(np.sqrt(T["q"] / 2.0)))
    else:
        to = T["centre"][None, :] - o
        d = np.sqrt((to * to).sum(1))
        a = to / d[:, None]
        theta_max = np.arcsin(np.minimum(T["radius"] / d, 1.0))
    # (the angle from the cross product: arccos of a cosine near 1 has no digits left)
    theta = np.arctan2(np.sqrt((np.cross(a, w) ** 2).sum(1)), (a * w).sum(1))
    return theta <= theta_max, theta_max - theta


def cone_coordinates(light, origins, direction):
    """float64: (u, v) in [0, 1)^2 of a direction in the light's cone — u = (1 - cos theta) / q, v = phi / 2 pi in the contract's frame;
    uniform on the square when the directions are uniform on the cone"""
    s = sample(light, origins, np.zeros((len(origins), 2)))
    a = s["axis"]
    w = np.asarray(direction, np.float64)
    t0, t1 = frame(a)
    x, y = (w * t0).sum(1), (w * t1).sum(1)
    sin_half2 = ((w - a) ** 2).sum(1) / 4.0  # 1 - cos theta = 2 sin^2(theta / 2) = |w - a|^2 / 2 for unit vectors
    with np.errstate(divide="ignore", invalid="ignore"):
        u = 2.0 * sin_half2 / s["q"]
    return u, np.mod(np.arctan2(y, x) / (2.0 * np.pi), 1.0)


def plane_estimator(light, x, normal, rho, r, dtype=np.float64, naive_q=False):
    """One light sample per row of r for the Lambertian point x (normal `normal`, albedo rho), one light in the scene: rho / pi x cos x
    factor, counted only when the direction meets the light (its radiance comes from its surface) and leaves the surface upwards."""
    o = np.repeat(np.asarray(x, np.float64)[None, :], len(r), 0)
    s = sample(light, o, r, dtype, naive_q)
    w = s["direction"].astype(np.float64)
    cos_s = (w * np.asarray(normal, np.float64)[None, :]).sum(1)
    hit, _ = hits_light(light, o, w)
    return np.where((s["ok"] & hit & (cos_s > 0))[:, None], (rho / np.pi) * cos_s[:, None] * s["factor"].astype(np.float64), 0.0)


def closed_form(light, x, normal, rho):
    """rho / pi x I cos / d^2 (x att) for POINT / SPOT — the sphere wholly above the horizon —, rho / pi x E cos for DIRECTIONAL — the disc
    wholly above the horizon (pi L sin^2 alpha cos is exact there)"""
    T = table(light)
    x, nrm = np.asarray(x, np.float64), np.asarray(normal, np.float64)
    if T["kind"] == DIRECTIONAL:
        cos_s = float(-(T["axis"] * nrm).sum())
        assert np.arcsin(cos_s) > 2.0 * np.arcsin(np.sqrt(T["q"] / 2.0)), "the disc must be wholly above the horizon"
        return rho / np.pi * T["power"] * cos_s
    to = T["centre"] - x
    d = np.sqrt((to * to).sum())
    cos_s = float((to * nrm).sum() / d)
    assert d * cos_s > T["radius"], "the sphere must be wholly above the horizon"
    att = float(np.clip(-(to / d * T["axis"]).sum() * T["scale"] + T["offset"], 0.0, 1.0)) ** 2
    return rho / np.pi * T["power"] * att * cos_s / (d * d)


RIM_CAP = 2.0 ** -23  # radians: one binary32 ulp of a unit vector's component


def deviation(light, origins, r):
    """The rule in binary32 against the rule in float64 on the same inputs.  Returns (worst relative deviation of direction — the error
    vector's length, directions being unit —, of tmax, of factor — relative to the UNATTENUATED factor: att is a difference of products
    that cancels towards the outer cone, its error is absolute on att's scale of 1 —, and the mask of draws that count: ok, and not within
    RIM_CAP of the cone's rim in float64, where "does it hit" and the chord's length are condition-limited)."""
    a, b = sample(light, origins, r, np.float32), sample(light, origins, r, np.float64)
    _, margin = hits_light(light, origins, b["direction"])
    keep = b["ok"] & a["ok"] & ((margin > RIM_CAP) | (np.asarray(b["q"]) == 0))
    dev_dir = np.sqrt(((a["direction"].astype(np.float64) - b["direction"]) ** 2).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        dev_t = np.abs(a["tmax"].astype(np.float64) - b["tmax"]) / np.abs(b["tmax"])
        dev_f = np.abs(a["factor"].astype(np.float64) - b["factor"]).max(1) / b["unattenuated"].max(1)
    return dev_dir, dev_t, dev_f, keep
