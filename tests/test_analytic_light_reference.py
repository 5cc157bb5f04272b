"""The float64 reference of the analytic lights' sampling rule (tests/analytic_light_reference.py) against closed forms, and the tolerance the
device's sampling hook is held to (tests/test_gpu_analytic_lights.py), DERIVED here: the rule evaluated in numpy binary32 against the same
rule in float64 on the very inputs the device gets; the bar is 4 x the worst relative deviation (the project's 4 x rule).  No GPU."""
import functools

import numpy as np

from nexus_amd import capi, pod
from tests import analytic_light_reference as R

RHO = 0.6


# ---- the reference estimator against closed forms ----------------------------------------------------------------------------------

def _mc(light, x, normal, n=200_000, seed=11, **kw):
    r = np.random.RandomState(seed).rand(n, 2)
    e = R.plane_estimator(light, x, normal, RHO, r, **kw)[:, 0]
    return e.mean(), e.std(ddof=1) / np.sqrt(n)


CLOSED_FORM_CASES = {
    "point": (pod.make_analytic_light(pod.ALIGHT_POINT, position=(0.3, 1.5, -0.2), colour=(1.0, 0.8, 0.6), intensity=5.0), (1.0, 0.0, 0.5), (0, 1, 0)),
    "point, tilted plane": (pod.make_analytic_light(pod.ALIGHT_POINT, position=(0.3, 1.5, -0.2), colour=(1.0, 0.8, 0.6), intensity=5.0), (1.0, 0.0, 0.5),
                            (np.sin(0.6), np.cos(0.6), 0.0)),
    "sphere r 0.5": (pod.make_analytic_light(pod.ALIGHT_POINT, position=(0.0, 2.0, 0.0), intensity=7.0, radius=0.5), (1.2, 0.0, -0.7), (0, 1, 0)),
    "sphere r 2e-3": (pod.make_analytic_light(pod.ALIGHT_POINT, position=(0.0, 2.0, 0.0), intensity=7.0, radius=2e-3), (1.2, 0.0, -0.7), (0, 1, 0)),
    "spot, inside": (pod.make_analytic_light(pod.ALIGHT_SPOT, position=(0, 2, 0), direction=(0.1, -1, 0.05), intensity=9.0, inner_cone=0.3, outer_cone=0.6), (0.3, 0, 0.1), (0, 1, 0)),
    "spot, falloff band": (pod.make_analytic_light(pod.ALIGHT_SPOT, position=(0, 2, 0), direction=(0.1, -1, 0.05), intensity=9.0, inner_cone=0.3, outer_cone=0.6), (1.1, 0, 0.2), (0, 1, 0)),
    "spot sphere, band": (pod.make_analytic_light(pod.ALIGHT_SPOT, position=(0, 2, 0), direction=(0.1, -1, 0.05), intensity=9.0, inner_cone=0.3, outer_cone=0.6, radius=0.2), (1.1, 0, 0.2), (0, 1, 0)),
    "delta sun": (pod.make_analytic_light(pod.ALIGHT_DIRECTIONAL, direction=(0.4, -0.8, 0.3), colour=(1.0, 0.9, 0.7), intensity=3.0), (0.5, 0, 0.5), (0, 1, 0)),
    "disc 0.05 at 40 degrees": (pod.make_analytic_light(pod.ALIGHT_DIRECTIONAL, direction=(np.cos(np.radians(40)), -np.sin(np.radians(40)), 0.0), intensity=3.0, angular_radius=0.05),
                                (0.5, 0, 0.5), (0, 1, 0)),
}


def test_the_reference_estimator_reproduces_the_closed_forms():
    for name, (light, x, normal) in CLOSED_FORM_CASES.items():
        normal = np.asarray(normal, np.float64)
        mean, se = _mc(light, x, normal)
        want = R.closed_form(light, x, normal, RHO)[0]
        print("%-26s estimate %.9g +- %.2g, closed form %.9g" % (name, mean, se, want))
        assert want > 0
        assert abs(mean - want) < 5.0 * se + 1e-9 * want, name
        assert se < 2e-3 * want, "the estimate is too noisy for its pass to mean anything"
    # the spot's falloff is in force: the band case is dimmer than the bare inverse-square law, by att
    light, x, normal = CLOSED_FORM_CASES["spot, falloff band"]
    T = R.table(light)
    to = T["centre"] - np.asarray(x, np.float64)
    d = np.sqrt((to * to).sum())
    bare = RHO / np.pi * 9.0 * (to[1] / d) / (d * d)
    att = R.closed_form(light, x, np.asarray(normal, np.float64), RHO)[0] / bare
    assert 0.05 < att < 0.95


def test_the_factor_is_radiance_over_the_cone_density():
    """2 / (d^2 (1 + cos thetaMax)) x I is L / pdf with L = I / (pi r^2), pdf = 1 / (2 pi q); and E / (pi sin^2 alpha) x 2 pi q for the disc"""
    light = CLOSED_FORM_CASES["sphere r 0.5"][0]
    o = np.array([[1.2, 0.0, -0.7], [0.2, 1.0, 0.1], [5.0, -3.0, 2.0]])
    s = R.sample(light, o, np.full((3, 2), 0.37))
    literal = 7.0 / (np.pi * 0.25) * 2.0 * np.pi * s["q"]
    assert np.allclose(s["factor"][:, 0], literal, rtol=1e-13)
    disc = CLOSED_FORM_CASES["disc 0.05 at 40 degrees"][0]
    s = R.sample(disc, o, np.full((3, 2), 0.37))
    assert np.allclose(s["factor"][:, 0], 3.0 / (np.pi * np.sin(np.float64(np.float32(0.05))) ** 2) * 2.0 * np.pi * s["q"], rtol=1e-13)
    # the limits: I / d^2 and E
    point = CLOSED_FORM_CASES["point"][0]
    s = R.sample(point, o, np.full((3, 2), 0.37))
    d2 = ((np.array([0.3, 1.5, -0.2], np.float32).astype(np.float64) - o) ** 2).sum(1)
    assert np.allclose(s["factor"][:, 0], 5.0 / d2, rtol=1e-13) and np.all(s["tmax"] == s["d"])
    sun = CLOSED_FORM_CASES["delta sun"][0]
    s = R.sample(sun, o, np.full((3, 2), 0.37))
    assert np.allclose(s["factor"], [[3.0, float(np.float32(0.9)) * 3.0, float(np.float32(0.7)) * 3.0]] * 3, rtol=1e-13) and np.all(s["tmax"] == 1e30)


def test_control_the_cancelling_q_in_binary32_is_refused():
    """q = 1 - sqrt(1 - s^2) in binary32 at radius / d = 1e-3: the cone no longer fits the sphere, and the estimator that stands on the
    contract's factor is off by per cent — the check above must refuse it (and accept the stated form in the same number format)."""
    light = pod.make_analytic_light(pod.ALIGHT_POINT, position=(0.0, 2.0, 0.0), intensity=7.0, radius=2e-3)
    x, normal = (0.0, 0.0, 0.0), np.array([0.0, 1.0, 0.0])
    want = R.closed_form(light, x, normal, RHO)[0]
    s32, s64 = R.sample(light, [x], [[0.5, 0.5]], np.float32, naive_q=True), R.sample(light, [x], [[0.5, 0.5]])
    print("q naive binary32 %.6g, q float64 %.6g: ratio %.4f" % (s32["q"][0], s64["q"][0], s32["q"][0] / s64["q"][0]))
    assert abs(s32["q"][0] / s64["q"][0] - 1.0) > 0.03
    good = R.sample(light, [x], [[0.5, 0.5]], np.float32)
    assert abs(good["q"][0] / s64["q"][0] - 1.0) < 2e-7
    mean, se = _mc(light, x, normal, dtype=np.float32, naive_q=True)
    # (what goes wrong depends on the side the rounding falls: a cone too wide throws draws past the sphere — the estimate drops —, a cone
    #  too narrow leaves the rim of the sphere unsampled — the cone's coverage shows it.  Both are looked at; one must refuse.)
    r = np.random.RandomState(5).rand(100_000, 2)
    o = np.repeat(np.asarray(x, np.float64)[None, :], len(r), 0)
    u, _ = R.cone_coordinates(light, o, R.sample(light, o, r, np.float32, naive_q=True)["direction"].astype(np.float64))
    print("naive estimate %.6g +- %.2g against %.6g; largest cone coordinate %.4f" % (mean, se, want, u.max()))
    refused_by_mean = not abs(mean - want) < 5.0 * se + 1e-9 * want
    refused_by_coverage = not 0.999 < u.max() <= 1.0 + 1e-3
    assert refused_by_mean or refused_by_coverage
    mean, se = _mc(light, x, normal, dtype=np.float32)
    u, _ = R.cone_coordinates(light, o, R.sample(light, o, r, np.float32)["direction"].astype(np.float64))
    assert abs(mean - want) < 5.0 * se + 3e-4 * want and 0.999 < u.max() <= 1.0 + 1e-3  # (binary32 directions: a few 1e-4 of the draws graze past the rim)


# ---- the sampling hook's inputs and its derived tolerance ---------------------------------------------------------------------------

HOOK_N = 50_000
HOOK_LIGHTS = np.array([
    pod.make_analytic_light(pod.ALIGHT_POINT, position=(0.3, 1.5, -0.2), colour=(1.0, 0.8, 0.6), intensity=5.0),
    pod.make_analytic_light(pod.ALIGHT_POINT, position=(-1.0, 2.0, 0.5), colour=(0.9, 1.0, 0.4), intensity=7.0, radius=0.5),
    pod.make_analytic_light(pod.ALIGHT_POINT, position=(0.25, 0.5, 0.125), intensity=2.0, radius=1e-3),
    pod.make_analytic_light(pod.ALIGHT_SPOT, position=(0.0, 2.0, 0.0), direction=(0.6, -2.0, 0.4), colour=(1.0, 0.5, 0.25), intensity=9.0, radius=0.05, inner_cone=0.3, outer_cone=0.6),
    pod.make_analytic_light(pod.ALIGHT_DIRECTIONAL, direction=(0.8, -1.6, 0.6), colour=(1.0, 0.9, 0.7), intensity=3.0, angular_radius=0.05),
], dtype=pod.ALIGHT_DT)
# distances from the centre, log-uniform: far enough from the sphere and near enough that the cone stays wide against one binary32 ulp
# (2 RIM_CAP / thetaMax of the draws fall in the rim cap: r = 1e-3 at d <= 1.5 is 3.6e-4)
HOOK_DISTANCES = [(0.05, 20.0), (0.6, 6.0), (0.005, 1.5), (0.2, 6.0), (0.5, 5.0)]
HOOK_INSIDE = 16  # origins inside the sphere (d <= radius: ok = 0), for the lights that have one


@functools.lru_cache(maxsize=None)
def hook_inputs(k):
    """(origins float32[n, 3], r float32[n, 2]) for HOOK_LIGHTS[k]; the r include 0 and 1 - 2^-24, the origins some inside the sphere"""
    rng = np.random.RandomState(100 + k)
    lo, hi = HOOK_DISTANCES[k]
    w = rng.randn(HOOK_N, 3)
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    d = np.exp(rng.uniform(np.log(lo), np.log(hi), HOOK_N))
    radius = float(HOOK_LIGHTS[k]["radius"])
    if radius > 0:
        d[:HOOK_INSIDE] = radius * rng.uniform(0.1, 1.0, HOOK_INSIDE)
    o = (HOOK_LIGHTS[k]["position"].astype(np.float64)[None, :] + w * d[:, None]).astype(np.float32)
    r = rng.rand(HOOK_N, 2).astype(np.float32)
    r = np.minimum(r, np.float32(1.0 - 2.0 ** -24))
    edge = [0.0, 1.0 - 2.0 ** -24]
    at = HOOK_INSIDE
    for a in edge:
        for b in edge + [0.5]:
            r[at] = (a, b)
            r[at + 1] = (b, a)
            at += 2
    return o, r


@functools.lru_cache(maxsize=None)
def hook_tolerance(k):
    """(bar for the direction, for tmax, for factor; the mask of draws that count; the float64 reference) for HOOK_LIGHTS[k]"""
    o, r = hook_inputs(k)
    dev_dir, dev_t, dev_f, keep = R.deviation(HOOK_LIGHTS[k], o, r)
    finite_t = keep & (R.sample(HOOK_LIGHTS[k], o, r)["tmax"] < 1e29)
    worst = (dev_dir[keep].max(), dev_t[finite_t].max() if finite_t.any() else 0.0, dev_f[keep].max())
    return tuple(4.0 * w for w in worst), keep, R.sample(HOOK_LIGHTS[k], o, r)


def test_the_hook_tolerance_is_derived_and_the_rim_cap_is_small():
    names = ["point", "sphere r 0.5", "sphere r 1e-3", "spot r 0.05", "disc 0.05"]
    for k, name in enumerate(names):
        (bd, bt, bf), keep, ref = hook_tolerance(k)
        left_out = (ref["ok"] & ~keep).mean()
        print("%-14s bar: direction %.3g, tmax %.3g, factor %.3g (4 x the binary32 rule's worst deviation); ok %d of %d, rim cap %.2g of the draws"
              % (name, bd, bt, bf, ref["ok"].sum(), len(keep), left_out))
        assert left_out <= 1e-3, "the float64 reference alone must keep the rim cap below 1e-3 of the draws"
        # the format's precision, not an accident of the inputs: a few ulp of 1 for the direction and the factor (the spot's falloff is a
        # difference scaled by angleScale = 7.7); tmax is d cos - sqrt(r^2 - d^2 sin^2), whose root loses digits like 1 / sqrt(distance to
        # the rim) — outside the rim cap that is bounded by sqrt(theta_max / RIM_CAP) ulp, about 1e3 ulp for the widest cone here
        assert 2.0 ** -24 < bd < 64 * 2.0 ** -24 and bt < 4096 * 2.0 ** -24 and 2.0 ** -25 < bf < 256 * 2.0 ** -24, name
        # every reference direction is inside its light
        hit, margin = R.hits_light(HOOK_LIGHTS[k], hook_inputs(k)[0], ref["direction"])
        assert np.all(hit[ref["ok"]] | (margin[ref["ok"]] > -1e-12))
        if float(HOOK_LIGHTS[k]["radius"]) > 0:
            assert (~ref["ok"]).sum() == HOOK_INSIDE


def test_record_sizes_agree_on_both_sides():
    assert pod.ALIGHT_DT.itemsize == 64
    words = capi.abi_words()
    at = words.index(pod.LIGHT_DT.itemsize) + 2  # (behind nx_light's two words, as in nxhip_header_abi_stamp)
    assert words[at:at + 5] == [64, 16, 32, 48, 56]
    assert capi.lib().nxhip_abi_stamp() == capi.abi_stamp()  # (the library hashes sizeof(nx_analytic_light) and its offsets: a 60-byte idea of it is refused)
