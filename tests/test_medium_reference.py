"""The float64 statement of the medium's rule (tests/medium_reference.py) checked against itself and against closed forms, and the bars of the
device tests derived from it: the same formulas in numpy binary32 on the hooks' inputs, worst deviation from float64, times 4 (the
project's convention).  No GPU."""
import numpy as np

from nexus_amd import capi, pod
from tests import medium_reference as R

W = H = 64

# ---- the hooks' medium and inputs (tests/test_gpu_medium.py runs the device on exactly these) -------------------------------------------

HOOK_N = 20000
HOOK_G = (0.7, 0.0, -0.4)


def hook_medium(g=0.7):
    return pod.make_medium(box_min=(-1.0, -0.5, -1.5), box_max=(1.0, 1.0, 0.5), sigma_t=0.8, g=g, albedo=(0.9, 0.8, 0.7))


def hook_inputs():
    """origins in [-3, 3]^3, unit directions (one in eight along an axis plane: d_i == 0), tEnd in (0.2, 8) or inf, xi: 23-bit numbers"""
    rng = np.random.default_rng(20261019)
    o = rng.uniform(-3.0, 3.0, (HOOK_N, 3)).astype(np.float32)
    d = rng.normal(size=(HOOK_N, 3))
    d[::8, rng.integers(0, 3)] = 0.0
    d[4::16, 0] = 0.0
    d[4::16, 1] = 0.0
    d = (d / np.sqrt((d * d).sum(1))[:, None]).astype(np.float32)
    o[::5] = rng.uniform(-0.5, 0.5, (len(o[::5]), 3)).astype(np.float32)  # a fifth of the origins inside the box
    o[3::40, 0] = -1.0  # ... and some on a face
    t_end = rng.uniform(0.2, 8.0, HOOK_N).astype(np.float32)
    t_end[::3] = np.inf
    xi = (rng.integers(0, 1 << 23, HOOK_N) / float(1 << 23)).astype(np.float32)
    xi2 = (rng.integers(0, 1 << 23, HOOK_N) / float(1 << 23)).astype(np.float32)
    return o, d, t_end, xi, xi2


def segment_reference(dt=np.float64):
    m = hook_medium()
    o, d, t_end, xi, _ = hook_inputs()
    t0, L, crosses = R.segment(m["boxMin"], m["boxMax"], o, d, t_end, dt)
    s = R.flight(m["sigmaT"], xi, dt)
    scat = crosses & (s < L)
    return dict(t0=t0, L=L, crosses=crosses, T=np.where(crosses, R.transmittance(m["sigmaT"], L, dt), dt(1)), scatter=scat,
                scatter_t=np.where(scat, t0 + s, dt(-1)))


def segment_bars():
    """(bars, keep, ref): absolute bars on t0, L, transmittance and scatterT; keep = draws whose decisions agree between binary32 and float64"""
    ref, f32 = segment_reference(np.float64), segment_reference(np.float32)
    keep = (ref["crosses"] == f32["crosses"]) & (ref["scatter"] == f32["scatter"])
    bars = {k: 4.0 * float(np.abs(f32[k].astype(np.float64) - ref[k])[keep].max()) for k in ("t0", "L", "T", "scatter_t")}
    return bars, keep, ref


def phase_reference(g, dt=np.float64):
    _, d, _, xi1, xi2 = hook_inputs()
    d = d[(d[:, 2] > -0.999)]  # (the frame's pole: 1 / (1 + d.z) amplifies the rounding of d; covered by the direction check with its own bar)
    n = len(d)
    return d, xi1[:n], xi2[:n], R.phase_sample(g, d.astype(np.float64) if dt == np.float64 else d, xi1[:n], xi2[:n], dt)


def phase_bars(g):
    """(direction bar: Euclidean distance; pdf bar: relative), and the float64 reference"""
    d, xi1, xi2, (w64, p64) = phase_reference(g, np.float64)
    _, _, _, (w32, p32) = phase_reference(g, np.float32)
    bar_w = 4.0 * float(np.sqrt(((w32.astype(np.float64) - w64) ** 2).sum(1)).max())
    bar_p = 4.0 * float((np.abs(p32.astype(np.float64) - p64) / p64).max())
    return (bar_w, bar_p), (d, xi1, xi2, w64, p64)


# ---- the single-scattering scene (tests/test_gpu_medium.py renders it) -----------------------------------------------------------------

SS_FRAMES = 256
SS_LIGHT = np.array((0.0, 0.9, 0.5))
SS_INTENSITY = np.array((3.0, 2.5, 2.0))
SS_ALBEDO = 0.9


def ss_medium(g):
    return pod.make_medium(box_min=(-1, -1, -1), box_max=(1, 1, 1), sigma_t=0.8, g=g, albedo=(SS_ALBEDO,) * 3)


def ss_camera():
    return capi.camera_init((0.0, 0.0, 4.0), (0.0, 0.0, -1.0), 14.0, W, H, 5.0, 0.0)


def block_means(per_pixel):
    jj, ii = np.mgrid[0:H, 0:W]
    ids = ((jj // 16) * (W // 16) + ii // 16).reshape(-1)
    return np.bincount(ids, weights=per_pixel, minlength=16) / np.bincount(ids, minlength=16)


def ss_expectation(g, sub):
    """block means (16,) of the expectation and of the per-path variance, per unit intensity and albedo 1"""
    pos, dirs = R.camera_rays(ss_camera(), W, H, sub)
    mean, second = np.zeros(W * H), np.zeros(W * H)
    for k in range(len(dirs)):
        m, s2 = R.single_scatter(ss_medium(g), SS_LIGHT, 1.0, pos, dirs[k])
        mean += m / len(dirs)
        second += s2 / len(dirs)
    bm = block_means(mean)
    return bm, block_means(second) - block_means(mean ** 2)  # (the variance of one path of a block's pixel, pixel to pixel spread left out)


SS_SUB = 2

# ---- tests -----------------------------------------------------------------------------------------------------------------------------


def test_inversion_reproduces_the_pdf():
    rng = np.random.default_rng(5)
    n = 400000
    for g in (0.7, -0.4, 0.0, 0.99):
        xi = rng.integers(0, 1 << 23, n) / float(1 << 23)
        c = R.hg_invert(g, xi)
        edges = np.linspace(-1.0, 1.0, 65)
        # the cdf of p(c) 2 pi: closed form
        cdf = (lambda x: (1.0 + x) / 2.0) if g == 0.0 else (lambda x: (1.0 - g * g) / (2.0 * g) * (1.0 / np.sqrt(1.0 + g * g - 2.0 * g * x) - 1.0 / (1.0 + g)))
        e = n * np.diff(cdf(edges))
        got = np.histogram(c, edges)[0]
        use = e > 5
        chi2, dof = ((got - e) ** 2 / e)[use].sum(), use.sum() - 1
        assert (chi2 - dof) / np.sqrt(2 * dof) < 5, (g, chi2)
        assert abs(c.mean() - g) < 5 * c.std() / np.sqrt(n), (g, c.mean())


def test_pdf_integrates_to_one():
    x, w = np.polynomial.legendre.leggauss(200)
    cuts = np.array([-1.0, -0.999, -0.99, -0.9, 0.0, 0.9, 0.99, 0.999, 0.9999, 1.0])  # (g = 0.99 peaks at 2e3 x its mean: panels towards the poles)
    for g in (0.0, 0.3, -0.6, 0.9, 0.99, -0.99):
        total = sum(0.5 * (b - a) * (R.hg_pdf(g, 0.5 * (a + b) + 0.5 * (b - a) * x) * w).sum() for a, b in zip(cuts[:-1], cuts[1:]))
        assert abs(2.0 * np.pi * total - 1.0) < 1e-9, (g, total)


def test_segment_rule_on_hand_made_cases():
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    cases = [  # origin, direction, tEnd -> t0, L
        ((0, 0, 0), (1, 0, 0), np.inf, 0.0, 1.0),          # inside
        ((-1, 0, 0), (1, 0, 0), np.inf, 0.0, 2.0),         # on a face, going in
        ((-1, 0, 0), (-1, 0, 0), np.inf, 0.0, 0.0),        # on a face, going out: L = 0, nothing
        ((-3, 0.5, 0), (1, 0, 0), np.inf, 2.0, 2.0),       # d_y == d_z == 0 inside their slabs
        ((-3, 1.5, 0), (1, 0, 0), np.inf, 0.0, 0.0),       # d_y == 0 outside its slab: empty
        ((3, 0, 0), (1, 0, 0), np.inf, 0.0, 0.0),          # the box behind the ray
        ((-3, 0, 0), (1, 0, 0), 2.5, 2.0, 0.5),            # tEnd inside the box
        ((-3, 0, 0), (1, 0, 0), 1.5, 0.0, 0.0),            # tEnd in front of it
        ((-3, -3, 0), (0.6, 0.8, 0), np.inf, 10.0 / 3.0, 5.0 - 10.0 / 3.0),
    ]
    o, d, te = np.array([c[0] for c in cases], float), np.array([c[1] for c in cases], float), np.array([c[2] for c in cases], float)
    for dt in (np.float64, np.float32):
        t0, L, crosses = R.segment(lo, hi, o, d, te, dt)
        assert np.allclose(t0, [c[3] for c in cases], atol=1e-6) and np.allclose(L, [c[4] for c in cases], atol=1e-6)
        assert np.array_equal(crosses, np.array([c[4] for c in cases]) > 0)


def test_quadrature_meets_the_closed_form_of_the_thin_limit():
    pos, dirs = R.camera_rays(ss_camera(), W, H, 1)
    m = ss_medium(0.0)
    m["sigmaT"] = 1e-7
    mean, _ = R.single_scatter(m, SS_LIGHT, 1.0, pos, dirs[0])
    t0, L, crosses = R.segment(m["boxMin"], m["boxMax"], np.broadcast_to(pos, dirs[0].shape), dirs[0], np.full(W * H, np.inf))
    assert crosses.all()
    want = 1e-7 * R.isotropic_limit(SS_LIGHT, 1.0, pos, dirs[0], t0, t0 + L)
    assert np.abs(mean / want - 1.0).max() < 1e-5


def test_single_scattering_scene_is_planned_right():
    pos, dirs = R.camera_rays(ss_camera(), W, H, 1)
    rel = SS_LIGHT - pos
    dist = np.sqrt(np.maximum((rel * rel).sum() - (dirs[0] @ rel) ** 2, 0.0))
    assert dist.min() >= 0.35, dist.min()
    for g in (0.0, 0.7):
        a, var = ss_expectation(g, SS_SUB)
        b, _ = ss_expectation(g, 2 * SS_SUB)
        assert np.abs(a / b - 1.0).max() < 1e-4, np.abs(a / b - 1.0).max()  # sub and 2 sub agree: no systematic allowance
        rel_se = np.sqrt(var / 256.0 / SS_FRAMES) / a
        print("g %.1f: relative standard error of a block over %d frames: max %.3g" % (g, SS_FRAMES, rel_se.max()))
        assert rel_se.max() <= 0.02


def test_hook_bars_and_the_decision_cap():
    bars, keep, ref = segment_bars()
    print("segment bars", bars, "left out", (~keep).sum(), "crossing", ref["crosses"].sum(), "scattering", ref["scatter"].sum())
    assert (~keep).mean() <= 1e-3  # binary32 alone flips no more decisions than the cap allows
    assert ref["crosses"].sum() > HOOK_N // 10 and ref["scatter"].sum() > HOOK_N // 20 and (ref["crosses"] & ~ref["scatter"]).sum() > HOOK_N // 40
    assert all(0 < b < 1e-4 for b in bars.values()), bars
    for g in HOOK_G:
        (bar_w, bar_p), _ = phase_bars(g)
        print("phase bars g %.1f: direction %.3g, pdf %.3g" % (g, bar_w, bar_p))
        assert 0 < bar_w < 1e-3 and 0 < bar_p < 1e-3


def test_record_size_agrees_on_both_sides():
    assert pod.MEDIUM_DT.itemsize == 48 and [pod.MEDIUM_DT.fields[n][1] for n in pod.MEDIUM_DT.names] == [0, 12, 16, 28, 32, 44]
    assert pod.MEDIUM_DT.itemsize in capi.abi_words()
    assert capi.lib().nxhip_abi_stamp() == capi.abi_stamp()
