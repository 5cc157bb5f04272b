"""The float64 yardstick of NX_MAT_METALROUGH (tests/metalrough_reference.py) checked against itself, the binary32 bar the device tests
use, and the material record's byte layout.  No GPU."""
import numpy as np

from nexus_amd import pod
from tests import metalrough_reference as R


def test_the_rule_is_reciprocal():
    """f(wi, wo) = f(wo, wi): f = f cos / cos(theta_o), for a coloured base at every (roughness, metallic) of the eval pin.  1e-9: binary64
    rounding (1.1e-16) of the half vector, amplified in D by up to 1 / alpha^2 = 4e5 at r = 0.05, with room for the dozen operations behind it"""
    rs = np.random.RandomState(2)
    a = rs.normal(size=(4000, 3))
    b = rs.normal(size=(4000, 3))
    a[:, 2], b[:, 2] = np.abs(a[:, 2]) + 0.02, np.abs(b[:, 2]) + 0.02
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    for r, m in R.EVAL_CASES + ((0.05, 0.5),):
        ref = R.MetalRough(R.BASE, r, 1.5, m)
        for k in range(0, 4000, 400):
            f_ab = ref.eval(a[k], b[k:k + 1])[0][0] / b[k, 2]
            f_ba = ref.eval(b[k], a[k:k + 1])[0][0] / a[k, 2]
            assert np.allclose(f_ab, f_ba, rtol=1e-9, atol=0.0), (r, m, k, f_ab, f_ba)


def test_albedo_and_pdf_stay_below_one():
    """white base colour over r in {0.05, 0.15, 0.3, 0.5, 1}, m in {0, 0.5, 1}, cos_i in {0.05, 0.5, 0.95}: the directional albedo and the
    integral of the pdf are at most 1 + the quadrature's own error — the 1500 x 1500 midpoint grid against the 750 x 750 one (at 1200 x
    1200 the r = 0.05 lobe is under-resolved and reads 1.07)."""
    fine, dw_f = R.upper_grid(1500, 1500)
    coarse, dw_c = R.upper_grid(750, 750)
    worst = 0.0
    for r in (0.05, 0.15, 0.3, 0.5, 1.0):
        for m in (0.0, 0.5, 1.0):
            ref = R.MetalRough((1.0, 1.0, 1.0), r, 1.5, m)
            for c in (0.05, 0.5, 0.95):
                wi = R.wi_of(c)
                f1, p1, _ = ref.eval(wi, fine)
                f2, p2, _ = ref.eval(wi, coarse)
                alb, alb_c = float(f1[:, 0].sum() * dw_f), float(f2[:, 0].sum() * dw_c)
                ip, ip_c = float(p1.sum() * dw_f), float(p2.sum() * dw_c)
                worst = max(worst, alb)
                assert alb <= 1.0 + abs(alb - alb_c) + 1e-9, ("albedo", r, m, c, alb, alb_c)
                assert ip <= 1.0 + abs(ip - ip_c) + 1e-9, ("pdf", r, m, c, ip, ip_c)
    print("largest directional albedo %.4f" % worst)
    # out of scope and stated: no multiple-scattering compensation — a white metal at r = 1 reflects about a third at cos_i = 0.9
    f, _, _ = R.MetalRough((1.0, 1.0, 1.0), 1.0, 1.5, 1.0).eval(R.wi_of(0.9), fine)
    assert abs(float(f[:, 0].sum() * dw_f) - 0.33) < 0.02


def test_sample_is_the_mixture_estimator_of_eval():
    """thr x pdf == f cos at the sampled direction, three numbers per sample on both branches, and the weight stays below about 1.7"""
    rng = np.random.RandomState(3).randint(1, 2**32 - 1, size=1 << 16, dtype=np.uint64).astype(np.uint32)
    top = 0.0
    for r, m in R.EVAL_CASES:
        ref = R.MetalRough(R.BASE, r, 1.5, m)
        for c in R.EVAL_COS:
            wi = R.wi_of(c)
            s = ref.sample(wi, rng)
            f, p, same = ref.eval(wi, s["wo"])
            ok = s["ok"]
            assert np.array_equal(same & (p > 1e-4) & np.isfinite(p), ok)
            assert np.allclose(s["thr"][ok] * s["pdf"][ok][:, None], f[ok], rtol=1e-12, atol=0.0)
            x = rng.copy()
            for _ in range(3):
                x = R.xorshift(x)[0]
            assert np.array_equal(s["rng_out"], x)
            assert 0 < s["spec"].mean() <= 1.0 and (m == 1.0) == bool(s["spec"].all()), "a pure metal has no diffuse lobe to pick"
            top = max(top, float(s["thr"][ok].max()))
    print("largest sample weight %.3f" % top)
    assert top < 1.75


def test_the_binary32_yardstick():
    """The rule in numpy float32 against the rule in float64 over the eval pin's grid, where pdf > 1e-3: the largest relative deviation
    measured is 1.84e-6 (f cos of the (0.6, 0) case at cos_i 0.9).  Four times that — 7.3e-6 — is the tolerance of the device's eval pin
    (tests/test_gpu_metalrough.py): the device's arithmetic has no exp and differs from numpy's in the order of operations and in the
    fused multiply-adds of its dot products only.  Above 3e-3 the formula's binary32 form would be wrong (the D denominator)."""
    y = R.binary32_yardstick()
    print("binary32 yardstick %.3g, eval tolerance %.3g" % (y, 4 * y))
    assert 1e-7 < y < 3e-3 / 4
    assert y < 1e-5, "the form of D that does not cancel: a few ulp, not a per cent"


def test_make_material_metalrough_byte_offsets():
    m = pod.make_material(pod.MAT_METALROUGH, albedo=(0.25, 0.5, 0.75), roughness=0.125, ior=1.75, metallic=0.625, emissive=(1, 2, 3), intensity=4.0, opacity=0.5,
                          diffuse_map=7, emissive_map=9)
    raw = np.frombuffer(m.tobytes(), dtype=np.uint8)
    assert pod.MAT_METALROUGH == 4 and raw.size == 60
    f = lambda at: float(np.frombuffer(raw[at:at + 4].tobytes(), np.float32)[0])  # noqa: E731
    assert [f(0), f(4), f(8)] == [0.25, 0.5, 0.75] and f(12) == 0.125 and f(16) == 1.75 and f(20) == 0.625 and f(24) == 0.0
    assert [f(28), f(32), f(36)] == [1.0, 2.0, 3.0] and f(40) == 4.0 and f(44) == 0.5
    assert np.frombuffer(raw[48:56].tobytes(), np.int32).tolist() == [7, 9] and int(raw[56].view(np.int8)) == 4
    assert float(pod.make_material(pod.MAT_METALROUGH)["u"][5]) == 1.0, "glTF's default metallicFactor"
    assert float(pod.make_material(pod.MAT_PLASTIC, roughness=0.3)["u"][5]) == 0.0, "the other types' records do not change"
