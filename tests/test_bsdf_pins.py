"""Algorithm-independent pins of the microfacet BSDFs and of the code that consumes them (NEE / MIS): VERDICT r5 item 2.

tests/test_physics_pins.py pins the Lambertian transport.  The rough dielectric, the rough plastic and the conductor
(Cuda/BSDF/DielectricBSDF.cuh:28-117, PlasticBSDF.cuh:30-106, ConductorBSDF.cuh:23-47 — the conductor's Eval is this repository's
own extension, the headline workload's material) were only ever compared device == oracle.  Here each side — the oracle on the CPU,
the device through the C-ABI hooks (-m gpu) — is held against things neither side's code can influence:

  (A) PUBLISHED FORMULAS restated a third time, in numpy, from the papers and not from either code: Beckmann's distribution and
      Smith's shadowing with Walter's rational fit (Walter et al. 2007, eq. 25-27), the half-vector Jacobians of reflection and
      refraction (eq. 13-17, 21, 38-41), the unpolarised Fresnel reflectance of a dielectric (as Snell's law + the sine / tangent
      form, not the cosine form the code uses) and of a conductor (complex index, complex arithmetic).  Eval and the pdf of every
      BSDF are compared pointwise with them.  Where the reference deviates from the published form, the deviation is a named,
      quantified QUIRK (the `Rperp` denominator of Fresnel.cuh:27-28), not a tolerance.
  (B) IDENTITIES between Sample, Eval and the pdf that hold for any correct importance sampler, evaluated by quadrature and Monte
      Carlo on the functions themselves: the pdf integrates to the probability that a sample is accepted; the samples are
      distributed with that pdf (a histogram over the sphere); E_sample[throughput] = the integral of Eval's f cos.  The plastic
      BSDF violates two of them BY CONSTRUCTION in the reference — its Sample returns the pdf of the lobe it picked where its Eval
      returns the mixture's, and picks the diffuse lobe with the Fresnel term of the sampled microfacet normal where Eval takes the
      half vector's (PlasticBSDF.cuh:52-63 against :75-103) — and the size of each violation is measured and bounded, not hidden.
  (C) TRANSPORT: a rectangular emitter mirrored in a glossy floor (plastic, dielectric, extended conductor), rendered by BSDF
      sampling alone and by NEE + MIS, each against a numpy quadrature of the estimator's expectation built from (A) — for the
      conductor and the dielectric the two expectations are the same integral; for the plastic floor they are NOT (the lobe pdf in
      the MIS weight: the weights of the three techniques do not sum to one near the highlight), and the prediction says by how
      much: the reference's plastic highlight under MIS is darker than the same highlight without MIS.  Mirrored, quantified, not
      fixed.  And a conductor furnace: a conductor floor under a uniform sky returns sky x directional albedo, the smooth one the
      Fresnel reflectance of (A) pixel by pixel, the rough one the quadrature of (A)'s lobe.

z-scores per block and colour channel as in test_physics_pins.py; every bar is stated where it is used."""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen, workloads
from tests import oracle_lib as O
from tests import scene_helpers as SH
from tests.test_physics_pins import _Estimate, _assert_agree, _z

# ---- (A) the published formulas, in numpy ---------------------------------------------------------------------------------


def np_alpha(cos_i, roughness):
    """the reference's roughness -> Beckmann width mapping (DielectricBSDF.cuh:24, PlasticBSDF.cuh:24, ConductorBSDF.cuh:19): not a
    published formula, a definition of the material — restated, because every lobe below is a function of it"""
    return np.clip((1.2 - 0.2 * np.sqrt(np.abs(cos_i))) * roughness * roughness, 1.0e-4, 1.0)


def np_beckmann_d(alpha, cos_m):
    """Walter 2007 eq. 25"""
    c2 = cos_m * cos_m
    return np.exp(-(1.0 - c2) / (c2 * alpha * alpha)) / (np.pi * alpha * alpha * c2 * c2)


def np_smith_g1(alpha, cos_v):
    """Walter 2007 eq. 27 (the rational fit), a = 1 / (alpha tan theta)"""
    s = np.sqrt(np.maximum(1.0 - cos_v * cos_v, 1e-12))
    a = cos_v / (alpha * s)
    return np.where(a < 1.6, (3.535 * a + 2.181 * a * a) / (1.0 + 2.276 * a + 2.577 * a * a), 1.0)


def np_fresnel_dielectric(n_i_over_n_t, cos_i, quirk):
    """Unpolarised reflectance of a dielectric interface.  quirk False: Snell + the sine / tangent form of Fresnel's equations
    (Born & Wolf 1.5.2) — an algebraically different route from the code's.  quirk True: what Fresnel.cuh:9-31 computes — the
    cosine form with `eta * cosThetaT + cosThetaT` in the denominator of its `Rperp` (:28) where the equation has
    `eta * cosThetaT + cosThetaI`."""
    eta = np.where(cos_i < 0.0, 1.0 / n_i_over_n_t, n_i_over_n_t) * np.ones_like(cos_i)
    ci = np.abs(cos_i)
    s2t = eta * eta * (1.0 - ci * ci)
    tir = s2t > 1.0
    s2t = np.minimum(s2t, 1.0)
    if quirk:
        ct = np.sqrt(np.maximum(0.0, 1.0 - s2t))
        a = (eta * ci - ct) / (eta * ci + ct)
        with np.errstate(divide="ignore", invalid="ignore"):
            b = (eta * ct - ci) / (eta * ct + ct)
        r = 0.5 * (a * a + b * b)
    else:
        ti, tt = np.arccos(np.clip(ci, 0.0, 1.0)), np.arcsin(np.sqrt(s2t))
        with np.errstate(divide="ignore", invalid="ignore"):
            rs = (np.sin(ti - tt) / np.sin(ti + tt)) ** 2
            rp = (np.tan(ti - tt) / np.tan(ti + tt)) ** 2
        normal = ti < 1e-6
        r0 = ((1.0 - eta) / (1.0 + eta)) ** 2
        r = np.where(normal, r0, 0.5 * (rs + rp))
    return np.where(tir, 1.0, r)


def np_fresnel_conductor(eta, k, cos_i):
    """Unpolarised reflectance of a conductor in air: Fresnel's equations with the complex index n = eta + i k"""
    c = np.clip(cos_i, 0.0, 1.0).astype(np.complex128)
    n = eta + 1j * k
    root = np.sqrt(n * n - (1.0 - c * c))
    rs = (c - root) / (c + root)
    rp = (n * n * c - root) / (n * n * c + root)
    return 0.5 * (np.abs(rs) ** 2 + np.abs(rp) ** 2)


class Lobes:
    """f cos and the pdfs of one material for directions given in the local frame (z = normal), from the formulas above.
    spec_f: reflection lobe x cos(theta_o) (RGB); spec_pdf: density with which Sample produces a reflected direction (selection
    probability included); sel: that selection probability's Fresnel term at the half vector."""

    def __init__(self, mat, quirk=True):
        self.type = int(mat["type"])
        u = mat["u"]
        self.quirk = quirk
        if self.type == pod.MAT_CONDUCTOR:
            self.eta, self.k, self.rough = np.array(u[0:3], np.float64), np.array(u[3:6], np.float64), float(u[6])
        else:
            self.albedo, self.rough, self.ior = np.array(u[0:3], np.float64), float(u[3]), float(u[4])

    def fresnel(self, wi_dot_m):
        if self.type == pod.MAT_CONDUCTOR:
            return np.stack([np_fresnel_conductor(self.eta[c], self.k[c], wi_dot_m) for c in range(3)], -1)
        return np_fresnel_dielectric(1.0 / self.ior, wi_dot_m, self.quirk)[..., None] * np.ones(3)

    def reflection(self, wi, wo):
        """wi (3,), wo (..., 3), same side.  Returns f cos (..., 3), the lobe's own pdf D (m.n) / (4 wi.m) (...,), Fresnel (..., 3)"""
        alpha = np_alpha(wi[2], self.rough)
        h = wi + wo
        h = h / np.linalg.norm(h, axis=-1, keepdims=True) * np.sign(wi[2])
        wi_m = np.abs(h @ wi)
        D = np_beckmann_d(alpha, np.abs(h[..., 2]))
        G = np_smith_g1(alpha, np.abs(wo[..., 2])) * np_smith_g1(alpha, abs(wi[2]))
        F = self.fresnel(h @ wi)
        return F * (G * D / (4.0 * abs(wi[2])))[..., None], D * np.abs(h[..., 2]) / (4.0 * wi_m), F

    def eval(self, wi, wo):
        """Eval's f cos (..., 3) and pdf (...,) for wo on the reflection side of wi (the transmission side: refraction())"""
        f, p, F = self.reflection(wi, wo)
        if self.type == pod.MAT_CONDUCTOR:
            return f, p
        if self.type == pod.MAT_DIELECTRIC:
            return f, F[..., 0] * p
        cos_o = np.abs(wo[..., 2])
        return f + (1.0 - F) * self.albedo * (cos_o / np.pi)[..., None], F[..., 0] * p + (1.0 - F[..., 0]) * cos_o / np.pi

    def refraction(self, wi, wo):
        """dielectric, wo on the other side: Walter eq. 21 x cos(theta_o) and eq. 17 / 41's pdf, eta = n_i / n_t"""
        alpha = np_alpha(wi[2], self.rough)
        eta = self.ior if wi[2] < 0.0 else 1.0 / self.ior
        h = -(eta * wi + wo)
        h = h / np.linalg.norm(h, axis=-1, keepdims=True)
        wi_m, wo_m = h @ wi, np.sum(h * wo, -1)
        D = np_beckmann_d(alpha, np.abs(h[..., 2]))
        G = np_smith_g1(alpha, np.abs(wo[..., 2])) * np_smith_g1(alpha, abs(wi[2]))
        F = np_fresnel_dielectric(1.0 / self.ior, wi_m, self.quirk)
        den = (eta * wi_m + wo_m) ** 2
        f = np.abs(wi_m * wo_m) * (1.0 - F) * G * D / (abs(wi[2]) * den)
        pdf = (1.0 - F) * D * np.abs(h[..., 2]) * np.abs(wo_m) / den
        # (a half vector on the wrong side of the macro surface is no microfacet of a height field: the code evaluates D(m.z) with a
        #  negative m.z like a positive one; those directions are excluded by the caller)
        return f[..., None] * self.albedo, pdf, h[..., 2]


MATS = {
    "conductor r0.3": pod.make_material(pod.MAT_CONDUCTOR, roughness=0.3, conductor_ior=(0.2, 0.9, 1.1), conductor_k=(3.9, 2.4, 2.2)),  # configs[1]'s mesh
    "conductor r0.6": pod.make_material(pod.MAT_CONDUCTOR, roughness=0.6, conductor_ior=(1.1, 0.8, 0.6), conductor_k=(6.8, 5.0, 4.1)),
    "plastic r0.4": pod.make_material(pod.MAT_PLASTIC, albedo=(0.8, 0.3, 0.2), roughness=0.4, ior=1.5),
    "plastic r0.6": pod.make_material(pod.MAT_PLASTIC, albedo=(0.2, 0.5, 0.9), roughness=0.6, ior=1.33),
    "dielectric r0.5": pod.make_material(pod.MAT_DIELECTRIC, albedo=(0.95, 0.97, 1.0), roughness=0.5, ior=1.45),  # (configs[3]'s BSDF at a width a grid resolves)
    "dielectric r0.7": pod.make_material(pod.MAT_DIELECTRIC, albedo=(1.0, 0.9, 0.8), roughness=0.7, ior=1.8),
}


def _wi(cos_i, phi=0.7):
    s = np.sqrt(1.0 - cos_i * cos_i)
    return np.array([s * np.cos(phi), s * np.sin(phi), cos_i])


def _sphere_grid(n_theta, n_phi, lower):
    """midpoints in (cos theta, phi) — equal solid angles; the upper hemisphere, or the whole sphere"""
    lo = -1.0 if lower else 0.0
    cz = lo + (np.arange(n_theta) + 0.5) * (1.0 - lo) / n_theta
    ph = (np.arange(n_phi) + 0.5) * 2.0 * np.pi / n_phi
    czz, pp = np.meshgrid(cz, ph, indexing="ij")
    s = np.sqrt(1.0 - czz * czz)
    wo = np.stack([s * np.cos(pp), s * np.sin(pp), czz], -1).reshape(-1, 3)
    return wo, (1.0 - lo) * 2.0 * np.pi / (n_theta * n_phi)


def _queries(wi, wo=None, n=None, seed=1):
    n = len(wo) if wo is not None else n
    q = np.zeros(n, dtype=pod.BSDF_QUERY_DT)
    q["wi"] = wi.astype(np.float32)
    if wo is not None:
        q["wo"] = wo.astype(np.float32)
    q["rng"] = np.random.RandomState(seed).randint(1, 2**32 - 1, size=n, dtype=np.uint64).astype(np.uint32)
    return q


# ---- (A) pointwise: Eval against the published formulas ---------------------------------------------------------------------

def _check_eval_against_formulas(eval_batch):
    for name, mat in MATS.items():
        lob = Lobes(mat)
        both = int(mat["type"]) == pod.MAT_DIELECTRIC
        for cos_i in ((0.9, 0.5, 0.2, -0.7) if both else (0.9, 0.5, 0.2)):
            wi = _wi(cos_i)
            wo, _ = _sphere_grid(96, 192, lower=both)
            r = eval_batch(mat, _queries(wi, wo))
            same = wo[:, 2] * wi[2] > 0.0
            f, p = lob.eval(wi, wo[same])
            # where the lobe has any weight at all (binary32 exp underflows long before the formulas do)
            sig = p > 1e-3
            if both:
                # (at the critical angle the reflectance has an infinite slope in cos: binary32 and binary64 may differ by a per cent
                #  within a hair of it — left out, on the formula's own numbers)
                hh = wi + wo[same]
                hh /= np.linalg.norm(hh, axis=-1, keepdims=True)
                ee = np.where(hh @ wi * np.sign(wi[2]) < 0.0, lob.ior, 1.0 / lob.ior) if wi[2] > 0 else lob.ior
                sig &= np.abs(ee * ee * (1.0 - (hh @ wi) ** 2) - 1.0) > 5e-3
            got_f, got_p = r["throughput"][same].astype(np.float64), r["pdf"][same].astype(np.float64)
            assert np.allclose(got_p[sig], p[sig], rtol=2e-4), (name, cos_i, "pdf", np.abs(got_p[sig] / p[sig] - 1).max())
            assert np.allclose(got_f[sig], f[sig], rtol=3e-4, atol=1e-7), (name, cos_i, "f cos", np.abs(got_f[sig] / np.maximum(f[sig], 1e-12) - 1).max())
            # the validity rule (Sampler.cuh:58-61) is part of the function: valid iff pdf > 1e-4 (undecided within rounding of the bar)
            clear = np.abs(p - 1e-4) > 1e-6
            assert np.array_equal(r["ok"][same][clear] == 1, (p > 1e-4)[clear]), (name, cos_i, "validity")
            if both:
                f2, p2, mz = lob.refraction(wi, wo[~same])
                ok = (mz > 0.0) & (p2 > 1e-3)
                g_f, g_p = r["throughput"][~same].astype(np.float64), r["pdf"][~same].astype(np.float64)
                assert ok.sum() > 150
                # (3e-3: (eta wi.m + wo.m)^2 is a difference of two O(1) terms in binary32 — the reflection lobes above hold 3e-4)
                assert np.allclose(g_p[ok], p2[ok], rtol=3e-3), (name, cos_i, "refraction pdf", np.abs(g_p[ok] / p2[ok] - 1).max())
                assert np.allclose(g_f[ok], f2[ok], rtol=3e-3, atol=1e-7), (name, cos_i, "refraction f cos")
    # and the quirk itself, quantified (so that a reader knows what "mirrored" costs): reflectance at ior 1.5
    c = np.cos(np.radians([0.0, 30.0, 45.0, 60.0, 75.0, 85.0]))
    exact, quirk = np_fresnel_dielectric(1 / 1.5, c, False), np_fresnel_dielectric(1 / 1.5, c, True)
    print("Fresnel.cuh:28 at ior 1.5, 0/30/45/60/75/85 deg: exact %s, reference %s" % (np.round(exact, 4), np.round(quirk, 4)))
    assert abs(exact[0] - 0.04) < 1e-3 and abs(quirk[0] - exact[0]) < 1e-9, "equal at normal incidence"
    assert abs(exact[3] - quirk[3]) < 1e-3 and 0.02 < exact[4] - quirk[4] < 0.05 and 0.15 < exact[5] - quirk[5] < 0.25, "the reference under-reflects towards grazing: -0.03 at 75 deg, -0.19 at 85 deg"


# ---- (B) identities between Sample, Eval and the pdf -------------------------------------------------------------------------

N_SAMPLES = 1 << 19


def _check_identities(sample_batch, eval_batch):
    report = []
    for name, mat in MATS.items():
        lob = Lobes(mat)
        mtype = int(mat["type"])
        both = mtype == pod.MAT_DIELECTRIC
        for cos_i in ((0.9, 0.45, -0.7) if both else (0.9, 0.45)):
            wi = _wi(cos_i)
            s = sample_batch(mat, _queries(wi, n=N_SAMPLES, seed=int(abs(cos_i) * 100) + mtype))
            ok = s["ok"] == 1
            thr = np.where(ok[:, None], s["throughput"].astype(np.float64), 0.0)
            assert np.isfinite(thr).all()
            mc, mc_se = thr.mean(0), thr.std(0) / np.sqrt(N_SAMPLES)
            p_ok, p_ok_se = ok.mean(), np.sqrt(ok.mean() * (1 - ok.mean()) / N_SAMPLES)
            wo, dw = _sphere_grid(648, 1296, lower=both)  # (multiples of the histogram's 12 or 24 x 24 cells: every grid point lies inside one cell)
            r = eval_batch(mat, _queries(wi, wo))
            valid = r["ok"] == 1
            i_pdf = float(np.where(valid, r["pdf"].astype(np.float64), 0.0).sum() * dw)
            i_f = np.where(valid[:, None], r["throughput"].astype(np.float64), 0.0).sum(0) * dw
            # (a density integrates to at most one.  The reference's plastic Eval does not: F(wi.h) pdfSpecular + (1 - F(wi.h)) pdfDiffuse is a
            #  convex combination per DIRECTION with a weight that varies over the sphere, not a mixture of two densities — up to 1.06
            #  at oblique incidence; reported in the plastic branch below, asserted for the others)
            assert mtype == pod.MAT_PLASTIC or (both and cos_i < 0.0) or i_pdf < 1.0 + 2e-3, (name, cos_i, "the pdf integrates to more than one", i_pdf)
            # -- histogram of the accepted samples against the pdf: 12 x 24 cells of equal solid angle
            nt, nphi = 12 * (2 if both else 1), 24
            lo = -1.0 if both else 0.0
            w = s["wo"][ok].astype(np.float64)
            ct = np.clip(((w[:, 2] - lo) / (1.0 - lo) * nt).astype(int), 0, nt - 1)
            cp = np.clip((np.mod(np.arctan2(w[:, 1], w[:, 0]), 2 * np.pi) / (2 * np.pi) * nphi).astype(int), 0, nphi - 1)
            counts = np.bincount(ct * nphi + cp, minlength=nt * nphi).astype(np.float64)
            gt = np.clip(((wo[:, 2] - lo) / (1.0 - lo) * nt).astype(int), 0, nt - 1)
            gp = np.clip((np.mod(np.arctan2(wo[:, 1], wo[:, 0]), 2 * np.pi) / (2 * np.pi) * nphi).astype(int), 0, nphi - 1)
            expect = np.bincount(gt * nphi + gp, weights=np.where(valid, r["pdf"].astype(np.float64), 0.0) * dw, minlength=nt * nphi) * N_SAMPLES
            big = expect > 200.0
            zc = (counts[big] - expect[big]) / np.sqrt(expect[big] + (2e-3 * expect[big]) ** 2)  # (2e-3: the quadrature of a cell)
            if both and cos_i < 0.0:
                # From INSIDE the glass the reference's reflectance is not a probability: Fresnel.cuh:28's denominator `eta cosT + cosT`
                # goes to zero towards the critical angle, so "F" exceeds one for the microfacets just below total reflection (and is 1
                # above).  Sample then always reflects there (rand < F), Eval multiplies the reflection pdf by F > 1 and gets a negative
                # refraction pdf (1 - F < 0: invalid, dropped).  So the identities cannot hold; what must hold is each side's OWN model:
                alpha = np_alpha(wi[2], lob.rough)
                rs = np.random.RandomState(5)
                t2 = -alpha * alpha * np.log(1.0 - rs.rand(400000))
                cm = 1.0 / np.sqrt(1.0 + t2)
                ph = 2 * np.pi * rs.rand(400000)
                m = np.stack([np.sqrt(1 - cm * cm) * np.cos(ph), np.sqrt(1 - cm * cm) * np.sin(ph), cm], -1)
                wim = m @ wi
                F = np_fresnel_dielectric(1.0 / lob.ior, wim, True)
                refl = 2.0 * wim[:, None] * m - wi
                stays = refl[:, 2] * wi[2] > 0.0
                want_refl = float((np.minimum(F, 1.0) * stays).mean())
                want_refr_max = float(np.maximum(1.0 - F, 0.0).mean())
                got_refl = float((ok & (s["wo"][:, 2] * wi[2] > 0.0)).mean())
                got_refr = float((ok & (s["wo"][:, 2] * wi[2] < 0.0)).mean())
                assert abs(got_refl - want_refl) < 6e-3, (name, cos_i, got_refl, want_refl)
                assert got_refr < want_refr_max + 6e-3 and got_refr > want_refr_max - 0.03, (name, cos_i, got_refr, want_refr_max)  # (minus the rejected refractions)
                refl_side = wo[:, 2] * wi[2] > 0.0
                i_refl = float(np.where(valid & refl_side, r["pdf"].astype(np.float64), 0.0).sum() * dw)
                want_i_refl = float((F * stays).mean())
                report.append("%-16s cos %.2f (inside): 'F' > 1 for %.1f %% of the microfacets (max %.1f); the sampler reflects with probability %.3f "
                              "(E min(F, 1) = %.3f) where Eval's reflection pdf integrates to %.3f" %
                              (name, cos_i, 100.0 * (F > 1.0 + 1e-6).mean(), F.max(), got_refl, want_refl, i_refl))
                assert (F > 1.0 + 1e-6).mean() > 0.004 and F.max() > 10.0, "the quirk is there: a thin shell of microfacets just below the critical angle, with an unbounded value"
                continue
            if mtype != pod.MAT_PLASTIC:
                # a correct sampler: accepted mass = the integral of the pdf, E[throughput] = the integral of f cos, histogram = pdf
                assert abs(i_pdf - p_ok) < 4.5 * p_ok_se + 2e-3, (name, cos_i, "accepted mass", i_pdf, p_ok)
                zf = (mc - i_f) / np.sqrt(mc_se ** 2 + (3e-3 * i_f) ** 2)
                assert np.abs(zf).max() < 4.5, (name, cos_i, "E[throughput] against the integral of f cos", mc, i_f)
                assert np.abs(zc).max() < 5.0 and (zc * zc).mean() < 1.8, (name, cos_i, "histogram", np.abs(zc).max(), (zc * zc).mean())
                report.append("%-16s cos %.2f: accepted %.4f = int pdf %.4f; E[thr] %s = int f cos %s; histogram max |z| %.1f over %d cells" %
                              (name, cos_i, p_ok, i_pdf, np.round(mc, 4), np.round(i_f, 4), np.abs(zc).max(), big.sum()))
            else:
                # The reference's plastic (PlasticBSDF.cuh:75-103): the microfacet normal m is drawn first, the lobe is picked with F(wi.m)
                # — so the diffuse lobe is picked with probability 1 - Fbar, Fbar = E_m[F(wi.m)], and its throughput is the bare albedo —
                # while Eval weights the diffuse term with 1 - F(wi.h) of the half vector.  Both are legitimate models of "specular
                # coat over diffuse base"; they are not the same model.  Measured: the two diffuse weights, per direction of incidence.
                alpha = np_alpha(wi[2], lob.rough)
                rs = np.random.RandomState(5)
                t2 = -alpha * alpha * np.log(1.0 - rs.rand(200000))
                cm = 1.0 / np.sqrt(1.0 + t2)
                ph = 2 * np.pi * rs.rand(200000)
                m = np.stack([np.sqrt(1 - cm * cm) * np.cos(ph), np.sqrt(1 - cm * cm) * np.sin(ph), cm], -1)
                fbar = float(np_fresnel_dielectric(1.0 / lob.ior, m @ wi, True).mean())
                up, dwu = _sphere_grid(256, 512, lower=False)
                _, _, F = lob.reflection(wi, up)
                eval_diffuse = float(((1.0 - F[:, 0]) * up[:, 2] / np.pi).sum() * dwu)  # the diffuse lobe's weight in Eval
                spec_f, spec_p, Fh = lob.reflection(wi, up)
                spec_mass = float((Fh[:, 0] * spec_p).sum() * dwu)
                # Sample's accepted mass and mean throughput, predicted from the formulas with ITS model ...
                want_ok = spec_mass + (1.0 - fbar)
                want_mc = (spec_f.sum(0) * dwu) + (1.0 - fbar) * lob.albedo
                assert abs(p_ok - want_ok) < 4.5 * p_ok_se + 3e-3, (name, cos_i, p_ok, want_ok)
                assert np.abs((mc - want_mc) / np.sqrt(mc_se ** 2 + (4e-3 * want_mc) ** 2)).max() < 4.5, (name, cos_i, mc, want_mc)
                # ... and Eval's integrals with Eval's
                assert abs(i_pdf - (spec_mass + eval_diffuse)) < 3e-3, (name, cos_i, i_pdf, spec_mass + eval_diffuse)
                assert np.abs(i_f - (spec_f.sum(0) * dwu + eval_diffuse * lob.albedo)).max() < 3e-3
                gap = (1.0 - fbar) - eval_diffuse
                report.append("%-16s cos %.2f: diffuse weight in Sample %.4f (1 - E_m F(wi.m)), in Eval %.4f (int (1 - F(wi.h)) cos / pi): gap %+.4f; "
                              "accepted %.4f, int pdf %.4f" % (name, cos_i, 1.0 - fbar, eval_diffuse, gap, p_ok, i_pdf))
                assert abs(gap) < 0.2, "measured: up to 0.12 at roughness 0.6, 63 degrees of incidence (the report above carries every case)"
                assert i_pdf < 1.08, "PlasticBSDF.cuh:58-63: Eval's pdf is not normalised (see above); it stays within 8 % of a density"
    print("\n".join(report))


# ---- (C) transport ------------------------------------------------------------------------------------------------------------

FLOOR_LIGHT = (-3.4, -2.2, -0.7, 0.5, 1.0)  # x0, x1, z0, z1, height: where the floor mirrors it towards the camera
FLOOR_LE = 6.0
EYE = np.array((3.0, 0.8, 0.3))
BLOCK = 8


def _floor_scene(W, H, mat, use_mis, sky=0.0):
    x0, x1, z0, z1, h = FLOOR_LIGHT
    floor = scenegen.quad((-8, 0, -8), (-8, 0, 8), (8, 0, 8), (8, 0, -8))  # (normal +y: the dielectric is entered from the air)
    meshes, placements = [floor], [(0, 0, workloads.IDENTITY)]
    mats = [mat]
    if sky == 0.0:
        meshes.append(scenegen.quad((x0, h, z0), (x1, h, z0), (x1, h, z1), (x0, h, z1)))
        placements.append((1, 1, workloads.IDENTITY))
        mats.append(pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), emissive=(1.0, 1.0, 1.0), intensity=FLOOR_LE))
    fwd = np.array((0.0, 0.0, 0.0)) - EYE
    cam = capi.camera_init(tuple(EYE), fwd / np.linalg.norm(fwd), 20.0, W, H, 5.0, 0.0)
    sc = SH.BuiltScene(meshes, placements, materials=np.array(mats, dtype=pod.MAT_DT), camera=cam,
                       settings=workloads.make_settings(use_mis=use_mis, path_length=2, background=(1, 1, 1), background_intensity=sky))
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    return sc


def _pixel_geometry(scene, W, H):
    """per pixel centre: the floor point and the unit direction back to the camera, in the floor's local frame (x, z, y -> x, y, z)"""
    cam = scene.camera
    pos = cam["position"].astype(np.float64)
    jj, ii = np.mgrid[0:H, 0:W]
    x, y = ((ii + 0.5) / W).reshape(-1, 1), ((jj + 0.5) / H).reshape(-1, 1)
    d = cam["lowerLeftCorner"].astype(np.float64) + cam["viewportX"].astype(np.float64) * x + cam["viewportY"].astype(np.float64) * y - pos
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = -pos[1] / d[:, 1]
    assert np.all(t > 0)
    p = pos + d * t[:, None]
    assert np.all(np.abs(p[:, 0]) < 8) and np.all(np.abs(p[:, 2]) < 8)
    to_local = lambda v: np.stack([v[..., 0], v[..., 2], v[..., 1]], -1)
    return to_local(p), to_local(-d)


def _block_mean(values, W, H):
    jj, ii = np.mgrid[0:H, 0:W]
    ids = ((jj // BLOCK) * (W // BLOCK) + ii // BLOCK).reshape(-1)
    nb = (W // BLOCK) * (H // BLOCK)
    return np.stack([np.bincount(ids, weights=values[:, c], minlength=nb) for c in range(3)], 1) / np.bincount(ids, minlength=nb)[:, None]


def _rectangle_nodes(n_light=28):
    """the rectangular emitter FLOOR_LIGHT as a light for _floor_expectation: seen from the floor point p (local frame), the unit
    directions to n_light x n_light midpoints, their solid angles, the radiance and the light sample's pdf per solid angle"""
    x0, x1, z0, z1, h = FLOOR_LIGHT
    area = (x1 - x0) * (z1 - z0)
    gx = x0 + (np.arange(n_light) + 0.5) * (x1 - x0) / n_light
    gz = z0 + (np.arange(n_light) + 0.5) * (z1 - z0) / n_light
    lx, lz = np.meshgrid(gx, gz, indexing="ij")
    Y = np.stack([lx.reshape(-1), lz.reshape(-1), np.full(lx.size, h)], -1)  # local frame: (x, z, height)
    dA = area / Y.shape[0]

    def nodes(p):
        v = Y - p
        d2 = np.sum(v * v, -1)
        wo = v / np.sqrt(d2)[:, None]
        cos_l = np.abs(wo[:, 2])                  # the emitter is parallel to the floor
        # p_light: 1 / (lights x triangles x triangle area) x d^2 / cos (PathTracer.cu:262-266)
        return wo, cos_l * dA / d2, FLOOR_LE, d2 / (area * cos_l)

    return nodes


def _floor_expectation(mat, scene, W, H, light=None, n_m=96, light_is_hit=True, pixels=None):
    """E[radiance] per block of the two estimators, from the formulas of (A) and the reference's estimator structure
    (PathTracer.cu:213-308 NEE, :352-385 emission MIS, the BSDFs' Sample): (naive, mis), each (blocks, 3).

    `light(p)`: the light as quadrature nodes seen from the floor point p — (omega (n, 3) in the local frame, d(omega) (n,), radiance
    L (scalar or (n, 3)), p_light (n,): the pdf per solid angle with which the light sample draws that direction; optionally a fifth,
    the light pdf the BSDF sample's weight is formed with, where a test of the checker makes the two differ); default: the
    rectangular emitter.  `light_is_hit`: a BSDF-sampled ray that finds the light HITS a surface (an emitter): it goes through the
    roulette and, under MIS, an invalid p_light gives it weight 0; False (the environment): it leaves the scene, which is accounted
    before the roulette, and an invalid p_light leaves it unweighted.  `pixels`: the pixels (a boolean mask) the blocks' means are
    taken over — default all; a regular subset where the light costs many nodes."""
    lob = Lobes(mat)
    P, WI = _pixel_geometry(scene, W, H)
    light = light if light is not None else _rectangle_nodes()
    use = np.ones(len(P), bool) if pixels is None else pixels
    naive, mis = np.zeros((len(P), 3)), np.zeros((len(P), 3))
    wsum = np.ones(len(P))  # the two techniques' weights on the SPECULAR part of the integrand, summed and averaged over the highlight
    rs = np.random.RandomState(11)
    power = lambda a, b: a * a / (a * a + b * b)
    for k in np.flatnonzero(use):
        wi = WI[k]
        wo, dw, L, p_l, *other = light(P[k])
        p_b = other[0] if other else p_l  # (a checker's edit: another light pdf in the BSDF sample's weight than in the light sample's)
        L = np.asarray(L, np.float64) * np.ones((len(wo), 3))
        spec_f, spec_p, F = lob.reflection(wi, wo)
        f_e, p_e = lob.eval(wi, wo)
        sel = np.ones(len(wo)) if lob.type == pod.MAT_CONDUCTOR else F[:, 0]
        p_s = sel * spec_p                        # the pdf Sample returns for a reflected direction
        ok_s, ok_e, ok_l = p_s > 1e-4, p_e > 1e-4, p_l > 1e-4
        if lob.type == pod.MAT_CONDUCTOR:
            ok_s = np.ones_like(ok_s)             # (ConductorBSDF.cuh:47 returns true whatever the pdf)
        # The reference's Russian roulette (PathTracer.cu:167-175): a path that HITS something survives with probability max(throughput),
        # un-clamped, and is divided by it.  Where a sample's throughput exceeds one — Walter's weight wi.m G2 / (wi.n m.n) at grazing
        # incidence does — it "survives with probability > 1" and is still divided: E[throughput] drops by 1 / max(throughput).
        # A quirk of the reference, mirrored by device and oracle; here it is part of the estimator whose expectation is predicted
        # (the furnace below is free of it: a miss is accounted before the roulette, :151-164).
        with np.errstate(divide="ignore", invalid="ignore"):
            T = np.where(p_s[:, None] > 0.0, spec_f / p_s[:, None], 0.0)
        rr = np.minimum(1.0, 1.0 / np.maximum(T.max(-1), 1e-30)) if light_is_hit else 1.0
        w_s = np.where(p_b > 1e-4, power(p_s, p_b), 0.0 if light_is_hit else 1.0)  # the BSDF sample's weight under MIS
        n = (spec_f * L * (ok_s * rr * dw)[:, None]).sum(0)
        m = (f_e * L * (ok_e * ok_l * power(p_l, p_e) * dw)[:, None]).sum(0) + (spec_f * L * (ok_s * rr * w_s * dw)[:, None]).sum(0)
        g = spec_f[:, 1] * ok_l * dw
        if g.sum() > 0.0:
            wsum[k] = float((g * (ok_e * power(p_l, p_e) + ok_s * power(p_s, p_l))).sum() / g.sum())
        if lob.type == pod.MAT_PLASTIC:
            # the diffuse lobe, picked with 1 - F(wi.m) of a DRAWN microfacet normal, pdf (1 - F(wi.m)) cos / pi
            alpha = np_alpha(wi[2], lob.rough)
            t2 = -alpha * alpha * np.log(1.0 - rs.rand(n_m))
            cm = 1.0 / np.sqrt(1.0 + t2)
            ph = 2 * np.pi * rs.rand(n_m)
            mm = np.stack([np.sqrt(1 - cm * cm) * np.cos(ph), np.sqrt(1 - cm * cm) * np.sin(ph), cm], -1)
            Fm = np_fresnel_dielectric(1.0 / lob.ior, mm @ wi, True)                    # (n_m,)
            c = wo[:, 2] / np.pi                                                        # (light points,)
            p_d = (1.0 - Fm)[:, None] * c[None, :]
            ok_d = p_d > 1e-4
            pick = ((1.0 - Fm)[:, None] * ok_d).mean(0)                                 # E_m[(1 - F_m) valid]
            pick_w = ((1.0 - Fm)[:, None] * ok_d * np.where(ok_l[None, :], power(p_d, p_l[None, :]), 0.0)).mean(0)
            n = n + lob.albedo * (L * (pick * c * dw)[:, None]).sum(0)
            m = m + lob.albedo * (L * (pick_w * c * dw)[:, None]).sum(0)
        naive[k], mis[k] = n, m
    if pixels is not None:  # the blocks' means over the chosen pixels only
        count = _block_mean(np.repeat(use[:, None].astype(np.float64), 3, 1), W, H)
        assert np.all(count > 0)
        return _block_mean(naive * use[:, None], W, H) / count, _block_mean(mis * use[:, None], W, H) / count, _block_mean(wsum[:, None] * use[:, None] * np.ones(3), W, H)[:, 0] / count[:, 0]
    return _block_mean(naive, W, H), _block_mean(mis, W, H), _block_mean(np.repeat(wsum[:, None], 3, 1), W, H)[:, 0]


def _check_glossy_floor(estimate, frames, rel_se_bar):
    floors = {
        "conductor (extended)": MATS["conductor r0.3"],
        "plastic": pod.make_material(pod.MAT_PLASTIC, albedo=(0.6, 0.4, 0.2), roughness=0.45, ior=1.5),
        "dielectric": pod.make_material(pod.MAT_DIELECTRIC, albedo=(1.0, 1.0, 1.0), roughness=0.45, ior=1.5),
    }
    for name, mat in floors.items():
        est = {}
        for use_mis in (False, True):
            est[use_mis] = estimate(lambda W, H: _floor_scene(W, H, mat, use_mis), frames)
        e = est[True]
        want_naive, want_mis, wsum = _floor_expectation(mat, _floor_scene(e.W, e.H, mat, True), e.W, e.H)
        lit = want_naive.max(1) > 0.05 * want_naive.max()
        assert lit.mean() > 0.3, "the camera must see the emitter's reflection"
        assert np.median(est[True].se[lit] / want_mis[lit]) < rel_se_bar, "the estimate is too noisy for its pass to mean anything"
        ratio = (want_mis[lit] / want_naive[lit])
        print("%s floor: predicted E[NEE + MIS] / E[BSDF sampling] over the lit blocks: min %.3f, mean %.3f, max %.3f" % (name, ratio.min(), ratio.mean(), ratio.max()))
        # (1 %: pixel-centre evaluation of the expectation inside a block, the quadrature over the emitter, the offset of the shadow rays' origins)
        _assert_agree(_z(est[False].mean, est[False].se, want_naive, 0.0, systematic=1e-2)[lit], "%s floor, BSDF sampling alone, against the formulas" % name)
        _assert_agree(_z(est[True].mean, est[True].se, want_mis, 0.0, systematic=1e-2)[lit], "%s floor, NEE + MIS, against the formulas" % name)
        if "plastic" not in name:
            # One integral, two estimators — up to the roulette (see _floor_expectation): it takes from the BSDF-sampled hits only, so the
            # NEE + MIS image is never the darker one, and is the brighter one where Walter's weight exceeds one (grazing incidence)
            # (the weights sum to one wherever both pdfs are `valid`; the dielectric's reflection pdf carries F ~ 0.04 and falls below the
            #  rule's 1e-4 in the lobe's skirt, where both techniques then contribute nothing: Sampler.cuh:58-61, the loss round 5's furnace found)
            print("%s floor: the two weights on the specular lobe sum to %.4f .. %.4f over the lit blocks" % (name, wsum[lit].min(), wsum[lit].max()))
            assert ratio.min() > 1.0 - 2e-3 and wsum[lit].max() < 1.0 + 1e-9 and (wsum[lit].min() > 0.999 or "conductor" not in name)
            assert np.median(est[True].se[lit]) < np.median(est[False].se[lit])
        else:
            # PlasticBSDF.cuh: Sample's pdf is the picked lobe's, Eval's the mixture's -> the power heuristic's weights do not sum to one
            # where both lobes matter: under MIS the reference loses part of the highlight.  Quantified here, mirrored on both sides.
            print("plastic floor: the power heuristic's two weights on the specular lobe sum to %.3f .. %.3f over the lit blocks (1 = unbiased)" % (wsum[lit].min(), wsum[lit].max()))
            assert wsum[lit].min() < 0.98, "the prediction itself must show the loss (in this geometry the emitter's pdf is large against both lobes, so NEE carries most of the weight: 4 % at most; the loss grows as the emitter's pdf approaches the lobe's)"


def _check_conductor_furnace(estimate, frames):
    """a conductor floor under a uniform sky of radiance 1: radiance = directional albedo of the lobe (rays reflected below the floor
    are dropped by Sample: ConductorBSDF.cuh:41-42; the quadrature covers the upper hemisphere only, so it drops them too)"""
    for name, mat in (("smooth", pod.make_material(pod.MAT_CONDUCTOR, roughness=0.0, conductor_ior=(0.2, 0.9, 1.1), conductor_k=(3.9, 2.4, 2.2))),
                      ("rough 0.5", pod.make_material(pod.MAT_CONDUCTOR, roughness=0.5, conductor_ior=(0.2, 0.9, 1.1), conductor_k=(3.9, 2.4, 2.2)))):
        e = estimate(lambda W, H: _floor_scene(W, H, mat, True, sky=1.0), frames)
        lob = Lobes(mat)
        _, WI = _pixel_geometry(_floor_scene(e.W, e.H, mat, True, sky=1.0), e.W, e.H)
        want = np.zeros((len(WI), 3))
        if name == "smooth":
            # alpha = 1e-4: a mirror; G = 1 at these angles: the Fresnel reflectance of the complex index, nothing else
            want = np.stack([np_fresnel_conductor(lob.eta[c], lob.k[c], WI[:, 2]) for c in range(3)], -1)
        else:
            up, dw = _sphere_grid(192, 384, lower=False)
            for k in range(len(WI)):
                f, _, _ = lob.reflection(WI[k], up)
                want[k] = f.sum(0) * dw
        want = _block_mean(want, e.W, e.H)
        print("conductor furnace, %s: albedo over the blocks %s .. %s" % (name, np.round(want.min(0), 4), np.round(want.max(0), 4)))
        _assert_agree(_z(e.mean, e.se, want, 0.0, systematic=3e-3), "conductor furnace, %s" % name)


# ---- estimators ----------------------------------------------------------------------------------------------------------------

class _BlockEstimate(_Estimate):
    def __init__(self, W, H):
        jj, ii = np.mgrid[0:H, 0:W]
        self.ids, self.nb = ((jj // BLOCK) * (W // BLOCK) + ii // BLOCK).reshape(-1), (W // BLOCK) * (H // BLOCK)
        self.per_block = np.bincount(self.ids, minlength=self.nb).astype(np.float64)
        self.n = 0
        self.s = np.zeros((self.nb, 3))
        self.s2 = np.zeros((self.nb, 3))
        self.W, self.H = W, H


def _oracle_estimator(W, H):
    def estimate(make_scene, frames):
        scene = make_scene(W, H)
        w = O.Wavefront(scene.oracle(), W * H, None, pod.RNG_PIXEL_KEYED, pod.CONDUCTOR_EXTENDED)
        e = _BlockEstimate(W, H)
        for f in range(1, frames + 1):
            w.render(f, threads=8)
            e.add(w.radiance())
        w.close()
        return e
    return estimate


def _gpu_estimator(gpu_ctx_factory, W, H, per_pass=64):
    def estimate(make_scene, frames):
        ctx = gpu_ctx_factory(W, H)
        make_scene(W, H).upload(ctx)
        ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
        ctx.set_frames_per_pass(per_pass)
        ctx.reset_frame_number()
        e = _BlockEstimate(W, H)
        assert frames % per_pass == 0
        for _ in range(frames // per_pass):
            ctx.render_frame()
            r = ctx.read_radiance().reshape(per_pass, W * H, 3)
            for k in range(per_pass):
                e.add(r[k])
        return e
    return estimate


# ---- oracle twins (CPU) --------------------------------------------------------------------------------------------------------

def test_oracle_eval_matches_the_published_formulas():
    _check_eval_against_formulas(O.bsdf_eval_batch)


def test_oracle_sample_eval_and_pdf_satisfy_the_sampling_identities():
    _check_identities(O.bsdf_sample_batch, O.bsdf_eval_batch)


def test_oracle_glossy_floors_match_the_estimators_expectations():
    _check_glossy_floor(_oracle_estimator(32, 32), 768, 0.06)


def test_oracle_conductor_furnace():
    _check_conductor_furnace(_oracle_estimator(32, 32), 96)


# ---- device (through the C-ABI) -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_device_eval_matches_the_published_formulas(gpu_ctx_factory):
    ctx = gpu_ctx_factory(16, 16)
    _check_eval_against_formulas(ctx.bsdf_eval_batch)


@pytest.mark.gpu
def test_device_sample_eval_and_pdf_satisfy_the_sampling_identities(gpu_ctx_factory):
    ctx = gpu_ctx_factory(16, 16)
    _check_identities(ctx.bsdf_sample_batch, ctx.bsdf_eval_batch)


@pytest.mark.gpu
def test_device_glossy_floors_match_the_estimators_expectations(gpu_ctx_factory):
    _check_glossy_floor(_gpu_estimator(gpu_ctx_factory, 64, 64), 8192, 0.02)


@pytest.mark.gpu
def test_device_conductor_furnace(gpu_ctx_factory):
    _check_conductor_furnace(_gpu_estimator(gpu_ctx_factory, 64, 64), 1024)
