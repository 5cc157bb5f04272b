"""The NX_MAT_METALROUGH shading rule of include/nexus_hip.h (nxhip_set_materials) in numpy: the yardstick of the type's tests.

One text, two number formats: `MetalRough(..., dtype=np.float64)` is the reference, `dtype=np.float32` the same operations rounded to
binary32 after every step — the difference between the two over a grid is what binary32 itself costs the formula, and the tests'
tolerances are multiples of THAT number, never of anything the device code returns.  Written from the rule, in its order; the sampler is
replayed from the xorshift stream (three numbers per sample on both branches)."""
import numpy as np

from nexus_amd import pod


def xorshift(state):
    """one step of the device's generator (nx_rng.h rng_next): (new state uint32[n], the number in [0, 1) as float32[n])"""
    s = state.astype(np.uint32).copy()
    s ^= (s << np.uint32(13)) & np.uint32(0xffffffff)
    s ^= s >> np.uint32(17)
    s ^= (s << np.uint32(5)) & np.uint32(0xffffffff)
    f = ((s >> np.uint32(9)) | np.uint32(0x3f800000)).view(np.float32) - np.float32(1.0)
    return s, f


def clamp_metallic(m):
    """m clamped to [0, 1], NaN -> 0"""
    m = np.asarray(m, dtype=np.float64)
    return np.where(m > 0.0, np.minimum(m, 1.0), 0.0)


def material(albedo, roughness, metallic, ior=1.5, **kw):
    return pod.make_material(pod.MAT_METALROUGH, albedo=albedo, roughness=roughness, ior=ior, metallic=metallic, **kw)


class MetalRough:
    def __init__(self, albedo, roughness, ior, metallic, dtype=np.float64):
        dt = self.dt = dtype
        # the material's numbers are binary32 in the record: both formats start from those
        self.c = np.asarray(albedo, np.float32).astype(dt)
        r = dt(np.float32(roughness))
        self.ior = dt(np.float32(ior))
        self.m = dt(clamp_metallic(np.float32(metallic)))
        self.alpha = dt(min(max(r * r, dt(1.0e-3)), dt(1.0)))
        self.a2 = dt(self.alpha * self.alpha)
        q = dt((self.ior - dt(1)) / (self.ior + dt(1)))
        self.f0d = dt(q * q)
        self.F0 = (self.f0d + (self.c - self.f0d) * self.m).astype(dt)
        self.base = (self.c * (dt(1) - self.m)).astype(dt)
        self.pi = dt(np.float32(3.14159265)) if dt is np.float32 else dt(np.pi)
        self.inv_pi = dt(np.float32(0.31830988618)) if dt is np.float32 else dt(1.0 / np.pi)

    @classmethod
    def of(cls, mat, dtype=np.float64):
        u = mat["u"]
        return cls(u[0:3], u[3], u[4], u[5], dtype)

    def _pow5(self, x):
        x2 = x * x
        return (x2 * x2) * x

    def fd(self, x):
        dt = self.dt
        return self.f0d + (dt(1) - self.f0d) * self._pow5(dt(1) - x)

    def lam(self, x):
        return np.sqrt(self.a2 + (self.dt(1) - self.a2) * (x * x))

    def lobe_probability(self, ci):
        """ps and whether ws + wd > 0, from wi alone"""
        dt = self.dt
        ci = dt(ci)
        Fi = self.F0 + (dt(1) - self.F0) * self._pow5(dt(1) - ci)
        third = dt(1) / dt(3)
        ws = dt(((Fi[0] + Fi[1]) + Fi[2]) * third)
        wd = dt((((self.base[0] + self.base[1]) + self.base[2]) * third) * (dt(1) - self.fd(ci)))
        s = dt(ws + wd)
        return (dt(ws / s) if s > 0 else dt(0)), bool(s > 0)

    def eval(self, wi, wo):
        """wi (3,), wo (n, 3) -> f cos (n, 3), pdf (n,), same side (n,) — values on the other side are 0"""
        dt = self.dt
        wi = np.asarray(wi).astype(dt)
        wo = np.asarray(wo).astype(dt)  # (a caller that compares with the device passes the binary32 directions it sent)
        same = wi[2] * wo[:, 2] > 0
        ps, ok = self.lobe_probability(abs(wi[2]))
        ci = dt(abs(wi[2]))
        co = np.abs(wo[:, 2])
        with np.errstate(divide="ignore", invalid="ignore"):
            h = wi + wo
            h = h * (dt(1) / np.sqrt(h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1] + h[:, 2] * h[:, 2]))[:, None]
            u = wi[0] * h[:, 0] + wi[1] * h[:, 1] + wi[2] * h[:, 2]
            F = self.F0[None, :] + (dt(1) - self.F0)[None, :] * self._pow5(dt(1) - u)[:, None]
            den = self.a2 * (h[:, 2] * h[:, 2]) + (h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1])
            D = self.a2 / ((self.pi * den) * den)
            li, lo = self.lam(ci), self.lam(co)
            G2 = ((dt(2) * ci) * co) / (co * li + ci * lo)
            G1 = (dt(2) * ci) / (ci + li)
            kd = (dt(1) - self.fd(ci)) * (dt(1) - self.fd(co))
            f = F * ((D * G2) / ((dt(4) * ci) * co))[:, None] + self.base[None, :] * (self.inv_pi * kd)[:, None]
            fcos = f * co[:, None]
            pdf = ps * ((G1 * D) / (dt(4) * ci)) + (dt(1) - ps) * (co * self.inv_pi)
        good = same & ok
        return np.where(good[:, None], fcos, 0).astype(dt), np.where(good, pdf, 0).astype(dt), same

    def valid(self, pdf):
        return np.isfinite(pdf) & (pdf > 1.0e-4)

    def sample(self, wi, rng):
        """the sampler replayed from the stream: rng uint32 (n,) -> dict(wo, thr, pdf, ok, rng_out, u0, ps)"""
        dt = self.dt
        wi = np.asarray(wi).astype(dt)
        n = len(rng)
        s, u0 = xorshift(np.asarray(rng, np.uint32))
        s, u1 = xorshift(s)
        s, u2 = xorshift(s)
        u0, u1, u2 = u0.astype(dt), u1.astype(dt), u2.astype(dt)
        ps, ok = self.lobe_probability(abs(wi[2]))
        side = dt(-1.0 if wi[2] < 0 else 1.0)
        spec = u0 < ps
        # specular: visible normals of GGX (Heitz 2018)
        a = dt(np.sqrt(self.a2))
        V = wi * side
        Vh = np.array([a * V[0], a * V[1], V[2]], dtype=dt)
        Vh = Vh * (dt(1) / np.sqrt(Vh[0] * Vh[0] + Vh[1] * Vh[1] + Vh[2] * Vh[2]))
        lensq = dt(Vh[0] * Vh[0] + Vh[1] * Vh[1])
        T1 = (np.array([-Vh[1], Vh[0], 0], dtype=dt) * (dt(1) / np.sqrt(lensq))) if lensq > 0 else np.array([1, 0, 0], dtype=dt)
        T2 = np.array([Vh[1] * T1[2] - Vh[2] * T1[1], Vh[2] * T1[0] - Vh[0] * T1[2], Vh[0] * T1[1] - Vh[1] * T1[0]], dtype=dt)
        rr = np.sqrt(u1)
        phi = 2.0 * np.pi * u2.astype(np.float64)  # (the device forms the angle and its sine / cosine in binary64, then rounds the products)
        t1 = (np.cos(phi) * rr.astype(np.float64)).astype(dt)
        t2 = (np.sin(phi) * rr.astype(np.float64)).astype(dt)
        sw = dt(0.5) * (dt(1) + Vh[2])
        t2 = (dt(1) - sw) * np.sqrt(np.maximum(dt(0), dt(1) - t1 * t1)) + sw * t2
        Nh = (T1[None, :] * t1[:, None] + T2[None, :] * t2[:, None]) + Vh[None, :] * np.sqrt(np.maximum(dt(0), (dt(1) - t1 * t1) - t2 * t2))[:, None]
        hh = np.stack([a * Nh[:, 0], a * Nh[:, 1], np.maximum(dt(0), Nh[:, 2])], -1)
        hh = hh * (dt(1) / np.sqrt(hh[:, 0] * hh[:, 0] + hh[:, 1] * hh[:, 1] + hh[:, 2] * hh[:, 2]))[:, None] * side
        d = hh[:, 0] * wi[0] + hh[:, 1] * wi[1] + hh[:, 2] * wi[2]
        wo_s = -wi[None, :] + (hh * dt(2)) * d[:, None]  # reflect(-wi, h) = -wi - 2 h (h . -wi)
        # diffuse: cosine_hemisphere, first number the angle, second the radius
        B = np.sqrt(u2)
        ph = 2.0 * np.pi * u1.astype(np.float64)
        wo_d = np.stack([(np.cos(ph) * B.astype(np.float64)).astype(dt), (np.sin(ph) * B.astype(np.float64)).astype(dt), np.sqrt(dt(1) - u2) * side], -1)
        wo = np.where(spec[:, None], wo_s, wo_d).astype(dt)
        fcos, pdf, same = self.eval(wi, wo)
        good = same & ok
        with np.errstate(divide="ignore", invalid="ignore"):
            thr = np.where(good[:, None], fcos / pdf[:, None], 0)
        return dict(wo=wo, thr=thr.astype(dt), pdf=pdf, ok=good & self.valid(pdf), rng_out=s, u0=u0, ps=ps, spec=spec)



# ---- the eval pin's cases and the binary32 yardstick (one place: the CPU test measures it, the GPU tests use it) -------------------------

BASE = (1.0, 0.77, 0.34)
EVAL_CASES = ((0.15, 1.0), (0.3, 0.5), (0.6, 0.0), (1.0, 1.0))  # (roughness, metallic)
EVAL_COS = (0.9, 0.5, 0.2)
_yardstick = {}


def wi_of(cos_i, phi=0.7):
    s = np.sqrt(1.0 - cos_i * cos_i)
    return np.array([s * np.cos(phi), s * np.sin(phi), cos_i])


def upper_grid(n_theta=96, n_phi=192):
    """midpoints in (cos theta, phi) of the upper hemisphere, equal solid angles: directions (n, 3) and the solid angle of one"""
    cz = (np.arange(n_theta) + 0.5) / n_theta
    ph = (np.arange(n_phi) + 0.5) * 2.0 * np.pi / n_phi
    czz, pp = np.meshgrid(cz, ph, indexing="ij")
    s = np.sqrt(1.0 - czz * czz)
    return np.stack([s * np.cos(pp), s * np.sin(pp), czz], -1).reshape(-1, 3), 2.0 * np.pi / (n_theta * n_phi)


def binary32_yardstick():
    """the largest relative deviation of the rule evaluated in numpy float32 from the rule in float64 — f cos per channel and the pdf —
    over the eval pin's grid (EVAL_CASES x EVAL_COS x the 96 x 192 hemisphere), where the float64 pdf exceeds 1e-3.  Measured on this
    reference alone; the device never enters."""
    if "eval" not in _yardstick:
        worst = 0.0
        wo = upper_grid()[0].astype(np.float32)
        for r, m in EVAL_CASES:
            lo, hi = MetalRough(BASE, r, 1.5, m, np.float32), MetalRough(BASE, r, 1.5, m, np.float64)
            for c in EVAL_COS:
                wi = wi_of(c).astype(np.float32)  # (the binary32 directions a device query carries)
                f32, p32, _ = lo.eval(wi, wo)
                f64, p64, _ = hi.eval(wi, wo)
                sig = p64 > 1e-3
                worst = max(worst, float(np.abs(p32[sig] / p64[sig] - 1.0).max()), float(np.abs(f32[sig] / f64[sig] - 1.0).max()))
        _yardstick["eval"] = worst
    return _yardstick["eval"]
