"""Every compiled material and medium instance (nx_variants.h) as a test case: which scene launches the set, and the float64 expectation the
set's frames are held to — composed from the references the per-feature tests already hold, no device output enters.

The case tables (SCAN_CASES, MEDIUM_CASES, TAIL_CASES, CLASSIC_CASES, TRACE_CASES) are keyed by the instance set, spelled with the names
of nx_variants.h's constants (parsed from the header: constants()); tests/test_instance_ledger.py holds them to the units' Instances<...>
lists, tests/test_gpu_instance_matrix.py renders them, tests/test_instance_matrix_reference.py shows on the CPU what the expectations can
tell apart.

The material launch.  The scene is feature_product_reference.scene() without the fog, with a mesh emitter above and behind the eye
(EMITTER: the normal map leans towards the camera's side, and the emitter's shadows under the analytic lights fall outside the view) — a
two-triangle floor, a two-triangle pane above every mesh, a two-triangle emitter, paths of two vertices, MIS on.  For the floor point x the camera sees, about the shading normal ns(x):

    E[radiance] = the emitter term + [ANALYTIC] sum over the three lights l of  E_l(x) f cos(wi, to l) T_pane(x -> l)

    the emitter term    test_gpu_metalrough._floor_expectation's estimator, over N x N nodes of the emitter: the light sample weighted
                        against the BSDF's pdf, the BSDF sample against the light's, the pdf cut-off of either, the un-clamped roulette on
                        a BSDF-sampled hit.  The emitter is below the pane, so the pane's factor on its segments is 1 (no crossing) and
                        both techniques reach every node: w_light + w_bsdf = 1 wherever the roulette takes nothing, which is why uniform,
                        table and tree sampling share one expectation (their pdfs differ only in the pick among triangles).
    E_l                 feature_product_reference.closed_form_many with the direction to the light as the normal and rho = pi: the light's
                        irradiance on a surface that faces it
    f cos               Lambert, or metalrough_reference's rule (metal_eval_many restates MetalRough.eval for points with a metalness each;
                        the CPU test holds the two against each other) with r, m from the roughness map's lookup (detail_reference)
    T_pane              BLEND: transmittance_reference's 1 - o a; MASK: 0 or 1 by o a against the cutoff, with alpha_test_reference's
                        bilinear alpha; the emitter itself is opaque and black

A floor under NX_ALPHA_OPAQUE never passes through; the same floor under NX_ALPHA_BLEND lets 1 - opacity of the camera rays through
into nothing, and returns `opacity` of the expectation.

The medium.  test_gpu_medium's lamp in LAMP_FOG at a path length of 2, the lamp outside the view: single scattering of a rectangular
lamp (lamp_single_scatter: medium_reference.single_scatter's quadrature with nodes over the lamp, the lamp's cosine over r^2, the phase
function, transmittance on both segments — grid_medium_reference's optical depth for the grid form), plus the point light's
(the same quadrature with a point for the lamp's nodes: the CPU test holds it to medium_reference.single_scatter), plus, with METAL, the direct light on an NX_MAT_METALROUGH backdrop behind the box by the material
quadrature above."""
import functools
import os
import re

import numpy as np

from nexus_amd import pod, scenegen, workloads
from tests import alpha_test_reference as ATR
from tests import detail_reference as DR
from tests import feature_product_reference as F
from tests import metalrough_reference as MRR
from tests import scene_helpers as SH
from tests import test_gpu_analytic_lights as AL
from tests import test_gpu_detail_maps as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "nexus_amd", "csrc", "device")
W, H, BLOCKS = F.W, F.H, F.BLOCKS
N_UP = F.N_UP


# ---- the names of the sets ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def constants():
    """{name: value} of nx_variants.h's kMf* and kTf* constants, as the header spells them"""
    text = open(os.path.join(DEVICE, "nx_variants.h")).read()
    out = {name: int(value) for name, value in re.findall(r"^constexpr unsigned (k[MT]f[A-Z]\w*) = (\d+)u;", text, re.M)}
    assert len(out) >= 15, out
    return out


def mf(*names):
    """the material set of the named features: mf("Power", "Detail") = kMfPower | kMfDetail"""
    c = constants()
    return sum(c["kMf" + n] for n in names)


def tf(*names):
    c = constants()
    return sum(c["kTf" + n] for n in names)


def set_name(value, prefix="kMf"):
    names = [n[len(prefix):] for n, v in constants().items() if n.startswith(prefix) and not n.endswith("All") and not n.endswith("Reads") and v & value and bin(v).count("1") == 1]
    return "|".join(names) if names else "0"


# ---- the case tables ---------------------------------------------------------------------------------------------------------------------------

# what the scene's light sampling adds to a set, and what its floor does
SAMPLING = {"uniform": (), "table": ("Power",), "tree": ("Tree", "Power")}
FAMILY = {"no_maps": ("NoMaps",), "base": (), "detail": ("Detail",), "metal": ("Detail", "Metal"), "solid": ("Detail", "Metal", "Solid")}


def _cases(families, samplings, extra=lambda family, sampling: True):
    out = {}
    for family in families:
        for sampling in samplings:
            if not extra(family, sampling):
                continue
            for analytic in (False, True):
                key = mf(*FAMILY[family], *SAMPLING[sampling], *(("Analytic",) if analytic else ()))
                assert key not in out
                out[key] = dict(family=family, sampling=sampling, analytic=analytic)
    return out


# the SCAN pipeline's material launch (the light tree has no map-free form)
SCAN_CASES = _cases(FAMILY, SAMPLING, lambda family, sampling: not (family == "no_maps" and sampling == "tree"))
# the tail kernel: no map-free form (a map-free scene launches the general one: family "base" covers it), no SOLID one, no TREE one
TAIL_CASES = _cases(("base", "detail", "metal"), ("uniform", "table"))
# the medium's scatter kernel reads the light sample's three features and the fifth type's hit code; each set in a homogeneous and a grid form
MEDIUM_CASES = {}
for _metal in (False, True):
    for _sampling in SAMPLING:
        for _analytic in (False, True):
            MEDIUM_CASES[mf(*SAMPLING[_sampling], *(("Metal",) if _metal else ()), *(("Analytic",) if _analytic else ()))] = dict(metal=_metal, sampling=_sampling, analytic=_analytic)
# the classic pipeline's material kernels, by (the kernel's type is NX_MAT_METALROUGH, set): the type says what METAL would.  The floor's
# family decides which unit's list the host looks the kernel up in (nx_host.h kernels::shade)
CLASSIC_CASES = {}
for _family, _metal_type, _bits in (("base", False, ()), ("detail", False, ("Detail",)), ("metal", True, ("Detail",)), ("solid", False, ("Detail", "Solid")), ("solid", True, ("Detail", "Solid"))):
    for _sampling in ("uniform", "table"):
        for _analytic in (False, True):
            CLASSIC_CASES[(_metal_type, mf(*_bits, *SAMPLING[_sampling], *(("Analytic",) if _analytic else ())))] = dict(family=_family, sampling=_sampling, analytic=_analytic)
# trace_kernel: the four switches of a context, and whether the IDENTITY instances are forced general (nxhip_debug_pass_flavor); `word`: the
# word of nxhip_debug_pass_instances the set is read from
TRACE_CASES = {}
for _mask in (False, True):
    for _transmit in (False, True):
        for _stats in (False, True):
            for _entry in (False, True):
                for _general in (False, True):
                    _sw = dict(mask=_mask, transmit=_transmit, stats=_stats, entry=_entry, general=_general)
                    _special = not (_mask or _stats)  # the counting variants and the ALPHA_TEST instances are general ones
                    _id = ("Identity",) if _special and not _general else ()
                    _words = {
                        "primary": tf(*_id, *(("Entry",) if _entry and _special else ()), *(("Counting",) if _stats else ()), *(("AlphaTest",) if _mask else ())),
                        "closest": tf(*_id, *(("Counting",) if _stats else ()), *(("AlphaTest",) if _mask else ())),
                        "any_hit": tf("AnyHit", *(() if _transmit else _id), *(("Counting",) if _stats else ()), *(("Transmit",) if _transmit else ()), *(("AlphaTest",) if _mask else ())),
                    }
                    for _word, _set in _words.items():
                        TRACE_CASES.setdefault(_set, dict(word=_word, **_sw))


def scan_id(key):
    return "scan-" + set_name(key)


# ---- the material launch's scene ---------------------------------------------------------------------------------------------------------------

# beside the floor the camera sees (its view runs along -x about z = 0 .. 0.3): x0, x1, z0, z1, height.  Above the eye, below the pane.
EMITTER = (3.0, 5.0, -0.8, 1.2, 1.6)
# ... with the far corner pulled in by this much along x: the quad's two triangles then differ in area, so uniform sampling (a triangle
# index), the table (by area x luminance) and the tree draw different light samples from the same random numbers
EMITTER_CUT = 0.8
EMITTER_LE = 6.0
EMITTER_COLOUR = np.array([1.0, 0.9, 0.8])
METAL_BASE = (0.9, 0.7, 0.4)
METAL_ROUGHNESS, METAL_FACTOR, METAL_IOR = 0.5, 1.0, 1.5
METAL_B = (51, 204)       # the two metalness values of the map's texels: 0.2 and 0.8
FLOOR_OPACITY = 0.7       # SOLID: the floor is NX_ALPHA_OPAQUE, so this must not show
PANE_CUTOFF = 0.35        # SOLID: the pane is NX_ALPHA_MASK — between its o a of 0.5 (solid) and 0.2 (no crossing)


def metal_map():
    """4 x 4 roughness / metalness image: G = 255 (the roughness factor stands), B a two-valued checker"""
    img = np.zeros((4, 4, 4), np.uint8)
    yy, xx = np.mgrid[0:4, 0:4]
    img[..., 1] = 255
    img[..., 2] = np.where((xx + yy) % 2 == 0, METAL_B[0], METAL_B[1])
    img[..., 3] = 255
    return img


def floor_material(family, opacity=None):
    if family in ("metal", "solid"):
        return MRR.material(METAL_BASE, METAL_ROUGHNESS, METAL_FACTOR, ior=METAL_IOR, opacity=(FLOOR_OPACITY if family == "solid" else 1.0) if opacity is None else opacity)
    return pod.make_material(pod.MAT_DIFFUSE, albedo=(F.RHO,) * 3)


def emitter_corners():
    """the emitter's corners in scenegen.quad's order — its triangles are (p0, p1, p2) and (p0, p2, p3): (4, 3)"""
    x0, x1, z0, z1, h = EMITTER
    return np.array([(x0, h, z0), (x1, h, z0), (x1 - EMITTER_CUT, h, z1), (x0, h, z1)])


def scene(family, sampling="uniform", path_length=2, floor_mode=None, pane_mode=None):
    """the scene of a SCAN case (the lights are the caller's: set_analytic_lights).  floor_mode / pane_mode: the alpha modes of a SOLID
    scene's floor and pane, for the neighbours (default NX_ALPHA_OPAQUE and NX_ALPHA_MASK)."""
    detail = family in ("detail", "metal", "solid")
    sc = F.scene(fog=False, pane=True, detail=detail, transmit=True, path_length=path_length, use_mis=True)
    quad = scenegen.quad(*(tuple(c) for c in emitter_corners()))
    mats = [floor_material(family), sc.materials[1].copy(), pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), emissive=tuple(EMITTER_COLOUR), intensity=EMITTER_LE)]
    if family == "no_maps":
        mats[1]["diffuseMapId"] = -1
    placements = [(int(i["bvhIdx"]), int(i["materialId"]), workloads.IDENTITY) for i in sc.instances] + [(len(sc.meshes), 2, workloads.IDENTITY)]
    out = SH.BuiltScene(list(sc.meshes) + [quad], placements, materials=np.array(mats, dtype=pod.MAT_DT), camera=sc.camera, diffuse_maps=[] if family == "no_maps" else [F.pane_alpha_map()],
                        settings=sc.settings)
    out.lights = SH.mesh_lights(out.instances, out.materials)
    out.shadow_transmittance = pod.SHADOWS_TRANSMIT
    if detail:
        out.normal_maps = [F.normal_map()]
        metal = family in ("metal", "solid")
        out.roughness_maps = [metal_map()] if metal else []
        out.material_detail = np.array([pod.make_material_detail(0, 0 if metal else -1, 1.0), pod.make_material_detail(), pod.make_material_detail()], dtype=pod.DETAIL_DT)
    if family == "solid":
        out.material_alpha = np.array([pod.make_material_alpha(pod.ALPHA_OPAQUE if floor_mode is None else floor_mode),
                                       pod.make_material_alpha(pod.ALPHA_MASK if pane_mode is None else pane_mode, PANE_CUTOFF), pod.make_material_alpha()], dtype=pod.ALPHA_DT)
    out.light_sampling = pod.LIGHTS_UNIFORM if sampling == "uniform" else pod.LIGHTS_POWER
    out.light_importance = pod.LIGHT_IMPORTANCE_POSITION if sampling == "tree" else pod.LIGHT_IMPORTANCE_POWER
    return out


def _quad_surface(rect, opacity, rgba8=None, mode=ATR.BLEND, cutoff=0.5, corners=None):
    x0, x1, z0, z1, h = rect
    q = scenegen.quad(*(((x0, h, z0), (x1, h, z0), (x1, h, z1), (x0, h, z1)) if corners is None else (tuple(c) for c in corners)))
    pos = np.stack([q["pos%d" % k] for k in range(3)], 1)
    uvs = np.stack([q["texCoord%d" % k] for k in range(3)], 1)
    return ATR.Surface(pos, uvs, opacity=opacity, rgba8=rgba8, mode=mode, cutoff=cutoff)


def occluders(family, pane_mode=None):
    """what a shadow segment of the floor can cross, as alpha_test_reference takes it: the pane and the (opaque, black) emitter"""
    if family == "solid":
        mode = {None: ATR.MASK, pod.ALPHA_MASK: ATR.MASK, pod.ALPHA_BLEND: ATR.BLEND}[pane_mode]
    else:
        mode = ATR.BLEND
    pane = _quad_surface(F.PANE, F.PANE_OPACITY, None if family == "no_maps" else F.pane_alpha_map(), mode, PANE_CUTOFF)
    return [pane, _quad_surface(EMITTER, 1.0, corners=emitter_corners())]


# ---- f cos and the pdf, for points with a normal, a roughness and a metalness each -------------------------------------------------------------

def lambert_many(rho, ns, wi, wo):
    """f cos (n, k, 3), pdf (n, k), same side (n, k) of a Lambert surface about the normals ns (n, 3): view wi (n, 3), towards wo (n, k, 3)"""
    ci = (wi * ns).sum(-1)[:, None]
    co = (wo * ns[:, None, :]).sum(-1)
    same = (ci * co) > 0
    c = np.where(same, np.abs(co), 0.0)
    return c[..., None] * (np.asarray(rho, np.float64) * np.ones(3) / np.pi), c / np.pi, same


def metal_eval_many(base, rough, ior, metallic, ns, wi, wo):
    """metalrough_reference.MetalRough.eval for n points, each with its roughness, metalness (clamped as the rule does) and normal: f cos
    (n, k, 3), pdf (n, k), same side (n, k).  The rule is isotropic, so the local frame enters through the cosines with ns alone."""
    c = np.asarray(base, np.float32).astype(np.float64)
    m = MRR.clamp_metallic(metallic)[:, None]
    alpha = np.clip(np.asarray(rough, np.float64) ** 2, 1.0e-3, 1.0)[:, None]
    a2 = alpha * alpha
    f0d = ((np.float64(np.float32(ior)) - 1.0) / (np.float64(np.float32(ior)) + 1.0)) ** 2
    F0 = f0d + (c[None, :] - f0d) * m      # (n, 3)
    bse = c[None, :] * (1.0 - m)          # (n, 3)
    pow5 = lambda x: (x * x) * (x * x) * x  # noqa: E731
    fd = lambda x: f0d + (1.0 - f0d) * pow5(1.0 - x)  # noqa: E731
    lam = lambda x: np.sqrt(a2 + (1.0 - a2) * (x * x))  # noqa: E731
    ciz = (wi * ns).sum(-1)[:, None]        # (n, 1)
    coz = (wo * ns[:, None, :]).sum(-1)     # (n, k)
    same = ciz * coz > 0
    ci, co = np.abs(ciz), np.abs(coz)
    Fi = F0 + (1.0 - F0) * pow5(1.0 - ci)
    ws = Fi.mean(-1, keepdims=True)
    wd = bse.mean(-1, keepdims=True) * (1.0 - fd(ci))
    s = ws + wd
    ps = np.where(s > 0, ws / np.where(s > 0, s, 1.0), 0.0)  # (n, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = wi[:, None, :] + wo
        h = h / np.sqrt((h * h).sum(-1))[..., None]
        u = (wi[:, None, :] * h).sum(-1)
        hz = (h * ns[:, None, :]).sum(-1)
        Fr = F0[:, None, :] + (1.0 - F0)[:, None, :] * pow5(1.0 - u)[..., None]
        den = a2 * (hz * hz) + np.maximum(1.0 - hz * hz, 0.0)
        D = a2 / ((np.pi * den) * den)
        li, lo = lam(ci), lam(co)
        G2 = ((2.0 * ci) * co) / (co * li + ci * lo)
        G1 = (2.0 * ci) / (ci + li)
        kd = (1.0 - fd(ci)) * (1.0 - fd(co))
        f = Fr * ((D * G2) / ((4.0 * ci) * co))[..., None] + bse[:, None, :] * (kd / np.pi)[..., None]
        fcos = f * co[..., None]
        pdf = ps * ((G1 * D) / (4.0 * ci)) + (1.0 - ps) * (co / np.pi)
    good = same & (s > 0)
    return np.where(good[..., None], fcos, 0.0), np.where(good, pdf, 0.0), same


# ---- the emitter term ----------------------------------------------------------------------------------------------------------------------------

NODES = 10  # per side of the emitter: tests/test_instance_matrix_reference.py measures what that leaves against 2 x NODES


def emitter_nodes(P, n=NODES, pick="table"):
    """the emitter seen from the points P (m, 3): unit directions (m, n^2, 3) to the midpoints of an n x n grid in the quad's bilinear
    coordinates, their solid angles, and the light sample's pdf per solid angle for ONE light in the pick (test_bsdf_pins._rectangle_nodes,
    for a quad that is no rectangle and not above the origin).  pick: "table" — a point of the emitter's area, what the table and (up to
    the position's influence) the tree draw; "uniform" — a triangle first, then a point of it."""
    c = emitter_corners()
    g = (np.arange(n) + 0.5) / n
    s, t = (a.reshape(-1, 1) for a in np.meshgrid(g, g, indexing="ij"))
    Y = (1 - s) * (1 - t) * c[0] + s * (1 - t) * c[1] + s * t * c[2] + (1 - s) * t * c[3]
    ds, dt = (1 - t) * (c[1] - c[0]) + t * (c[2] - c[3]), (1 - s) * (c[3] - c[0]) + s * (c[2] - c[1])
    dA = np.sqrt((np.cross(ds, dt) ** 2).sum(-1)) / (n * n)  # (linear in s and t: the midpoint rule sums to the area exactly)
    tri = [0.5 * np.linalg.norm(np.cross(c[1] - c[0], c[2] - c[0])), 0.5 * np.linalg.norm(np.cross(c[2] - c[0], c[3] - c[0]))]
    assert abs(dA.sum() - sum(tri)) < 1e-12 * sum(tri)
    first = np.cross(c[2] - c[0], Y - c[0])[:, 1] > 0  # on p1's side of the diagonal p0 p2: the triangle (p0, p1, p2)
    assert np.cross(c[2] - c[0], c[1] - c[0])[1] > 0
    per_area = np.full(len(Y), 1.0 / sum(tri)) if pick == "table" else np.where(first, 0.5 / tri[0], 0.5 / tri[1])
    v = Y[None, :, :] - P[:, None, :]
    d2 = (v * v).sum(-1)
    wo = v / np.sqrt(d2)[..., None]
    cos_l = np.abs(wo[..., 1])  # the emitter is parallel to the floor, and emits to both sides
    return wo, cos_l * dA[None, :] / d2, per_area[None, :] * d2 / cos_l


def mis_estimator(fcos, pdf, same, radiance, p_light, dw):
    """test_gpu_metalrough._floor_expectation's NEE + MIS estimator for arrays of points: the light sample weighted against the BSDF's
    pdf, the BSDF sample against the light's, either pdf's cut-off at 1e-4, the un-clamped roulette on the BSDF-sampled hit: (n, 3)"""
    power = lambda a, b: a * a / (a * a + b * b)  # noqa: E731
    ok, ok_l = same & (pdf > 1e-4), p_light > 1e-4
    with np.errstate(divide="ignore", invalid="ignore"):
        T = np.where(ok[..., None], fcos / pdf[..., None], 0.0)
        rr = np.minimum(1.0, 1.0 / np.maximum(T.max(-1), 1e-30))
        w_l = np.where(ok & ok_l, power(p_light, pdf), 0.0)
        w_s = np.where(ok & ok_l, power(pdf, p_light), 0.0)
    return (fcos * ((w_l + rr * w_s) * dw)[..., None]).sum(1) * np.asarray(radiance)[None, :]


# ---- the expectation -----------------------------------------------------------------------------------------------------------------------------

def _irradiance(light, P):
    """the light's irradiance on a surface that faces it at the points P, the unit direction to it and the segment's length"""
    d, length = F.shadow_segment(light, P)
    E, falloff = F.closed_form_many(light, P, d, np.pi)
    return E, d, length, falloff


FLOOR_KIND = {"no_maps": "lambert", "base": "lambert", "detail": "mapped lambert", "metal": "metal", "solid": "metal"}
PANE_KIND = {"no_maps": "opacity", "base": "blend", "detail": "blend", "metal": "blend", "solid": "mask"}
_FLOOR_SCENE = {"lambert": "base", "mapped lambert": "detail", "metal": "metal"}


@functools.lru_cache(maxsize=None)
def floor_points(sub):
    """the floor points of sub x sub positions in every pixel (test_gpu_analytic_lights._floor_points): (sub^2, pixels, 3)"""
    return AL._floor_points(scene("base"), N_UP, sub)


@functools.lru_cache(maxsize=None)
def floor_factors(kind, sub=4, nodes=NODES, shadings=None):
    """what the floor of one kind returns at the sub x sub positions of every pixel, computed once — arrays with the leading shape
    (sub^2, pixels):
      emitter[shading][picks]   the emitter term; shading "mapped" (the kind's own), "flat" (the geometric normal), "lambert" (Lambert with
                                the base colour in place of GGX: the metal floor only); picks: lights in the sample's pick (1, or 4 with
                                the three analytic lights)
      term[light][shading]      E_l f cos of an analytic light, before the pane
      falloff[light]            the spot falloff's argument before the clamp
      fell_back                 the view is below the mapped horizon there"""
    sc = scene(_FLOOR_SCENE[kind])
    metal, detail = kind == "metal", kind != "lambert"
    P = floor_points(sub)
    S, n = len(P), P.shape[1]
    if shadings is None:
        shadings = ("mapped",) + (("flat",) if detail else ()) + (("lambert",) if metal else ())
    out = dict(fell_back=np.zeros((S, n), bool), emitter={s: {k: np.zeros((S, n, 3)) for k in (1, 4)} for s in shadings},
               term={name: {s: np.zeros((S, n, 3)) for s in shadings} for name in F.ALL}, falloff={name: np.ones((S, n)) for name in F.ALL})
    for k in range(S):
        p = P[k]
        ref = DM._reference(sc, p, F.normal_map() if detail else None)
        out["fell_back"][k] = ref["fell_back"]
        wi = F.EYE[None, :] - p
        wi /= np.sqrt((wi * wi).sum(1))[:, None]
        normals = {"mapped": ref["ns"], "flat": np.broadcast_to(N_UP, p.shape), "lambert": ref["ns"]}
        if metal:
            mr = DR.tex2d_linear(metal_map(), ref["texcoord"][:, 0], ref["texcoord"][:, 1])
            rough, metalness = METAL_ROUGHNESS * mr[:, 1], METAL_FACTOR * mr[:, 2]

        def bsdf(shading, wo):
            if metal and shading != "lambert":
                return metal_eval_many(METAL_BASE, rough, METAL_IOR, metalness, normals[shading], wi, wo)
            return lambert_many(np.asarray(METAL_BASE) if metal else F.RHO, normals[shading], wi, wo)

        wo, dw, p_l = emitter_nodes(p, nodes)
        for s in shadings:
            fcos, pdf, same = bsdf(s, wo)
            for picks in (1, 4):
                out["emitter"][s][picks][k] = mis_estimator(fcos, pdf, same, EMITTER_LE * EMITTER_COLOUR, p_l / picks, dw)
        for name in F.ALL:
            E, d, _, out["falloff"][name][k] = _irradiance(F.LIGHTS[name], p)
            for s in shadings:
                fcos, pdf, same = bsdf(s, d[:, None, :])
                out["term"][name][s][k] = E * np.where((same & (pdf > 1e-4))[..., None], fcos, 0.0)[:, 0, :]
    return out


@functools.lru_cache(maxsize=None)
def pane_factors(kind, sub=4):
    """what the analytic lights' shadow segments cross, per light — arrays (sub^2, pixels): t_pane (the factor: alpha_test_reference's T over
    the pane and the opaque emitter), crossed (the pane's crossings that count), crossed_emitter, unclear (transmittance_reference's EDGE band,
    from the surfaces without a map so that the weight rule does not enter).  kind: "opacity" (no map), "blend", "mask"."""
    P = floor_points(sub)
    S, n = len(P), P.shape[1]
    family = {"opacity": "no_maps", "blend": "base", "mask": "solid"}[kind]
    surfaces = occluders(family)
    bare = [_quad_surface(F.PANE, F.PANE_OPACITY), surfaces[1]]
    out = {name: dict(t_pane=np.ones((S, n)), crossed=np.zeros((S, n), np.int64), crossed_emitter=np.zeros((S, n), bool), unclear=np.zeros((S, n), bool)) for name in F.ALL}
    for k in range(S):
        for name in F.ALL:
            f = out[name]
            d, length = F.shadow_segment(F.LIGHTS[name], P[k])
            tmax = np.where(np.isfinite(length), length, 1.0e3)  # (the pane is 2 above the floor: a sun ray meets it within 1 000 units or never)
            t = ATR.trace(P[k], d, tmax, surfaces[:1])
            e = ATR.trace(P[k], d, tmax, bare[1:])
            f["crossed_emitter"][k] = e["crossings"] > 0
            f["t_pane"][k], f["crossed"][k] = t["T"] * e["T"], t["crossings"] - t["rejected"]
            f["unclear"][k] = ATR.trace(P[k], d, tmax, bare[:1])["unclear"] | e["unclear"]
    return out


def _pane_kind(family, pane_mode=None):
    return "blend" if family == "solid" and pane_mode == pod.ALPHA_BLEND else PANE_KIND[family]


def expectation(family, analytic, sub=4, nodes=NODES, shading="mapped", lights=F.ALL, pane_mode=None, floor_mode=None, shadings=None):
    """block means (16, 3).  shading: "mapped" (the family's own), "flat" (the geometric normal), "lambert" (Lambert with the base colour in
    place of GGX); lights: the analytic lights that count (the emitter's pick stays what `analytic` says); pane_mode / floor_mode: pod.ALPHA_BLEND
    for the neighbours of a SOLID case"""
    Ff = floor_factors(FLOOR_KIND[family], sub, nodes, shadings)
    total = Ff["emitter"][shading][4 if analytic else 1].copy()
    if analytic and lights:
        Fp = pane_factors(_pane_kind(family, pane_mode), sub)
        for name in lights:
            total = total + Ff["term"][name][shading] * Fp[name]["t_pane"][..., None]
    if family == "solid" and floor_mode == pod.ALPHA_BLEND:
        total = total * FLOOR_OPACITY
    return F.blocks(total.mean(0))


# What the quadratures leave, relative, per kind of floor and over the kept blocks, as tests/test_instance_matrix_reference.py measures it
# (and holds these constants to: not below the measurement, not above twice it): NODES against 2 x NODES emitter nodes per side, and 4 x 4
# against 8 x 8 positions per pixel.
NODES_TERM = {"lambert": 7.1e-4, "mapped lambert": 3.8e-4, "metal": 6.8e-4}
SUB_TERM = {"lambert": 2.1e-5, "mapped lambert": 9.1e-5, "metal": 2.0e-4}
# ... and a bound on the share of shadow segments in transmittance_reference's EDGE band (feature_product_reference.UNCLEAR_TERM), asserted there too
UNCLEAR_TERM = 5.0e-4


def systematic(family, analytic):
    """what the device comparison allows the expectation, relative: the reference's own residue"""
    kind = FLOOR_KIND[family]
    return NODES_TERM[kind] + SUB_TERM[kind] + (UNCLEAR_TERM if analytic else 0.0)


DARK = 0.05


def left_out(family, analytic, sub=4):
    """{reason: (16,) bool}: feature_product_reference.left_out's reasons, decided from the reference alone.  Without analytic lights only
    the horizon can take a block away: the emitter term is smooth."""
    Ff = floor_factors(FLOOR_KIND[family], sub)
    edge, seam, rim = np.zeros(BLOCKS, bool), np.zeros(BLOCKS, bool), np.zeros(BLOCKS, bool)
    picks = 4 if analytic else 1
    bare = Ff["emitter"]["mapped"][picks].mean(0)
    if analytic:
        Fp = pane_factors(PANE_KIND[family], sub)
        jj, ii = np.mgrid[0:H, 0:W]
        ids = ((jj // 16) * (W // 16) + ii // 16).reshape(-1)
        for name in F.ALL:
            f = Fp[name]
            edge |= F._any_in_block(f["crossed"] > 0) & F._any_in_block(f["crossed"] == 0)
            edge |= F._any_in_block(f["crossed_emitter"]) & F._any_in_block(~f["crossed_emitter"])
            through = f["crossed"] > 0
            for b in range(BLOCKS):
                t = f["t_pane"][:, ids == b][through[:, ids == b]]
                seam[b] |= t.size > 0 and t.max() - t.min() > 1e-9
            bare = bare + Ff["term"][name]["mapped"].mean(0)
        x = Ff["falloff"]["spot"]
        rim = F._any_in_block(x < 0.0) & F._any_in_block(x > 0.0)
    full = expectation(family, analytic, sub)
    return {"pane edge": edge, "alpha edge": seam & ~edge, "cone rim": rim, "horizon": F._any_in_block(Ff["fell_back"]), "dark": np.any(full < DARK * F.blocks(bare), 1)}


def kept(family, analytic, sub=4):
    out = np.zeros(BLOCKS, bool)
    for mask in left_out(family, analytic, sub).values():
        out |= mask
    return ~out


def unclear_share(family, sub=4):
    """the largest share, over the blocks and the lights, of shadow segments in the EDGE band (feature_product_reference.unclear_share)"""
    Fp = pane_factors(PANE_KIND[family], sub)
    return max(float(F.blocks(Fp[name]["unclear"].mean(0)[:, None]).max()) for name in F.ALL)


def neighbours(family, analytic):
    """{name: block means}: what an instance that dropped or swapped ONE thing the case's set stands for would render"""
    out = {}
    if analytic:
        out["without the analytic lights"] = expectation(family, analytic, lights=())
    if family in ("detail", "metal", "solid"):
        out["with the geometric normal"] = expectation(family, analytic, shading="flat")
    if family in ("metal", "solid"):
        out["Lambert in place of GGX"] = expectation(family, analytic, shading="lambert")
    if family == "solid":
        out["the floor as BLEND"] = expectation(family, analytic, floor_mode=pod.ALPHA_BLEND)
        if analytic:  # (the emitter is below the pane: only the analytic lights' segments cross it)
            out["the pane as BLEND"] = expectation(family, analytic, pane_mode=pod.ALPHA_BLEND)
    return out


# ---- the medium's scene ----------------------------------------------------------------------------------------------------------------------------

FOG_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
FOG = pod.make_medium(box_min=FOG_BOX[0], box_max=FOG_BOX[1], sigma_t=0.9, g=0.5, albedo=(0.9, 0.9, 0.9))  # test_gpu_medium.LAMP_FOG
FOG_EYE, FOG_FOV = (0.0, 0.0, 4.0), 30.0  # test_gpu_medium._lamp_scene's camera: it sees the box and nothing beside it
LAMP = (-0.6, 0.6, -0.6, 0.6, 1.5)        # x0, x1, z0, z1, height: above the box, outside the view
LAMP_LE = 6.0
LAMP_COLOUR = np.array([1.0, 0.9, 0.8])
FOG_POINT = pod.make_analytic_light(pod.ALIGHT_POINT, position=(1.6, 0.4, 0.6), colour=(0.6, 0.8, 1.0), intensity=3.0)  # beside the box, outside the view
BACKDROP_Z, BACKDROP_HALF = -1.6, 3.0      # behind the box, facing the camera, wider than the view
BACKDROP_METALLIC = 0.5


def fog_density():
    """feature_product_reference.density(): the Gaussian puff of 0.2 .. 1.8 on a grid that is no multiple of the brick, over the fog's box"""
    return F.density()


def fog_scene(metal, sampling="uniform", grid=False, path_length=2):
    """test_gpu_medium's lamp in LAMP_FOG with the lamp moved out of the view; metal: an NX_MAT_METALROUGH backdrop behind the box"""
    from nexus_amd import capi
    cam = capi.camera_init(FOG_EYE, (0.0, 0.0, -1.0), FOG_FOV, W, H, 5.0, 0.0)
    far = np.array((1.0e4, 1.0e4, 1.0e4))
    x0, x1, z0, z1, h = LAMP
    meshes = [scenegen.quad(tuple(far), tuple(far + (1e-3, 0, 0)), tuple(far + (1e-3, 1e-3, 0)), tuple(far + (0, 1e-3, 0))), scenegen.quad((x0, h, z0), (x1, h, z0), (x1, h, z1), (x0, h, z1))]
    mats = [pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0)), pod.make_material(pod.MAT_DIFFUSE, albedo=(0, 0, 0), emissive=tuple(LAMP_COLOUR), intensity=LAMP_LE)]
    if metal:
        b, z = BACKDROP_HALF, BACKDROP_Z
        meshes.append(scenegen.quad((-b, -b, z), (b, -b, z), (b, b, z), (-b, b, z)))
        mats.append(MRR.material(METAL_BASE, METAL_ROUGHNESS, BACKDROP_METALLIC, ior=METAL_IOR))
    sc = SH.BuiltScene(meshes, [(k, k, workloads.IDENTITY) for k in range(len(meshes))], materials=np.array(mats, dtype=pod.MAT_DT), camera=cam,
                       settings=workloads.make_settings(use_mis=True, path_length=path_length, background=(1, 1, 1), background_intensity=0.0))
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    sc.medium = FOG
    sc.medium_density = fog_density() if grid else None
    sc.light_sampling = pod.LIGHTS_UNIFORM if sampling == "uniform" else pod.LIGHTS_POWER
    sc.light_importance = pod.LIGHT_IMPORTANCE_POSITION if sampling == "tree" else pod.LIGHT_IMPORTANCE_POWER
    return sc


# ---- the medium's expectation ------------------------------------------------------------------------------------------------------------------------

FOG_LATTICE = 32     # camera rays per image side: the centres of 2 x 2 pixels (the glow is smooth: the CPU test measures 32 against 64)
FOG_T_NODES = 12     # Gauss-Legendre nodes on the camera segment in the box
LAMP_NODES = 8       # per side of the lamp
FOG_PANELS = 3       # of 8 Gauss-Legendre nodes per segment through the grid


def _lattice_rays(res):
    from nexus_amd import capi
    from tests import medium_reference as MR
    cam = capi.camera_init(FOG_EYE, (0.0, 0.0, -1.0), FOG_FOV, W, H, 5.0, 0.0)
    pos, dirs = MR.camera_rays(cam, res, res, 1)
    return pos, dirs[0]


def lattice_blocks(per_ray, res):
    """means over the 4 x 4 blocks of the image, of values on a res x res lattice of camera rays: (16, channels)"""
    jj, ii = np.mgrid[0:res, 0:res]
    ids = ((jj // (res // 4)) * 4 + ii // (res // 4)).reshape(-1)
    per_ray = np.asarray(per_ray, np.float64).reshape(res * res, -1)
    return np.stack([np.bincount(ids, weights=per_ray[:, c], minlength=16) for c in range(per_ray.shape[1])], 1) / np.bincount(ids, minlength=16)[:, None]


def _optical_depth(grid, o, d, t_end, panels, medium=None):
    """sigmaT x the integral of the density along the part of (o, d, t_end) in the fog's box: sigmaT x the length in it without a grid"""
    from tests import grid_medium_reference as G
    from tests import medium_reference as MR
    medium = FOG if medium is None else medium
    sigma = float(medium["sigmaT"])
    if grid is None:
        return sigma * MR.segment(medium["boxMin"].astype(np.float64), medium["boxMax"].astype(np.float64), o, d, t_end)[1]
    return G.optical_depth(grid, medium["boxMin"], medium["boxMax"], sigma, o, d, t_end, panels=panels)


def lamp_nodes(n=LAMP_NODES, rect=None):
    """midpoints of an n x n grid on the lamp and the area each stands for"""
    x0, x1, z0, z1, h = LAMP if rect is None else rect
    gx = x0 + (np.arange(n) + 0.5) * (x1 - x0) / n
    gz = z0 + (np.arange(n) + 0.5) * (z1 - z0) / n
    lx, lz = np.meshgrid(gx, gz, indexing="ij")
    return np.stack([lx.reshape(-1), np.full(lx.size, h), lz.reshape(-1)], -1), (x1 - x0) * (z1 - z0) / (n * n)


def lamp_single_scatter(o, d, grid=None, g=None, t_nodes=FOG_T_NODES, n_lamp=LAMP_NODES, panels=FOG_PANELS, rect=None, point=None, cosine=False, medium=None):
    """medium_reference.single_scatter extended to a rectangular lamp (and a density grid): per camera ray (o, d[k]) the expectation of
    the rule's estimator per unit of the lamp's radiance and albedo 1 — the path scatters at t with the density of a real collision,
    sigma rho(x) exp(-tau(t0 -> t)), and collects from every node y of the lamp  p(c) exp(-tau(x -> y)) cos_lamp dA / |y - x|^2.
    point: a position instead of the lamp — per unit of radiant intensity, what single_scatter computes for a homogeneous box (cosine: with
    the cosine a horizontal lamp shrunk to that point would carry).  medium: another homogeneous medium than FOG."""
    from tests import grid_medium_reference as G
    from tests import medium_reference as MR
    medium = FOG if medium is None else medium
    sigma = float(medium["sigmaT"])
    g = float(medium["g"]) if g is None else g
    d = np.asarray(d, np.float64).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(o, np.float64), d.shape)
    lo, hi = medium["boxMin"].astype(np.float64), medium["boxMax"].astype(np.float64)
    t0, L, crosses = MR.segment(lo, hi, o, d, np.full(len(d), np.inf))
    x, w = np.polynomial.legendre.leggauss(t_nodes)
    t = t0[:, None] + 0.5 * L[:, None] * (x[None, :] + 1.0)
    wt = 0.5 * L[:, None] * w[None, :]
    X = o[:, None, :] + d[:, None, :] * t[:, :, None]  # (rays, t_nodes, 3)
    n, m = X.shape[:2]
    D = np.broadcast_to(d[:, None, :], X.shape).reshape(-1, 3)
    if grid is None:
        dens = sigma * np.exp(-sigma * (t - t0[:, None]))
    else:
        rho = G.lookup(grid, FOG["boxMin"], FOG["boxMax"], X.reshape(-1, 3)).reshape(n, m)
        tau = _optical_depth(grid, np.broadcast_to(o[:, None, :], X.shape).reshape(-1, 3), D, t.reshape(-1), panels).reshape(n, m)
        dens = sigma * rho * np.exp(-tau)
    if point is not None:
        Y, dA = np.asarray(point, np.float64).reshape(1, 3), 1.0
    else:
        Y, dA = lamp_nodes(n_lamp, rect)
    total = np.zeros((n, m))
    Xf = X.reshape(-1, 3)
    for y in Y:
        to = y[None, :] - Xf
        dist = np.sqrt((to * to).sum(-1))
        u = to / dist[:, None]
        c = (u * D).sum(-1)
        T = np.exp(-_optical_depth(grid, Xf, u, dist, panels, medium))
        cos_l = 1.0 if point is not None and not cosine else np.abs(u[:, 1])  # the lamp is horizontal and emits to both sides
        total += (MR.hg_pdf(g, c) * T * cos_l * dA / (dist * dist)).reshape(n, m)
    return np.where(crosses, (dens * total * wt).sum(1), 0.0)


def backdrop_direct(o, d, grid=None, n_lamp=LAMP_NODES, panels=FOG_PANELS, shading="metal"):
    """the direct light on the NX_MAT_METALROUGH backdrop behind the box, seen through the fog: per camera ray (lamp term (n, 3), point
    light's term (n, 3)) — the material quadrature above (mis_estimator over the lamp's nodes, E_l f cos for the point light) with the fog's
    transmittance on the camera segment and on both shadow segments"""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(o, np.float64), d.shape)
    s = (BACKDROP_Z - o[:, 2]) / d[:, 2]
    x = o + d * s[:, None]
    assert np.all(s > 0) and np.abs(x[:, :2]).max() < BACKDROP_HALF
    T_cam = np.exp(-_optical_depth(grid, o, d, s, panels))
    ns, wi = np.broadcast_to(np.array([0.0, 0.0, 1.0]), x.shape), -d
    Y, dA = lamp_nodes(n_lamp)
    v = Y[None, :, :] - x[:, None, :]
    d2 = (v * v).sum(-1)
    wo = v / np.sqrt(d2)[..., None]
    cos_l = np.abs(wo[..., 1])
    T = np.stack([np.exp(-_optical_depth(grid, x, wo[:, k], np.sqrt(d2[:, k]), panels)) for k in range(len(Y))], 1)
    area = dA * len(Y)
    rough, metal = np.full(len(x), METAL_ROUGHNESS), np.full(len(x), BACKDROP_METALLIC)
    bsdf = (lambda w: metal_eval_many(METAL_BASE, rough, METAL_IOR, metal, ns, wi, w)) if shading == "metal" else (lambda w: lambert_many(np.asarray(METAL_BASE), ns, wi, w))
    fcos, pdf, same = bsdf(wo)
    lamp = mis_estimator(fcos, pdf, same, LAMP_LE * LAMP_COLOUR, d2 / (area * cos_l), cos_l * dA / d2 * T) * T_cam[:, None]
    E, u, length, _ = _irradiance(FOG_POINT, x)
    fcos, pdf, same = bsdf(u[:, None, :])
    Tp = np.exp(-_optical_depth(grid, x, u, length, panels))
    point = E * np.where((same & (pdf > 1e-4))[..., None], fcos, 0.0)[:, 0, :] * (Tp * T_cam)[:, None]
    return lamp, point


@functools.lru_cache(maxsize=None)
def fog_terms(grid, res=FOG_LATTICE, t_nodes=FOG_T_NODES, n_lamp=LAMP_NODES, g=None):
    """block means (16, 3) of the four terms of the medium's expectation: the lamp's and the point light's single scattering, and the
    lamp's and the point light's direct light on the backdrop"""
    rho = fog_density() if grid else None
    o, d = _lattice_rays(res)
    albedo = FOG["albedo"].astype(np.float64)
    T = AR_table_point()
    lamp = lamp_single_scatter(o, d, rho, g, t_nodes, n_lamp)[:, None] * (albedo * LAMP_LE * LAMP_COLOUR)[None, :]
    point = lamp_single_scatter(o, d, rho, g, t_nodes, n_lamp, point=T["centre"])[:, None] * (albedo * T["power"])[None, :]
    back_lamp, back_point = backdrop_direct(o, d, rho, n_lamp)
    return {k: lattice_blocks(v, res) for k, v in (("lamp", lamp), ("point", point), ("backdrop lamp", back_lamp), ("backdrop point", back_point))}


def AR_table_point():
    from tests import analytic_light_reference as AR
    return AR.table(FOG_POINT)


def fog_expectation(metal, analytic, grid, lamp=True, point=True, **kw):
    t = fog_terms(grid, **kw)
    total = np.zeros((BLOCKS, 3))
    if lamp:
        total = total + t["lamp"] + (t["backdrop lamp"] if metal else 0.0)
    if analytic and point:
        total = total + t["point"] + (t["backdrop point"] if metal else 0.0)
    return total


def fog_kept(metal, analytic, grid):
    """every block the fog's glow reaches: the scene has no edge to leave out"""
    return np.all(fog_expectation(metal, analytic, grid) > 0, 1)


def fog_neighbours(metal, analytic, grid):
    out = {"without the lamp": fog_expectation(metal, analytic, grid, lamp=False), "g = 0 in place of %.1f" % float(FOG["g"]): fog_expectation(metal, analytic, grid, g=0.0)}
    if analytic:
        out["without the point light"] = fog_expectation(metal, analytic, grid, point=False)
    return out


# What the medium's quadratures leave, relative, homogeneous and grid, as tests/test_instance_matrix_reference.py measures it: every count
# doubled (the lattice, the nodes on the camera segment, the lamp's nodes per side), one at a time, summed
FOG_TERM = {False: 4.1e-3, True: 6.6e-3}


def fog_systematic(metal, grid):
    return FOG_TERM[grid]
