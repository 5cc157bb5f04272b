"""NX_MAT_METALROUGH on the device: the BSDF hooks against the float64 rule of tests/metalrough_reference.py (eval pin, replayed sample
stream, the sampling identities with the bars of tests/test_bsdf_pins.py), the type's inputs at a hit against tests/detail_reference.py's
lookup, light transport on a glossy floor against a float64 quadrature, and the wiring: pipelines, queue sizes, the flavor word.
The oracle does not know the type; nothing here compares with it."""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen, workloads
from tests import detail_reference as DR
from tests import metalrough_reference as R
from tests import scene_helpers as SH
from tests import test_bsdf_pins as BP
from tests.test_physics_pins import _assert_agree, _z

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(16, 16)


# ---- 1. eval pin --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.EVAL_CASES, ids=lambda c: "r%g-m%g" % c)
def test_eval_matches_the_rule(ctx, case):
    """Device eval against the float64 rule on the 96 x 192 hemisphere grid, cos_i in {0.9, 0.5, 0.2}, coloured base.  Tolerance: four
    times the binary32 yardstick measured on the reference itself (tests/test_metalrough_reference.py: 1.84e-6 -> 7.3e-6), relative,
    where the reference pdf exceeds 1e-3; the validity flag wherever |pdf - 1e-4| > 1e-6.  Measured on an MI355X over the twelve cases: pdf
    at most 1.08e-6, f cos at most 1.84e-6 (r 0.6, m 0, cos_i 0.9)."""
    tol = 4.0 * R.binary32_yardstick()
    r, m = case
    mat = R.material(R.BASE, r, m)
    ref = R.MetalRough.of(mat)
    wo, _ = BP._sphere_grid(96, 192, False)
    for cos_i in R.EVAL_COS:
        q = BP._queries(BP._wi(cos_i), wo)
        got = ctx.bsdf_eval_batch(mat, q)
        f, p, same = ref.eval(q["wi"][0], q["wo"])
        assert same.all()
        sig = p > 1e-3
        dp = np.abs(got["pdf"].astype(np.float64)[sig] / p[sig] - 1.0).max()
        df = np.abs(got["throughput"].astype(np.float64)[sig] / f[sig] - 1.0).max()
        print("r %g m %g cos %.1f: %d points, largest relative deviation pdf %.3g, f cos %.3g (bar %.3g)" % (r, m, cos_i, sig.sum(), dp, df, tol))
        assert dp <= tol and df <= tol, (case, cos_i, dp, df, tol)
        clear = np.abs(p - 1e-4) > 1e-6
        assert np.array_equal(got["ok"][clear] == 1, (p > 1e-4)[clear]), (case, cos_i, "validity")
    # the other side of the surface is no reflection
    q = BP._queries(BP._wi(0.5), wo * np.array([1.0, 1.0, -1.0]))
    assert not ctx.bsdf_eval_batch(mat, q)["ok"].any()


# ---- 2. the sample stream -----------------------------------------------------------------------------------------------------------------

N_STREAM = 1 << 19


@pytest.mark.parametrize("case", R.EVAL_CASES, ids=lambda c: "r%g-m%g" % c)
def test_sample_replays_the_stream(ctx, case):
    """2^19 device samples against the reference's replay of the same xorshift states: the state after the call is the state after
    exactly three steps (exact), the lobe, the direction, the pdf and the weight are the reference's.  Queries within 1e-6 of the lobe
    decision (|u0 - ps| < 1e-6: about 2e-6 of a batch) are left out and must stay under 0.1 %; so must those within rounding of the two
    bars the validity flag depends on (|wo.z| <= 1e-5, |pdf - 1e-4| <= 1e-6), which only the flag's comparison leaves out.  Tolerances: what binary32 costs the
    SAMPLER, measured on the reference (float32 replay against float64 replay of the same states), times four — absolute for the
    direction, relative for pdf and weight where the reference pdf exceeds 1e-3."""
    r, m = case
    mat = R.material(R.BASE, r, m)
    hi, lo = R.MetalRough.of(mat), R.MetalRough.of(mat, np.float32)
    for cos_i in (0.9, 0.3):
        q = BP._queries(BP._wi(cos_i), n=N_STREAM, seed=7)
        got = ctx.bsdf_sample_batch(mat, q)
        want, own = hi.sample(q["wi"][0], q["rng"]), lo.sample(q["wi"][0], q["rng"])
        assert np.array_equal(got["rngOut"], want["rng_out"]), "exactly three numbers on both branches"
        keep = np.abs(want["u0"] - want["ps"]) >= 1e-6
        assert (~keep).mean() < 1e-3
        # decided within rounding of a bar, on the reference's own numbers: the side test of the reflected direction (wo.z against 0) and the
        # validity bar (the eval pin's rule) — each share printed and held to the 0.1 % of the lobe decision
        near_side, near_bar = np.abs(want["wo"][:, 2]) <= 1e-5, np.abs(want["pdf"] - 1e-4) <= 1e-6
        print("left out of the validity comparison: %.3g at the side test, %.3g at the pdf bar" % (near_side.mean(), near_bar.mean()))
        assert near_side.mean() < 1e-3 and near_bar.mean() < 1e-3
        keep &= ~near_side & ~near_bar
        assert np.array_equal(got["ok"][keep] == 1, want["ok"][keep])
        ok = keep & want["ok"] & (want["pdf"] > 1e-3)
        both = ok & own["ok"]
        bar_wo = 4.0 * np.abs(own["wo"][both].astype(np.float64) - want["wo"][both]).max()
        bar_pdf = 4.0 * np.abs(own["pdf"][both].astype(np.float64) / want["pdf"][both] - 1.0).max()
        bar_thr = 4.0 * np.abs(own["thr"][both].astype(np.float64) / want["thr"][both] - 1.0).max()
        d_wo = np.abs(got["wo"][ok].astype(np.float64) - want["wo"][ok]).max()
        d_pdf = np.abs(got["pdf"][ok].astype(np.float64) / want["pdf"][ok] - 1.0).max()
        d_thr = np.abs(got["throughput"][ok].astype(np.float64) / want["thr"][ok] - 1.0).max()
        print("r %g m %g cos %.1f: %d of %d compared (%.2g left out at the lobe decision); wo %.3g (bar %.3g), pdf %.3g (bar %.3g), weight %.3g (bar %.3g)" %
              (r, m, cos_i, ok.sum(), N_STREAM, (np.abs(want["u0"] - want["ps"]) < 1e-6).mean(), d_wo, bar_wo, d_pdf, bar_pdf, d_thr, bar_thr))
        assert d_wo <= bar_wo and d_pdf <= bar_pdf and d_thr <= bar_thr
        # sample and eval are one model: weight x pdf = eval's f cos at the sampled direction, on the device's own numbers
        e = ctx.bsdf_eval_batch(mat, BP._queries(q["wi"][0].astype(np.float64), got["wo"].astype(np.float64)))
        sel = ok & (e["ok"] == 1)
        prod = got["throughput"][sel].astype(np.float64) * got["pdf"][sel].astype(np.float64)[:, None]
        assert np.abs(prod / e["throughput"][sel].astype(np.float64) - 1.0).max() <= 3 * bar_thr + 3 * 2.0 ** -23


# ---- 3. the sampling identities (the scheme and the bars of tests/test_bsdf_pins.py) -----------------------------------------------------------

@pytest.mark.parametrize("case", ((0.3, 1.0), (0.3, 0.5), (0.6, 0.0), (1.0, 1.0)), ids=lambda c: "r%g-m%g" % c)
def test_sampling_identities(ctx, case):
    """accepted mass = the integral of the pdf; E[weight] = the integral of f cos (|z| < 4.5 with a 3e-3 quadrature term); the 12 x 24
    histogram of the samples against the pdf.  All on the device's own functions, by quadrature and Monte Carlo."""
    r, m = case
    mat = R.material(R.BASE, r, m)
    N = BP.N_SAMPLES
    wo, dw = BP._sphere_grid(648, 1296, False)
    for cos_i in (0.9, 0.45):
        wi = BP._wi(cos_i)
        s = ctx.bsdf_sample_batch(mat, BP._queries(wi, n=N, seed=int(cos_i * 100) + 4))
        ok = s["ok"] == 1
        thr = np.where(ok[:, None], s["throughput"].astype(np.float64), 0.0)
        assert np.isfinite(thr).all()
        mc, mc_se = thr.mean(0), thr.std(0) / np.sqrt(N)
        p_ok, p_ok_se = ok.mean(), np.sqrt(ok.mean() * (1 - ok.mean()) / N)
        e = ctx.bsdf_eval_batch(mat, BP._queries(wi, wo))
        valid = e["ok"] == 1
        pdf = np.where(valid, e["pdf"].astype(np.float64), 0.0)
        i_pdf = float(pdf.sum() * dw)
        i_f = np.where(valid[:, None], e["throughput"].astype(np.float64), 0.0).sum(0) * dw
        assert i_pdf < 1.0 + 2e-3, (case, cos_i, "the pdf integrates to more than one", i_pdf)
        assert abs(i_pdf - p_ok) < 4.5 * p_ok_se + 2e-3, (case, cos_i, "accepted mass", i_pdf, p_ok)
        zf = (mc - i_f) / np.sqrt(mc_se ** 2 + (3e-3 * i_f) ** 2)
        assert np.abs(zf).max() < 4.5, (case, cos_i, "E[weight] against the integral of f cos", mc, i_f)
        nt, nphi = 12, 24
        w = s["wo"][ok].astype(np.float64)
        cell = lambda d: np.clip((d[:, 2] * nt).astype(int), 0, nt - 1) * nphi + np.clip((np.mod(np.arctan2(d[:, 1], d[:, 0]), 2 * np.pi) / (2 * np.pi) * nphi).astype(int), 0, nphi - 1)  # noqa: E731
        counts = np.bincount(cell(w), minlength=nt * nphi).astype(np.float64)
        expect = np.bincount(cell(wo), weights=pdf * dw, minlength=nt * nphi) * N
        big = expect > 200.0
        zc = (counts[big] - expect[big]) / np.sqrt(expect[big] + (2e-3 * expect[big]) ** 2)
        print("r %g m %g cos %.2f: accepted %.4f = int pdf %.4f; E[weight] %s = int f cos %s; histogram max |z| %.1f over %d cells" %
              (r, m, cos_i, p_ok, i_pdf, np.round(mc, 4), np.round(i_f, 4), np.abs(zc).max(), big.sum()))
        assert np.abs(zc).max() < 5.0 and (zc * zc).mean() < 1.8, (case, cos_i, "histogram", np.abs(zc).max(), (zc * zc).mean())


# ---- 4. the inputs at a hit ----------------------------------------------------------------------------------------------------------------

def _checker_map():
    """4 x 4 metallic-roughness image: B a checker of 0 and 255, G varying, R unused"""
    img = np.zeros((4, 4, 4), np.uint8)
    yy, xx = np.mgrid[0:4, 0:4]
    img[..., 2] = np.where((xx + yy) % 2 == 0, 255, 0)
    img[..., 1] = 40 + 13 * (yy * 4 + xx)
    img[..., 0] = 17
    img[..., 3] = 255
    return img


DIFFUSE_TEXEL = (188, 128, 64, 255)  # the diffuse map of the inputs test: one sRGB colour in every texel


def _textured_quad_scene(diffuse):
    q = scenegen.quad((-1, 0, -1), (-1, 0, 1), (1, 0, 1), (1, 0, -1))
    for k in range(3):
        q["texCoord%d" % k][:, 0] = (q["pos%d" % k][:, 0] + 1.0) / 2.0
        q["texCoord%d" % k][:, 1] = (q["pos%d" % k][:, 2] + 1.0) / 2.0
    mats = np.array([R.material((0.9, 0.6, 0.3), 0.8, 0.75, diffuse_map=0 if diffuse else -1)], dtype=pod.MAT_DT)
    sc = SH.BuiltScene([q], [(0, 0, workloads.IDENTITY)], materials=mats, diffuse_maps=[np.tile(np.array(DIFFUSE_TEXEL, np.uint8), (4, 4, 1))] if diffuse else ())
    sc.roughness_maps, sc.material_detail = [_checker_map()], np.array([pod.make_material_detail(-1, 0, 1.0)], dtype=pod.DETAIL_DT)
    return sc, q


@pytest.mark.parametrize("diffuse", [False, True], ids=["factor", "diffuse-map"])
def test_inputs_at_a_hit(gpu_ctx_factory, diffuse):
    """c, r, m at 64 hits of the textured quad — 24 of them on texel borders of the B checker — against tests/detail_reference.py's
    tex2d_linear at the hit's binary32 texture coordinates: r = roughness x G, m = metallic x B of the same lookup; then the clamp."""
    sc, quad = _textured_quad_scene(diffuse)
    c = gpu_ctx_factory(16, 16)
    sc.upload(c)
    rs = np.random.RandomState(8)
    b = rs.uniform(0, 1, (64, 2))
    fold = b.sum(1) > 1
    b[fold] = 1 - b[fold]
    # 24 of the hits ON texel borders of the checker: barycentrics that are multiples of 1 / 4 put u and v on multiples of 1 / 4
    grid = np.array([(i / 4.0, j / 4.0) for i in range(5) for j in range(5 - i)])
    b[:24] = grid[rs.permutation(len(grid))[:12]].repeat(2, 0)
    tri = rs.randint(0, len(quad), 64)
    tri[:24:2], tri[1:24:2] = 0, 1
    b32 = b.astype(np.float32)
    uv = DR.hit_texcoord(quad["texCoord0"][tri], quad["texCoord1"][tri], quad["texCoord2"][tri], b32[:, 0], b32[:, 1])  # (the kernels' bary2, in binary32)
    assert np.all(np.mod(uv[:24] * 4.0, 1.0) == 0.0)
    col, rough, metal = c.material_inputs_batch(0, tri, b32)
    mr = DR.tex2d_linear(_checker_map(), uv[:, 0], uv[:, 1])
    tol = 8 * 2.0 ** -24  # (the lookup's two lerps as in the detail maps' lookup test — 4 x 2^-24 — and the product with the factor)
    assert np.abs(rough.astype(np.float64) - 0.8 * mr[:, 1]).max() < tol
    assert np.abs(metal.astype(np.float64) - 0.75 * mr[:, 2]).max() < tol
    assert metal.min() >= 0.0 and metal.max() <= 0.75 + 1e-6 and np.ptp(metal) > 0.3, "the checker's both fields are met"
    if not diffuse:
        assert np.array_equal(col, np.tile(np.array([0.9, 0.6, 0.3], np.float32), (64, 1)))
    else:
        # the map holds one colour, so c is its sRGB decoding (IEC 61966-2-1, in float64) whatever the hit: an independent number
        x = np.array(DIFFUSE_TEXEL[:3], np.float64) / 255.0
        want = np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
        assert np.abs(col.astype(np.float64) - want).max() < 4 * 2.0 ** -23  # (the table's binary32 pow, the blend of four equal taps)
    # the clamp: a factor above one, and a NaN
    for factor, want_m in ((3.0, None), (float("nan"), 0.0), (-1.0, 0.0)):
        sc.materials[0]["u"][5] = factor
        c.set_materials(sc.materials)
        _, _, mm = c.material_inputs_batch(0, tri, b32)
        assert np.isfinite(mm).all() and mm.min() >= 0.0 and mm.max() <= 1.0
        if want_m is not None:
            assert np.all(mm == want_m)
        else:
            assert np.allclose(mm, np.minimum(1.0, 3.0 * mr[:, 2]), atol=1e-5)


# ---- 5. transport ------------------------------------------------------------------------------------------------------------------------------

def _floor_expectation(mat, scene, W, H):
    """E[radiance] per block of BSDF sampling alone and of NEE + MIS on tests/test_bsdf_pins.py's glossy floor, for the METALROUGH rule in
    float64: the estimator structure of BP._floor_expectation (the light sample weighted against eval's pdf, the BSDF sample against the
    light's, the reference's un-clamped roulette on a hit) with ONE pdf — sample's and eval's are the same mixture."""
    ref = R.MetalRough.of(mat)
    P, WI = BP._pixel_geometry(scene, W, H)
    light = BP._rectangle_nodes()
    naive, mis = np.zeros((len(P), 3)), np.zeros((len(P), 3))
    power = lambda a, b: a * a / (a * a + b * b)  # noqa: E731
    for k in range(len(P)):
        wo, dw, L, p_l = light(P[k])
        f, p, same = ref.eval(WI[k], wo)
        ok, ok_l = same & (p > 1e-4), p_l > 1e-4
        with np.errstate(divide="ignore", invalid="ignore"):
            T = np.where(ok[:, None], f / p[:, None], 0.0)
        rr = np.minimum(1.0, 1.0 / np.maximum(T.max(-1), 1e-30))
        w_s = np.where(ok_l, power(p, p_l), 0.0)
        naive[k] = (f * (L * ok * rr * dw)[:, None]).sum(0)
        mis[k] = (f * (L * ok * ok_l * power(p_l, p) * dw)[:, None]).sum(0) + (f * (L * ok * rr * w_s * dw)[:, None]).sum(0)
    return BP._block_mean(naive, W, H), BP._block_mean(mis, W, H)


@pytest.mark.parametrize("case", ((0.3, 1.0), (0.5, 0.0)), ids=lambda c: "r%g-m%g" % c)
def test_glossy_floor_transport(gpu_ctx_factory, case):
    """A METALROUGH floor mirrors the rectangular emitter towards the camera (64 x 64, paths of two vertices): block means of BSDF
    sampling alone and of NEE + MIS against the float64 quadrature with the existing z-bar (1 % systematic, as the other floors), and the
    two estimators against each other."""
    r, m = case
    mat = R.material((0.9, 0.7, 0.4), r, m)
    estimate = BP._gpu_estimator(gpu_ctx_factory, 64, 64)
    est = {mis: estimate(lambda W, H: BP._floor_scene(W, H, mat, mis), 4096) for mis in (False, True)}
    e = est[True]
    want_naive, want_mis = _floor_expectation(mat, BP._floor_scene(e.W, e.H, mat, True), e.W, e.H)
    lit = want_naive.max(1) > 0.05 * want_naive.max()
    assert lit.mean() > 0.3, "the camera must see the emitter's reflection"
    assert np.median(e.se[lit] / want_mis[lit]) < 0.03, "the estimate is too noisy for its pass to mean anything"
    _assert_agree(_z(est[False].mean, est[False].se, want_naive, 0.0, systematic=1e-2)[lit], "metalrough floor %s, BSDF sampling alone" % (case,))
    _assert_agree(_z(est[True].mean, est[True].se, want_mis, 0.0, systematic=1e-2)[lit], "metalrough floor %s, NEE + MIS" % (case,))
    # one integral, two estimators — up to the roulette, which takes from BSDF-sampled hits only (predicted, so it is subtracted)
    z = _z(est[True].mean - (want_mis - want_naive), est[True].se, est[False].mean, est[False].se, systematic=1e-2)[lit]
    _assert_agree(z, "metalrough floor %s, MIS on against off" % (case,))
    ratio = want_mis[lit] / want_naive[lit]
    assert ratio.min() > 1.0 - 2e-3 and ratio.max() < 1.1


# ---- 6. pipelines, queue sizes, the flavor word ------------------------------------------------------------------------------------------

def _five_type_scene(W=48, H=48, metal=True):
    """tests/scene_helpers.py's material zoo without the environment map, plus a torus and a textured quad of the fifth type whose
    metallic-roughness map is the B checker"""
    sc = SH.material_zoo_scene(W, H, path_length=5, hdr=False, textures=True)
    mats = list(sc.materials)
    n = len(mats)
    if metal:
        mats += [R.material((1.0, 0.77, 0.34), 0.35, 1.0), R.material((0.8, 0.8, 0.8), 0.9, 1.0)]
    else:
        mats += [pod.make_material(pod.MAT_PLASTIC, albedo=(1.0, 0.77, 0.34), roughness=0.35), pod.make_material(pod.MAT_PLASTIC, albedo=(0.8, 0.8, 0.8), roughness=0.9)]
    quad = scenegen.quad((-1, 0, -1), (-1, 0, 1), (1, 0, 1), (1, 0, -1))
    for k in range(3):
        quad["texCoord%d" % k][:, 0] = (quad["pos%d" % k][:, 0] + 1.0) * 2.0
        quad["texCoord%d" % k][:, 1] = (quad["pos%d" % k][:, 2] + 1.0) * 2.0
    torus = scenegen.displaced_torus(40, 20, seed=4, major=0.5, minor=0.22)
    floor = scenegen.quad((-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4))
    light = scenegen.quad((-0.8, 0, -0.8), (0.8, 0, -0.8), (0.8, 0, 0.8), (-0.8, 0, 0.8))
    placements = [
        (1, 0, capi.mat4_from_trs((0, 0, 0))),
        (0, 1, capi.mat4_from_trs((-1.4, 0.55, 0.0), (20, 30, 0))),
        (0, 2, capi.mat4_from_trs((0.0, 0.55, 0.3), (90, 0, 15), (1.1, 1.1, 1.1))),
        (0, 3, capi.mat4_from_trs((1.4, 0.6, -0.2), (0, 60, 40), (1.0, 1.3, 1.0))),
        (0, 5, capi.mat4_from_trs((0.2, 0.5, 1.6), (45, 0, 0), (0.7, 0.7, 0.7))),
        (2, 4, capi.mat4_from_trs((0, 3.0, 0), (180, 0, 0))),
        (0, n, capi.mat4_from_trs((-0.6, 0.5, 1.4), (60, 10, 0), (0.8, 0.8, 0.8))),
        (3, n + 1, capi.mat4_from_trs((1.2, 0.02, 1.6), (0, 25, 0), (0.9, 0.9, 0.9))),
    ]
    out = SH.BuiltScene([torus, floor, light, quad], placements, materials=np.array(mats, dtype=pod.MAT_DT), camera=sc.camera, settings=sc.settings,
                        diffuse_maps=sc.diffuse_maps, emissive_maps=sc.emissive_maps)
    out.lights = SH.mesh_lights(out.instances, out.materials)
    det = [pod.make_material_detail()] * (n + 1) + [pod.make_material_detail(-1, 0, 1.0)]
    out.roughness_maps, out.material_detail = [_checker_map()], np.array(det, dtype=pod.DETAIL_DT)
    return out


def _frames(c, n=3):
    c.reset_frame_number()
    out = []
    for _ in range(n):
        c.render_frame()
        out.append(c.read_radiance().copy())
    return np.stack(out)


def test_pipelines_queue_sizes_and_the_flavor_word(gpu_ctx_factory):
    """48 x 48, all five types and a detail map, pixel-keyed numbers: the tail kernel on equals the tail kernel off bit for bit; the fifth
    type's queue row counts hits at bounce 1; the flavor bit is set only while a type-4 material exists; replacing the material restores
    the old flavor word and the old frames; the classic pipeline equals SCAN bit for bit, queue sizes included."""
    sc = _five_type_scene()
    c = gpu_ctx_factory(48, 48)
    sc.upload(c)
    c.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    c.set_tail_bounce(0)
    level = _frames(c)
    flavor = c.debug_pass_flavor()
    assert flavor & capi.FLAVOR_METAL and not flavor & capi.FLAVOR_NO_MAPS
    sizes = c.read_material_queue_sizes(pod.MAT_METALROUGH)
    assert sizes[1] > 0 and sizes[2] > 0 and sizes[0] == 0
    q = c.read_queue_sizes()
    assert np.array_equal(c.read_material_queue_sizes(pod.MAT_PLASTIC), q["plasticSize"]) and np.array_equal(c.read_material_queue_sizes(pod.MAT_DIFFUSE), q["diffuseSize"])
    assert np.isfinite(level).all() and level.mean() > 0.01
    c.set_tail_bounce(2)
    assert np.array_equal(_frames(c).view(np.uint32), level.view(np.uint32)), "tail kernel from bounce 2 against the level-by-level pass"
    c.set_tail_bounce(0)
    # the metal differs from the plastic it would otherwise have been
    plain = _five_type_scene(metal=False)
    c2 = gpu_ctx_factory(48, 48)
    plain.upload(c2)
    c2.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    c2.set_tail_bounce(0)
    before = _frames(c2)
    flavor_before = c2.debug_pass_flavor()
    assert not flavor_before & capi.FLAVOR_METAL
    assert np.all(c2.read_material_queue_sizes(pod.MAT_METALROUGH) == 0)
    assert not np.array_equal(before, level)
    # the same context with the material swapped in and out again
    c2.set_materials(sc.materials)
    with_metal = _frames(c2)
    assert c2.debug_pass_flavor() == flavor_before | capi.FLAVOR_METAL
    assert np.array_equal(with_metal.view(np.uint32), level.view(np.uint32))
    c2.set_materials(plain.materials)
    assert np.array_equal(_frames(c2).view(np.uint32), before.view(np.uint32)) and c2.debug_pass_flavor() == flavor_before
    # the classic pipeline (ordered compaction: the logic kernel, the fifth queue, one material kernel per type) equals SCAN bit for bit
    _frames(c)  # (level by level again: the tail kernel's pass above counts no queue items behind its first bounce)
    scan_sizes = {t: c.read_material_queue_sizes(t).copy() for t in range(5)}
    c.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_ORDERED, pod.CONDUCTOR_EXTENDED)
    classic = _frames(c)
    assert c.debug_pass_flavor() & capi.FLAVOR_METAL and not c.debug_pass_flavor() & 1
    assert np.array_equal(classic.view(np.uint32), level.view(np.uint32)), "classic pipeline against SCAN"
    for t in range(5):
        assert np.array_equal(c.read_material_queue_sizes(t), scan_sizes[t]), ("queue sizes of type", t)
    # ... and runs under the reference's slot-keyed numbers too, where the fifth queue's second roulette draw must be the logic kernel's
    c.set_modes(pod.RNG_REFERENCE_SLOT, pod.COMPACT_ORDERED, pod.CONDUCTOR_EXTENDED)
    slot_keyed = _frames(c)
    assert np.isfinite(slot_keyed).all() and c.read_material_queue_sizes(pod.MAT_METALROUGH)[1] == scan_sizes[pod.MAT_METALROUGH][1], "every camera hit survives bounce 1"
    assert slot_keyed.mean() > 0.01
    c.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    c.enable_kernel_timing(True)
    c.read_kernel_times(reset=True)
    _frames(c, 2)
    t = c.read_kernel_times()
    print("material launches of the five-type scene, 48 x 48: %.4f ms over %d launches" % (t["shade"]["ms"], t["shade"]["launches"]))
    c.enable_kernel_timing(False)


def test_fog_over_the_fifth_type(gpu_ctx_factory):
    """The medium's free-flight kernel reads the hit records in front of the material launch and must treat the fifth type's code as a hit:
    a medium whose box no ray crosses leaves every bit of the frames, one that fills the scene scatters in front of the metal too."""
    sc = _five_type_scene()
    c = gpu_ctx_factory(48, 48)
    sc.upload(c)
    c.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    c.set_tail_bounce(0)
    clear = _frames(c)
    hits = c.read_material_queue_sizes(pod.MAT_METALROUGH).copy()
    c.set_medium(pod.make_medium(box_min=(50, 50, 50), box_max=(51, 51, 51), sigma_t=0.7, g=0.3, albedo=(0.9, 0.9, 0.9)))
    away = _frames(c)
    assert c.debug_pass_flavor() & capi.FLAVOR_MEDIUM and c.debug_pass_flavor() & capi.FLAVOR_METAL
    assert np.array_equal(away.view(np.uint32), clear.view(np.uint32))
    assert np.array_equal(c.read_material_queue_sizes(pod.MAT_METALROUGH), hits)
    c.set_medium(pod.make_medium(box_min=(-6, -1, -6), box_max=(6, 6, 6), sigma_t=0.25, g=0.3, albedo=(0.9, 0.9, 0.9)))
    fog = _frames(c)
    thick = c.read_material_queue_sizes(pod.MAT_METALROUGH)
    assert np.isfinite(fog).all() and not np.array_equal(fog, clear)
    assert 0 < thick[1] < hits[1], "some camera paths scatter in front of the metal, the rest still reach it"
    c.set_medium(None)
    assert np.array_equal(_frames(c).view(np.uint32), clear.view(np.uint32))


def test_glossy_floor_transport_in_the_classic_pipeline(gpu_ctx_factory):
    """test_glossy_floor_transport's (0.3, 1) floor under NEE + MIS again, rendered by the classic pipeline (ordered compaction) with the
    reference's slot-keyed numbers — a stream SCAN's bit-equality does not cover — against the same float64 quadrature and z-bar."""
    mat = R.material((0.9, 0.7, 0.4), 0.3, 1.0)
    W = H = 64
    ctx = gpu_ctx_factory(W, H)
    BP._floor_scene(W, H, mat, True).upload(ctx)
    ctx.set_modes(pod.RNG_REFERENCE_SLOT, pod.COMPACT_ORDERED, pod.CONDUCTOR_EXTENDED)
    ctx.set_frames_per_pass(64)
    ctx.reset_frame_number()
    e = BP._BlockEstimate(W, H)
    for _ in range(2048 // 64):
        ctx.render_frame()
        for frame in ctx.read_radiance().reshape(64, W * H, 3):
            e.add(frame)
    _, want_mis = _floor_expectation(mat, BP._floor_scene(W, H, mat, True), W, H)
    lit = want_mis.max(1) > 0.05 * want_mis.max()
    assert np.median(e.se[lit] / want_mis[lit]) < 0.03
    _assert_agree(_z(e.mean, e.se, want_mis, 0.0, systematic=1e-2)[lit], "metalrough floor, classic pipeline, slot-keyed numbers, NEE + MIS")


def test_the_feature_buffers_albedo_is_the_base_colour(gpu_ctx_factory):
    """the AOV albedo of the type is c: on the floor scene every camera ray hits the METALROUGH floor or the black emitter"""
    mat = R.material((0.9, 0.7, 0.4), 0.3, 1.0)
    ctx = gpu_ctx_factory(32, 32)
    BP._floor_scene(32, 32, mat, True).upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    ctx.set_aov(True)
    ctx.reset_frame_number()
    ctx.render_frame()
    ctx.accumulate()
    albedo, _ = ctx.read_aov_frame()
    assert np.all(albedo[:, 3] == 1.0), "every camera ray hits something"
    floor = np.all(albedo[:, :3] == np.float32([0.9, 0.7, 0.4]), axis=1)
    emitter = np.all(albedo[:, :3] == 0.0, axis=1)
    assert np.all(floor | emitter) and floor.mean() > 0.5
