"""The float64 expectations of tests/instance_matrix_reference.py on the CPU, no device: that the composition restates its parts, that every
case keeps at least 12 of its 16 blocks, what the quadratures leave (the systematic allowance tests/test_gpu_instance_matrix.py compares
the device with is this measurement, not a choice), and that the neighbours of every case differ from it by several times the 2 % bar."""
import numpy as np
import pytest

from nexus_amd import pod
from tests import alpha_test_reference as ATR
from tests import feature_product_reference as F
from tests import instance_matrix_reference as M
from tests import metalrough_reference as MRR
from tests import test_gpu_analytic_lights as AL

SE_BAR = 0.02
FAMILIES = tuple(M.FAMILY)
CASES = [(family, analytic) for family in FAMILIES for analytic in (False, True)]


def test_the_scene_is_what_the_expectation_assumes():
    x0, x1, z0, z1, h = M.EMITTER
    P = M.floor_points(2).reshape(-1, 3)
    # the emitter is above the eye and below the pane; no camera ray reaches it or the pane on its way to the floor
    assert F.PANE[4] > h > F.EYE[1]
    eye = np.broadcast_to(F.EYE, P.shape)
    assert np.all(AL._visible(eye, P, F.PANE)) and np.all(AL._visible(eye, P, M.EMITTER))
    # no analytic light's shadow segment from the floor the camera sees meets the emitter: its shadows fall outside the view
    for name in F.ALL:
        assert not M.pane_factors("blend", 2)[name]["crossed_emitter"].any(), name
    # the emitter's segments cross nothing: both of the estimator's techniques reach every node
    wo, _, p_l = M.emitter_nodes(P[::97], 4)
    for k in range(wo.shape[1]):
        t = ATR.trace(P[::97], wo[:, k], np.full(len(wo), 1.0e3), M.occluders("base")[:1])
        assert not t["crossings"].any()
    # the light sample's pdf stays far above the validity rule's 1e-4 with four lights in the pick, and no albedo is above one
    assert (p_l / 4).min() > 1e-2 and max(M.METAL_BASE) <= 1.0 and F.RHO <= 1.0
    for family in FAMILIES:
        sc = M.scene(family)
        assert len(sc.meshes) == 3 and all(len(m) == 2 for m in sc.meshes), "a two-triangle floor, pane and emitter"
        assert int(sc.settings["pathLength"]) == 2 and len(sc.lights) == 1 and float(sc.settings["backgroundIntensity"]) == 0.0
        assert (family == "no_maps") == bool(np.all(sc.materials["diffuseMapId"] == -1))
        assert (int(sc.materials[0]["type"]) == pod.MAT_METALROUGH) == (family in ("metal", "solid"))
    solid = M.scene("solid")
    assert float(solid.materials[0]["opacity"]) == np.float32(M.FLOOR_OPACITY) and list(solid.material_alpha["mode"]) == [pod.ALPHA_OPAQUE, pod.ALPHA_MASK, pod.ALPHA_BLEND]
    o_a = [F.PANE_OPACITY * a / 255.0 for a in F.PANE_ALPHA]
    assert min(o_a) < M.PANE_CUTOFF < max(o_a), "the cutoff lies between the pane's two values of o a"
    # both metalness values are met, and the lookup blends them (the per-texel path)
    mr = M.metal_map()[..., 2]
    assert sorted(np.unique(mr)) == sorted(M.METAL_B)


def test_metal_eval_many_restates_the_rule():
    """metal_eval_many against metalrough_reference.MetalRough.eval, point by point in the point's own local frame"""
    rs = np.random.RandomState(5)
    n, k = 40, 30
    ns = rs.normal(size=(n, 3))
    ns /= np.linalg.norm(ns, axis=1, keepdims=True)
    wi = rs.normal(size=(n, 3))
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    wi = np.where(((wi * ns).sum(1) < 0)[:, None], -wi, wi)
    wo = rs.normal(size=(n, k, 3))
    wo /= np.linalg.norm(wo, axis=2, keepdims=True)
    rough, metal = rs.uniform(0.02, 1.0, n).astype(np.float32).astype(np.float64), rs.uniform(-0.2, 1.2, n).astype(np.float32).astype(np.float64)  # (the rule starts from binary32 records)
    f, p, same = M.metal_eval_many(M.METAL_BASE, rough, M.METAL_IOR, metal, ns, wi, wo)
    for j in range(n):
        t = np.cross(ns[j], [1.0, 0.0, 0.0] if abs(ns[j][0]) < 0.9 else [0.0, 1.0, 0.0])
        t /= np.linalg.norm(t)
        frame = np.stack([t, np.cross(ns[j], t), ns[j]])
        ref = MRR.MetalRough(M.METAL_BASE, rough[j], M.METAL_IOR, metal[j])
        f1, p1, s1 = ref.eval(frame @ wi[j], wo[j] @ frame.T)
        assert np.array_equal(same[j], s1)
        assert np.allclose(f[j], f1, rtol=1e-9, atol=1e-300) and np.allclose(p[j], p1, rtol=1e-9, atol=1e-300)
    assert same.mean() > 0.3 and (f > 0).any()
    # ... and the Lambert form integrates to rho over the hemisphere
    grid, dw = MRR.upper_grid()
    fl, pl, _ = M.lambert_many(0.6, np.array([[0.0, 0.0, 1.0]]), np.array([[0.6, 0.0, 0.8]]), grid[None])
    assert abs(fl[0, :, 0].sum() * dw - 0.6) < 1e-3 and abs(pl[0].sum() * dw - 1.0) < 1e-3


def test_the_estimator_is_the_integral_where_nothing_is_cut_off():
    """w_light + w_bsdf = 1 and the roulette takes nothing on a Lambert floor: the MIS estimator's expectation is the plain integral,
    whatever the light sample's pdf — which is why uniform, table and tree sampling share one expectation"""
    P = M.floor_points(1)[0][::53]
    wi = F.EYE[None, :] - P
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    wo, dw, p_l = M.emitter_nodes(P)
    f, p, same = M.lambert_many(F.RHO, np.broadcast_to(M.N_UP, P.shape), wi, wo)
    plain = (f * dw[..., None]).sum(1)
    for scale in (1.0, 0.25, 3.0):
        assert np.allclose(M.mis_estimator(f, p, same, np.ones(3), p_l * scale, dw), plain, rtol=1e-12)
    # uniform sampling picks a triangle first: another pdf on the emitter's two unequal triangles, the same expectation
    p_u = M.emitter_nodes(P, pick="uniform")[2]
    assert np.abs(p_u / p_l - 1.0).max() > 0.2
    assert np.allclose(M.mis_estimator(f, p, same, np.ones(3), p_u, dw), plain, rtol=1e-12)
    # the glossy floor: a pick probability other than the table's moves the expectation by less than the allowance (the roulette's share)
    fm, pm, sm = M.metal_eval_many(M.METAL_BASE, np.full(len(P), M.METAL_ROUGHNESS), M.METAL_IOR, np.full(len(P), 0.5), np.broadcast_to(M.N_UP, P.shape), wi, wo)
    a, b = M.mis_estimator(fm, pm, sm, np.ones(3), p_l, dw), M.mis_estimator(fm, pm, sm, np.ones(3), p_u / 4, dw)
    print("the glossy floor under uniform sampling's pdf with four lights in the pick, against the table's with one: largest relative change %.3g" % np.abs(b / a - 1.0).max())
    assert np.abs(b / a - 1.0).max() < 0.1 * M.systematic("metal", False)


@pytest.mark.parametrize("family,analytic", CASES)
def test_every_case_keeps_at_least_twelve_blocks(family, analytic):
    reasons = M.left_out(family, analytic)
    kept = M.kept(family, analytic)
    print("%s, analytic %s: kept %d of %d; left out: %s" % (family, analytic, kept.sum(), M.BLOCKS, {w: np.flatnonzero(m).tolist() for w, m in reasons.items() if m.any()}))
    assert kept.sum() >= 12
    assert np.all(M.expectation(family, analytic)[kept] > 0)
    assert not reasons["horizon"].any(), "the map leans towards the camera's side"


def _residue(a, b, keep):
    return float((np.abs(a - b) / b)[keep].max())


@pytest.mark.parametrize("kind", sorted(set(M.FLOOR_KIND.values())))
def test_the_systematic_allowance_is_the_quadratures_residue(kind):
    """N against 2 N emitter nodes per side (at 2 x 2 positions per pixel: the node quadrature's residue does not depend on them), and 4 x 4
    against 8 x 8 positions per pixel (at N / 2 nodes per side, for the same reason), over the kept blocks of the kind's families with and
    without the analytic lights.  The constants of instance_matrix_reference are these measurements: not below, not above twice."""
    families = [f for f in FAMILIES if M.FLOOR_KIND[f] == kind]
    half = M.NODES // 2
    nodes_term = sub_term = 0.0
    for family in families:
        for analytic in (False, True):
            keep = M.kept(family, analytic)
            assert np.array_equal(keep, M.kept(family, analytic, 8) if analytic else keep), "the finer quadrature leaves the same blocks out"
            E = lambda sub, nodes: M.expectation(family, analytic, sub, nodes, shadings=("mapped",))  # noqa: E731
            nodes_term = max(nodes_term, _residue(E(2, M.NODES), E(2, 2 * M.NODES), keep))
            sub_term = max(sub_term, _residue(E(4, half), E(8, half), keep))
    print("%s: N = %d against %d nodes per side %.3g (NODES_TERM %.3g); 4 x 4 against 8 x 8 positions %.3g (SUB_TERM %.3g)" % (kind, M.NODES, 2 * M.NODES, nodes_term, M.NODES_TERM[kind], sub_term,
                                                                                                                        M.SUB_TERM[kind]))
    assert nodes_term <= M.NODES_TERM[kind] <= 2.0 * nodes_term, "measure again and write the measurement into instance_matrix_reference.NODES_TERM"
    assert sub_term <= M.SUB_TERM[kind] <= 2.0 * sub_term, "measure again and write the measurement into instance_matrix_reference.SUB_TERM"
    for family in families:
        for analytic in (False, True):
            assert M.systematic(family, analytic) <= 1e-2, "not above what the glossy floors already use: refine the quadrature"


def test_the_edge_band_share():
    for family in FAMILIES:
        share = M.unclear_share(family)
        print("%s: largest share of shadow segments in the EDGE band %.3g" % (family, share))
        assert share <= M.UNCLEAR_TERM


@pytest.mark.parametrize("family,analytic", CASES)
def test_the_neighbours_differ_by_several_times_the_bar(family, analytic):
    keep = M.kept(family, analytic)
    full = M.expectation(family, analytic)
    near = M.neighbours(family, analytic)
    want = set()
    if analytic:
        want.add("without the analytic lights")
    if family in ("detail", "metal", "solid"):
        want.add("with the geometric normal")
    if family in ("metal", "solid"):
        want.add("Lambert in place of GGX")
    if family == "solid":
        want.add("the floor as BLEND")
        if analytic:
            want.add("the pane as BLEND")
    assert set(near) == want
    for what, v in near.items():
        rel = np.abs(v / full - 1.0).max(1)[keep]
        print("%-8s analytic %-5s %-30s differs by a median of %.3f (min %.3f, max %.3f) over %d kept blocks" % (family, analytic, what, np.median(rel), rel.min(), rel.max(), keep.sum()))
        assert np.median(rel) >= 3.0 * SE_BAR and (rel > 5.0 * SE_BAR).mean() >= 0.25, what


# ---- the medium ------------------------------------------------------------------------------------------------------------------------------------

FOG_CASES = [(metal, analytic, grid) for grid in (False, True) for metal in (False, True) for analytic in (False, True)]


def test_the_fog_scene_is_what_the_expectation_assumes():
    from tests import medium_reference as MR
    o, d = M._lattice_rays(64)
    lo, hi = np.array(M.FOG_BOX[0]), np.array(M.FOG_BOX[1])
    # every camera ray crosses the box and none starts in it; the lamp and the point light are outside the box and outside the view
    t0, L, crosses = MR.segment(lo, hi, np.broadcast_to(o, d.shape), d, np.full(len(d), np.inf))
    assert crosses.all() and t0.min() > 0
    x0, x1, z0, z1, h = M.LAMP
    assert h > hi[1]
    s = (h - o[1]) / d[:, 1]
    at = o + d * s[:, None]
    assert not np.any((s > 0) & (at[:, 0] > x0) & (at[:, 0] < x1) & (at[:, 2] > z0) & (at[:, 2] < z1)), "a camera ray meets the lamp"
    q = M.FOG_POINT["position"].astype(np.float64)
    assert np.any((q < lo) | (q > hi))
    to = q - o
    assert ((to / np.linalg.norm(to)) @ d.T).max() < np.cos(np.radians(3.0)), "no camera ray passes within three degrees of the point light"
    # the backdrop is behind the box and wider than the view
    assert M.BACKDROP_Z < lo[2]
    sb = (M.BACKDROP_Z - o[2]) / d[:, 2]
    assert np.abs((o + d * sb[:, None])[:, :2]).max() < M.BACKDROP_HALF
    assert all(n % 8 for n in M.fog_density().shape) and M.fog_density().shape == F.GRID_SHAPE
    for metal in (False, True):
        sc = M.fog_scene(metal, grid=True)
        assert int(sc.settings["pathLength"]) == 2 and len(sc.lights) == 1 and (pod.MAT_METALROUGH in list(sc.materials["type"])) == metal


@pytest.mark.parametrize("g", [0.0, 0.7])
def test_the_rectangle_quadrature_shrunk_to_a_point_is_the_point_lights(g):
    """lamp_single_scatter's source loop with a point in place of the lamp's nodes reproduces medium_reference.single_scatter and
    test_medium_reference.ss_expectation on their own scene; and a lamp shrunk to that point is that loop with the lamp's cosine"""
    from tests import medium_reference as MR
    from tests import test_medium_reference as TR
    medium = TR.ss_medium(g)
    pos, dirs = MR.camera_rays(TR.ss_camera(), TR.W, TR.H, TR.SS_SUB)
    mean = np.zeros(TR.W * TR.H)
    for k in range(len(dirs)):
        mine = M.lamp_single_scatter(pos, dirs[k], point=TR.SS_LIGHT, medium=medium, t_nodes=96)
        if k == 0:
            theirs, _ = MR.single_scatter(medium, TR.SS_LIGHT, 1.0, pos, dirs[k])
            assert np.allclose(mine, theirs, rtol=1e-12, atol=0.0)
        mean += mine / len(dirs)
    assert np.allclose(TR.block_means(mean), TR.ss_expectation(g, TR.SS_SUB)[0], rtol=1e-12, atol=0.0)
    eps = 1e-4
    x, y, z = TR.SS_LIGHT
    rays = dirs[0][::37]
    small = M.lamp_single_scatter(pos, rays, medium=medium, t_nodes=96, n_lamp=2, rect=(x - eps / 2, x + eps / 2, z - eps / 2, z + eps / 2, y)) / (eps * eps)
    point = M.lamp_single_scatter(pos, rays, medium=medium, t_nodes=96, point=TR.SS_LIGHT, cosine=True)
    assert np.allclose(small, point, rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("grid", [False, True], ids=["homogeneous", "grid"])
def test_the_fogs_allowance_is_its_quadratures_residue(grid):
    """every count doubled, one at a time — the lattice of camera rays, the nodes on the camera segment, the lamp's nodes per side — over
    the four cases of the form; the sum of the three largest relative changes is instance_matrix_reference.FOG_TERM"""
    terms = {}
    for name, kw in (("lattice", dict(res=2 * M.FOG_LATTICE)), ("segment nodes", dict(t_nodes=2 * M.FOG_T_NODES)), ("lamp nodes", dict(n_lamp=2 * M.LAMP_NODES))):
        terms[name] = max(float(np.abs(M.fog_expectation(metal, analytic, grid, **kw) / M.fog_expectation(metal, analytic, grid) - 1.0).max()) for metal in (False, True) for analytic in (False, True))
    total = sum(terms.values())
    print("%s: %s; sum %.3g (FOG_TERM %.3g)" % ("grid" if grid else "homogeneous", ", ".join("%s %.3g" % kv for kv in terms.items()), total, M.FOG_TERM[grid]))
    assert total <= M.FOG_TERM[grid] <= 2.0 * total, "measure again and write the measurement into instance_matrix_reference.FOG_TERM"
    assert M.FOG_TERM[grid] <= 1e-2, "not above what the glossy floors already use: refine the quadrature"


@pytest.mark.parametrize("metal,analytic,grid", FOG_CASES)
def test_the_fogs_neighbours_differ_by_several_times_the_bar(metal, analytic, grid):
    keep = M.fog_kept(metal, analytic, grid)
    assert keep.sum() >= 12
    full = M.fog_expectation(metal, analytic, grid)
    near = M.fog_neighbours(metal, analytic, grid)
    assert len(near) == (3 if analytic else 2)
    for what, v in near.items():
        rel = np.abs(v / full - 1.0).max(1)[keep]
        print("metal %-5s analytic %-5s grid %-5s %-26s differs by a median of %.3f (min %.3f, max %.3f) over %d kept blocks" % (metal, analytic, grid, what, np.median(rel), rel.min(), rel.max(), keep.sum()))
        assert np.median(rel) >= 3.0 * SE_BAR and (rel > 5.0 * SE_BAR).mean() >= 0.25, what
