"""The all-features product (tests/feature_product_reference.py) on the CPU, no device: that the composition restates its parts, and that the
chosen scene can tell the factors apart — few blocks left out, each for a stated reason; every factor and every light moves the
expectation by more than 10 % in at least a quarter of the kept blocks; the sub-pixel quadrature has converged (its residue is the
`systematic` term tests/test_gpu_feature_products.py compares the device with)."""
import numpy as np

from tests import analytic_light_reference as AR
from tests import feature_product_reference as F
from tests import grid_medium_reference as G
from tests import test_gpu_analytic_lights as AL
from tests import test_gpu_detail_maps as DM

SUB = 4


def test_the_scene_is_what_the_product_assumes():
    sc = F.scene()
    lo, hi = np.array(F.BOX_MIN), np.array(F.BOX_MAX)
    x0, x1, z0, z1, h = F.PANE
    P = AL._floor_points(sc, F.N_UP, 2)
    # no ray starts inside the box: the eye is outside it, the floor below it, the lights above it
    assert F.EYE[0] > hi[0] and lo[1] > 0.0
    for name, light in F.LIGHTS.items():
        assert name == "sun" or light["position"][1] > hi[1]
    # no camera ray reaches the pane (a pass-through would spend a bounce), and the pane is black and above the box
    assert h > F.EYE[1] > hi[1] and np.abs(P[..., 1]).max() < 1e-12 and np.all(AL._visible(np.broadcast_to(F.EYE, P.shape), P, F.PANE))
    assert np.all(sc.materials[1]["u"][0:3] == 0) and float(sc.materials[1]["opacity"]) == F.PANE_OPACITY and int(sc.materials[1]["diffuseMapId"]) == 0
    # the point light shines through the pane, the spot from below it
    assert F.LIGHTS["point"]["position"][1] > h > F.LIGHTS["spot"]["position"][1]
    # the medium absorbs only; the grid's dimensions are no multiples of the brick; the walk is far from the refusal bar
    grid = F.density()
    assert np.all(F.MEDIUM["albedo"] == 0) and all(n % G.BRICK for n in grid.shape) and grid.shape == F.GRID_SHAPE
    assert 0.19 < grid.min() < 0.25 and 1.7 < grid.max() <= 1.8
    bar = F.SIGMA_T * float(grid.max()) * float(np.linalg.norm(hi - lo))
    print("sigmaT x max rho x diagonal = %.2f (the refusal bar is 512)" % bar)
    assert bar < 512.0 / 10
    # paths of two vertices, and nothing but the floor reflects or emits
    assert int(sc.settings["pathLength"]) == 2 and len(sc.lights) == 0 and float(sc.settings["backgroundIntensity"]) == 0.0


def test_closed_form_many_restates_closed_form():
    sc = F.scene()
    P = AL._floor_points(sc, F.N_UP, 1)[0][::37]
    ns = DM._reference(sc, P, F.normal_map())["ns"]
    for name, light in F.LIGHTS.items():
        many, _ = F.closed_form_many(light, P, ns, F.RHO)
        flat, _ = F.closed_form_many(light, P, np.broadcast_to(F.N_UP, P.shape), F.RHO)
        lit = 0
        for k in range(len(P)):
            for normal, got in ((ns[k], many[k]), (F.N_UP, flat[k])):
                d, _ = F.shadow_segment(light, P[k:k + 1])
                if d[0] @ normal <= 1e-9:
                    assert np.all(got == 0.0)
                    continue
                assert np.allclose(got, AR.closed_form(light, P[k], normal, F.RHO), rtol=1e-12, atol=0.0), name
                lit += 1
        assert lit > len(P), name


def test_the_grid_quadrature_is_fine_enough():
    """F.PANELS panels of 8 nodes against 256: the residue in T on the scene's own segments"""
    F_ = F.factors(SUB)
    P = F_["P"][0][::16]
    worst = 0.0
    for name in F.ALL:
        d, length = F.shadow_segment(F.LIGHTS[name], P)
        worst = max(worst, np.abs(F.grid_transmittance(P, d, length) - F.grid_transmittance(P, d, length, panels=256)).max())
    to = P - F.EYE
    dist = np.linalg.norm(to, axis=1)
    worst = max(worst, np.abs(F.grid_transmittance(np.broadcast_to(F.EYE, P.shape), to / dist[:, None], dist) -
                              F.grid_transmittance(np.broadcast_to(F.EYE, P.shape), to / dist[:, None], dist, panels=256)).max())
    print("T with %d panels against 256: worst difference %.3g" % (F.PANELS, worst))
    assert worst < 1e-5


def _table(name, values):
    print("%-44s min %.2f  median %.2f  max %.2f" % (name, values.min(), np.median(values), values.max()))


def test_few_blocks_are_left_out_each_for_a_stated_reason():
    F_ = F.factors(SUB)
    _table("T_grid on the camera segments", F_["t_camera"])
    for name in F.ALL:
        _table("T_grid on the %s's shadow segments" % name, F_[name]["t_shadow"])
        _table("the pane's factor on the %s's shadow segments" % name, F_[name]["t_pane"])
    reasons = F.left_out(SUB)
    for why, mask in reasons.items():
        print("left out, %s: blocks %s" % (why, np.flatnonzero(mask).tolist()))
    kept = F.kept(SUB)
    share = 1.0 - kept.mean()
    print("share of blocks left out: %.1f %% (%d of %d)" % (100 * share, (~kept).sum(), F.BLOCKS))
    assert share <= 0.30
    # the scene exercises what the reasons are about: both alpha blocks and a lit, clear light
    crossed = [np.unique(np.round(F_[n]["t_pane"][F_[n]["crossed"] > 0], 6)) for n in F.ALL]
    seen = np.unique(np.concatenate(crossed))
    assert np.any(np.isclose(seen, 0.5)) and np.any(np.isclose(seen, 1.0 - 0.5 * 102 / 255.0, atol=1e-6)), seen
    assert not (F_["spot"]["crossed"] > 0).any() and (F_["point"]["crossed"] == 1).all()
    assert not reasons["horizon"].any(), "the map leans towards the camera's side"
    share_unclear = F.unclear_share(SUB)
    print("largest share of shadow segments in the EDGE band: %.3g" % share_unclear)
    assert share_unclear <= F.UNCLEAR_TERM


def test_every_factor_and_every_light_has_power():
    kept = F.kept(SUB)
    full = F.expectation(SUB)
    assert np.all(full[kept] > 0)
    variants = {"without " + f.replace("_", " on the ") if f.startswith("fog") else "without the " + f: F.expectation(SUB, **{f: False}) for f in F.FACTORS}
    variants.update({"without the %s light" % n: F.expectation(SUB, lights=tuple(m for m in F.ALL if m != n)) for n in F.ALL})
    assert len(variants) == 7
    for what, v in variants.items():
        rel = np.abs(v / full - 1.0).max(1)[kept]
        print("%-32s differs by more than 10 %% in %2d of %d kept blocks (median %.2f, max %.2f)" % (what, (rel > 0.10).sum(), kept.sum(), np.median(rel), rel.max()))
        assert (rel > 0.10).mean() >= 0.25, what


def test_the_sub_pixel_quadrature_has_converged():
    kept = F.kept(SUB)
    assert np.array_equal(kept, F.kept(8)), "the finer quadrature leaves the same blocks out"
    coarse, fine = F.expectation(SUB), F.expectation(8)
    term = (np.abs(coarse - fine) / fine)[kept].max()
    print("sub = 4 against sub = 8 over the kept blocks: largest relative difference %.3g (QUADRATURE_TERM %.3g)" % (term, F.QUADRATURE_TERM))
    assert term <= F.QUADRATURE_TERM, "measure again and write the measurement into feature_product_reference.QUADRATURE_TERM"
    assert F.QUADRATURE_TERM <= 2.0 * term, "the constant is the measurement, not an allowance"
    # ... and every left-out variant converges alike
    for f in F.FACTORS:
        a, b = F.expectation(SUB, **{f: False}), F.expectation(8, **{f: False})
        assert (np.abs(a - b) / b)[kept].max() <= 2.0 * F.QUADRATURE_TERM, f


# ---- the scene of the estimator pair ---------------------------------------------------------------------------------------------------------

def test_the_estimator_pair_integrates_one_integral():
    """p_light of the mesh emitter stays above the validity rule's 1e-4 everywhere on the floor (the rule drops no configuration); no
    albedo is above 1 (the un-clamped roulette takes nothing); and what the pane's pass-through can cost BSDF sampling is bounded"""
    sc = F.pair_scene(True)
    assert len(sc.lights) == 1 and np.all(sc.materials["u"][:, 0:3] <= 1.0) and np.all(F.PAIR_FOG["albedo"] <= 1.0) and int(sc.settings["pathLength"]) >= 3
    x0, x1, z0, z1, h = F.EMITTER
    assert F.BOX_MAX[1] < h < F.PAIR_PANE[4] and h > F.EYE[1], "above the fog and the eye, below the pane"
    n_lights = 3  # the emitter, the point light, the sampled environment
    P = AL._floor_points(sc, F.N_UP, 2).reshape(-1, 3)
    worst = np.inf
    for x in np.linspace(x0, x1, 5):
        for z in np.linspace(z0, z1, 5):
            to = np.array([x, h, z]) - P
            d2 = (to * to).sum(1)
            worst = min(worst, (d2 / (n_lights * (x1 - x0) * (z1 - z0) * (to[:, 1] / np.sqrt(d2)))).min())
    print("smallest p_light over the floor: %.3g (the validity rule asks for more than 1e-4)" % worst)
    assert worst > 1e-2
    # the point light's shadow segments from the floor the camera sees all cross the pane
    d, length = F.shadow_segment(F.PAIR_LIGHT, P)
    assert not np.any(AL._visible(P, P + d * length[:, None], F.PAIR_PANE))
    # the environment is lit below PAIR_BAND_TOP only, and from the fog box the pane lies above it
    env = F.pair_environment()
    lit = np.flatnonzero(env.max((1, 2)) > 0)
    assert lit.min() == F.PAIR_ENV_LIT[0] and lit.max() == F.PAIR_ENV_LIT[1] - 1 and env.max() == F.PAIR_ENV_MAX
    low = F.pair_pane_elevation()
    print("the pane from the fog box: at least %.1f degrees up; the lit band ends at %.2f degrees; bound on MIS - naive: %.3g"
          % (np.degrees(low), np.degrees(F.PAIR_BAND_TOP), F.pair_bound()))
    assert low > F.PAIR_BAND_TOP + np.radians(1.0)
    assert F.pair_bound() < 1e-3
