"""All shading features at once on the device: analytic lights, TRANSMIT shadows, detail maps, the medium and its density grid, power
sampling — the kernel instances and pass graphs that exist only in combination.

 a. the product: the floor of tests/feature_product_reference.py against its float64 expectation by z-scores per 16 x 16 block (the bars
    of tests/test_physics_pins.py), and every one-factor-left-out and one-light-left-out expectation refused by the same frames;
 b. one integral, two estimators: MIS against BSDF sampling alone with everything on and a scattering grid;
 c. every way of rendering the all-features fixture (tests/feature_scenes.py) gives the bits of one pass at a time;
 d. one live context through fifteen flavor words — more than a slot's graph cache holds — against fresh contexts.

The oracle knows none of these features; nothing here compares with it."""
import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import feature_product_reference as F
from tests import feature_scenes as FS
from tests import test_gpu_analytic_lights as AL
from tests import test_physics_pins as PP

pytestmark = pytest.mark.gpu

SCAN = AL.SCAN
EVERYTHING = capi.FLAVOR_ANALYTIC | capi.FLAVOR_TRANSMIT | capi.FLAVOR_DETAIL | capi.FLAVOR_MEDIUM | capi.FLAVOR_MEDIUM_GRID
FLAVOR_LIGHT_POWER, FLAVOR_AOV, FLAVOR_ENTRY, FLAVOR_ENV_MAP = 128, 64, 8, 4  # kFlavorLightPower, kFlavorAov, kFlavorEntry, kFlavorEnvMap (nxhip_render.hip)
MAX_GRAPH_INSTANCES = 8  # kMaxGraphInstances (nxhip_render.hip)


# ---- a. the product --------------------------------------------------------------------------------------------------------------------------

PER_PASS, MAX_FRAMES = 64, 4096
SE_BAR = 0.02  # the largest relative standard error of a kept block: what test_gpu_medium._pin demands


def _agrees(z):
    return np.abs(z).max() < 4.5 and (z * z).mean() < 1.6


@pytest.mark.parametrize("how", ["uniform", "power", "uniform, two passes in flight"])
def test_the_product_of_every_factor(gpu_ctx_factory, how):
    """Measured on an MI355X (printed by the test): 128 frames bring the 14 kept blocks under the 2 % bar (largest relative standard error
    1.3 %, median 0.6 %); against the product max |z| 1.93 and mean z^2 1.28 over 42 comparisons; with a factor or a light left out
    the mean z^2 is between 205 (the mapped normal) and 13 044 (the fog on the camera segment): all seven refused.  The three ways give
    the same statistics: power sampling picks among analytic lights as uniform sampling does, and passes in flight change no bit.
    The systematic term is derived, not measured: the quadrature's residue and the EDGE band's share (feature_product_reference)."""
    power, in_flight = how == "power", 2 if "two passes" in how else 1
    kept = F.kept()
    want = F.expectation()
    ctx = gpu_ctx_factory(F.W, F.H)
    sc = F.scene()
    sc.light_sampling = pod.LIGHTS_POWER if power else pod.LIGHTS_UNIFORM
    sc.upload(ctx)
    ctx.set_analytic_lights(F.light_array())
    ctx.set_modes(*SCAN)
    ctx.set_frames_per_pass(PER_PASS)
    ctx.set_passes_in_flight(in_flight)
    if in_flight > 1:
        ctx.set_queue_budget(4)  # 2 x 2 + 1 lanes do not fit: the chain shape, with the medium's three-launch levels
        assert ctx.queue_budget()[1]
    ctx.reset_frame_number()
    e = PP._Estimate(F.W, F.H)
    flavors = set()
    while True:
        ctx.render_frame()
        r = ctx.read_radiance().reshape(PER_PASS, F.W * F.H, 3)
        flavors.add(ctx.debug_pass_flavor())
        for k in range(PER_PASS):
            e.add(r[k])
        rel = (e.se / want)[kept].max()
        if (e.n >= 2 * PER_PASS and rel <= SE_BAR) or e.n >= MAX_FRAMES:
            break
    if in_flight > 1:
        nodes, edges, fan_out = ctx.debug_last_graph()
        assert (edges, fan_out) == (nodes - 1, 1), "not a chain: %s" % ((nodes, edges, fan_out),)
    ctx.close()
    print("%s: flavor words %s; %d frames; relative standard error of the kept blocks: median %.3g, max %.3g" % (how, sorted("%#x" % f for f in flavors), e.n, np.median((e.se / want)[kept]), rel))
    assert len(flavors) == 1
    flavor = flavors.pop()
    assert flavor & EVERYTHING == EVERYTHING and bool(flavor & FLAVOR_LIGHT_POWER) == power, "flavor %#x" % flavor
    assert rel <= SE_BAR, "%d frames do not bring the kept blocks under the 2 %% bar" % e.n
    assert np.all(np.isfinite(e.mean))
    PP._assert_agree(PP._z(e.mean, e.se, want, 0.0, systematic=F.SYSTEMATIC)[kept], "the product, " + how)
    wrong = {"without " + f: F.expectation(**{f: False}) for f in F.FACTORS}
    wrong.update({"without the %s light" % n: F.expectation(lights=tuple(m for m in F.ALL if m != n)) for n in F.ALL})
    for what, v in wrong.items():
        z = PP._z(e.mean, e.se, v, 0.0, systematic=F.SYSTEMATIC)[kept]
        print("%-28s max |z| %6.1f, mean z^2 %8.1f: %s" % (what, np.abs(z).max(), (z * z).mean(), "agrees" if _agrees(z) else "refused"))
        assert not _agrees(z), "the check has no power: " + what


# ---- b. one integral, two estimators ------------------------------------------------------------------------------------------------------------

PAIR_FRAMES = 1024


@pytest.mark.parametrize("light_sampling", [pod.LIGHTS_UNIFORM, pod.LIGHTS_POWER], ids=["uniform", "power"])
def test_mis_equals_naive_with_everything_on(gpu_ctx_factory, light_sampling):
    """Measured on an MI355X (printed by the test): 1 024 frames each, relative standard errors of the block means 0.33 % (MIS) and 0.75 %
    (naive) in the median, MIS / naive per block 0.986 .. 1.009; max |z| 1.78, mean z^2 0.56; naive x 1.05: mean z^2 28.8, refused.  The
    bound on the difference by construction (feature_product_reference.pair_bound, 5.4e-4) is derived, not measured."""
    est = {}
    for use_mis in (True, False):
        ctx = gpu_ctx_factory(F.W, F.H)
        sc = F.pair_scene(use_mis)
        sc.light_sampling = light_sampling
        sc.upload(ctx)
        ctx.set_analytic_lights(np.array([F.PAIR_LIGHT], dtype=pod.ALIGHT_DT))
        ctx.set_modes(*SCAN)
        ctx.set_frames_per_pass(PER_PASS)
        ctx.reset_frame_number()
        e = PP._Estimate(F.W, F.H)
        for _ in range(PAIR_FRAMES // PER_PASS):
            ctx.render_frame()
            r = ctx.read_radiance().reshape(PER_PASS, F.W * F.H, 3)
            for k in range(PER_PASS):
                e.add(r[k])
        flavor = ctx.debug_pass_flavor()
        ctx.close()
        assert flavor & EVERYTHING == EVERYTHING and flavor & FLAVOR_ENV_MAP and bool(flavor & FLAVOR_LIGHT_POWER) == (light_sampling == pod.LIGHTS_POWER), "flavor %#x" % flavor
        est[use_mis] = e
    mis, naive = est[True], est[False]
    assert np.all(naive.mean > 0) and np.all(np.isfinite(mis.mean))
    print("MIS / naive per block:", np.round(mis.mean[:, 0] / naive.mean[:, 0], 3), "relative standard errors, median (MIS, naive): %.3g, %.3g"
          % (np.median(mis.se / mis.mean), np.median(naive.se / naive.mean)))
    # (MIS may exceed naive by at most F.pair_bound(), by construction: an absolute term beside naive's standard error)
    bound = F.pair_bound()
    print("bound on MIS - naive: %.3g, %.3g of the darkest block" % (bound, bound / naive.mean.min()))
    PP._assert_agree(PP._z(mis.mean, mis.se, naive.mean, np.sqrt(naive.se ** 2 + bound ** 2)), "MIS against naive with everything on")
    z = PP._z(mis.mean, mis.se, naive.mean * 1.05, np.sqrt((naive.se * 1.05) ** 2 + bound ** 2))
    print("control, naive x 1.05: max |z| %.1f, mean z^2 %.1f" % (np.abs(z).max(), (z * z).mean()))
    assert not _agrees(z), "the check has no power"


# ---- c. every way of rendering gives the same bits ---------------------------------------------------------------------------------------------

W, H = 96, 40            # 3 840 pixels = 60 whole 8 x 8 tiles: both pixel orders apply
FRAMES, PASSES = 3, 10   # as tests/test_gpu_queue_budget.py: 10 passes are no multiple of R = 4
BUDGETS = (4, 24, 1)
# Kernel nodes of a slot's pass graph for the fixture at pathLength 4, SCAN pipeline, R > 1 (no thin level; TRANSMIT and the medium rule
# the tail kernel out), from frame_levels: generate, the primary launch, then per bounce medium_scatter + material + closest-hit +
# medium_shadow + any-hit, and the feature launch beside the bounce-1 material launch: 2 + 4 x 5 + 1.
GRAPH_NODES = 2 + 4 * 5 + 1
# The parallel shape's widest fan-out, from the medium's levels: the material launch (and the feature launch beside it) is waited for by
# the closest-hit launch and by medium_shadow — the any-hit launch waits for medium_shadow alone, so it is not a third — and
# medium_scatter at bounce 1 by the material and the feature launch: 2, as the zoo's.
PARALLEL_FAN_OUT = 2


def _chained(R, budget):
    return R > 1 and 2 * R + 1 > budget


def _render(gpu_ctx_factory, features=FS.ALL_ON, frames=FRAMES, passes=PASSES, order=pod.ORDER_ROWS, entry=True, in_flight=1, budget=None, pixel_map=None, stats=False, timing=None,
            compact=pod.COMPACT_FAST, want_graph=None):
    """(accumulation, rgba8) in row order, and the flavor word of the last pass"""
    ctx = gpu_ctx_factory(W, H)
    FS.all_features_scene(W, H, features).upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, compact, pod.CONDUCTOR_EXTENDED)
    ctx.set_pixel_order(order)
    if pixel_map is not None:
        ctx.set_pixel_map(pixel_map)
    ctx.set_entry_points(entry)
    ctx.enable_trace_stats(stats)
    if timing is not None:
        ctx.enable_kernel_timing(True, **timing)
    ctx.set_frames_per_pass(frames)
    ctx.set_passes_in_flight(in_flight)
    if budget is not None:
        ctx.set_queue_budget(budget)
        assert ctx.queue_budget()[:2] == (budget, _chained(in_flight, budget))
    ctx.reset_frame_number()
    for _ in range(passes):
        ctx.render_frame()
        ctx.accumulate()
    ctx.sync()
    acc, rgba8, flavor = ctx.read_accumulation(), ctx.read_rgba8(), ctx.debug_pass_flavor()
    if want_graph is not None:
        nodes, edges, fan_out = ctx.debug_last_graph()
        assert nodes == GRAPH_NODES, (in_flight, budget, nodes)
        if want_graph == "chain":
            assert (edges, fan_out) == (nodes - 1, 1), "not a chain: %s" % ((in_flight, budget, nodes, edges, fan_out),)
        else:
            assert fan_out == PARALLEL_FAN_OUT and edges > nodes - 1, "not the parallel graph: %s" % ((in_flight, budget, nodes, edges, fan_out),)
    ctx.close()
    if order == pod.ORDER_TILES:  # back to rows
        pm = capi.tile_pixel_map(W, H, 1, 0, 1, tiled=True)
        rows = [np.zeros_like(acc), np.zeros_like(rgba8)]
        rows[0][pm], rows[1][pm] = acc, rgba8
        acc, rgba8 = rows
    return acc, rgba8, flavor


def _same(got, want, what):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "accumulation differs: %s" % (what,)
    assert np.array_equal(got[1], want[1]), "rgba8 differs: %s" % (what,)


@pytest.fixture(scope="module")
def fixture_image(gpu_ctx_factory):
    """one pass at a time, 10 passes of 3 frames, every feature on"""
    got = _render(gpu_ctx_factory)
    print("the fixture's flavor word: %#x" % got[2])
    assert got[2] & EVERYTHING == EVERYTHING and got[2] & FLAVOR_LIGHT_POWER and got[2] & FLAVOR_AOV and got[2] & FLAVOR_ENTRY and got[2] & FLAVOR_ENV_MAP
    assert np.all(np.isfinite(got[0])) and got[0].max() > 0.1
    return got


@pytest.fixture(scope="module")
def fixture_image_64(gpu_ctx_factory):
    """64 passes of one frame"""
    return _render(gpu_ctx_factory, frames=1, passes=64)


@pytest.mark.parametrize("frames", [4, 64])
def test_frames_per_pass(gpu_ctx_factory, fixture_image_64, frames):
    _same(_render(gpu_ctx_factory, frames=frames, passes=64 // frames), fixture_image_64, "%d frames per pass" % frames)


VARIANTS = {
    "pixel order tiles": dict(order=pod.ORDER_TILES),
    "pixel order tiles, root": dict(order=pod.ORDER_TILES, entry=False),
    "entry points off": dict(entry=False),
    "trace statistics": dict(stats=True),
    "kernel timing, eager": dict(timing=dict()),
    "kernel timing, in the graph": dict(timing=dict(in_graph=True)),
    "kernel timing, last replay only": dict(timing=dict(in_graph=True, last_replay_only=True)),
}


@pytest.mark.parametrize("what", list(VARIANTS))
def test_every_way_of_rendering_gives_the_same_bits(gpu_ctx_factory, fixture_image, what):
    got = _render(gpu_ctx_factory, **VARIANTS[what])
    _same(got, fixture_image, what)
    assert got[2] & EVERYTHING == EVERYTHING


def test_a_two_way_pixel_split_equals_the_full_frame(gpu_ctx_factory, fixture_image):
    rows = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    for part in (rows[0::2].reshape(-1), rows[1::2].reshape(-1)):
        _same(_render(gpu_ctx_factory, pixel_map=part), (fixture_image[0][part], fixture_image[1][part]), "pixel split")


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("R", [2, 4])
def test_passes_in_flight_under_every_queue_budget(gpu_ctx_factory, fixture_image, R, budget):
    got = _render(gpu_ctx_factory, in_flight=R, budget=budget, want_graph="chain" if _chained(R, budget) else "parallel")
    _same(got, fixture_image, (R, budget))


def test_the_feature_buffers_change_no_radiance_bit(gpu_ctx_factory, fixture_image):
    got = _render(gpu_ctx_factory, features=FS.ALL_ON - {"aov"})
    assert got[2] == fixture_image[2] & ~FLAVOR_AOV
    _same(got, fixture_image, "AOV off")


def test_classic_pipeline_equals_scan_without_the_medium(gpu_ctx_factory):
    """(the classic pipeline refuses a medium: with every other feature on)"""
    features = FS.ALL_ON - {"medium", "grid"}
    scan = _render(gpu_ctx_factory, features=features)
    classic = _render(gpu_ctx_factory, features=features, compact=pod.COMPACT_ORDERED)
    assert scan[2] & 1 and not classic[2] & 1, "kFlavorScan"
    assert not scan[2] & capi.FLAVOR_MEDIUM and scan[2] & (EVERYTHING & ~(capi.FLAVOR_MEDIUM | capi.FLAVOR_MEDIUM_GRID)) == EVERYTHING & ~(capi.FLAVOR_MEDIUM | capi.FLAVOR_MEDIUM_GRID)
    _same(classic, scan, "classic against SCAN")


# ---- d. one live context through many flavors -----------------------------------------------------------------------------------------------

# one feature toggled per step (a Gray-code walk); the grid only ever beside the medium, whose bit it needs
WALK = ["+analytic", "+transmit", "+detail", "+medium", "+grid", "+power", "+aov", "+entry", "+env", "-analytic", "-detail", "-grid", "-transmit", "-power"]


def _subsets():
    out, now = [frozenset()], set()
    for step in WALK:
        (now.add if step[0] == "+" else now.discard)(step[1:])
        out.append(frozenset(now))
    return out


def _two_passes(ctx):
    ctx.reset_frame_number()
    for _ in range(2):
        ctx.render_frame()
        ctx.accumulate()
    ctx.sync()
    return ctx.read_accumulation(), ctx.debug_pass_flavor()


_FRESH = {}


def _fresh(gpu_ctx_factory, features):
    """a fresh context given the subset from the start, one pass at a time: (accumulation, flavor) — made once per subset"""
    if features not in _FRESH:
        ctx = gpu_ctx_factory(W, H)
        FS.all_features_scene(W, H, features).upload(ctx)
        ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
        ctx.set_frames_per_pass(2)
        _FRESH[features] = _two_passes(ctx)
        ctx.close()
    return _FRESH[features]


def _toggle(ctx, scene, feature, on):
    """the setter of one feature, on the live context"""
    if feature == "analytic":
        ctx.set_analytic_lights(FS.LIGHTS if on else np.zeros(0, pod.ALIGHT_DT))
    elif feature == "transmit":
        ctx.set_shadow_transmittance(pod.SHADOWS_TRANSMIT if on else pod.SHADOWS_OPAQUE)
    elif feature == "detail":
        ctx.set_material_detail(scene.detail_table if on else [])
    elif feature == "medium":
        ctx.set_medium(FS.FOG if on else None)
    elif feature == "grid":
        ctx.set_medium_density(FS.fog_grid() if on else None)
    elif feature == "power":
        ctx.set_light_sampling(pod.LIGHTS_POWER if on else pod.LIGHTS_UNIFORM)
    elif feature == "aov":
        ctx.set_aov(on)
    elif feature == "entry":
        ctx.set_entry_points(on)
    else:
        assert feature == "env" and on, "the environment is removed by a new upload only"
        ctx.upload_env_float(FS.environment())
        ctx.set_env_sampling(True)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_one_live_context_through_many_flavors(gpu_ctx_factory, in_flight):
    subsets = _subsets()
    assert len(set(subsets)) == len(subsets) >= 12
    ctx = gpu_ctx_factory(W, H)
    scene = FS.all_features_scene(W, H, subsets[0])
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    ctx.set_frames_per_pass(2)
    ctx.set_passes_in_flight(in_flight)
    flavors, first = [], None
    for k, features in enumerate(subsets):
        if k:
            step = WALK[k - 1]
            ctx.reset_frame_number()  # (the feature buffers are switched between images only: colour and features cover the same frames)
            _toggle(ctx, scene, step[1:], step[0] == "+")
        acc, flavor = _two_passes(ctx)
        want, want_flavor = _fresh(gpu_ctx_factory, features)
        # (the thin level belongs to one pass at a time: the one bit a context with passes in flight does not share with the fresh one)
        assert flavor | 16 == want_flavor | 16, "step %d (%s): flavor %#x, a fresh context's %#x" % (k, sorted(features), flavor, want_flavor)
        assert np.array_equal(acc.view(np.uint32), want.view(np.uint32)), "step %d: %s" % (k, sorted(features))
        flavors.append(flavor)
        first = acc if first is None else first
        assert ctx.queue_budget()[2] <= MAX_GRAPH_INSTANCES
    print("flavor words of the walk:", ["%#x" % f for f in flavors])
    assert len(set(flavors)) == len(subsets) > MAX_GRAPH_INSTANCES, "every subset has a flavor word of its own"
    # the cache is full — more instances were built than it holds, so the oldest were evicted
    assert ctx.queue_budget()[2] == MAX_GRAPH_INSTANCES
    # the first subset again, whose graph was evicted: everything off, the environment removed by a new upload
    ctx.reset_frame_number()
    scene.upload(ctx)
    again, flavor = _two_passes(ctx)
    assert flavor == flavors[0] and np.array_equal(again.view(np.uint32), first.view(np.uint32)), "the revisit"
    assert ctx.queue_budget()[2] == MAX_GRAPH_INSTANCES
    ctx.close()
