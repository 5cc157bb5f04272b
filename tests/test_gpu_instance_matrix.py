"""Every compiled kernel instance on the device (tests/instance_matrix_reference.py's case tables; tests/test_instance_ledger.py holds the
tables to the units' lists).  Every case asks nxhip_debug_pass_instances whether its pass launched exactly the set it is named for.

 a. the SCAN material launch, one case per set: block means against the float64 expectation with the bars of tests/test_physics_pins.py
    (max |z| < 4.5, mean z^2 < 1.6) once every kept block is under 2 % relative standard error, and the expectations of the case's
    neighbours refused by the same frames;
 b. the same cases under a pixel map cut at 1999 | 2097 (no multiple of a wave), the NO_MAPS instances against their general forms, and
    the three sampling modes against each other: equal bits, or bits that must differ;
 c. the medium's scatter kernel, one case per set and form;
 d. the families that promise equal bits: every tail set against the level-by-level graph, every classic set against SCAN, every trace set
    over the four switches of a context.

The oracle knows none of these features; nothing here compares with it."""
import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import feature_product_reference as F
from tests import instance_matrix_reference as M
from tests import test_physics_pins as PP

pytestmark = pytest.mark.gpu

SCAN = (pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
CLASSIC = (pod.RNG_PIXEL_KEYED, pod.COMPACT_ORDERED, pod.CONDUCTOR_EXTENDED)
PER_PASS, MAX_FRAMES = 64, 4096  # (the cap of test_gpu_metalrough.test_glossy_floor_transport)
SE_BAR = 0.02                    # the largest relative standard error of a kept block: what test_gpu_medium._pin demands
W, H = M.W, M.H


def _agrees(z):
    return np.abs(z).max() < 4.5 and (z * z).mean() < 1.6


def _upload(gpu_ctx_factory, sc, analytic, modes=SCAN, lights=None):
    ctx = gpu_ctx_factory(W, H)
    sc.upload(ctx)
    if analytic:
        ctx.set_analytic_lights(F.light_array() if lights is None else lights)
    ctx.set_modes(*modes)
    return ctx


# ---- a. the material launch against float64 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(M.SCAN_CASES), ids=M.scan_id)
def test_material_launch_against_float64(gpu_ctx_factory, key):
    """Measured on an MI355X (printed by the test; profiles/instance_matrix.txt holds every case's line): every one of the 28 cases is under
    the 2 % bar after 128 frames (largest relative standard error of a kept block 0.20 % .. 0.97 %); max |z| between 1.49 and 2.49, mean z^2
    between 0.39 and 0.83 over 14 to 16 blocks x 3 channels.  The neighbours' mean z^2: without the analytic lights 19 158 .. 65 862, with the
    geometric normal 1 762 .. 133 163, Lambert in place of GGX 3 060 .. 120 260, the floor as BLEND 1 972 .. 25 642, the pane as BLEND
    2 866 .. 2 873: all refused.  The allowance is the reference's own residue (instance_matrix_reference.systematic: 0.07 % .. 0.14 %)."""
    case = M.SCAN_CASES[key]
    family, analytic = case["family"], case["analytic"]
    kept, want, systematic = M.kept(family, analytic), M.expectation(family, analytic), M.systematic(family, analytic)
    ctx = _upload(gpu_ctx_factory, M.scene(family, case["sampling"]), analytic)
    ctx.set_frames_per_pass(PER_PASS)
    ctx.reset_frame_number()
    e = PP._Estimate(W, H)
    while True:
        ctx.render_frame()
        r = ctx.read_radiance().reshape(PER_PASS, W * H, 3)
        inst = ctx.debug_pass_instances()
        assert inst["scan"] == key, "the pass launched the material set %s, the case is %s" % (M.set_name(inst["scan"]), M.set_name(key))
        assert inst["tail"] is None and inst["medium"] is None and inst["logic"] is None and inst["any_hit"] == M.tf("AnyHit", "Transmit", *(("AlphaTest",) if family == "solid" else ()))
        for k in range(PER_PASS):
            e.add(r[k])
        rel = (e.se / want)[kept].max()
        if (e.n >= 2 * PER_PASS and rel <= SE_BAR) or e.n >= MAX_FRAMES:
            break
    ctx.close()
    z = PP._z(e.mean, e.se, want, 0.0, systematic=systematic)[kept]
    near = {what: PP._z(e.mean, e.se, v, 0.0, systematic=systematic)[kept] for what, v in M.neighbours(family, analytic).items()}
    print("%-32s %4d frames, %2d blocks, relative standard error max %.4f, max |z| %.2f, mean z^2 %.2f; neighbours' mean z^2: %s" %
          (M.scan_id(key), e.n, kept.sum(), rel, np.abs(z).max(), (z * z).mean(), ", ".join("%s %.0f" % (w, (v * v).mean()) for w, v in near.items()) or "none"))
    assert rel <= SE_BAR, "%d frames do not bring the kept blocks under the 2 %% bar" % e.n
    assert np.all(np.isfinite(e.mean))
    PP._assert_agree(z, M.scan_id(key))
    for what, v in near.items():
        assert not _agrees(v), "the check has no power: " + what


# ---- b. equal bits, and bits that must differ --------------------------------------------------------------------------------------------------------

CUT = 1999  # | 2097: neither part is a multiple of a wave
_FULL = {}


def _two_passes(ctx):
    ctx.reset_frame_number()
    for _ in range(2):
        ctx.render_frame()
        ctx.accumulate()
    ctx.sync()
    return ctx.read_accumulation().copy()


def _full_frame(gpu_ctx_factory, key):
    """the case's scene, two passes of two frames: the accumulation's bits — made once per case"""
    if key not in _FULL:
        case = M.SCAN_CASES[key]
        ctx = _upload(gpu_ctx_factory, M.scene(case["family"], case["sampling"]), case["analytic"])
        ctx.set_frames_per_pass(2)
        _FULL[key] = _two_passes(ctx)
        assert ctx.debug_pass_instances()["scan"] == key
        ctx.close()
        assert np.all(np.isfinite(_FULL[key])) and _FULL[key].max() > 0
    return _FULL[key]


@pytest.mark.parametrize("key", sorted(M.SCAN_CASES), ids=M.scan_id)
def test_material_launch_under_a_pixel_map(gpu_ctx_factory, key):
    case = M.SCAN_CASES[key]
    full = _full_frame(gpu_ctx_factory, key)
    pixels = np.arange(W * H, dtype=np.uint32)
    for part in (pixels[:CUT], pixels[CUT:]):
        assert len(part) % 64
        ctx = _upload(gpu_ctx_factory, M.scene(case["family"], case["sampling"]), case["analytic"])
        ctx.set_pixel_map(part)
        ctx.set_frames_per_pass(2)
        got = _two_passes(ctx)
        assert ctx.debug_pass_instances()["scan"] == key
        ctx.close()
        assert np.array_equal(got.view(np.uint32), full[part].view(np.uint32)), "%d pixels from %d on" % (len(part), part[0])
    if case["family"] == "no_maps":
        # the map-free instance against its general form (nexus_hip.h promises equal bits)
        ctx = _upload(gpu_ctx_factory, M.scene(case["family"], case["sampling"]), case["analytic"])
        ctx.debug_pass_flavor(force_general=capi.FLAVOR_NO_MAPS)
        ctx.set_frames_per_pass(2)
        got = _two_passes(ctx)
        assert ctx.debug_pass_instances()["scan"] == key & ~M.mf("NoMaps") and not ctx.debug_pass_flavor() & capi.FLAVOR_NO_MAPS
        ctx.close()
        assert np.array_equal(got.view(np.uint32), full.view(np.uint32)), "NO_MAPS against the general instance"


@pytest.mark.parametrize("family", list(M.FAMILY))
@pytest.mark.parametrize("analytic", [False, True], ids=["mesh", "analytic"])
def test_the_sampling_modes_render_different_frames(gpu_ctx_factory, family, analytic):
    """the sampling mode changes no expectation, so the float64 comparison cannot tell the modes apart: the frames' bits must"""
    keys = [k for k, c in M.SCAN_CASES.items() if c["family"] == family and c["analytic"] == analytic]
    assert len(keys) == (2 if family == "no_maps" else 3)
    frames = [_full_frame(gpu_ctx_factory, k) for k in keys]
    for a in range(len(keys)):
        for b in range(a + 1, len(keys)):
            assert not np.array_equal(frames[a], frames[b]), (M.scan_id(keys[a]), M.scan_id(keys[b]))


# ---- c. the medium -----------------------------------------------------------------------------------------------------------------------------------

MEDIUM_PARAMS = [(key, grid) for key in sorted(M.MEDIUM_CASES) for grid in (False, True)]


def medium_id(param):
    return "medium-%s-%s" % (M.set_name(param[0]), "grid" if param[1] else "homogeneous")


@pytest.mark.parametrize("param", MEDIUM_PARAMS, ids=medium_id)
def test_medium_against_float64(gpu_ctx_factory, param):
    """Measured on an MI355X (printed by the test; profiles/instance_matrix.txt holds every case's line): all 24 cases under the 2 % bar
    after 128 frames (largest relative standard error of a block 0.69 % .. 1.77 %, the grid forms the noisier), all 16 blocks kept; max |z|
    between 1.39 and 2.39, mean z^2 between 0.32 and 1.23.  The neighbours' mean z^2: without the lamp 4 613 .. 143 311, g = 0 in place of
    0.5 818 .. 4 529, without the point light 1 657 .. 9 642: all refused.  The allowance is the quadrature's residue (0.41 % homogeneous,
    0.66 % grid)."""
    key, grid = param
    case = M.MEDIUM_CASES[key]
    want, near = M.fog_expectation(case["metal"], case["analytic"], grid), M.fog_neighbours(case["metal"], case["analytic"], grid)
    kept = M.fog_kept(case["metal"], case["analytic"], grid)
    systematic = M.fog_systematic(case["metal"], grid)
    ctx = _upload(gpu_ctx_factory, M.fog_scene(case["metal"], case["sampling"], grid), case["analytic"], lights=np.array([M.FOG_POINT], dtype=pod.ALIGHT_DT))
    ctx.set_frames_per_pass(PER_PASS)
    ctx.reset_frame_number()
    e = PP._Estimate(W, H)
    while True:
        ctx.render_frame()
        r = ctx.read_radiance().reshape(PER_PASS, W * H, 3)
        inst = ctx.debug_pass_instances()
        assert (inst["medium"], inst["medium_grid"]) == (key, grid), "the pass launched the medium set %s (grid %s), the case is %s" % (M.set_name(inst["medium"]), inst["medium_grid"], medium_id(param))
        assert inst["tail"] is None and inst["scan"] is not None
        for k in range(PER_PASS):
            e.add(r[k])
        rel = (e.se / want)[kept].max()
        if (e.n >= 2 * PER_PASS and rel <= SE_BAR) or e.n >= MAX_FRAMES:
            break
    ctx.close()
    z = PP._z(e.mean, e.se, want, 0.0, systematic=systematic)[kept]
    zs = {what: PP._z(e.mean, e.se, v, 0.0, systematic=systematic)[kept] for what, v in near.items()}
    print("%-52s %4d frames, %2d blocks, relative standard error max %.4f, max |z| %.2f, mean z^2 %.2f; neighbours' mean z^2: %s" %
          (medium_id(param), e.n, kept.sum(), rel, np.abs(z).max(), (z * z).mean(), ", ".join("%s %.0f" % (w, (v * v).mean()) for w, v in zs.items())))
    assert rel <= SE_BAR, "%d frames do not bring the kept blocks under the 2 %% bar" % e.n
    assert np.all(np.isfinite(e.mean))
    PP._assert_agree(z, medium_id(param))
    for what, v in zs.items():
        assert not _agrees(v), "the check has no power: " + what


# ---- d. the families that promise equal bits ---------------------------------------------------------------------------------------------------------

LONG = 4  # path length of the frames-against-frames cases
_LONG = {}


def _long_frames(gpu_ctx_factory, family, sampling, analytic, modes=SCAN, transmit=True, tail=0, want=None):
    """three one-frame passes of the case's scene at a path length of 4: (radiance of every pass, instances of the last pass, its flavor)"""
    sc = M.scene(family, sampling, path_length=LONG)
    sc.shadow_transmittance = pod.SHADOWS_TRANSMIT if transmit else pod.SHADOWS_OPAQUE
    ctx = _upload(gpu_ctx_factory, sc, analytic, modes=modes)
    ctx.set_tail_bounce(tail)
    ctx.reset_frame_number()
    out = []
    for _ in range(3):
        ctx.render_frame()
        out.append(ctx.read_radiance().copy())
    inst, flavor = ctx.debug_pass_instances(), ctx.debug_pass_flavor()
    ctx.close()
    out = np.stack(out)
    assert np.all(np.isfinite(out)) and out.max() > 0
    return out, inst, flavor


def _level_by_level(gpu_ctx_factory, family, sampling, analytic, transmit):
    key = (family, sampling, analytic, transmit)
    if key not in _LONG:
        _LONG[key] = _long_frames(gpu_ctx_factory, family, sampling, analytic, transmit=transmit)
    return _LONG[key]


@pytest.mark.parametrize("key", sorted(M.TAIL_CASES), ids=lambda k: "tail-" + M.set_name(k))
def test_tail_kernel_equals_the_level_by_level_graph(gpu_ctx_factory, key):
    """(no tail kernel under TRANSMIT over a see-through pane: the shadow rays of these passes take the pane as opaque)"""
    case = M.TAIL_CASES[key]
    level, inst0, _ = _level_by_level(gpu_ctx_factory, case["family"], case["sampling"], case["analytic"], False)
    assert inst0["tail"] is None and inst0["tail_bounce"] is None and inst0["scan"] == key
    tail, inst, _ = _long_frames(gpu_ctx_factory, case["family"], case["sampling"], case["analytic"], transmit=False, tail=2)
    assert (inst["tail"], inst["tail_bounce"]) == (key, 2), "the pass launched the tail set %s from bounce %s" % (inst["tail"], inst["tail_bounce"])
    assert np.array_equal(tail.view(np.uint32), level.view(np.uint32))


@pytest.mark.parametrize("key", sorted(M.CLASSIC_CASES), ids=lambda k: "classic-%s-%s" % ("fifth" if k[0] else "reference", M.set_name(k[1])))
def test_classic_pipeline_equals_scan(gpu_ctx_factory, key):
    """COMPACT_ORDERED against SCAN without medium and tree (test_gpu_feature_products.test_classic_pipeline_equals_scan_without_the_medium).
    The report has no word for the classic material kernels: the flavor word and the scene's material types say which were launched."""
    metal_type, set_ = key
    case = M.CLASSIC_CASES[key]
    scan, inst0, flavor0 = _level_by_level(gpu_ctx_factory, case["family"], case["sampling"], case["analytic"], True)
    assert flavor0 & 1 and inst0["logic"] is None and inst0["scan"] is not None
    classic, inst, flavor = _long_frames(gpu_ctx_factory, case["family"], case["sampling"], case["analytic"], modes=CLASSIC)
    assert not flavor & 1 and inst["scan"] is None and inst["tail"] is None and inst["logic"] == 0, "kFlavorScan clear, the two-item logic kernel"
    # the set of the case from the flavor's facts, as nx_variants.h names them
    facts = M.mf(*(("Power",) if flavor & 128 else ()), *(("Analytic",) if flavor & capi.FLAVOR_ANALYTIC else ()), *(("Detail",) if flavor & (capi.FLAVOR_DETAIL | capi.FLAVOR_SOLID) or metal_type else ()),
                 *(("Solid",) if flavor & capi.FLAVOR_SOLID else ()))
    assert facts == set_ and bool(flavor & capi.FLAVOR_METAL) == (case["family"] in ("metal", "solid")), "flavor %#x" % flavor
    assert inst["any_hit"] == inst0["any_hit"] and inst["closest"] == inst0["closest"] and inst["primary"] == inst0["primary"]
    assert np.array_equal(classic.view(np.uint32), scan.view(np.uint32))


TRACE_GROUPS = [(mask, transmit) for mask in (False, True) for transmit in (False, True)]
_TRACE_SEEN = {}


@pytest.mark.parametrize("mask,transmit", TRACE_GROUPS, ids=lambda v: str(v))
def test_trace_instances_within_a_group_render_equal_bits(gpu_ctx_factory, mask, transmit):
    """entry points, trace statistics and the IDENTITY instances change no bit (nexus_hip.h); TRANSMIT and the MASK table change the image,
    so they span the four groups"""
    base = None
    for stats in (False, True):
        for entry in (False, True):
            for general in (True, False):
                sc = M.scene("solid" if mask else "metal", "table", path_length=LONG)
                sc.shadow_transmittance = pod.SHADOWS_TRANSMIT if transmit else pod.SHADOWS_OPAQUE
                ctx = _upload(gpu_ctx_factory, sc, True)
                ctx.set_tail_bounce(0)
                ctx.set_entry_points(entry)
                ctx.enable_trace_stats(stats)
                if general:
                    ctx.debug_pass_flavor(force_general=capi.FLAVOR_IDENTITY)
                ctx.reset_frame_number()
                frames = []
                for _ in range(2):
                    ctx.render_frame()
                    frames.append(ctx.read_radiance().copy())
                inst = ctx.debug_pass_instances()
                ctx.close()
                frames = np.stack(frames)
                switches = dict(mask=mask, transmit=transmit, stats=stats, entry=entry, general=general)
                for word in ("primary", "closest", "any_hit"):
                    _TRACE_SEEN.setdefault(inst[word], []).append(dict(word=word, **switches))
                    want = M.TRACE_CASES[inst[word]]
                    if all(want[k] == v for k, v in switches.items()) and want["word"] == word:
                        print("trace set %-36s launched as the %s launch under %s" % (M.set_name(inst[word], "kTf"), word, switches))
                if base is None:
                    base = frames
                    assert np.all(np.isfinite(base)) and base.max() > 0
                assert np.array_equal(frames.view(np.uint32), base.view(np.uint32)), switches


def test_every_trace_set_was_launched_where_its_case_says(gpu_ctx_factory):
    for group in TRACE_GROUPS:  # (run alone, this test renders the groups itself)
        if not any(s["mask"] == group[0] and s["transmit"] == group[1] for seen in _TRACE_SEEN.values() for s in seen):
            test_trace_instances_within_a_group_render_equal_bits(gpu_ctx_factory, *group)
    assert set(_TRACE_SEEN) == set(M.TRACE_CASES), "launched and not a case: %s; a case and not launched: %s" % (sorted(set(_TRACE_SEEN) - set(M.TRACE_CASES)), sorted(set(M.TRACE_CASES) - set(_TRACE_SEEN)))
    for set_, case in M.TRACE_CASES.items():
        assert case in _TRACE_SEEN[set_], "trace set %s: not launched as %s" % (M.set_name(set_, "kTf"), case)
