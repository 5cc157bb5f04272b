"""The traversal stack beyond its LDS part: every kernel that walks the BVH8 keeps 32 entries per ray, the first kLdsDepth (8) in
LDS and the rest in a scratch array (nx_traverse.h), and the stack travels — to the thin kernel with a handed-over ray, into the
primary launch with an entry state.  The host builders' trees never fill more than five entries at test size, so the trees here are
made by hand (tests/bvh_craft.py): chains that take every ray going down to exactly the named depth, alone and under chains of
instances.  tests/test_bvh_craft.py proves the depths on the CPU; every test here asserts its depth classes from the oracle again
before it compares anything, and prints them.  All comparisons are bit for bit against the oracle."""
import numpy as np
import pytest

from nexus_amd import capi, multigpu, pod
from tests import bvh_craft as BC
from tests import oracle_lib as O
from tests import scene_helpers as SH
from tests.test_tlas_refit import _check_tlas_structure

pytestmark = pytest.mark.gpu

HAND_OVER_AFTER = (1, 2, 5, 9, 10, 17, 33, 40)


def _oracle_batch(scene, rays):
    """closest-hit records, any-hit limits and results, per-ray stack depths and visit counts of one batch"""
    orc = scene.oracle()
    st, st_any = O.TraceStats(), O.TraceStats()
    want = orc.trace_closest(rays, st)
    tmax = BC.shadow_tmax(want, seed=len(rays))
    want_any = orc.trace_any(rays, tmax, st_any)
    return dict(closest=want, tmax=tmax, any=want_any, depth=BC.per_ray_stack(orc, rays), counts=st.as_dict(), counts_any=st_any.as_dict())


def _trace_and_count(ctx, rays, tmax):
    """the batch through the product's kernels, then once more through their counting variants: records, any-hit results, visit counts"""
    got, got_any = ctx.trace_batch(rays), ctx.trace_shadow_batch(rays, tmax)
    ctx.enable_trace_stats(True)
    ctx.read_trace_stats(reset=True)
    counted, counted_any = ctx.trace_batch(rays), ctx.trace_shadow_batch(rays, tmax)
    closest, shadow = ctx.read_trace_stats(reset=True)
    ctx.enable_trace_stats(False)
    return got, got_any, counted, counted_any, closest, shadow


def _same_as_oracle(ctx, rays, ref, what):
    got, got_any, counted, counted_any, closest, shadow = _trace_and_count(ctx, rays, ref["tmax"])
    assert SH.hit_records_equal(got, ref["closest"]), "%s: closest-hit records differ from the oracle's" % what
    assert np.array_equal(got_any, ref["any"]), "%s: any-hit results differ from the oracle's" % what
    assert SH.hit_records_equal(counted, ref["closest"]) and np.array_equal(counted_any, ref["any"]), "%s: the counting kernels' results" % what
    assert closest["rays"] == len(rays) and shadow["rays"] == len(rays)
    for k in ("nodes", "tris", "instances"):
        assert closest[k] == ref["counts"][k], "%s: closest-hit %s visited" % (what, k)
        assert shadow[k] == ref["counts_any"][k], "%s: any-hit %s visited" % (what, k)


@pytest.mark.parametrize("D", BC.CHAIN_LEVELS)
def test_trace_kernels_with_stacks_of_7_to_32_entries(gpu_ctx_factory, D):
    """1. One chain of D levels under an identity instance: depths 7 (the last LDS entry), 8 (the first spilled one), 9, 16, 31 and
    32 (the last entry there is).  Deep rays, shallow rays and rays that miss the root share every wave."""
    scene, rays = BC.chain_case(D)
    ref = _oracle_batch(scene, rays)
    depth, want = ref["depth"], ref["closest"]
    deep = depth == D - 1
    popped_far = deep & (want["triIdx"] >= 8) & (want["triIdx"] < D - 1)  # level i's stub is the entry at stack position i
    print("D = %d: %.3f of the rays at depth %d, %.3f at depth <= 1; %.3f of the deep rays end on a triangle popped from position >= 8; any-hit limits: "
          "%.3f at 10" % (D, deep.mean(), D - 1, (depth <= 1).mean(), popped_far.sum() / deep.sum(), (ref["tmax"] == 10.0).mean()))
    assert deep.mean() >= 0.3 and (depth <= 1).mean() >= 0.2 and depth.max() == D - 1
    assert D < 10 or popped_far.sum() >= 0.25 * deep.sum()
    assert (ref["tmax"][deep] == 10.0).mean() > 0.2 and (ref["tmax"][deep] < 10.0).mean() > 0.4
    ctx = gpu_ctx_factory(128, 128)  # (16 384 rays per launch: the batch takes two)
    scene.upload(ctx)
    _same_as_oracle(ctx, rays, ref, "chain of %d levels" % D)


@pytest.mark.parametrize("mixed", [False, True], ids=["identity", "mixed"])
@pytest.mark.parametrize("name", list(BC.TOWERS))
def test_instances_entered_deep_in_the_stack(gpu_ctx_factory, name, mixed):
    """2. A TLAS chain over BLAS chains: the top instance is entered with 7, 8, 9 or 20 entries on the stack (8: the TLAS leaf group
    itself is the first spilled entry), the instance of level i with i, and the BLASes take the ray on to 32 and 31 entries — so the
    instance exit `sp == instSp`, the parked world ray and its restore run with instSp on both sides of the LDS boundary.  identity:
    every placement is the identity (the scene-wide shortcut); mixed: every second one is rotated, tilted, scaled and shifted."""
    scene, rays = BC.tower_case(name, mixed)
    T, last, _D = BC.TOWERS[name]
    ref = _oracle_batch(scene, rays)
    depth = ref["depth"]
    hist = np.bincount(depth, minlength=33)
    print("%s (%d TLAS levels, %d instances in the last leaf), %s: rays at depth 32: %d, 31: %d, <= 2: %d of %d" % (
        name, T, last, "mixed" if mixed else "identity", hist[32], hist[31], hist[:3].sum(), len(rays)))
    assert depth.max() == 32 and hist[32] >= 0.3 * len(rays) and hist[:3].sum() >= 0.2 * len(rays)
    hit = ref["closest"]["triIdx"] != 0xffffffff
    assert len(np.unique(ref["closest"]["instanceIdx"][hit])) == len(scene.instances)
    ctx = gpu_ctx_factory(128, 128)
    scene.upload(ctx)
    _same_as_oracle(ctx, rays, ref, name)


def _hand_over_scenes():
    return [("chain of 33", BC.chain_case(33)), ("chain of 17", BC.chain_case(17)), ("twin triangles, chain of 20", BC.chain_case(20, per_level=2)),
            ("tower, instSp 8, mixed", BC.tower_case("instSp 8", True)), ("tower, instSp 20, identity", BC.tower_case("instSp 20", False))]


@pytest.mark.parametrize("which", range(5), ids=["chain33", "chain17", "twins20", "tower8mixed", "tower20identity"])
def test_rays_handed_to_the_thin_kernel_with_deep_stacks(gpu_ctx_factory, which):
    """3. The hand-over copies the stack (nx_trace.hip: `st->stack[k]`, LDS and scratch part) and the thin kernel's search is seeded from
    it; its in-order replay keeps a stack of its own in the wave's pool (STRIDE = 64).  Every ray still busy after k iterations is
    handed over, k = 1 ... 40: with sp = 0 ... 32.  Five of the scenes of cases 1 and 2, for the run time: the deepest chain, a middle
    one, one tower on each side of the LDS boundary that matters most (instSp 8 mixed: the first spilled entry is the instance's own;
    instSp 20 identity); the towers with instSp 7 and 9 are not handed over.
    What the oracle cannot tell is a ray's depth at the moment of the hand-over; stated instead: the share of the batch whose final
    depth is >= 9 — with k >= 9 only those are still busy — and, per k, how many rays of final depth >= 9 the oracle keeps busy for at least k + 2 steps
    (nodes + triangles: the device's iterations).  Any hit: a limit at the hit culls levels and ends two thirds of the rays early,
    so the any-hit condition rests on the third whose limit is 10: at least 2 000 rays busy that long in the oracle, at least 1 000
    handed over on the device (a wave counts its iterations from its last refill, so a ray may leave a few iterations late or retire
    first; half is the margin for that), for every k <= 17, closest hit and any hit alike.
    The twin-triangle chain has a second triangle at exactly every hit's distance, which by the thin kernel's own rule (r.second ==
    r.t) sends a continued ray that found a closer hit to the replay: that the replay runs with more than eight entries rests on this
    reading, the device reports no count of replays."""
    what, (scene, rays) = _hand_over_scenes()[which]
    ref = _oracle_batch(scene, rays)
    deep_share = (ref["depth"] >= 9).mean()
    assert deep_share >= 0.3 and ref["depth"].max() >= 16
    orc = scene.oracle()
    steps = BC.per_ray_stats(orc, rays)
    steps_any = BC.per_ray_stats(orc, rays, ref["tmax"])
    steps, steps_any, depth_any = steps["nodes"] + steps["tris"], steps_any["nodes"] + steps_any["tris"], steps_any["maxStack"]
    print("%s: any-hit rays with a final depth >= 9: %d of %d" % (what, (depth_any >= 9).sum(), len(rays)))
    assert (depth_any >= 9).sum() >= 2000
    ctx = gpu_ctx_factory(256, 256)  # (the whole batch in one launch: debug_thin_counts speaks of the last one)
    scene.upload(ctx)
    for k in HAND_OVER_AFTER:
        ctx.debug_set_thin(lanes=64, iters=k, in_hooks=True, any_time=True)
        got = ctx.trace_batch(rays)
        handed = ctx.debug_thin_counts()[0]
        got_any = ctx.trace_shadow_batch(rays, ref["tmax"])
        handed_any = ctx.debug_thin_counts()[1]
        print("%s, after %2d iterations: %5d closest-hit and %5d any-hit rays of %d handed over (final depth >= 9: %.3f of the batch, deepest %d)" % (
            what, k, handed, handed_any, len(rays), deep_share, ref["depth"].max()))
        assert SH.hit_records_equal(got, ref["closest"]), "%s: closest hit, handed over after %d iterations" % (what, k)
        assert np.array_equal(got_any, ref["any"]), "%s: any hit, handed over after %d iterations" % (what, k)
        busy, busy_any = int(((steps >= k + 2) & (ref["depth"] >= 9)).sum()), int(((steps_any >= k + 2) & (depth_any >= 9)).sum())
        print("    the oracle keeps %d closest-hit and %d any-hit rays of final depth >= 9 busy for %d steps or more" % (busy, busy_any, k + 2))
        if k <= 17:
            assert busy >= 2000 and busy_any >= 2000, "%s: too few long rays for k = %d" % (what, k)
            assert handed >= 1000, "%s: %d closest-hit rays handed over after %d iterations" % (what, handed, k)
            assert handed_any >= 1000, "%s: %d any-hit rays handed over after %d iterations" % (what, handed_any, k)
    # a pool kept small (seeds and children are put back and taken again), and the product's rule
    ctx.debug_set_thin_pool(96)
    for k in (9, 33):
        ctx.debug_set_thin(lanes=64, iters=k, in_hooks=True, any_time=True)
        assert SH.hit_records_equal(ctx.trace_batch(rays), ref["closest"]), "%s: small pool, k = %d" % (what, k)
        assert np.array_equal(ctx.trace_shadow_batch(rays, ref["tmax"]), ref["any"]), "%s: small pool, any hit, k = %d" % (what, k)
    ctx.debug_set_thin_pool(0)
    ctx.debug_set_thin(lanes=16, iters=16, in_hooks=True)
    assert SH.hit_records_equal(ctx.trace_batch(rays), ref["closest"]), "%s: the product's rule" % what
    print("%s, the product's rule (16 lanes, 16 iterations): %d rays handed over (only what a dry wave still holds: may be few)" % (what, ctx.debug_thin_counts()[0]))
    assert np.array_equal(ctx.trace_shadow_batch(rays, ref["tmax"]), ref["any"]), "%s: the product's rule, any hit" % what


FRAME_MODES = {"reference": (pod.RNG_REFERENCE_SLOT, pod.COMPACT_ORDERED, pod.CONDUCTOR_REFERENCE), "fast": (pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)}


def _oracle_frames(scene, pixel_map, modes, frames):
    """per frame 1 .. frames: radiance, accumulation, queue sizes; and the deepest stacks over all of them (closest hit, any hit)"""
    w = O.Wavefront(scene.oracle(), len(pixel_map), pixel_map, modes[0], modes[2])
    out = []
    for f in range(1, frames + 1):
        w.render(f, threads=4)
        w.accumulate(f)
        out.append((w.radiance().copy(), w.accumulation().copy(), w.queue_sizes()))
    closest, shadow = w.trace_stats()
    w.close()
    return out, closest["maxStack"], shadow["maxStack"]


def _frames_equal(ctx, want, passes, per_pass, what, queues=True):
    ctx.set_frames_per_pass(per_pass)
    ctx.reset_frame_number()
    for _ in range(passes):
        ctx.render_frame()
        ctx.accumulate()
    last = want[(passes - 1) * per_pass:passes * per_pass]
    assert SH.frames_identical(ctx.read_radiance(), np.concatenate([f[0] for f in last]), what), what
    assert np.array_equal(ctx.read_accumulation().view(np.uint32), last[-1][1].view(np.uint32)), what + ": accumulation"
    if queues:
        summed = {k: sum(f[2][k] for f in last) for k in SH.QUEUE_KEYS}
        assert SH.queue_sizes_identical(ctx.read_queue_sizes(), summed), what


@pytest.mark.parametrize("mixed", [False, True], ids=["identity", "mixed"])
@pytest.mark.parametrize("mode", list(FRAME_MODES))
def test_whole_frames_of_a_deep_scene(gpu_ctx_factory, mode, mixed):
    """4. The tower as a scene that renders (bvh_craft.frame_scene): camera above it, diffuse materials, the bottom instance a light,
    a lit background.  Primary rays, continuation rays and shadow rays of the pass graph, the tail kernel's traverse_wave, primary rays
    that start from an entry state, two passes in flight — every frame the oracle's.  (A chain instance turned by 180 degrees would NOT
    be deep for the rays that bounce up: the child order follows the octant of the world direction.  The scene has BLASes with the
    stub in the other slot instead.)
    What the depth condition shows: the closest-hit figure (32) is already reached by the primary rays.  The any-hit figure is the
    tail kernel's: every shadow ray of these frames belongs to bounce slot 2 or later (asserted below), which with set_tail_bounce(2)
    is traced by the tail kernel's traverse_wave, so its any-hit traversal does run to 32 entries there; how deep the continuation
    rays of the tail go (they start inside the tower and mostly go up, through 8-level BLASes) the oracle does not report per bounce.
    The tail setting takes effect in the pixel-keyed pair only; in the reference pair that block checks that it changes nothing."""
    W, H = 64, 48
    modes = FRAME_MODES[mode]
    scene = BC.frame_scene(W, H, mixed)
    # 8 x 8 pixel tiles: a run of 64 primary rays is then a compact bundle inside one octant, which is what an entry state needs (a
    # 64 x 1 row of this frame crosses x = 0 and starts at the root)
    pm = multigpu.tiled_order(np.arange(W * H, dtype=np.uint32), W)
    want, deepest, deepest_any = _oracle_frames(scene, pm, modes, 4)
    print("%s, %s: deepest stack over 4 frames: closest hit %d, any hit %d; trace queue sizes of frame 1 %s, shadow %s" % (
        mode, "mixed" if mixed else "identity", deepest, deepest_any, want[0][2]["traceSize"][:5].tolist(), want[0][2]["traceShadowSize"][:5].tolist()))
    assert deepest >= 24 and deepest_any >= 9
    assert all(f[2]["traceShadowSize"][:2].sum() == 0 and f[2]["traceShadowSize"][2:].sum() > 100 for f in want), "shadow rays from bounce slot 2 on only"
    assert want[0][2]["traceSize"][1] > 1000 and want[0][2]["traceShadowSize"].sum() > 100 and float(want[0][0].mean()) > 0.05
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(*modes)
    ctx.set_pixel_map(pm)
    ctx.set_tail_bounce(0)
    _frames_equal(ctx, want, 2, 1, "level by level")
    ctx.set_entry_points(True)
    _frames_equal(ctx, want, 2, 1, "entry points on")
    states = ctx.read_entry_states()
    assert len(states) == W * H // 64
    print("entry states: %d runs, node steps saved %s, stack entries carried %s" % (len(states), np.bincount(states[:, 19]).tolist(), np.bincount(states[:, 16]).tolist()))
    assert states[:, 16].max() <= 6, "an entry state has room for six entries"
    if not mixed:  # (the walk goes through identity instances only.  On a chain every node step pushes: four steps take the walk to
        #  kEntryMaxStack - 2 entries, where it must stop — one more step may push two)
        assert states[:, 19].max() >= 4 and 4 <= states[:, 16].max()
    # (slot-keyed random numbers depend on a path's queue slot, and a pass of several frames puts them all into one queue: only the
    #  pixel-keyed pipeline is the oracle's frame by frame when frames are batched)
    per_pass = 2 if modes[0] == pod.RNG_PIXEL_KEYED else 1
    ctx.set_passes_in_flight(2)
    _frames_equal(ctx, want, 2, per_pass, "entry points on, %d frames per pass, two passes in flight" % per_pass)
    ctx.set_entry_points(False)
    _frames_equal(ctx, want, 2, per_pass, "%d frames per pass, two passes in flight" % per_pass)
    ctx.set_passes_in_flight(1)
    ctx.set_tail_bounce(2)  # (takes effect with pixel-keyed random numbers and racing compaction; the other pipeline must not change)
    _frames_equal(ctx, want, 2, 1, "tail kernel from bounce 2", queues=False)
    ctx.set_entry_points(True)
    _frames_equal(ctx, want, 2, per_pass, "tail kernel from bounce 2, entry points on, %d frames per pass" % per_pass, queues=False)
    ctx.sync()


def test_device_refit_of_a_tlas_of_thirty_levels(gpu_ctx_factory):
    """5. nxhip_set_instance_transforms on a TLAS chain of 30 levels: the refit runs one launch per level of the tree, 30 here against
    the three or four of a built tree.  The refitted tree bounds the moved instances, equals the host refit byte for byte, and traces
    like the oracle on the nodes read back — with the stack still at 31."""
    T = 30
    scene = BC.tower_scene(T, [3] * T, 1, True, seed=5)
    rays = BC.mixed_rays(scene, 12000, seed=6, slope=0.01)
    ctx = gpu_ctx_factory(128, 128)
    scene.upload(ctx)
    assert SH.hit_records_equal(ctx.trace_batch(rays), scene.oracle().trace_closest(rays))
    rng = np.random.RandomState(8)
    ids = rng.permutation(T).astype(np.uint32)
    xfs = np.array([capi.mat4_from_trs((rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(-0.01, 0.01)), (rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(0, 360)),
                                       (rng.uniform(0.8, 1.0), rng.uniform(0.8, 1.0), 1.0)) for _ in ids], dtype=np.float32)
    ctx.set_instance_transforms(ids, xfs)
    moved = scene.instances.copy()
    for i, xf in zip(ids, xfs):
        moved[i] = capi.instance_init(int(scene.instances[i]["bvhIdx"]), int(scene.instances[i]["materialId"]), xf, scene.blas[int(scene.instances[i]["bvhIdx"])][0][0])
    got_nodes, got_inst = ctx.read_tlas(len(scene.tlas_nodes), T)
    assert got_inst.tobytes() == moved.tobytes()
    _check_tlas_structure(got_nodes, scene.tlas_idx, moved)
    for f in ("imask", "childBaseIdx", "triangleBaseIdx", "meta"):
        assert np.array_equal(got_nodes[f], scene.tlas_nodes[f]), f
    assert got_nodes.tobytes() == capi.tlas_refit(scene.tlas_nodes, scene.tlas_idx, moved).tobytes(), "device refit against the host refit"
    assert got_nodes.tobytes() != np.ascontiguousarray(scene.tlas_nodes).tobytes()
    after = scene.variant(instances=moved, tlas_nodes=got_nodes)
    orc = after.oracle()
    want = orc.trace_closest(rays)
    depth = BC.per_ray_stack(orc, rays)
    print("refitted TLAS of %d levels: %d of %d rays at depth %d, %.3f of the rays hit" % (T, (depth == depth.max()).sum(), len(rays), depth.max(), (want["hitDistance"] < 1e29).mean()))
    assert depth.max() == 31 and (depth == 31).mean() >= 0.3
    assert SH.hit_records_equal(ctx.trace_batch(rays), want)
    sub = slice(0, 2000)
    assert np.array_equal(want["hitDistance"][sub].view(np.uint32), orc.brute_closest(rays[sub])["hitDistance"].view(np.uint32))


@pytest.mark.parametrize("D", BC.LIMIT_LEVELS)
def test_pushes_beyond_the_32nd_entry_are_dropped_and_nothing_else_is(gpu_ctx_factory, D):
    """6. The limit.  A ray that needs more than 32 entries loses what it pushes from the 33rd on: stack_push writes nothing there,
    stack_pop returns an empty group (nx_traverse.h; every index is behind an `sp <` test, the hand-over's copy loop and the thin
    kernel's seed clamp sp to 32, an entry state carries six entries at most).  On a chain every level pushes on the way down, before
    the first triangle is tested, so the dropped entries are the stubs of levels 32 .. D - 2: the device's records for those rays are
    the oracle's on the same tree with those stubs' triangles made zero-area (bvh_craft.without_levels).  Rays of depth <= 32 in the
    same waves keep the oracle's records on the tree as it is: a dropped push touches no neighbour's LDS entry.  Any hit: a limit at
    the hit culls levels and shifts which level sits at which position, so the rays whose any-hit depth exceeds 32 get the limit 10,
    which culls nothing.  Read as well: deep stacks beyond 32 on the routes that are not run here.  The hand-over stores sp and instSp
    as they are and copies min(sp, 32) entries; the thin kernel's seed clamps sp to 32 and leaves instSp alone, and that is right:
    `lane < instSp` with instSp >= 32 puts all 32 kept entries into the TLAS frame, which is where the loop pushed them, the two
    current groups take the instance's frame from instSp >= 0, and the loop's own `sp == instSp` compares the unclamped counters (the
    pops between 32 and instSp return empty groups and the exit happens at the right count).  An entry state carries at most six
    entries.  No index or comparison needed a fix.  This pins the rule the code states, "dropped ... as in the reference" — it does not recommend it."""
    scene, rays = BC.limit_case(D)
    cut = BC.without_levels(scene, 32)
    orc, orc_cut = scene.oracle(), cut.oracle()
    depth = BC.per_ray_stack(orc, rays)
    full, lost = orc.trace_closest(rays), orc_cut.trace_closest(rays)
    over = depth > 32
    want = np.where(over, lost, full)
    differ = over & (full["triIdx"] != lost["triIdx"])
    print("D = %d: %d of %d rays need %d entries, %d of them lose their closest hit to the limit; %d rays at depth <= 1" % (D, over.sum(), len(rays), D - 1, differ.sum(), (depth <= 1).sum()))
    assert over.mean() >= 0.3 and np.all(depth[over] == D - 1) and differ.sum() >= 1000 and (depth <= 1).mean() >= 0.2
    tmax = BC.shadow_tmax(full, seed=D)
    tmax[BC.per_ray_stack(orc, rays, tmax) > 32] = 10.0
    any_depth = BC.per_ray_stack(orc, rays, tmax)
    assert np.all((any_depth <= 32) | (tmax == 10.0)) and np.all(any_depth[tmax == 10.0] == depth[tmax == 10.0])
    want_any = np.where(any_depth > 32, orc_cut.trace_any(rays, tmax), orc.trace_any(rays, tmax))
    differ_any = want_any != orc.trace_any(rays, tmax)
    print("any hit: %d rays over the limit, %d of them no longer occluded" % ((any_depth > 32).sum(), differ_any.sum()))
    assert differ_any.sum() >= 20
    ctx = gpu_ctx_factory(128, 128)
    scene.upload(ctx)
    got = ctx.trace_batch(rays)
    assert SH.hit_records_equal(got[~over], full[~over]), "rays within the limit"
    assert SH.hit_records_equal(got, want), "rays over the limit: the stubs of levels 32 .. %d are lost, nothing else" % (D - 2)
    assert np.array_equal(ctx.trace_shadow_batch(rays, tmax), want_any)
