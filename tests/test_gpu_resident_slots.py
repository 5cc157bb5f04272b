"""Resident slots (nxhip_resident_slots_for): of R passes in flight only as many are on the chip at once as the queue budget serves,
and the persistent trace launches are sized as the shares of that many slots.  The round robin still runs over all R slots, and R
stays the number of passes that may await their accumulate.  How many workgroups a trace launch has changes no sample, so every
image must equal the one rendered one pass at a time, bit for bit."""
import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

W, H = 96, 40            # the fixture of tests/test_gpu_queue_budget.py
FRAMES, PASSES = 3, 10   # 10 passes: no multiple of R = 3, 4 or 6
MAX_GRAPH_INSTANCES = 8  # kMaxGraphInstances (nxhip_render.hip)
BUDGETS = (1, 4, 6, 24)
ROOMY = 32               # a budget every R up to 8 fits (2 R + 1 <= 32): resident = R


@pytest.fixture(scope="module")
def zoo():
    return SH.material_zoo_scene(W, H, path_length=4)


def _prepare(ctx, scene, entry=True, order=pod.ORDER_ROWS, frames=FRAMES):
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    ctx.set_pixel_order(order)
    ctx.set_entry_points(entry)
    ctx.set_frames_per_pass(frames)


def _render(ctx, passes=PASSES):
    ctx.reset_frame_number()
    for _ in range(passes):
        ctx.render_frame()
        ctx.accumulate()
    return ctx.read_accumulation(), ctx.read_rgba8()


def _same(got, want, what):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "accumulation differs: %s" % (what,)
    assert np.array_equal(got[1], want[1]), "rgba8 differs: %s" % (what,)


@pytest.fixture(scope="module")
def one_at_a_time(gpu_ctx_factory, zoo):
    """the image of ten passes one at a time, and the trace grid of n slots that all fit their budget, n = 1 .. 6"""
    ctx = gpu_ctx_factory(W, H)
    _prepare(ctx, zoo)
    want = _render(ctx)
    assert want[0].max() > 0.1
    ctx.set_queue_budget(ROOMY)
    grids = {}
    for n in range(1, 7):
        ctx.set_passes_in_flight(n)
        resident, grids[n], _ = ctx.debug_resident_slots()
        assert resident == n
    ctx.set_passes_in_flight(1)
    assert grids[1] > grids[2] > grids[4] > grids[6] > 0, grids  # (the shares differ: a wrong count would show)
    for image in want:
        image.setflags(write=False)
    return want, grids


@pytest.mark.parametrize("R", [2, 3, 4, 6])
def test_every_budget_renders_the_image_of_one_pass_at_a_time(gpu_ctx_factory, zoo, one_at_a_time, R):
    want, grids = one_at_a_time
    ctx = gpu_ctx_factory(W, H)
    _prepare(ctx, zoo)
    ctx.set_passes_in_flight(R)
    for budget in BUDGETS:
        ctx.set_queue_budget(budget)
        resident = capi.resident_slots_for(R, budget)
        ctx.reset_frame_number()
        used = set()
        for _ in range(PASSES):
            ctx.render_frame()
            used.add(ctx.debug_resident_slots()[2])
            ctx.accumulate()
        _same((ctx.read_accumulation(), ctx.read_rgba8()), want, (R, budget))
        got, blocks, _ = ctx.debug_resident_slots()
        assert got == resident, (R, budget, got)
        assert blocks == grids[resident], (R, budget, blocks, grids)
        assert used == set(range(R)), (R, budget, used)  # (the round robin runs over all R slots, whatever the resident count)
    assert ctx.queue_budget()[2] <= MAX_GRAPH_INSTANCES  # (the trace grid is part of an instance's key: one instance per budget here)


@pytest.mark.parametrize("budget", [4, 24])
def test_four_renders_then_one_accumulate(gpu_ctx_factory, zoo, one_at_a_time, budget):
    """R passes may await their accumulate whatever the resident count: every one of them is folded in, oldest first."""
    want, _ = one_at_a_time
    ctx = gpu_ctx_factory(W, H)
    _prepare(ctx, zoo)
    ctx.set_passes_in_flight(4)
    ctx.set_queue_budget(budget)
    ctx.reset_frame_number()
    for group in (4, 4, 2):
        slots = []
        for _ in range(group):
            ctx.render_frame()
            slots.append(ctx.debug_resident_slots()[2])
        assert len(set(slots)) == group, "a pass was rendered over one not yet folded in: %s" % (slots,)
        ctx.accumulate()
    _same((ctx.read_accumulation(), ctx.read_rgba8()), want, "4 + 4 + 2 passes, budget %d" % budget)


def test_switching_budget_and_passes_in_flight_between_passes(gpu_ctx_factory, zoo, one_at_a_time):
    want, _ = one_at_a_time
    ctx = gpu_ctx_factory(W, H)
    _prepare(ctx, zoo)
    ctx.set_passes_in_flight(4)
    ctx.reset_frame_number()
    for budget, passes in ((4, 4), (24, 3), (4, 3)):  # no reset in between: one image
        ctx.set_queue_budget(budget)
        for _ in range(passes):
            ctx.render_frame()
            ctx.accumulate()
        assert ctx.debug_resident_slots()[0] == capi.resident_slots_for(4, budget)
    _same((ctx.read_accumulation(), ctx.read_rgba8()), want, "budget 4 -> 24 -> 4")

    ctx.set_queue_budget(4)
    ctx.reset_frame_number()
    for R, passes in ((4, 4), (2, 3), (6, 3)):
        ctx.set_passes_in_flight(R)
        for _ in range(passes):
            ctx.render_frame()
            ctx.accumulate()
        assert ctx.debug_resident_slots()[0] == capi.resident_slots_for(R, 4)
    _same((ctx.read_accumulation(), ctx.read_rgba8()), want, "R 4 -> 2 -> 6")
    assert ctx.queue_budget()[2] <= MAX_GRAPH_INSTANCES


GROUPS = (1, 1, 1, 4, 2)  # nine passes: three folded one by one, then four and two awaiting their accumulate at once


def _grouped(ctx, R):
    """nine passes; with passes in flight, several renders per accumulate (one pass at a time keeps one: a second render would replace the first)"""
    ctx.set_passes_in_flight(R)
    ctx.set_queue_budget(4)
    ctx.reset_frame_number()
    used = set()
    for group in GROUPS if R > 1 else (1,) * sum(GROUPS):
        for _ in range(group):
            ctx.render_frame()
            used.add(ctx.debug_resident_slots()[2])
        ctx.accumulate()
    assert len(used) == R, used  # (every slot rendered, those beyond the resident count too)
    return ctx.read_accumulation(), ctx.read_rgba8()


def test_entry_tables_in_tile_order(gpu_ctx_factory, zoo):
    """Entry points on, 8 x 8 tile order, R = 4 on four queues (the shares of three): each of the four slots walks and keeps its own entry table."""
    images = []
    for R in (1, 4):
        ctx = gpu_ctx_factory(W, H)
        _prepare(ctx, zoo, entry=True, order=pod.ORDER_TILES, frames=2)
        images.append(_grouped(ctx, R))
    _same(images[1], images[0], "tile order, R = 4 on four queues")


def test_short_last_region(gpu_ctx_factory):
    """1 337 of the 1 500 pixels of a 50 x 30 view (the map and seed of tests/test_gpu_queue_budget.py::
    test_partial_run_and_short_last_region): 20 runs of 64 and one of 57, and a last queue region shorter than the others, in every slot."""
    w, h = 50, 30
    scene = SH.material_zoo_scene(w, h, path_length=4)
    pm = np.sort(np.random.default_rng(7).choice(w * h, size=1337, replace=False)).astype(np.uint32)
    images = []
    for R in (1, 4):
        ctx = gpu_ctx_factory(w, h)
        scene.upload(ctx)
        ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
        ctx.set_pixel_map(pm)
        ctx.set_entry_points(True)
        ctx.set_frames_per_pass(2)
        images.append(_grouped(ctx, R))
    _same(images[1], images[0], "pixel map of 1 337, R = 4 on four queues")


def test_one_pass_at_a_time_keeps_its_grid_at_any_budget(gpu_ctx_factory, zoo, one_at_a_time):
    """R = 1: one resident slot and the grid of a single pass whatever the budget — with the launches that
    tests/test_gpu_queue_budget.py::test_one_pass_at_a_time_is_unchanged_at_any_budget counts, the parent commit's graph."""
    want, grids = one_at_a_time
    ctx = gpu_ctx_factory(W, H)
    _prepare(ctx, zoo)
    graphs = set()
    for budget in BUDGETS:
        ctx.set_queue_budget(budget)
        _same(_render(ctx), want, budget)
        assert ctx.debug_resident_slots() == (1, grids[1], 0), budget
        graphs.add(ctx.debug_last_graph())
    assert len(graphs) == 1 and ctx.queue_budget()[2] == 1, graphs  # one instance, replayed at every budget
