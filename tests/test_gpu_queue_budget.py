"""The queue budget (nxhip_set_queue_budget): R passes in flight need 2 R + 1 lanes; where the budget has fewer, every slot's
pass graph is a single chain.  Only dependency edges differ, so every image must equal the one rendered one pass at a time,
bit for bit, whatever R and the budget are."""
import ctypes as C

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

W, H = 96, 40            # 3 840 pixels = 60 whole 8 x 8 tiles: both pixel orders apply
FRAMES, PASSES = 3, 10   # 10 passes: no multiple of R = 4
MAX_GRAPH_INSTANCES = 8  # kMaxGraphInstances (nxhip_render.hip)
BUDGETS = (4, 24, 1)


def _chained(R, budget):
    return R > 1 and 2 * R + 1 > budget


# Kernel nodes of a slot's pass graph for the zoo at pathLength 4, SCAN pipeline, no thin level (R > 1): generate, the primary launch,
# then per bounce material + closest-hit + any-hit.  R = 4: four bounces = 14.  R = 2: the tail kernel takes over at bounce 3
# (passes of up to 2.5 frames' worth of paths in at most three slots) = 2 + 2 x 3 + 1 = 9.
GRAPH_NODES = {2: 9, 4: 14}


def _assert_graph(ctx, R, budget):
    """The shape of the graph the last pass replayed, from the runtime's own node and edge lists (not from the library's rule)."""
    nodes, edges, fan_out = ctx.debug_last_graph()
    assert nodes == GRAPH_NODES[R], (R, budget, nodes)
    if _chained(R, budget):
        assert (edges, fan_out) == (nodes - 1, 1), "not a chain: %s" % ((R, budget, nodes, edges, fan_out),)
    else:
        assert fan_out == 2 and edges > nodes - 1, "not the parallel graph: %s" % ((R, budget, nodes, edges, fan_out),)


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


@pytest.mark.parametrize("order", [pod.ORDER_ROWS, pod.ORDER_TILES], ids=["rows", "tiles"])
@pytest.mark.parametrize("entry", [True, False], ids=["entry", "root"])
def test_every_shape_renders_the_image_of_one_pass_at_a_time(gpu_ctx_factory, zoo, entry, order):
    ctx = gpu_ctx_factory(W, H)
    _prepare(ctx, zoo, entry, order)
    want = _render(ctx)
    assert want[0].max() > 0.1
    for R in (2, 4):
        for budget in BUDGETS:
            ctx.set_passes_in_flight(R)
            ctx.set_queue_budget(budget)
            assert ctx.queue_budget()[:2] == (budget, _chained(R, budget))
            _same(_render(ctx), want, (R, budget))
            _assert_graph(ctx, R, budget)
    assert ctx.queue_budget()[2] <= MAX_GRAPH_INSTANCES


def test_partial_run_and_short_last_region(gpu_ctx_factory):
    """1 337 of the 1 500 pixels of a 50 x 30 view: 20 runs of 64 and one of 57, and a last queue region shorter than the others."""
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
        ctx.set_passes_in_flight(R)
        ctx.set_queue_budget(4)
        assert ctx.queue_budget()[1] == (R == 4)
        images.append(_render(ctx, passes=9))
    _same(images[1], images[0], "pixel map of 1 337")


def test_switching_the_budget_between_passes(gpu_ctx_factory, zoo):
    ref = gpu_ctx_factory(W, H)
    _prepare(ref, zoo)
    want = _render(ref)
    ctx = gpu_ctx_factory(W, H)
    _prepare(ctx, zoo)
    ctx.set_passes_in_flight(4)
    ctx.reset_frame_number()
    for budget, passes in ((4, 4), (24, 3), (4, 3)):  # no reset in between: one image
        ctx.set_queue_budget(budget)
        assert ctx.queue_budget()[1] == _chained(4, budget)
        for _ in range(passes):
            ctx.render_frame()
            ctx.accumulate()
        _assert_graph(ctx, 4, budget)
    _same((ctx.read_accumulation(), ctx.read_rgba8()), want, "budget 4 -> 24 -> 4")
    assert 2 <= ctx.queue_budget()[2] <= MAX_GRAPH_INSTANCES  # (a slot holds the chain and the parallel instance, built once each)


def test_the_callers_stream_sees_every_accumulated_pass(zoo):
    """A context on the caller's stream: a copy the caller enqueues on that stream right behind accumulate() reads the image as of
    that pass, and the next accumulate does not overtake the copy.  No host synchronisation until every pass has been issued."""
    hip = C.CDLL("libamdhip64.so.7")  # the HIP runtime libnexus_amd.so is already bound to (matched by soname)
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipHostFree.argtypes = [C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    n_bytes = W * H * 16  # the accumulation: one float4 per pixel

    with capi.Context(W, H) as ref:
        _prepare(ref, zoo)
        ref.reset_frame_number()
        want = []
        for _ in range(PASSES):
            ref.render_frame()
            ref.accumulate()
            want.append(ref.read_accumulation())

    stream, pinned = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0  # hipStreamNonBlocking
    assert hip.hipHostMalloc(C.byref(pinned), PASSES * n_bytes, 0) == 0
    try:
        with capi.Context(W, H, stream=stream.value) as ctx:
            _prepare(ctx, zoo)
            ctx.set_passes_in_flight(4)
            ctx.set_queue_budget(4)
            assert ctx.queue_budget()[1]
            ctx.reset_frame_number()
            src = C.c_void_p(ctx.accumulation_device_ptr())
            for i in range(PASSES):
                ctx.render_frame()
                ctx.accumulate()
                assert hip.hipMemcpyAsync(C.c_void_p(pinned.value + i * n_bytes), src, n_bytes, 2, stream) == 0  # device to host
            assert hip.hipStreamSynchronize(stream) == 0
            got = np.ctypeslib.as_array(C.cast(pinned, C.POINTER(C.c_float)), shape=(PASSES, W * H, 4)).copy()
            ctx.sync()
    finally:
        hip.hipHostFree(pinned)
        hip.hipStreamDestroy(stream)
    for i in range(PASSES):
        assert np.array_equal(got[i, :, :3].view(np.uint32), want[i].view(np.uint32)), "the copy behind pass %d" % (i + 1)


def test_setter_and_resolution(gpu_ctx_factory, monkeypatch):
    ctx = gpu_ctx_factory(W, H)
    for bad in (33, -1):
        with pytest.raises(capi.NexusError):
            ctx.set_queue_budget(bad)
    ctx.set_queue_budget(32)
    assert ctx.queue_budget()[0] == 32
    # (values the runtime itself accepts only; what out-of-range and malformed text resolves to: tests/test_queue_budget_text.py, no device)
    for text, want in (("7", 7), ("32", 32), ("1", 1)):
        monkeypatch.setenv("GPU_MAX_HW_QUEUES", text)
        ctx.set_queue_budget(0)
        assert ctx.queue_budget()[0] == want, text
    monkeypatch.delenv("GPU_MAX_HW_QUEUES")
    ctx.set_queue_budget(0)
    assert ctx.queue_budget()[0] == 4  # the runtime's own default


# What the parent commit launches for two 3-frame passes of the zoo (pathLength 4, entry points on) one at a time, by kernel class, with
# in-graph timing — counted on a build of that commit: per pass generate, 1 + 4 closest-hit, 4 any-hit, 4 material launches, a thin
# launch behind each of the 9 trace launches, one accumulate — and the flavor word of its graph (SCAN, miss kernel, environment map,
# entry points, thin level).  A timing run of a context set to R = 4 renders one pass at a time too, without the thin level.
PARENT_LAUNCHES = {"generate": 2, "trace": 10, "shadow": 8, "logic": 0, "shade": 8, "accumulate": 2, "thin": 18}
PARENT_FLAVOR = {1: 1 | 2 | 4 | 8 | 16, 4: 1 | 2 | 4 | 8}


def test_one_pass_at_a_time_is_unchanged_at_any_budget(gpu_ctx_factory, zoo):
    """R = 1 — and a timing run of a context set to R = 4 — replay the parent's parallel graph whatever the budget: its flavor, its
    launches class by class, closest-hit beside any-hit."""
    ctx = gpu_ctx_factory(W, H)
    _prepare(ctx, zoo)
    _render(ctx, passes=1)  # (the entry-state walk in front of a context's first pass is a launch of its own: not one of the graph's)
    images = []
    for R in (1, 4):
        ctx.set_passes_in_flight(R)
        ctx.enable_kernel_timing(True, in_graph=True)
        for budget in BUDGETS:
            ctx.set_queue_budget(budget)
            assert ctx.queue_budget()[1] is False
            ctx.read_kernel_times(reset=True)
            images.append(_render(ctx, passes=2))
            launches = {k: v["launches"] for k, v in ctx.read_kernel_times().items()}
            want = dict(PARENT_LAUNCHES, thin=PARENT_LAUNCHES["thin"] if R == 1 else 0)
            assert launches == want, (R, budget, launches)
            assert ctx.debug_pass_flavor() == PARENT_FLAVOR[R], (R, budget)
            assert ctx.debug_last_graph()[2] == 2, (R, budget)
        ctx.enable_kernel_timing(False)
    for image in images[1:]:
        _same(image, images[0], "timing runs")
