"""Error behaviour of the C-ABI on a GPU: misuse returns a status and a message (the reference's CheckCudaErrors prints,
resets the device and exit(99)s, Utils/Utils.cpp:3-12), nothing is launched with bad indices, and the context stays usable."""
import numpy as np
import pytest

from nexus_amd import capi, pod
from nexus_amd.capi import NexusError
from tests import oracle_lib as O
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu


def test_render_before_a_scene_is_set(gpu_ctx_factory):
    ctx = gpu_ctx_factory(32, 32)
    with pytest.raises(NexusError, match="TLAS"):
        ctx.render_frame()
    scene = SH.soup_scene(n=200, seed=2)
    for nodes, tris, idx in scene.blas:
        ctx.upload_blas(nodes, tris, idx)
    ctx.set_tlas(scene.tlas_nodes, scene.tlas_idx, scene.instances)
    with pytest.raises(NexusError, match="materials"):
        ctx.render_frame()


def test_malformed_bvh_uploads_are_rejected(gpu_ctx_factory):
    ctx = gpu_ctx_factory(32, 32)
    scene = SH.soup_scene(n=300, seed=3)
    nodes, tris, idx = scene.blas[0]
    bad_idx = idx.copy()
    bad_idx[5] = len(tris)
    with pytest.raises(NexusError, match="triangle index"):
        ctx.upload_blas(nodes, tris, bad_idx)
    bad_nodes = nodes.copy()
    bad_nodes["childBaseIdx"][0] = len(nodes) + 7
    with pytest.raises(NexusError, match="child index"):
        ctx.upload_blas(bad_nodes, tris, idx)
    bad_nodes = nodes.copy()
    bad_nodes["triangleBaseIdx"][:] = len(tris)
    with pytest.raises(NexusError, match="leaf range"):
        ctx.upload_blas(bad_nodes, tris, idx)
    with pytest.raises(NexusError, match="empty"):
        ctx.upload_blas(nodes[:0], tris, idx)
    # the kernels decode a slot from its meta byte alone: what that decoding would make of a damaged byte is checked too
    root = nodes[0]
    inner_slot = next(s for s in range(8) if (int(root["imask"]) >> s) & 1)
    leaf_node, leaf_slot = next((i, s) for i in range(len(nodes)) for s in range(8) if not (int(nodes[i]["imask"]) >> s) & 1 and int(nodes[i]["meta"][s]) >> 5)
    for field, node, slot, value, what in (
            ("imask", 0, None, int(root["imask"]) & ~(1 << inner_slot), "not announced in imask"),
            ("meta", 0, inner_slot, 0x60 | (24 + inner_slot), "more than one hit bit"),
            ("meta", 0, inner_slot, 0x20 | (24 + (inner_slot ^ 1)), "another slot's number"),
            ("meta", leaf_node, leaf_slot, 0xe0 | 22, "leave the 24-bit primitive mask")):
        bad_nodes = nodes.copy()
        if slot is None:
            bad_nodes[field][node] = value
        else:
            bad_nodes[field][node][slot] = value
        with pytest.raises(NexusError, match=what):
            ctx.upload_blas(bad_nodes, tris, idx)
    # instances that refer to a BLAS that was never uploaded
    with pytest.raises(NexusError, match="BLAS id"):
        ctx.set_tlas(scene.tlas_nodes, scene.tlas_idx, scene.instances)
    ctx.upload_blas(nodes, tris, idx)
    bad_inst_idx = scene.tlas_idx.copy()
    bad_inst_idx[0] = 5
    with pytest.raises(NexusError, match="instance index"):
        ctx.set_tlas(scene.tlas_nodes, bad_inst_idx, scene.instances)
    # and the good upload still works afterwards
    ctx.set_tlas(scene.tlas_nodes, scene.tlas_idx, scene.instances)
    rays = np.zeros(4, dtype=pod.RAY_DT)
    rays["origin"] = (0, 0, -5)
    rays["direction"] = (0, 0, 1)
    assert SH.hit_records_equal(ctx.trace_batch(rays), scene.oracle().trace_closest(rays))


def test_settings_modes_and_viewport_arguments(gpu_ctx_factory):
    W, H = 32, 24
    scene = SH.cornell_scene(W, H, path_length=2)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    for bad_len in (0, 99, 255):
        st = O.make_settings(path_length=4)
        st["pathLength"] = bad_len
        with pytest.raises(NexusError, match="pathLength"):
            ctx.set_render_settings(st)
    with pytest.raises(NexusError, match="mode"):
        ctx.set_modes(7, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    with pytest.raises(NexusError):
        ctx.set_frames_per_pass(0)
    with pytest.raises(NexusError):
        ctx.set_frames_per_pass(100000)
    with pytest.raises(NexusError, match="zero-sized"):
        ctx.resize(0, 16)
    with pytest.raises(NexusError, match="2\\^31"):
        ctx.resize(65536, 65536)
    assert (ctx.width, ctx.height) == (W, H)
    with pytest.raises(NexusError, match="out of range"):
        ctx.set_pixel_map(np.array([0, 1, W * H], dtype=np.uint32))
    with pytest.raises(NexusError, match="outside"):
        ctx.set_pixel_query(W, 0)
    cam = capi.camera_init((0.0, 1.0, 3.9), (0.0, 0.0, -1.0), 40.0, W * 2, H, 5.0, 0.0)
    with pytest.raises(NexusError, match="resolution"):
        ctx.set_camera(cam)
    with pytest.raises(NexusError):
        ctx.bind_radiance(ctx.accumulation_device_ptr(), 3)  # smaller than the path count
    with pytest.raises(NexusError):
        ctx.tex2d_batch("diffuse", 0, np.zeros((1, 2), np.float32))  # no such texture
    # none of the failed calls disturbed the context: it still renders the oracle's frame
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.reset_frame_number()
    ctx.render_frame()
    ctx.accumulate()
    w = O.Wavefront(scene.oracle(), W * H, None, pod.RNG_PIXEL_KEYED, pod.CONDUCTOR_REFERENCE)
    w.render(1, threads=4)
    assert SH.frames_identical(ctx.read_radiance(), w.radiance(), "after the refused calls")


def test_environment_hooks_refuse_what_they_cannot_answer(gpu_ctx_factory):
    """nxhip_read_env_tables / nxhip_env_sample_batch / nxhip_env_eval_batch: no map, sampler off, null arrays, numbers outside [0, 1),
    non-finite directions, a destination too small — a status each, nothing launched; count == 0 is fine"""
    import ctypes as C

    ctx = gpu_ctx_factory(16, 16)
    L = ctx.L
    d = np.array([[0.0, 1.0, 0.0], [0.6, 0.0, -0.8]], np.float32)
    r = np.array([[0.5, 0.25]], np.float32)
    for call in (ctx.read_env_tables, lambda: ctx.env_sample_batch(r), lambda: ctx.env_eval_batch(d), lambda: ctx.env_eval_batch(d, with_pdf=False),
                 lambda: ctx.env_sample_batch(np.zeros((0, 2), np.float32))):
        with pytest.raises(NexusError, match="no environment map"):
            call()
    ctx.upload_texture("hdr", SH.checker_texture(16, 8, 5))
    rgb, pdf, texel = ctx.env_eval_batch(d, with_pdf=False)  # the colours alone need no sampler
    assert pdf is None and texel is None and np.all(np.isfinite(rgb)) and rgb.max() > 0
    for call in (ctx.read_env_tables, lambda: ctx.env_sample_batch(r), lambda: ctx.env_eval_batch(d)):
        with pytest.raises(NexusError, match="sampling is off"):
            call()
    ctx.set_env_sampling(True)
    marginal, row, density = ctx.read_env_tables()
    assert marginal.shape == (8,) and row.shape == (8, 16) and density.shape == (8, 16)
    for bad in (1.0, -0.125, 2.0, np.nan, np.inf):
        for column in (0, 1):
            rr = np.array([[0.5, 0.5], [0.5, 0.5]], np.float32)
            rr[1, column] = bad
            with pytest.raises(NexusError, match=r"r must be in \[0, 1\)"):
                ctx.env_sample_batch(rr)
    for bad in (np.nan, np.inf, -np.inf):
        dd = d.copy()
        dd[1, 2] = bad
        with pytest.raises(NexusError, match="finite"):
            ctx.env_eval_batch(dd)
    # count == 0
    assert [len(a) for a in ctx.env_sample_batch(np.zeros((0, 2), np.float32))] == [0, 0, 0]
    assert len(ctx.env_eval_batch(np.zeros((0, 3), np.float32))[0]) == 0
    # null arrays with count > 0, a destination too small, a null context
    out3, out1, outi = np.zeros(3, np.float32), np.zeros(1, np.float32), np.zeros(1, np.uint32)
    p = capi._ptr
    assert L.nxhip_env_sample_batch(ctx.h, None, 1, p(out3), p(out1), p(outi)) == 1
    assert L.nxhip_env_sample_batch(ctx.h, p(r), 1, None, p(out1), p(outi)) == 1
    assert L.nxhip_env_sample_batch(ctx.h, p(r), 1, p(out3), None, p(outi)) == 1
    assert L.nxhip_env_sample_batch(ctx.h, p(r), 1, p(out3), p(out1), None) == 1
    assert L.nxhip_env_eval_batch(ctx.h, None, 1, p(out3), None, None) == 1
    assert L.nxhip_env_eval_batch(ctx.h, p(d), 1, None, None, None) == 1
    assert L.nxhip_env_eval_batch(ctx.h, None, 0, None, None, None) == 0
    small = np.zeros(127, np.float32)
    assert L.nxhip_read_env_tables(ctx.h, None, p(small), None, 127, None, None) == 1
    assert b"too small" in capi.lib().nxhip_last_error()
    rows = np.zeros(8, np.float32)  # the marginal cdf alone: one entry per row is room enough
    assert L.nxhip_read_env_tables(ctx.h, p(rows), None, None, 8, None, None) == 0 and np.array_equal(rows, marginal)
    assert L.nxhip_read_env_tables(ctx.h, p(rows), None, None, 7, None, None) == 1
    assert L.nxhip_read_env_tables(None, None, None, None, 0, None, None) == 1
    assert L.nxhip_env_sample_batch(None, p(r), 1, p(out3), p(out1), p(outi)) == 1
    assert L.nxhip_env_eval_batch(None, p(d), 1, p(out3), None, None) == 1
    # the context is undisturbed, and turning the sampler off is heard by the hooks
    assert np.array_equal(ctx.env_eval_batch(d, with_pdf=False)[0], rgb)
    assert np.all(ctx.env_eval_batch(d)[1] > 0)
    ctx.set_env_sampling(False)
    with pytest.raises(NexusError, match="sampling is off"):
        ctx.env_sample_batch(r)
    ctx.clear_textures()
    with pytest.raises(NexusError, match="no environment map"):
        ctx.env_eval_batch(d, with_pdf=False)


def test_contexts_are_independent_and_closing_is_idempotent(gpu_ctx_factory):
    a = gpu_ctx_factory(16, 16)
    b = gpu_ctx_factory(16, 16)
    scene = SH.soup_scene(n=100, seed=4)
    scene.upload(a)
    with pytest.raises(NexusError):
        b.render_frame()  # b has no scene although a does
    a.render_frame()
    a.close()
    a.close()
    with pytest.raises(NexusError):
        b.render_frame()


def test_contexts_release_their_device_memory():
    """create -> upload -> render -> destroy, many times: free device memory returns to where it was (queues, BVH copies,
    textures, graph, events and streams are all owned by the context)."""
    import ctypes as C

    hip = C.CDLL("libamdhip64.so.7")  # the runtime libnexus_amd.so is bound to
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]

    def free_bytes():
        f, t = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    scene = SH.material_zoo_scene(256, 192, path_length=3)

    def cycle():
        ctx = capi.Context(256, 192, device=0)
        scene.upload(ctx)
        ctx.set_frames_per_pass(4)
        ctx.render_frame()
        ctx.accumulate()
        ctx.enable_kernel_timing(True, in_graph=True)
        ctx.render_frame()
        ctx.read_kernel_times(reset=True)
        ctx.resize(128, 96)
        ctx.close()

    for _ in range(6):  # the runtime's own pools (code objects, scratch, graph memory) settle during the first cycles
        cycle()
    before = free_bytes()
    for _ in range(24):
        cycle()
    after = free_bytes()
    # one context of this size holds about 60 MB: leaking it would cost 1.4 GB over these cycles; the runtime's pools wobble by a few MB
    assert before - after < 64 << 20, (before, after)


def test_a_failed_queue_growth_leaves_the_context_usable(gpu_ctx_factory):
    """Out of device memory half-way through the queue buffers (1 M pixels x 1024 frames per pass is about 350 GB of queues):
    the call fails, nothing is left dangling, and the context keeps rendering at its previous pass size."""
    import numpy as np
    from nexus_amd import pod
    from tests import scene_helpers as SH

    W = H = 1024
    scene = SH.cornell_scene(W, H, path_length=2)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    ctx.render_frame()
    ctx.accumulate()
    before = ctx.read_accumulation()
    with pytest.raises(capi.NexusError):
        ctx.set_frames_per_pass(1400)  # 1.47 G paths x 276 B: more than the 288 GiB of the card
    assert ctx.frames_per_pass == 1
    ctx.reset_frame_number()
    ctx.render_frame()
    ctx.accumulate()
    after = ctx.read_accumulation()
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))


def test_a_bvh_that_is_not_a_tree_ends_in_an_error_status_not_in_a_hang(gpu_ctx_factory):
    """A node whose child range points back at itself passes no upload (nxhip_upload_blas and nxhip_set_tlas insist on
    children behind their parent), so it is planted with the debug hook.  The trace kernels abandon the rays that go round in
    circles after kStallLimit iterations without a retirement, nxhip_sync reports NXHIP_ERR_TRAVERSAL once, and the context
    works again after the node is repaired."""
    import time

    import numpy as np
    from nexus_amd import pod, scenegen
    from tests import scene_helpers as SH

    scene = SH.soup_scene(n=800, seed=3)
    ctx = gpu_ctx_factory(64, 64)
    scene.upload(ctx)
    rays = np.concatenate([scenegen.random_rays(1024, seed=5, radius=5.0, target_extent=2.0), scenegen.interior_rays(1024, seed=6, extent=2.0)])
    want = scene.oracle().trace_closest(rays)
    assert SH.hit_records_equal(ctx.trace_batch(rays), want)
    ctx.sync()
    nodes, _ = ctx.read_blas(0, len(scene.blas[0][1]))
    assert nodes["imask"][0] != 0
    # upload refuses the cycle ...
    bad_nodes = nodes.copy()
    bad_nodes["childBaseIdx"][0] = 0
    with pytest.raises(capi.NexusError):
        ctx.upload_blas(bad_nodes, scene.blas[0][1], scene.blas[0][2])
    # ... the hook plants it: the root's first inner child is now the root itself
    ctx.debug_write_blas_node(0, 0, bad_nodes[0])
    t0 = time.time()
    ctx.trace_batch(rays)
    with pytest.raises(capi.NexusError, match="not a tree"):
        ctx.sync()
    assert time.time() - t0 < 60.0
    ctx.sync()  # reported once
    ctx.debug_write_blas_node(0, 0, nodes[0])
    assert SH.hit_records_equal(ctx.trace_batch(rays), want)
    ctx.sync()


def test_rays_that_requeue_themselves_end_in_a_status_within_seconds(gpu_ctx_factory):
    """VERDICT r5 item 7, from the failure in hand (gpurun_out/r5_10: an in-kernel restart whose rays came back into the queue ran to the
    host's 150 s watchdog): every such ray RETIRES, so the iteration count between two refill points never reaches its limit.  The
    per-launch check — a wave cannot be handed more rays than the queue holds — ends the launch; nxhip_sync reports
    NXHIP_ERR_TRAVERSAL once; frames and ray batches work again afterwards."""
    import time

    import numpy as np
    from nexus_amd import pod, scenegen
    from tests import scene_helpers as SH

    scene = SH.cornell_scene(128, 128, path_length=4)
    ctx = gpu_ctx_factory(128, 128)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    rays = scenegen.interior_rays(20000, seed=2, extent=0.9)
    rays["origin"][:, 1] += 1.0
    want = scene.oracle().trace_closest(rays)
    ctx.set_frames_per_pass(4)
    ctx.reset_frame_number()
    ctx.render_frame()
    ctx.accumulate()
    good = ctx.read_accumulation()
    ctx.debug_set_requeue(True)
    t0 = time.time()
    ctx.trace_batch(rays)  # (results void)
    with pytest.raises(capi.NexusError, match="re-enter the queue"):
        ctx.sync()
    ctx.reset_frame_number()
    ctx.render_frame()     # a whole pass of such launches
    with pytest.raises(capi.NexusError, match="status 4"):
        ctx.sync_timeout(20000)
    assert time.time() - t0 < 5.0, "seconds, not the host's watchdog"
    ctx.sync()  # reported once
    ctx.debug_set_requeue(False)
    assert SH.hit_records_equal(ctx.trace_batch(rays), want)
    ctx.reset_frame_number()
    ctx.render_frame()
    ctx.accumulate()
    ctx.sync()
    assert np.array_equal(ctx.read_accumulation().view(np.uint32), good.view(np.uint32))


def test_sync_with_a_wall_clock_limit_marks_the_context_dead():
    """nxhip_sync_timeout: work that finishes in time -> as nxhip_sync; a limit that expires -> NXHIP_ERR_TIMEOUT (status 6), every later
    call on the context answers with the same status without touching the device, closing it is safe.  (The expiry is provoked with
    a limit of 0 ms on a pass that takes tens of milliseconds — a real hang is not something to stage on a shared GPU.)"""
    from nexus_amd import pod, workloads
    from tests import scene_helpers as SH

    W, H = 512, 512
    scene = workloads.config2(W, H, 128, 64, 8, cls=SH.BuiltScene)
    ctx = capi.Context(W, H)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    ctx.set_frames_per_pass(64)
    ctx.render_frame()
    ctx.sync_timeout(30000)  # in time
    ctx.render_frame()
    with pytest.raises(capi.NexusError, match="status 6"):
        ctx.sync_timeout(0)
    for call in (ctx.render_frame, ctx.sync, ctx.accumulate, lambda: ctx.sync_timeout(1000)):
        with pytest.raises(capi.NexusError, match="status 6"):
            call()
    ctx.close()  # (the pass has long finished by now: a normal teardown; a context whose device never answers keeps its memory)


def test_released_queues_come_back_with_the_next_render(gpu_ctx_factory):
    """nxhip_release_queues (PathTracer::FreeDeviceBuffers): the image, the scene and the frame count survive, rendering and
    the ray-batch hook allocate again on demand; the same holds for the slots of passes in flight."""
    import numpy as np
    from nexus_amd import pod, scenegen
    from tests import scene_helpers as SH

    W = H = 96
    scene = SH.cornell_scene(W, H, path_length=3)
    ctx = gpu_ctx_factory(W, H)
    scene.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    for _ in range(2):
        ctx.render_frame()
        ctx.accumulate()
    two = ctx.read_accumulation()
    ctx.release_queues()
    assert np.array_equal(ctx.read_accumulation().view(np.uint32), two.view(np.uint32))
    rays = scenegen.interior_rays(2048, seed=2, extent=0.9)
    rays["origin"][:, 1] += 1.0
    assert SH.hit_records_equal(ctx.trace_batch(rays), scene.oracle().trace_closest(rays))
    ctx.release_queues()
    ctx.render_frame()
    ctx.accumulate()
    three = ctx.read_accumulation()
    # the same three frames without the releases in between
    ref = gpu_ctx_factory(W, H)
    scene.upload(ref)
    ref.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
    for _ in range(3):
        ref.render_frame()
        ref.accumulate()
    assert np.array_equal(three.view(np.uint32), ref.read_accumulation().view(np.uint32))
    # passes in flight: slot 0 gives its queues back while the passes render in the extra slots, and takes them again for the hook
    ctx.set_passes_in_flight(3)
    for _ in range(4):
        ctx.render_frame()
        ctx.accumulate()
    assert SH.hit_records_equal(ctx.trace_batch(rays), scene.oracle().trace_closest(rays))
    ctx.set_passes_in_flight(1)
    ctx.render_frame()
    ctx.accumulate()
    ref.set_passes_in_flight(1)
    for _ in range(5):
        ref.render_frame()
        ref.accumulate()
    assert np.array_equal(ctx.read_accumulation().view(np.uint32), ref.read_accumulation().view(np.uint32))


def test_binary_tree_hook_refuses_what_it_cannot_answer(gpu_ctx_factory):
    """nxhip_debug_keep_binary_tree / nxhip_debug_read_binary_tree: nothing stashed, a null count, a null context, a capacity too small
    (the count still comes back), a null array — NXHIP_ERR_INVALID each, the stash and the context untouched"""
    import ctypes as C

    from nexus_amd import scenegen

    ctx = gpu_ctx_factory(32, 32)
    L = ctx.L
    n, cost, builder = C.c_uint32(77), C.c_float(0.0), C.c_int32(5)
    nothing = (None,) * 7
    assert L.nxhip_debug_keep_binary_tree(None, 1) == 1
    assert L.nxhip_debug_read_binary_tree(None, 0, C.byref(n), None, None, *nothing) == 1
    with pytest.raises(NexusError, match="no binary tree is stashed"):
        ctx.debug_read_binary_tree()
    tris = np.ascontiguousarray(scenegen.random_soup(20, seed=1), dtype=pod.TRI_DT)
    ctx.build_blas(tris)
    assert L.nxhip_debug_read_binary_tree(ctx.h, 0, C.byref(n), None, None, *nothing) == 1 and n.value == 77, "off is the default"
    ctx.debug_keep_binary_tree(True)
    assert L.nxhip_debug_read_binary_tree(ctx.h, 0, C.byref(n), None, None, *nothing) == 1, "on, and no build since"
    ctx.build_blas(tris)
    assert L.nxhip_debug_read_binary_tree(ctx.h, 20, None, None, None, *nothing) == 1
    assert b"null n" in capi.lib().nxhip_last_error()
    assert L.nxhip_debug_read_binary_tree(ctx.h, 0, C.byref(n), C.byref(cost), C.byref(builder), *nothing) == 1
    assert b"capacity too small" in capi.lib().nxhip_last_error() and (n.value, cost.value, builder.value) == (20, 0.75, -1)
    p = capi._ptr
    i32 = [np.full(64, -7, np.int32) for _ in range(4)]
    box, order, table = np.zeros(39 * 6, np.float32), np.zeros(20, np.uint32), np.zeros(19 * 7, np.uint64)
    assert L.nxhip_debug_read_binary_tree(ctx.h, 19, C.byref(n), None, None, p(i32[0]), p(i32[1]), p(i32[2]), p(i32[3]), p(box), p(order), p(table)) == 1
    assert L.nxhip_debug_read_binary_tree(ctx.h, 20, C.byref(n), None, None, p(i32[0]), p(i32[1]), p(i32[2]), p(i32[3]), p(box), None, p(table)) == 1
    assert b"null destination" in capi.lib().nxhip_last_error() and all(np.all(a == -7) for a in i32), "nothing was written"
    assert L.nxhip_debug_read_binary_tree(ctx.h, 20, C.byref(n), None, None, p(i32[0]), p(i32[1]), p(i32[2]), p(i32[3]), p(box), p(order), p(table)) == 0
    assert np.all(i32[0][19:] == -7) and np.all(i32[2][39:] == -7) and sorted(order.tolist()) == list(range(20)) and i32[2][0] == -1
    T = ctx.debug_read_binary_tree()
    assert T["n"] == 20 and np.array_equal(T["left"], i32[0][:19]) and np.array_equal(T["parent"], i32[2][:39])
    assert ctx.build_blas(tris) == 2, "the context builds on"


def test_batched_blas_build_refuses_bad_input_and_falls_back_for_other_builders(gpu_ctx_factory):
    """nxhip_build_blas_batch: an empty batch, a mesh without triangles and a null mesh pointer are NXHIP_ERR_INVALID with the
    context untouched; with another builder selected (radix tree, clustering) the meshes are built one by one and still get
    consecutive ids."""
    import ctypes as C

    from nexus_amd import scenegen

    ctx = gpu_ctx_factory(32, 32)
    L = ctx.L  # (status 1 = NXHIP_ERR_INVALID, include/nexus_hip.h)
    a = np.ascontiguousarray(scenegen.random_soup(20, seed=1), dtype=pod.TRI_DT)
    ptrs = (C.c_void_p * 2)(a.ctypes.data, None)
    counts = np.array([20, 5], dtype=np.uint32)
    assert L.nxhip_build_blas_batch(ctx.h, ptrs, counts.ctypes.data, 2, None) == 1      # a null mesh
    ptrs = (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data)
    counts = np.array([20, 0], dtype=np.uint32)
    assert L.nxhip_build_blas_batch(ctx.h, ptrs, counts.ctypes.data, 2, None) == 1      # no triangles
    assert L.nxhip_build_blas_batch(ctx.h, ptrs, counts.ctypes.data, 0, None) == 1      # no meshes
    assert ctx.build_blas(a) == 0, "nothing of the refused calls stayed behind"
    for builder in (0, 8):
        ctx.set_device_builder(builder)
        first = ctx.build_blas_batch([a, a[:9], a[:3]])
        assert first == list(range(first[0], first[0] + 3))
        for bid, n in zip(first, (20, 9, 3)):
            nodes, idx = ctx.read_blas(bid, n)
            assert sorted(idx.tolist()) == list(range(n)) and len(nodes) >= 1
    ctx.set_device_builder(-1)
    ids = ctx.build_blas_batch([a, a[:9], a[:3]])
    trees = ctx.read_blas_batch(ids[0], [20, 9, 3])
    assert [len(t[1]) for t in trees] == [20, 9, 3]
