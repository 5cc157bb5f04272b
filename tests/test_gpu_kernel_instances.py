"""Compile-time kernel instances picked by what the scene lets them leave out (nxhip_render.hip pass_flavor): the trace launches of a
scene whose instances all carry the identity are the IDENTITY instances (nx_trace.hip), the SCAN pipeline's material launch of a context
whose materials name no map is the map-free one (nx_wavefront.hip).  Neither changes any arithmetic of an executed path, so every
comparison here is bit for bit: the specialised instances against the general ones on the same scene (nxhip_debug_pass_flavor forces
the general ones), and a live context after a change that ends the property against a fresh one given the changed scene from the start.
The hook also says which instances the last pass really ran, so "equal" cannot mean "the general ones both times"."""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen, workloads
from tests import oracle_lib as O
from tests import scene_helpers as SH

pytestmark = pytest.mark.gpu

ID, NM = capi.FLAVOR_IDENTITY, capi.FLAVOR_NO_MAPS
SCAN = (pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)          # one material launch per bounce (shade_scan_kernel)
CLASSIC = (pod.RNG_REFERENCE_SLOT, pod.COMPACT_ORDERED, pod.CONDUCTOR_EXTENDED)  # logic kernel + one material kernel per type
_CACHE = {}


def _box(lo, hi):
    """axis-aligned box, 12 triangles, faces outward"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    q = scenegen.quad
    return np.concatenate([
        q((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)), q((x1, y0, z0), (x0, y0, z0), (x0, y1, z0), (x1, y1, z0)),
        q((x1, y0, z1), (x1, y0, z0), (x1, y1, z0), (x1, y1, z1)), q((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)),
        q((x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (x0, y1, z0)), q((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1))])


def _materials(diffuse_map=-1, emissive_map=-1):
    return np.array([
        pod.make_material(pod.MAT_DIFFUSE, albedo=(0.7, 0.7, 0.7), diffuse_map=diffuse_map),
        pod.make_material(pod.MAT_PLASTIC, albedo=(0.8, 0.3, 0.2), roughness=0.4, ior=1.5),
        pod.make_material(pod.MAT_DIELECTRIC, albedo=(0.95, 0.97, 1.0), roughness=0.2, ior=1.45),
        pod.make_material(pod.MAT_CONDUCTOR, roughness=0.3),
        pod.make_material(pod.MAT_DIFFUSE, albedo=(0.8, 0.8, 0.8), emissive=(1.0, 0.9, 0.8), intensity=15.0, emissive_map=emissive_map),
    ], dtype=pod.MAT_DT)


def _zoo(W, H, background=0.0, placements=None, materials=None, diffuse_maps=(), emissive_maps=(), axis_view=False, path_length=4, mesh1=None):
    """All four material types and a mesh light, every mesh in world coordinates under the identity: a floor, three displaced tori, an
    axis-aligned box and a light quad.  axis_view: the camera ON the z axis (origin components +0 and -0), looking down it at the box —
    no primary ray is "ordinary" (nx_traverse.h ray_is_ordinary), and at odd resolutions the centre pixel's direction has zeros too."""
    meshes = [scenegen.quad((-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4)),
              scenegen.displaced_torus(40, 20, seed=4, major=0.5, minor=0.22, center=(-1.3, 0.5, 0.0)),
              scenegen.displaced_torus(36, 18, seed=5, major=0.45, minor=0.2, center=(1.3, 0.5, -0.2)),
              scenegen.displaced_torus(32, 16, seed=6, major=0.4, minor=0.18, center=(0.0, 0.45, 1.2)),
              _box((-0.5, 0.0, -0.5), (0.5, 1.0, 0.5)),
              scenegen.quad((-0.8, 3.0, -0.8), (0.8, 3.0, -0.8), (0.8, 3.0, 0.8), (-0.8, 3.0, 0.8))]
    if mesh1 is not None:
        meshes[1] = mesh1
    mat_of = [0, 1, 2, 3, 0, 4]
    if placements is None:
        placements = [(i, mat_of[i], workloads.IDENTITY) for i in range(len(meshes))]
    if axis_view:
        cam = capi.camera_init((0.0, -0.0, 5.0), (0.0, 0.0, -1.0), 40.0, W, H, 5.0, 0.0)
    else:
        fwd = np.array((0.0, -0.25, -0.97))
        cam = capi.camera_init((0.1, 1.7, 4.6), fwd / np.linalg.norm(fwd), 50.0, W, H, 5.0, 0.0)
    settings = O.make_settings(use_mis=True, path_length=path_length, background=(0.6, 0.7, 0.9), background_intensity=background)
    sc = SH.BuiltScene(meshes, placements, materials=materials if materials is not None else _materials(), camera=cam, settings=settings,
                       diffuse_maps=diffuse_maps, emissive_maps=emissive_maps)
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    return sc


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _ctx(factory, scene, modes=SCAN, entry=False, per_pass=2, thin=False, tail_off=True):
    w, h = int(scene.camera["resolution"][0]), int(scene.camera["resolution"][1])
    ctx = factory(w, h)
    scene.upload(ctx)
    ctx.set_modes(*modes)
    ctx.set_frames_per_pass(per_pass)
    ctx.set_entry_points(entry)
    if tail_off:
        ctx.set_tail_bounce(0)  # (every bounce through the level-by-level launches the instances belong to)
    if thin:
        ctx.debug_set_thin(64, 0)  # every ray of a dry wave goes to the thin kernel, from its first iteration on
    return ctx


def _render(ctx, passes=2, radiance=True):
    """`passes` passes from frame 0: what a caller can read afterwards, as bits; and the flavor of the graph the last pass replayed"""
    ctx.reset_frame_number()
    out = []
    for _ in range(passes):
        ctx.render_frame()
        ctx.accumulate()
        if radiance:
            out.append(ctx.read_radiance().view(np.uint32).copy())
    out.append(ctx.read_accumulation().view(np.uint32).copy())
    out.append(ctx.read_rgba8().copy())
    return out, ctx.read_queue_sizes(), ctx.debug_pass_flavor()


def _equal(a, b, slots=None):
    ok = len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    if not ok:
        print("images differ: %s" % [int((x != y).sum()) if x.shape == y.shape else -1 for x, y in zip(a[0], b[0])])
    return SH.queue_sizes_identical(a[1], b[1], slots) and ok


def _both(ctx, want_flavor, **kw):
    """the pass with the specialised instances (which must be the ones `want_flavor` names), then with the general ones forced"""
    ctx.debug_pass_flavor(force_general=0)
    spec = _render(ctx, **kw)
    assert spec[2] & (ID | NM) == want_flavor, "flavor %#x" % spec[2]
    ctx.debug_pass_flavor(force_general=ID | NM)
    gen = _render(ctx, **kw)
    assert gen[2] & (ID | NM) == 0, "flavor %#x with the general instances forced" % gen[2]
    assert spec[2] & ~(ID | NM) == gen[2] & ~(ID | NM), "nothing else of the pass's shape follows the hook"
    ctx.debug_pass_flavor(force_general=0)
    return spec, gen


# ---- identity scenes: the IDENTITY trace instances against the general ones -------------------------------------------------------

@pytest.mark.parametrize("thin", [False, True], ids=["", "thin"])
@pytest.mark.parametrize("entry", [False, True], ids=["root", "entry"])
@pytest.mark.parametrize("modes", [SCAN, CLASSIC], ids=["scan", "classic"])
def test_identity_scene_specialised_equals_general(gpu_ctx_factory, modes, entry, thin):
    for axis in (False, True):
        scene = _cached(("zoo", axis), lambda: _zoo(65 if axis else 96, 65 if axis else 64, axis_view=axis))
        ctx = _ctx(gpu_ctx_factory, scene, modes, entry, thin=thin)
        spec, gen = _both(ctx, ID | (NM if modes is SCAN else 0))
        assert _equal(spec, gen), "axis view" if axis else "free view"
        assert np.any(spec[0][-2] != 0), "the image is not black"
        if thin and modes is SCAN:
            assert sum(ctx.debug_thin_counts_of_pass(0)) > 0, "the thin kernel had rays"
        ctx.close()


def test_axis_view_rays_are_not_ordinary_and_match_the_oracle(gpu_ctx_factory):
    """The non-ordinary branch inside the IDENTITY instances: every primary ray of the axis view starts at (+0, -0, 5).  Hit records of
    such rays (the camera's, and axis-parallel ones with +-0 direction components) against the oracle; two frames of the pass against
    the oracle's wavefront, bit for bit, with the specialised instances."""
    W = H = 65
    scene = _cached(("zoo", True), lambda: _zoo(W, H, axis_view=True))
    assert np.signbit(scene.camera["position"][1]) and scene.camera["position"][0] == 0.0 and not np.signbit(scene.camera["position"][0])
    rays = workloads.pixel_centre_rays(scene.camera, W, H)
    centre = rays["direction"][(H // 2) * W + W // 2]
    assert centre[0] == 0.0 and centre[1] == 0.0, "the centre pixel looks exactly down the axis"
    axis = np.zeros(6, dtype=pod.RAY_DT)
    axis["origin"] = [(0.0, -0.0, 5.0), (-0.0, 0.5, 5.0), (5.0, 0.5, -0.0), (-5.0, 0.5, 0.0), (0.0, 5.0, -0.0), (0.25, 0.5, 5.0)]
    axis["direction"] = [(0.0, -0.0, -1.0), (-0.0, 0.0, -1.0), (-1.0, 0.0, -0.0), (1.0, -0.0, 0.0), (-0.0, -1.0, 0.0), (0.0, 0.0, -1.0)]
    rays = np.concatenate([rays, axis])
    orc = scene.oracle()
    ctx = _ctx(gpu_ctx_factory, scene, (pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE), entry=True, per_pass=1, tail_off=True)
    got = ctx.trace_batch(rays)
    assert SH.hit_records_equal(got, orc.trace_closest(rays))
    assert (got["hitDistance"] < pod.MISS_DISTANCE).mean() > 0.1, "the view sees the box and the tori (18 % of the frame)"
    ctx.reset_frame_number()
    w = O.Wavefront(orc, W * H, None, pod.RNG_PIXEL_KEYED, pod.CONDUCTOR_REFERENCE)
    for f in (1, 2):
        ctx.render_frame()
        ctx.accumulate()
        w.render(f)
        w.accumulate(f)
    assert ctx.debug_pass_flavor() & (ID | NM) == ID | NM
    assert SH.frames_identical(ctx.read_radiance(), w.radiance(), "axis view, frame 2")
    assert np.array_equal(ctx.read_rgba8(), w.rgba8())
    ctx.close()


def test_ray_batches_do_not_depend_on_the_flavor(gpu_ctx_factory):
    """The ray-batch hooks keep the run-time flag, so this does not run the IDENTITY instances (the image and queue-size comparisons
    do): it pins that a hook's records equal the oracle's whichever instances the passes around it ran."""
    scene = _cached(("zoo", False), lambda: _zoo(96, 64))
    rays = scenegen.interior_rays(20000, seed=7, extent=2.0)
    rays["origin"][:, 1] += 1.0
    ctx = _ctx(gpu_ctx_factory, scene)
    _render(ctx, 1)
    a = ctx.trace_batch(rays)
    ctx.debug_pass_flavor(force_general=ID | NM)
    _render(ctx, 1)
    b = ctx.trace_batch(rays)
    assert SH.hit_records_equal(a, b) and SH.hit_records_equal(a, scene.oracle().trace_closest(rays))
    ctx.close()


# ---- the flavor follows the scene -------------------------------------------------------------------------------------------------

ROTATION = capi.mat4_from_trs((0.15, 0.3, -0.1), (20.0, 35.0, 10.0), (1.0, 1.0, 1.0))


def _placed(k, xf):
    mat_of = [0, 1, 2, 3, 0, 4]
    return [(i, mat_of[i], xf if i == k else workloads.IDENTITY) for i in range(6)]


@pytest.mark.parametrize("entry", [False, True], ids=["root", "entry"])
def test_a_rotated_instance_ends_the_identity_flavor(gpu_ctx_factory, entry):
    scene = _cached(("zoo", False), lambda: _zoo(96, 64))
    ctx = _ctx(gpu_ctx_factory, scene, entry=entry)
    before = _render(ctx)
    assert before[2] & (ID | NM) == ID | NM
    ctx.set_instance_transforms(np.array([4], np.uint32), ROTATION.reshape(1, 16))
    got = _render(ctx)
    assert got[2] & (ID | NM) == NM, "the general trace instances, the map-free material launch still"
    fresh = _ctx(gpu_ctx_factory, _cached(("zoo", "rotated"), lambda: _zoo(96, 64, placements=_placed(4, ROTATION))), entry=entry)
    want = _render(fresh)
    assert want[2] & (ID | NM) == NM
    assert _equal(got, want) and not _equal(before, got)
    # ... and back: every matrix the identity itself again
    ctx.set_instance_transforms(np.array([4], np.uint32), workloads.IDENTITY.reshape(1, 16))
    again = _render(ctx)
    assert again[2] & ID == 0, "the scene-wide flag is only ever set by an instance upload"
    assert _equal(again, before)
    ctx.close()
    fresh.close()


def test_device_built_scene_refit_and_moved_instance(gpu_ctx_factory):
    """Device-built BLASes and TLAS; a BLAS refitted on the device (the deferred refresh of its instances' records leaves every matrix
    alone: the flavor stays, and so does the equality with the general instances); then the device-side refit path moves an instance:
    the general trace instances, and the image of a fresh context whose device-built scene had the refitted mesh and the moved instance from
    the start."""
    scene = _cached(("zoo", False), lambda: _zoo(96, 64))
    ctx = gpu_ctx_factory(96, 64)
    scene.upload(ctx, device_bvh=True, device_tlas=True)
    ctx.set_modes(*SCAN)
    ctx.set_frames_per_pass(2)
    ctx.set_entry_points(True)
    ctx.set_tail_bounce(0)
    spec, gen = _both(ctx, ID | NM)
    assert _equal(spec, gen)
    moved = scene.meshes[1].copy()
    for k in ("pos0", "pos1", "pos2"):
        moved[k] = ((moved[k] - np.float32((-1.3, 0.5, 0.0))) * np.float32(1.15) + np.float32((-1.3, 0.55, 0.0))).astype(np.float32)
    ctx.update_blas(1, moved)
    spec2, gen2 = _both(ctx, ID | NM)
    assert _equal(spec2, gen2) and not _equal(spec, spec2)
    scale = capi.mat4_from_trs((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.2, 0.9, 1.1))
    ctx.set_instance_transforms(np.array([2], np.uint32), scale.reshape(1, 16))
    after = _render(ctx)
    assert after[2] & (ID | NM) == NM and not _equal(after, spec2)
    fresh = gpu_ctx_factory(96, 64)
    _zoo(96, 64, placements=_placed(2, scale), mesh1=moved).upload(fresh, device_bvh=True, device_tlas=True)
    fresh.set_modes(*SCAN)
    fresh.set_frames_per_pass(2)
    fresh.set_entry_points(True)
    fresh.set_tail_bounce(0)
    want = _render(fresh)
    assert want[2] & (ID | NM) == NM
    assert _equal(after, want), "stale boxes or instance records after the switch to the general instances render another image"
    ctx.close()
    fresh.close()


@pytest.mark.parametrize("which", ["diffuse", "emissive"])
def test_a_material_that_names_a_map_ends_the_map_free_flavor(gpu_ctx_factory, which):
    scene = _cached(("zoo", False), lambda: _zoo(96, 64))
    tex = SH.checker_texture(64, 32, 1, alpha=True) if which == "diffuse" else SH.checker_texture(32, 32, 2)
    ctx = _ctx(gpu_ctx_factory, scene)
    before = _render(ctx)
    assert before[2] & (ID | NM) == ID | NM
    # an uploaded texture no material names changes nothing: the fact is the material table's
    assert ctx.upload_texture(which, tex) == 0
    same = _render(ctx)
    assert same[2] & (ID | NM) == ID | NM and _equal(same, before)
    mats = _materials(diffuse_map=0) if which == "diffuse" else _materials(emissive_map=0)
    ctx.set_materials(mats)
    got = _render(ctx)
    assert got[2] & (ID | NM) == ID, "the general material launch, the identity trace instances still"
    mapped = _cached(("zoo", which), lambda: _zoo(96, 64, materials=mats, **{which + "_maps": [tex]}))
    fresh = _ctx(gpu_ctx_factory, mapped)
    want = _render(fresh)
    assert want[2] & (ID | NM) == ID
    assert _equal(got, want) and not _equal(before, got)
    # ... and the table without maps again: the map-free launch again, the first image again
    ctx.set_materials(_materials())
    again = _render(ctx)
    assert again[2] & (ID | NM) == ID | NM and _equal(again, before)
    ctx.close()
    fresh.close()


def test_an_environment_map_keeps_the_general_material_launch(gpu_ctx_factory):
    """(the map-free instance measured slower than the general one where the environment's light sample and miss type run)"""
    scene = _cached(("zoo", "bg", 0.5), lambda: _zoo(96, 64, background=0.5))
    ctx = _ctx(gpu_ctx_factory, scene)
    before = _render(ctx)
    assert before[2] & (ID | NM) == ID | NM
    ctx.upload_texture("hdr", SH.checker_texture(128, 64, 3))
    spec, gen = _both(ctx, ID)
    assert _equal(spec, gen) and not _equal(spec, before)
    ctx.close()


def test_counting_variants_and_classic_pipeline_have_no_specialised_material_launch(gpu_ctx_factory):
    scene = _cached(("zoo", False), lambda: _zoo(96, 64))
    ctx = _ctx(gpu_ctx_factory, scene, CLASSIC)
    assert _render(ctx, 1)[2] & (ID | NM) == ID
    ctx.enable_trace_stats(True)
    assert _render(ctx, 1)[2] & (ID | NM) == 0, "the counting trace kernels keep the run-time flag"
    ctx.enable_trace_stats(False)
    with pytest.raises(capi.NexusError):
        ctx.debug_pass_flavor(force_general=1)
    ctx.close()


# ---- map-free material launch against the general one ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["uniform", "power", "background"])
def test_map_free_material_launch_equals_general(gpu_ctx_factory, case):
    """all four material types + a mesh light; NXHIP_LIGHTS_POWER (the POWER instances); a flat background that is not black (misses
    contribute: the miss type runs inside the map-free launch)"""
    bg = 0.5 if case == "background" else 0.0
    scene = _cached(("zoo", "bg", bg), lambda: _zoo(96, 64, background=bg))
    ctx = _ctx(gpu_ctx_factory, scene, per_pass=3)
    ctx.set_light_sampling(pod.LIGHTS_POWER if case == "power" else pod.LIGHTS_UNIFORM)
    spec, gen = _both(ctx, ID | NM)
    assert _equal(spec, gen)
    q = spec[1]
    assert all(q[k][1] > 0 for k in ("diffuseSize", "plasticSize", "dielectricSize", "conductorSize")), "every type shaded something"
    assert q["traceShadowSize"][1] > 0
    # only the material launch differs: identity forced general alone, maps forced general alone
    ctx.debug_pass_flavor(force_general=ID)
    only_maps = _render(ctx)
    ctx.debug_pass_flavor(force_general=NM)
    only_identity = _render(ctx)
    assert only_maps[2] & (ID | NM) == NM and only_identity[2] & (ID | NM) == ID
    assert _equal(only_maps, gen) and _equal(only_identity, gen)
    ctx.close()


def test_one_frame_pass_with_a_partial_last_tile(gpu_ctx_factory):
    """65 x 3 pixels, one frame per pass: 195 rays — one partially filled tile of the material launch's one-ray-per-thread scan —
    with the tail kernel off (every bounce a material launch) and on (the automatic choice for one-frame passes)."""
    scene = _cached(("zoo", "65x3"), lambda: _zoo(65, 3))
    for tail_off in (True, False):
        ctx = _ctx(gpu_ctx_factory, scene, per_pass=1, tail_off=tail_off)
        spec, gen = _both(ctx, ID | NM, passes=3)
        assert _equal(spec, gen) and spec[1]["traceSize"][0] == 195
        ctx.close()


def test_large_pass_takes_the_four_rays_per_thread_scan(gpu_ctx_factory):
    """The material launch reads four hit codes per thread while that still gives every starting workgroup four tiles: at 10 workgroups
    per CU on 256 CUs, 320 ranks per region over four types, from 4 x 1 024 x 80 = 327 680 rays per region on.  129 x 127 pixels x 200
    frames in one pass = 409 575 per region at bounce 1 (an odd count: the last tile is partial); the late bounces fall below the
    threshold and take the one-ray-per-thread scan in the same pass."""
    scene = _cached(("zoo", "129x127"), lambda: _zoo(129, 127))
    ctx = _ctx(gpu_ctx_factory, scene, per_pass=200)
    spec, gen = _both(ctx, ID | NM, passes=1, radiance=False)
    assert _equal(spec, gen)
    sizes = spec[1]["traceSize"]
    assert sizes[0] == 129 * 127 * 200 and sizes[0] // 8 >= 327680, "bounce 1: four rays per thread"
    assert 0 < sizes[3] // 8 < 327680, "bounce 4: one ray per thread"
    ctx.close()
