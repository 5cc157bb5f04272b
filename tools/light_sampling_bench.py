"""Light sampling by emitted power and by position (nxhip_set_light_sampling, nxhip_set_light_importance): what the modes cost and what
the table and the tree cost to build.

  python tools/light_sampling_bench.py [--width 3840 --height 2160 --path-length 16] [--steps 16 --warmup 4] [--out profiles/...txt]

bench.py has no light-sampling option; this tool times the same pass of configs[4] (workloads.config5: several emissive materials,
textured panels) in the three modes — uniform, power, power by position — in one process; --hall adds a hall of 256 small panels
(1920 x 1080, 8 bounces: Msamples/s and the mean squared error at equal render time):
  * Msamples/s over --steps frames after --warmup, one frame per pass, pixel-keyed random numbers, device-built BVHs, entry points —
    bench.py --config 5's settings;
  * the material launches' time per frame (nxhip_read_kernel_times, event nodes inside the pass graph), in a second short run;
  * the table build for the scene's emissive triangles: wall clock from the mode switch that marks it stale to the end of the stream,
    median of 10 (launch overhead and one host synchronisation included);
  * the same for a deforming emissive mesh of 1 M triangles (displaced torus, nxhip_update_blas_device + rebuilt table), against the
    update alone; and the mean of a 4096 x 4096 emissive map, which rides on the first build after its upload.  torch provides the device tensor; it must initialise the GPU before the library does."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nexus_amd import capi, pod, scenegen, workloads  # noqa: E402

MODES = (("uniform", pod.LIGHTS_UNIFORM, pod.LIGHT_IMPORTANCE_POWER), ("power", pod.LIGHTS_POWER, pod.LIGHT_IMPORTANCE_POWER),
         ("position", pod.LIGHTS_POWER, pod.LIGHT_IMPORTANCE_POSITION))


def table_now(ctx):
    """brings the light table up to date (no destinations: nothing is read back), then waits for the stream"""
    capi.check(ctx.L.nxhip_read_light_table(ctx.h, None, None, 0, None, None), "nxhip_read_light_table")
    ctx.sync()


def set_mode(ctx, mode, importance):
    ctx.set_light_sampling(mode)
    ctx.set_light_importance(importance)


def hall_scene(W, H, path_length, side=16):
    """a hall of side x side small ceiling panels (0.3 x 0.3, 2 apart, height 3) over a diffuse floor with a few objects: every floor
    point is near one or two panels and far from all the others"""
    span = 2.0 * side
    floor = scenegen.quad((-1, 0, -1), (-1, 0, span), (span, 0, span), (span, 0, -1))
    panel = scenegen.quad((-0.15, 0, -0.15), (0.15, 0, -0.15), (0.15, 0, 0.15), (-0.15, 0, 0.15))
    prop = scenegen.displaced_torus(48, 24, seed=4, major=0.5, minor=0.2, amp=0.03)
    mats = np.array([pod.make_material(pod.MAT_DIFFUSE, albedo=(0.7, 0.7, 0.7)),
                     pod.make_material(pod.MAT_DIFFUSE, albedo=(0.0, 0.0, 0.0), emissive=(1.0, 0.9, 0.8), intensity=40.0),
                     pod.make_material(pod.MAT_PLASTIC, albedo=(0.3, 0.6, 0.8), roughness=0.3, ior=1.5)], dtype=pod.MAT_DT)
    placements = [(0, 0, workloads.IDENTITY)]
    placements += [(1, 1, capi.mat4_from_trs((2.0 * i + 0.5, 3.0, 2.0 * j + 0.5), (0, 0, 0), (1, 1, 1))) for i in range(side) for j in range(side)]
    rng = np.random.RandomState(2)
    placements += [(2, 2, capi.mat4_from_trs((rng.uniform(0, span - 2), 0.3, rng.uniform(0, span - 2)), tuple(rng.uniform(0, 90, 3)), (1, 1, 1))) for _ in range(24)]
    eye = np.array((span / 2, 2.2, span + 4.0))
    fwd = np.array((span / 2, 0.5, span / 2)) - eye
    cam = capi.camera_init(tuple(eye), tuple(fwd / np.linalg.norm(fwd)), 60.0, W, H, 5.0, 0.0)
    sc = workloads.Workload([floor, panel, prop], placements, materials=mats, camera=cam,
                            settings=workloads.make_settings(use_mis=True, path_length=path_length, background=(1, 1, 1), background_intensity=0.0))
    sc.lights = workloads.mesh_lights(sc.instances, sc.materials)
    return sc


def hall(say, W, H, path_length, seconds, ref_frames):
    """Msamples/s in the three modes, and the mean squared error against a long reference at EQUAL RENDER TIME in POWER and POSITION"""
    sc = hall_scene(W, H, path_length)
    say("hall: %d panels (%d entries), %dx%d, pathLength %d, four frames per pass" % (len(sc.lights), 2 * len(sc.lights), W, H, path_length))
    ctx = capi.Context(W, H)
    sc.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    ctx.set_frames_per_pass(4)
    set_mode(ctx, pod.LIGHTS_POWER, pod.LIGHT_IMPORTANCE_POSITION)
    ctx.reset_frame_number()  # (the accumulation is a running mean by frame number: the reference is frames 1 .. ref_frames)
    for _ in range(ref_frames // 8):
        ctx.render_frame()
        ctx.accumulate()
    set_mode(ctx, pod.LIGHTS_POWER, pod.LIGHT_IMPORTANCE_POWER)  # (half of it in each mode: neither estimate is compared with itself)
    for _ in range(ref_frames // 8):
        ctx.render_frame()
        ctx.accumulate()
    ref = ctx.read_accumulation().astype(np.float64)
    for name, mode, importance in MODES:
        set_mode(ctx, mode, importance)
        ctx.set_frame_number(1 << 20)  # frames of the estimate's own (pixel-keyed numbers), summed on the host from the passes' radiance
        ctx.render_frame()  # (graph and table)
        ctx.sync()
        frames, spent, total = 0, 0.0, np.zeros((W * H, 3), np.float64)
        while spent < seconds:
            t0 = time.perf_counter()
            ctx.render_frame()
            ctx.sync()
            spent += time.perf_counter() - t0  # (render time alone: the read-back below is the measurement's, not the renderer's)
            total += ctx.read_radiance().reshape(4, W * H, 3).astype(np.float64).sum(axis=0)
            frames += 4
        est = total / frames
        say("  %-8s %8.1f Msamples/s; %4d frames in %.3f s of render time: mean squared error against %d reference frames %.6g (mean of the image %.5f, of the reference %.5f)" % (
            name, W * H * frames / spent / 1e6, frames, spent, ref_frames, float(((est - ref) ** 2).mean()), float(est.mean()), float(ref.mean())))
    ctx.close()
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--path-length", type=int, default=16)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--deform-nu", type=int, default=1024)
    ap.add_argument("--deform-nv", type=int, default=512)
    ap.add_argument("--map-size", type=int, default=4096, help="side of the emissive map whose mean is timed")
    ap.add_argument("--skip-config", action="store_true", help="only the 1 M-triangle table")
    ap.add_argument("--skip-deform", action="store_true", help="not the 1 M-triangle table")
    ap.add_argument("--hall", action="store_true", help="also the many-lights hall: 256 panels, 1920x1080, 8 bounces")
    ap.add_argument("--hall-seconds", type=float, default=0.1, help="render time of each mode's estimate (far shorter than the reference, whose own noise the error must not be)")
    ap.add_argument("--hall-reference-frames", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    torch.cuda.set_device(0)
    med = statistics.median
    if not args.skip_config:
        W, H = args.width, args.height
        sc = workloads.config5(W, H, args.path_length)
        emissive = sum(len(sc.meshes[int(sc.instances[int(l["meshId"])]["bvhIdx"])]) for l in sc.lights)
        say("configs[4]: %d triangles in the TLAS, %d lights with %d emissive triangles, %dx%d, pathLength %d, one frame per pass" % (
            sc.triangles, len(sc.lights), emissive, W, H, args.path_length))
        ctx = capi.Context(W, H)
        sc.upload(ctx, device_bvh=True, device_tlas=True)
        ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
        ctx.set_pixel_order(pod.ORDER_TILES)
        ctx.set_entry_points(True)
        ctx.set_frames_per_pass(1)
        for name, mode, importance in MODES:
            set_mode(ctx, mode, importance)
            ctx.reset_frame_number()
            for _ in range(args.warmup):
                ctx.render_frame()
                ctx.accumulate()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ctx.render_frame()
                ctx.accumulate()
            ctx.sync()
            dt = time.perf_counter() - t0
            say("  %-8s %8.1f Msamples/s   (%d frames in %.1f ms; mean of the image %.5f)" % (name, W * H * args.steps / dt / 1e6, args.steps, dt * 1e3, float(ctx.read_accumulation().mean())))
        for name, mode, importance in MODES:
            set_mode(ctx, mode, importance)
            ctx.enable_kernel_timing(True, in_graph=True)
            ctx.reset_frame_number()
            ctx.render_frame()
            ctx.accumulate()
            ctx.read_kernel_times(reset=True)
            for _ in range(4):
                ctx.render_frame()
                ctx.accumulate()
            t = ctx.read_kernel_times(reset=True)
            ctx.enable_kernel_timing(False)
            say("  %-8s material launches %8.3f ms per frame (%d launches), trace %.3f, shadow trace %.3f" % (
                name, t["shade"]["ms"] / 4, t["shade"]["launches"] // 4, t["trace"]["ms"] / 4, t["shadow"]["ms"] / 4))
        for what, importance in (("table build", pod.LIGHT_IMPORTANCE_POWER), ("table + tree build", pod.LIGHT_IMPORTANCE_POSITION)):
            set_mode(ctx, pod.LIGHTS_POWER, importance)
            table_now(ctx)
            builds = []
            for _ in range(10):
                ctx.set_light_sampling(pod.LIGHTS_UNIFORM)
                t0 = time.perf_counter()
                ctx.set_light_sampling(pod.LIGHTS_POWER)  # (marks the table stale; the buffers stay)
                table_now(ctx)
                builds.append((time.perf_counter() - t0) * 1e3)
            say("  %s, %d entries: median of 10 %.3f ms wall (min %.3f)" % (what, emissive, med(builds), min(builds)))
        ctx.close()
        say()

    if args.hall:
        hall(say, 1920, 1080, 8, args.hall_seconds, args.hall_reference_frames)
    if args.skip_deform:
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return

    # ---- a deforming emissive mesh
    nu, nv = args.deform_nu, args.deform_nv
    shapes = [scenegen.displaced_torus(nu, nv, seed=1, major=1.0, minor=0.45, amp=a, center=(0.0, 1.5, 0.0)) for a in (0.06, 0.12)]
    n = len(shapes[0])
    floor = scenegen.quad((-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6))
    ident = np.eye(4, dtype=np.float32).reshape(16)
    side = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(side)
    ctx = capi.Context(256, 256, stream=side.cuda_stream)
    ctx.set_materials(np.array([pod.make_material(), pod.make_material(emissive=(1.0, 0.8, 0.6), intensity=3.0)], dtype=pod.MAT_DT))
    ids = [ctx.build_blas(floor), ctx.build_blas(shapes[0])]
    insts = np.array([capi.instance_init(ids[0], 0, ident, ctx.read_blas(ids[0], len(floor))[0][0]),
                      capi.instance_init(ids[1], 1, ident, ctx.read_blas(ids[1], n)[0][0])], dtype=pod.INST_DT)
    ctx.rebuild_tlas(insts)
    lights = np.zeros(1, pod.LIGHT_DT)
    lights["meshId"], lights["type"] = 1, pod.LIGHT_MESH
    ctx.set_lights(lights)
    ctx.set_camera(capi.camera_init((0.0, 1.5, 6.0), (0.0, 0.0, -1.0), 50.0, 256, 256, 5.0, 0.0))
    ctx.set_render_settings(workloads.make_settings())
    ctx.set_light_sampling(pod.LIGHTS_POWER)
    dev = [torch.from_numpy(np.frombuffer(s.tobytes(), dtype=np.uint8).copy()).to("cuda") for s in shapes]
    torch.cuda.synchronize()
    ctx.update_blas_device(ids[1], dev[1].data_ptr(), n)  # first update: the refit plan
    table_now(ctx)
    both, alone, table = [], [], []
    for k in range(10):
        t0 = time.perf_counter()
        ctx.update_blas_device(ids[1], dev[k % 2].data_ptr(), n)
        table_now(ctx)
        both.append((time.perf_counter() - t0) * 1e3)
    for k in range(10):
        ctx.set_light_sampling(pod.LIGHTS_UNIFORM)
        t0 = time.perf_counter()
        ctx.update_blas_device(ids[1], dev[k % 2].data_ptr(), n)
        capi.check(ctx.L.nxhip_read_tlas(ctx.h, None, 0, None, 0), "nxhip_read_tlas")  # (the deferred refresh of bounds and TLAS, as above)
        ctx.sync()
        alone.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ctx.set_light_sampling(pod.LIGHTS_POWER)
        table_now(ctx)
        table.append((time.perf_counter() - t0) * 1e3)
    say("deforming emissive mesh, %d triangles (guide of %d entries), wall clock, medians of 10:" % (n, 1 << int(np.ceil(np.log2(n)))))
    say("  nxhip_update_blas_device + refresh + light table  %.3f ms" % med(both))
    say("  nxhip_update_blas_device + refresh alone          %.3f ms" % med(alone))
    say("  the light table alone                             %.3f ms (min %.3f)" % (med(table), min(table)))
    ctx.set_light_importance(pod.LIGHT_IMPORTANCE_POSITION)
    table_now(ctx)
    tree = []
    for k in range(10):
        ctx.set_light_sampling(pod.LIGHTS_UNIFORM)
        t0 = time.perf_counter()
        ctx.set_light_sampling(pod.LIGHTS_POWER)
        table_now(ctx)
        tree.append((time.perf_counter() - t0) * 1e3)
    ctx.set_light_importance(pod.LIGHT_IMPORTANCE_POWER)
    say("  the light table and the light tree                %.3f ms (min %.3f)" % (med(tree), min(tree)))
    # the mean of an emissive map (light_map_mean_kernel: one workgroup per map, once per uploaded map) rides on the first build after
    # the upload
    side_len = args.map_size
    img = np.full((side_len, side_len, 4), 255, np.uint8)
    img[..., :3] = (np.arange(side_len * side_len, dtype=np.uint32).reshape(side_len, side_len, 1) * np.array([1, 3, 7], np.uint32) >> 4).astype(np.uint8)
    with_mean = []
    for _ in range(3):
        ctx.upload_texture("emissive", img)  # (marks the table stale; its mean is due)
        t0 = time.perf_counter()
        table_now(ctx)
        with_mean.append((time.perf_counter() - t0) * 1e3)
    say("  the light table right after a %d x %d emissive map was uploaded (its mean included): fastest of 3 %.3f ms -> the mean: about %.3f ms" % (
        side_len, side_len, min(with_mean), min(with_mean) - med(table)))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
