"""Fog (nxhip_set_medium): what a medium over the whole scene costs, and how fast its two kernels stream.

  python tools/medium_bench.py [--width 1920 --height 1080] [--steps 16 --warmup 4] [--frames-per-pass 8] [--grid] [--out profiles/...txt]

Per scene (the Cornell box, configs[1]) in one process, without and with a fog box over the scene's bounds grown by 10 %: ms per frame over
`steps` passes; and from one timed replay (in-graph timers, nxhip_read_graph_timeline) the launches of medium_scatter_kernel, of
medium_shadow_kernel and of accumulate_kernel — the project's other pure streaming kernel — with the bytes they move per item and the rate
that makes.  Bytes per ray are the algorithmic ones: scatter 4 B code + 32 B ray for a coded record + 4 B distance, + 16 B path state and the
outputs (48 B continuation, 48 B shadow request, 4 B code) where it scatters; shadow 32 B per request + 32 B where the box is crossed.

--grid (nxhip_set_medium_density): per scene, tests/golden/fog_puff.npy over the same box against homogeneous fog of the grid's mean density
(sigmaT x mean(rho) equal in both): ms per frame, the two kernels' times from a timed replay of each, and the walk's iterations per ray — mean
and maximum of the hook's steps2 over the camera rays of 20 000 pixels, free flight and ratio tracking."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from nexus_amd import capi, pod, workloads  # noqa: E402
from tests import scene_helpers as SH  # noqa: E402


def world_bounds(sc):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst in sc.instances:
        m = np.asarray(inst["transform"], np.float64).reshape(4, 4)
        t = sc.meshes[int(inst["bvhIdx"])]
        p = np.concatenate([t["pos0"], t["pos1"], t["pos2"]]).astype(np.float64)
        w = p @ m[:3, :3].T + m[:3, 3]
        lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
    grow = 0.05 * (hi - lo)
    return lo - grow, hi + grow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--frames-per-pass", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=0.3)
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    W, H, per_pass = args.width, args.height, args.frames_per_pass

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def ms_per_frame(ctx):
        ctx.set_frames_per_pass(per_pass)
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
        return (time.perf_counter() - t0) * 1e3 / (args.steps * per_pass)

    def timeline(ctx, path_length):
        """(scatter ms, shadow ms, accumulate ms per launch) of one timed pass, and that pass's queue sizes"""
        ctx.enable_kernel_timing(True, in_graph=True)
        ctx.reset_frame_number()
        for _ in range(2):
            ctx.render_frame()
            ctx.accumulate()
        tl = ctx.read_graph_timeline()
        acc = ctx.read_kernel_times(reset=True)["accumulate"]
        q = ctx.read_queue_sizes()
        ctx.enable_kernel_timing(False)
        scatter = sum(d for (k, _, d), (k2, _, _) in zip(tl[:-1], tl[1:]) if k == "shade" and k2 == "shade")
        shadow = sum(d for (k, _, d), (k2, _, _) in zip(tl[:-1], tl[1:]) if k == "shade" and k2 == "shadow")
        return scatter, shadow, acc["ms"] / max(1, acc["launches"]), q

    def scene(name, sc, **upload):
        ctx = capi.Context(W, H)
        sc.upload(ctx, **upload)
        ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
        path_length = int(sc.settings["pathLength"])
        lo, hi = world_bounds(sc)
        fog = pod.make_medium(box_min=tuple(lo), box_max=tuple(hi), sigma_t=args.sigma / float((hi - lo).max()) * 3.0, g=0.5, albedo=(0.9, 0.9, 0.9))
        say("%s: %d triangles in the TLAS, %dx%d, pathLength %d, %d frames per pass; fog box %s .. %s, sigmaT %.4g" % (name, sc.triangles, W, H, path_length, per_pass, np.round(lo, 2), np.round(hi, 2), float(fog["sigmaT"])))
        off = ms_per_frame(ctx)
        ctx.set_medium(fog)
        on = ms_per_frame(ctx)
        scatter, shadow, acc_ms, q = timeline(ctx, path_length)
        trace_items = int(np.sum(q["traceSize"][:path_length]))      # records medium_scatter_kernel reads: the queues of bounces 0 .. pathLength - 1
        shadow_items = int(np.sum(q["traceShadowSize"][1:path_length + 1]))
        pixels = W * H
        say("  without fog %.3f ms per frame, with fog %.3f ms per frame (x %.2f); flavor %#x" % (off, on, on / off, ctx.debug_pass_flavor()))
        if scatter > 0 and shadow > 0:
            say("  medium_scatter_kernel: %.3f ms per pass over %d records: at least 40 B per record = %.0f GB/s (a scattering record moves 116 B more)" % (scatter, trace_items, trace_items * 40 / scatter / 1e6))
            say("  medium_shadow_kernel:  %.3f ms per pass over %d requests: 32 B per request (64 B where the box is crossed) = %.0f .. %.0f GB/s" % (shadow, shadow_items, shadow_items * 32 / shadow / 1e6, shadow_items * 64 / shadow / 1e6))
        say("  accumulate_kernel:     %.3f ms per launch over %d pixels x %d frames: %d B per pixel = %.0f GB/s" % (acc_ms, pixels, per_pass, 16 * per_pass + 36, pixels * (16 * per_pass + 36) / max(acc_ms, 1e-9) / 1e6))
        if args.grid:
            rho = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "fog_puff.npy"))
            cloud = fog.copy()
            cloud["sigmaT"] = float(fog["sigmaT"]) / float(rho.mean())
            ctx.set_medium(cloud)
            ctx.set_medium_density(rho)
            on_grid = ms_per_frame(ctx)
            g_scatter, g_shadow, _, _ = timeline(ctx, path_length)
            say("  density grid %s (mean %.4f, max %.4f, sigmaT %.4g: the same mean extinction): %.3f ms per frame (x %.2f of the homogeneous fog, x %.2f of no fog); flavor %#x"
                % ("x".join(str(k) for k in rho.shape[::-1]), rho.mean(), rho.max(), float(cloud["sigmaT"]), on_grid, on_grid / on, on_grid / off, ctx.debug_pass_flavor()))
            if g_scatter > 0 and g_shadow > 0:
                say("  medium_scatter_kernel: homogeneous %.3f ms per pass, grid instance %.3f ms (x %.2f)" % (scatter, g_scatter, g_scatter / max(scatter, 1e-9)))
                say("  medium_shadow_kernel:  homogeneous %.3f ms per pass, grid instance %.3f ms (x %.2f)" % (shadow, g_shadow, g_shadow / max(shadow, 1e-9)))
            cam = sc.camera
            rng = np.random.default_rng(1)
            u, v = rng.uniform(0, 1, 20000), rng.uniform(0, 1, 20000)
            pos = np.asarray(cam["position"], np.float64)
            d = np.asarray(cam["lowerLeftCorner"], np.float64) + np.outer(u, np.asarray(cam["viewportX"], np.float64)) + np.outer(v, np.asarray(cam["viewportY"], np.float64)) - pos
            d /= np.sqrt((d * d).sum(1))[:, None]
            seed = rng.integers(1, 1 << 32, len(d), dtype=np.uint64).astype(np.uint32)
            _, T, steps = ctx.medium_track_batch(np.broadcast_to(pos, d.shape), d, np.full(len(d), np.inf), seed)
            cross = steps[:, 0] > 0
            for name, w in (("free flight", steps[cross, 0]), ("ratio tracking", steps[cross, 1])):
                it, co = w & 0xffff, w >> 16
                say("  walk, %s: %d of %d camera rays cross the box; iterations per ray mean %.2f, max %d; tentative collisions mean %.2f, max %d"
                    % (name, cross.sum(), len(d), it.mean(), it.max(), co.mean(), co.max()))
            say("  mean transmittance of those rays %.4f" % float(T[cross].mean()))
        ctx.close()

    scene("Cornell box", SH.cornell_scene(W, H, path_length=4))
    scene("configs[1]", workloads.config2(W, H))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
