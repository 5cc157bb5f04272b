"""Detail maps (nxhip_set_material_detail): what the DETAIL instances of the material launch cost on configs[1] when its materials
carry a normal and a roughness map.

  python tools/detail_maps_bench.py [--width 1920 --height 1080] [--steps 16 --warmup 4] [--out profiles/...txt]

One context, three tables in turn — none, a table that names no map (the default instances, as without one), a normal and a roughness
map on every material — and per table: Msamples/s over `steps` one-frame passes and over passes of 8 frames, and the material
launches' time per frame from the in-graph timers (nxhip_read_kernel_times, class shade)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from nexus_amd import capi, pod, workloads  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def rate(ctx, pixels, per_pass):
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
        return pixels * per_pass * args.steps / (time.perf_counter() - t0) / 1e6

    def shade_ms(ctx):
        ctx.set_frames_per_pass(1)
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
        return t["shade"]["ms"] / 4.0

    W, H = args.width, args.height
    sc = workloads.config2(W, H)
    rng = np.random.RandomState(4)
    nmap = np.zeros((256, 256, 4), np.uint8)
    nmap[..., 0:2] = rng.randint(64, 193, (256, 256, 2))
    nmap[..., 2] = rng.randint(200, 256, (256, 256))
    nmap[..., 3] = 255
    rmap = rng.randint(0, 256, (256, 256, 4)).astype(np.uint8)
    ctx = capi.Context(W, H)
    sc.upload(ctx)
    ctx.upload_texture("normal", nmap)
    ctx.upload_texture("roughness", rmap)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    n = len(sc.materials)
    tables = (("no table", []), ("a table that names no map", [pod.make_material_detail()] * n), ("normal + roughness map on every material", [pod.make_material_detail(0, 0, 1.0)] * n))
    say("configs[1]: %d triangles in the TLAS, %d materials, %dx%d, pathLength %d; maps of 256 x 256 random texels" % (sc.triangles, n, W, H, int(sc.settings["pathLength"])))
    for label, table in tables:
        ctx.set_material_detail(np.array(table, dtype=pod.DETAIL_DT) if table else [])
        r1, r8 = rate(ctx, W * H, 1), rate(ctx, W * H, 8)
        flavor = ctx.debug_pass_flavor()
        say("  %-42s %8.1f Msamples/s at one frame per pass, %8.1f at 8; material launches %.3f ms per frame; flavor %#x%s"
            % (label, r1, r8, shade_ms(ctx), flavor, " (DETAIL instances)" if flavor & capi.FLAVOR_DETAIL else ""))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
