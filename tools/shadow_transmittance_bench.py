"""Transparent shadows (nxhip_set_shadow_transmittance): what the mode costs on scenes that have see-through materials, and what its two
restrictions (no any-hit hand-over to the thin kernel, no tail kernel) would cost on a scene that has none.

  python tools/shadow_transmittance_bench.py [--width 1920 --height 1080] [--steps 16 --warmup 4] [--skip-config5] [--out profiles/...txt]

Per scene and mode in one process: Msamples/s over `steps` one-frame passes and over passes of 8 frames, and the any-hit launches' time per
frame from the in-graph timers (nxhip_read_kernel_times, class shadow)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from nexus_amd import capi, pod, workloads  # noqa: E402
from tests import scene_helpers as SH  # noqa: E402

MODES = (("opaque", pod.SHADOWS_OPAQUE), ("transmit", pod.SHADOWS_TRANSMIT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--skip-config5", action="store_true")
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

    def kernel_ms(ctx):
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
        return {k: t[k]["ms"] / 4.0 for k in ("trace", "shadow", "thin", "shade")}

    def modes(name, sc, W, H, **upload):
        ctx = capi.Context(W, H)
        sc.upload(ctx, **upload)
        ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
        say("%s: %d triangles in the TLAS, %dx%d, pathLength %d" % (name, sc.triangles, W, H, int(sc.settings["pathLength"])))
        for label, mode in MODES:
            ctx.set_shadow_transmittance(mode)
            r1, r8 = rate(ctx, W * H, 1), rate(ctx, W * H, 8)
            flavor = ctx.debug_pass_flavor()
            mean = float(ctx.read_accumulation().mean())
            k = kernel_ms(ctx)
            say("  %-9s %8.1f Msamples/s at one frame per pass, %8.1f at 8; any-hit launches %.3f ms per frame (closest-hit %.3f, thin %.3f, material %.3f); flavor %#x%s; mean of the image %.5f"
                % (label, r1, r8, k["shadow"], k["trace"], k["thin"], k["shade"], flavor, " (TRANSMIT instance)" if flavor & capi.FLAVOR_TRANSMIT else "", mean))
        ctx.close()

    W, H = args.width, args.height
    modes("material zoo (tests/scene_helpers.py: opacity 0.6 and a diffuse map with alpha)", SH.material_zoo_scene(W, H, path_length=5), W, H)
    if not args.skip_config5:
        sc = workloads.config5(3840, 2160, 16)
        modes("configs[4]", sc, 3840, 2160, device_bvh=True, device_tlas=True)

    # the restrictions, on a scene without a see-through material (the mode itself changes nothing there): the same passes with the tail
    # kernel off, and with the hand-over off for BOTH kinds of ray (the hook has one rule for both: an upper bound for the any-hit half)
    sc = workloads.config2(W, H)
    ctx = capi.Context(W, H)
    sc.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    say("configs[1] (no see-through material), %dx%d: what the mode's restrictions would cost" % (W, H))
    never = 0x7fffffff  # iterations before a dry wave hands over: more than the stall guard allows, so no ray is ever listed
    for label, tail, iters in (("default", capi.Context.TAIL_AUTO, 16), ("no tail kernel", 0, 16), ("no hand-over (either kind), no tail kernel", 0, never)):
        ctx.set_tail_bounce(tail)
        ctx.debug_set_thin(lanes=16, iters=iters)
        say("  %-44s %8.1f Msamples/s at one frame per pass, %8.1f at 8" % (label, rate(ctx, W * H, 1), rate(ctx, W * H, 8)))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
