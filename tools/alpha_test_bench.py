"""Alpha-tested geometry (nxhip_set_material_alpha): what the ALPHA_TEST instances of the trace kernels cost on tests/golden/alpha_cutout.glb
read as MASK / OPAQUE, against the same file read as a stochastic blend with transparent shadows (NXHIP_SHADOWS_TRANSMIT) — the only way
to get holes before — and against the plain blend.

  python tools/alpha_test_bench.py [--width 1920 --height 1080] [--steps 16 --warmup 4] [--path-length 6] [--out profiles/alpha_test.txt]

Per reading in one process: Msamples/s over `steps` one-frame passes and over passes of 8 frames, and the trace launches' time per frame
from the in-graph timers (nxhip_read_kernel_times: classes trace, shadow, thin, shade)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from nexus_amd import capi, loaders, pod  # noqa: E402
from tests import scene_helpers as SH  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--path-length", type=int, default=6)
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

    W, H = args.width, args.height
    path = os.path.join(SH.GOLDEN, "alpha_cutout.glb")
    table = loaders.load_glb(path, alpha_modes=True).material_alpha
    readings = (("blend (the default)", None, pod.SHADOWS_OPAQUE),
                ("blend + TRANSMIT", None, pod.SHADOWS_TRANSMIT),
                ("alpha modes (MASK / OPAQUE)", table, pod.SHADOWS_OPAQUE),
                ("alpha modes + TRANSMIT", table, pod.SHADOWS_TRANSMIT))
    say("tests/golden/alpha_cutout.glb, %dx%d, pathLength %d, eye (0, 0.7, 3.6)" % (W, H, args.path_length))
    for label, alpha, shadows in readings:
        sc = SH.glb_scene(path, W, H, path_length=args.path_length, eye=(0.0, 0.7, 3.6), forward=(0.0, 0.0995, -0.995), hfov=50.0)
        sc.material_alpha, sc.shadow_transmittance = alpha, shadows
        ctx = capi.Context(W, H)
        sc.upload(ctx)
        ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_REFERENCE)
        r1, r8 = rate(ctx, W * H, 1), rate(ctx, W * H, 8)
        flavor = ctx.debug_pass_flavor()
        mean = float(ctx.read_accumulation().mean())
        k = kernel_ms(ctx)
        say("  %-28s %8.1f Msamples/s at one frame per pass, %8.1f at 8; per frame: closest-hit %.3f ms, any-hit %.3f, thin %.3f, material %.3f; flavor %#x; mean of the image %.5f"
            % (label, r1, r8, k["trace"], k["shadow"], k["thin"], k["shade"], flavor, mean))
        ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
