"""Feature buffers and denoiser on BASELINE.json configs[1] (the benchmarked workload: 1080p, 8 x 8 tile order, entry points, 20-frame
pass): what a pass costs with and without the feature buffers, what nxhip_denoise costs per iteration and step, and — for the choice
between the two tap paths of nx_aov.hip — the same with the plane variant forced for steps 1 and 2.

  python tools/aov_denoise_bench.py                       pass time with / without, denoise per step (library's choice of variant)
  NX_TUNING_KNOBS=1 NX_DENOISE_DIRECT=1 python tools/...  the plane variant for every step
  python tools/aov_denoise_bench.py --aov-only --passes 3 a short run for `rocprofv3 --kernel-trace --stats -- python ...` (aov_kernel's own time)
  python tools/aov_denoise_bench.py --sweep               the sigma sweep behind nxhip_denoise_defaults (Cornell 256 x 256, 16 frames
                                                          against 4 096): relative MSE of the tonemapped image, noisy and denoised
One JSON line per result."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from nexus_amd import capi, pod, workloads  # noqa: E402


def timed(ctx, fn, reps):
    out = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames-per-pass", type=int, default=20)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--aov-only", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    if args.sweep:
        return sweep()
    W, H = args.width, args.height
    sc = workloads.config2(W, H, 1024, 512, 8)
    ctx = capi.Context(W, H)
    sc.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    ctx.set_pixel_order(pod.ORDER_TILES)
    ctx.set_entry_points(True)
    ctx.set_frames_per_pass(args.frames_per_pass)

    def one_pass():
        ctx.render_frame()
        ctx.accumulate()

    result = {"tool": "aov_denoise_bench", "width": W, "height": H, "frames_per_pass": args.frames_per_pass,
              "denoise_direct_forced": os.environ.get("NX_TUNING_KNOBS") == "1" and os.environ.get("NX_DENOISE_DIRECT", "0") != "0"}
    for aov in ((True,) if args.aov_only else (False, True, False, True)):
        ctx.reset_frame_number()
        ctx.set_aov(aov)
        one_pass()  # (graph instantiation, allocations)
        ms = timed(ctx, one_pass, args.passes)
        result.setdefault("pass_ms_aov_on" if aov else "pass_ms_aov_off", []).extend(round(x, 3) for x in ms)
    for k in ("pass_ms_aov_on", "pass_ms_aov_off"):
        if k in result:
            result[k + "_median"] = round(statistics.median(result[k]), 3)
    if args.aov_only:
        print(json.dumps(result))
        return
    # the filter: per-class device time of the gather + the iterations (kernel timing: an event pair around every launch)
    px = W * H
    ctx.denoise()
    ctx.sync()
    steps = {}
    for it in range(0, 6):
        ctx.enable_kernel_timing(True)
        ctx.read_kernel_times(reset=True)
        for _ in range(5):
            ctx.denoise(iterations=it)
        ctx.sync()
        t = ctx.read_kernel_times(reset=True)
        ctx.enable_kernel_timing(False)
        steps[it] = t["accumulate"]["ms"] / 5.0
    result["denoise_ms_by_iterations"] = {str(k): round(v, 4) for k, v in steps.items()}
    per = {}
    for it in range(1, 6):
        ms = steps[it] - steps[it - 1]
        per[str(1 << (it - 1))] = {"ms": round(ms, 4), "GB_per_s_of_64B_per_pixel": round(px * 64 / ms / 1e6, 1), "share_of_8TB_per_s_peak": round(px * 64 / ms / 1e6 / 8000.0, 3)}
    result["denoise_per_step"] = per
    result["denoise_gather_ms"] = round(steps[0], 4)
    wall = timed(ctx, lambda: ctx.denoise(), 7)
    result["denoise_5_iterations_wall_ms_median"] = round(statistics.median(wall), 3)
    print(json.dumps(result))
    ctx.close()


def sweep():
    from tests import test_gpu_denoise as T

    made = []

    def factory(w, h):
        made.append(capi.Context(w, h))
        return made[-1]

    grid = [dict(sigma_color=c, sigma_normal=n, sigma_albedo=a, sigma_depth=z, iterations=5)
            for c in (0.05, 0.1, 0.2, 0.3, 0.6, 1.2, 2.5) for n in (0.15, 0.3, 0.6) for a in (0.05, 0.1, 0.2, 0.4) for z in (0.025, 0.05, 0.1)]
    grid += [dict(iterations=it) for it in (1, 2, 3, 4, 6)]  # the other parameters at their defaults
    grid.append({})  # the library's defaults
    res = T.measure_denoising(factory, params=grid)
    by = {}
    for seed, p, noisy, den in res:
        by.setdefault(json.dumps(p, sort_keys=True), []).append((seed, noisy, den))
    rows = []
    for key, v in by.items():
        ratio = statistics.mean(d / n for _s, n, d in v)
        rows.append((ratio, key, v))
    rows.sort()
    for ratio, key, v in rows:
        print(json.dumps({"params": json.loads(key), "mean_ratio_denoised_over_noisy": round(ratio, 4),
                          "per_seed": [{"seed": s, "noisy": round(n, 6), "denoised": round(d, 6), "ratio": round(d / n, 4)} for s, n, d in v]}))
    for c in made:
        c.close()


if __name__ == "__main__":
    main()
