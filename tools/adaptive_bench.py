"""Adaptive sampling (nx_adaptive.hip) at 1080p, 8 x 8 tile order, entry points: what estimating costs and what culling buys.

  python tools/adaptive_bench.py --estimate [--passes 7]     configs[1], 20-frame pass: wall time of a pass (render + accumulate + sync) and
                                                             device time of the accumulate class (kernel-timing hook), adaptive off against
                                                             estimate only (cull = 0), alternated
  python tools/adaptive_bench.py --estimate --short          one state each, 3 passes: for `rocprofv3 --kernel-trace --stats -- python ...`
  python tools/adaptive_bench.py --cull --config 0|1 --threshold T [--max-frames N]
                                                             nxhip_render_adaptive's loop driven from here so that every interval is timed:
                                                             cull = 1 against cull = 0 (same rule, same threshold), wall time and total samples
                                                             until no block is active, share of blocks alive and the update's own time per interval
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


def make_ctx(config, W, H):
    if config == 0:
        sc = workloads.config1(os.path.join(ROOT, "tests", "golden", "cornell_box.glb"), W, H, 4)
    else:
        sc = workloads.config2(W, H, 1024, 512, 8)
    ctx = capi.Context(W, H)
    sc.upload(ctx)
    ctx.set_modes(pod.RNG_PIXEL_KEYED, pod.COMPACT_FAST, pod.CONDUCTOR_EXTENDED)
    ctx.set_pixel_order(pod.ORDER_TILES)
    ctx.set_entry_points(True)
    return ctx


def estimate(args):
    W, H = args.width, args.height
    ctx = make_ctx(1, W, H)
    ctx.set_frames_per_pass(args.frames_per_pass)
    result = {"tool": "adaptive_bench --estimate", "width": W, "height": H, "frames_per_pass": args.frames_per_pass}

    def one_pass():
        ctx.render_frame()
        ctx.accumulate()

    states = (False, True) if args.short else (False, True, False, True)
    for on in states:
        ctx.reset_frame_number()
        if on:
            ctx.set_adaptive(threshold=0.05, cull=0)
        else:
            ctx.set_adaptive(on=False)
        one_pass()
        wall = []
        for _ in range(3 if args.short else args.passes):
            ctx.sync()
            t0 = time.perf_counter()
            one_pass()
            ctx.sync()
            wall.append((time.perf_counter() - t0) * 1e3)
        key = "estimate_only" if on else "off"
        result.setdefault("pass_ms_" + key, []).extend(round(x, 3) for x in wall)
        if not args.short:  # the accumulate class on its own: an event pair around every launch (the pass then runs kernel by kernel)
            ctx.enable_kernel_timing(True)
            ctx.read_kernel_times(reset=True)
            for _ in range(3):
                one_pass()
            ctx.sync()
            t = ctx.read_kernel_times(reset=True)
            ctx.enable_kernel_timing(False)
            result.setdefault("accumulate_class_ms_per_pass_" + key, []).append(round(t["accumulate"]["ms"] / 3.0, 4))
    for k in list(result):
        if k.startswith("pass_ms_"):
            result[k + "_median"] = round(statistics.median(result[k]), 3)
    px, S = W * H, args.frames_per_pass
    result["bytes_fused_kernel_must_move_per_pass"] = px * (16 * S + 2 * (16 + 8 + 4) + 4 + 4)
    print(json.dumps(result))
    ctx.close()


def cull(args):
    W, H = args.width, args.height
    out = {"tool": "adaptive_bench --cull", "config": args.config, "width": W, "height": H, "threshold": args.threshold, "min_samples": args.min_samples,
           "interval": args.interval, "max_frames": args.max_frames}
    for mode in (1, 0):
        ctx = make_ctx(args.config, W, H)
        ctx.set_frames_per_pass(args.interval)
        ctx.set_adaptive(threshold=args.threshold, min_samples=args.min_samples, cull=mode)
        ctx.render_adaptive(args.interval, args.interval)  # (graphs, allocations)
        ctx.reset_frame_number()
        ctx.sync()
        blocks_total = (ctx.local_count + 63) // 64
        timeline, frames, blocks = [], 0, blocks_total
        t_start = time.perf_counter()
        while blocks and frames < args.max_frames:
            # one interval exactly as nxhip_render_adaptive issues it, split so that the update is timed alone
            active = ctx.active_count()
            t0 = time.perf_counter()
            capacity = ctx.local_count * args.interval
            per = max(1, min(args.interval, capacity // max(active, 1)))
            done = 0
            while done < args.interval:
                n = min(per, args.interval - done)
                if n != ctx.frames_per_pass:
                    ctx.set_frames_per_pass(n)
                ctx.render_frame()
                ctx.accumulate()
                done += n
            ctx.sync()
            t1 = time.perf_counter()
            _, blocks = ctx.adaptive_update()
            t2 = time.perf_counter()
            frames += args.interval
            timeline.append({"frames": frames, "rendered_pixels": active, "render_ms": round((t1 - t0) * 1e3, 3), "update_ms": round((t2 - t1) * 1e3, 3),
                             "blocks_alive_share": round(blocks / blocks_total, 4)})
        wall = (time.perf_counter() - t_start) * 1e3
        counts = ctx.read_sample_counts()
        key = "cull" if mode else "estimate_only"
        out[key] = {"wall_ms": round(wall, 2), "frames_issued": frames, "total_samples": int(counts.astype(np.int64).sum()), "blocks_alive_at_end": blocks,
                    "samples_per_pixel_min_median_max": [int(counts.min()), float(np.median(counts)), int(counts.max())], "timeline": timeline}
        ctx.close()
    if out["cull"]["wall_ms"] > 0:
        out["wall_ratio_cull_over_estimate_only"] = round(out["cull"]["wall_ms"] / out["estimate_only"]["wall_ms"], 4)
        out["sample_ratio_cull_over_estimate_only"] = round(out["cull"]["total_samples"] / out["estimate_only"]["total_samples"], 4)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames-per-pass", type=int, default=20)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--estimate", action="store_true")
    ap.add_argument("--short", action="store_true")
    ap.add_argument("--cull", action="store_true")
    ap.add_argument("--config", type=int, default=1)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--min-samples", type=int, default=16)
    ap.add_argument("--interval", type=int, default=8)
    ap.add_argument("--max-frames", type=int, default=256)
    args = ap.parse_args()
    if args.estimate:
        estimate(args)
    if args.cull:
        cull(args)


if __name__ == "__main__":
    main()
