"""What a generated sky costs (nxhip_set_sky), beside the only other route to the same texels: the numpy model of tests/sky_reference.py
and nxhip_upload_env_float.

  device    events around the map kernel's launches (NX_TUNING_KNOBS=1 NX_ENV_TIMING=1: the library prints them, as for the sampler's
            tables), default steps 64 x 16, no disc and with the default sun's disc: 3 warm-up calls, then the median of 7
  call      wall time of the whole nxhip_set_sky (allocation, launch, wait, installation), the same 7 calls
  upload    wall time of nxhip_upload_env_float of a map of that size alone: the part of the host route a faster host could not remove
  numpy     tests/sky_reference.radiance on ROWS rows of the map, scaled to the whole map (the whole map takes minutes)

    python tools/sky_bench.py > profiles/sky.txt
"""
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((2048, 1024), (4096, 2048))
WARMUP, RUNS, ROWS = 3, 7, 8


def child():
    import numpy as np

    from nexus_amd import capi, pod
    from tests import sky_reference as R

    with capi.Context(16, 16) as ctx:
        for W, H in SIZES:
            for disc in (0, 1):
                sky = pod.Sky(width=W, height=H, sunDisc=disc)
                for k in range(WARMUP + RUNS):
                    t = time.perf_counter()
                    ctx.set_sky(sky)
                    print("CALL %d %d %d %d %.6f" % (W, H, disc, k, 1e3 * (time.perf_counter() - t)), flush=True)
            img = np.random.RandomState(1).uniform(0.0, 2.0, (H, W, 3)).astype(np.float32)
            for k in range(WARMUP + RUNS):
                t = time.perf_counter()
                ctx.upload_env_float(img)
                print("UPLOAD %d %d %d %.6f" % (W, H, k, 1e3 * (time.perf_counter() - t)), flush=True)
            P = R.Params(pod.Sky(width=W, height=H))
            d = R.map_directions(W, H)[H // 2 - ROWS // 2:H // 2 + ROWS // 2].reshape(-1, 3)
            t = time.perf_counter()
            R.radiance(P, d)
            print("NUMPY %d %d %.6f" % (W, H, 1e3 * (time.perf_counter() - t) * H / ROWS), flush=True)


def main():
    env = dict(os.environ, NX_TUNING_KNOBS="1", NX_ENV_TIMING="1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, cwd=ROOT)
    if run.returncode != 0:
        sys.exit("the measuring process failed:\n" + run.stdout[-2000:] + run.stderr[-2000:])
    device = {}
    for W, H, disc, ms in re.findall(r"\[sky\] device build (\d+) x (\d+), steps 64 x 16(, disc)?: ([0-9.]+) ms", run.stderr):
        device.setdefault((int(W), int(H), 1 if disc else 0), []).append(float(ms))
    calls, uploads, numpy_ms = {}, {}, {}
    for line in run.stdout.splitlines():
        f = line.split()
        if f[0] == "CALL":
            calls.setdefault((int(f[1]), int(f[2]), int(f[3])), []).append(float(f[5]))
        elif f[0] == "UPLOAD":
            uploads.setdefault((int(f[1]), int(f[2])), []).append(float(f[4]))
        elif f[0] == "NUMPY":
            numpy_ms[(int(f[1]), int(f[2]))] = float(f[3])
    commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=ROOT).stdout.strip() or "(no git here)"
    print("nxhip_set_sky on an MI355X — python tools/sky_bench.py; tree at or after commit %s" % commit)
    print("default steps 64 x 16; %d warm-up calls, median of %d (min .. max); milliseconds" % (WARMUP, RUNS))
    med = lambda v: "%9.3f (%.3f .. %.3f)" % (statistics.median(v[WARMUP:]), min(v[WARMUP:]), max(v[WARMUP:]))  # noqa: E731
    for W, H in SIZES:
        print("%d x %d" % (W, H))
        for disc in (0, 1):
            assert len(device[(W, H, disc)]) == WARMUP + RUNS
            print("  device, events around the launches%s  %s" % (", with the disc" if disc else "              ", med(device[(W, H, disc)])))
            print("  whole call, wall%s                 %s" % (", with the disc" if disc else "              ", med(calls[(W, H, disc)])))
        print("  nxhip_upload_env_float alone, wall                %s" % med(uploads[(W, H)]))
        print("  numpy float64 model, %d rows scaled to the map   %9.0f" % (ROWS, numpy_ms[(W, H)]))


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
