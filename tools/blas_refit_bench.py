"""Deforming meshes: what a refit costs against a rebuild, and what it does to the tree (nxhip_update_blas_device, nx_refit.hip).

  python tools/blas_refit_bench.py [--nu 1024 --nv 512] [--out profiles/r11_blas_refit.txt]

On the displaced torus of configs[1] (2 nu nv triangles; 1 048 576 by default), in one process:
  * nxhip_update_blas_device + the deferred refresh (instance bounds, traversal records, TLAS refit), between two events on the
    context's stream, median of 20.  The refresh is brought on by nxhip_read_tlas without destinations, which also waits for the
    stream: the interval ends with one host synchronisation (its ~10 us are inside the figure).  The update alone (no refresh,
    nothing waits) is timed too.
  * nxhip_build_blas of the same deformed triangles, median of 5 — the whole call (it takes host triangles: their transfer is part
    of it) and, measured separately, a transfer of as many bytes, so that the build proper can be told from the copy.
  * nxhip_update_blas (host triangles: the transfer and a synchronisation are part of the call), wall clock, median of 5.
  * node and triangle visits per ray (nxhip_read_trace_stats) on the refitted and on the rebuilt tree for three deformation
    amplitudes: when the refitted tree's visits have grown by more than a user cares to pay, a rebuild is due.
The bar: refit + refresh <= a third of the rebuild's time in this run.  torch provides the events and the device tensor; it must
initialise the GPU before the library does, so this tool imports it first."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nexus_amd import capi, pod, scenegen  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the card's specification


def torus(nu, nv, amp):
    return scenegen.displaced_torus(nu, nv, seed=1, major=1.0, minor=0.45, amp=amp, center=(0.0, 0.56, 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=int, default=1024)
    ap.add_argument("--nv", type=int, default=512)
    ap.add_argument("--rays", type=int, default=1 << 18)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    torch.cuda.set_device(0)
    side = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(side)
    base_amp, amps = 0.06, (0.09, 0.15, 0.24)
    base = torus(args.nu, args.nv, base_amp)
    n = len(base)
    shapes = [torus(args.nu, args.nv, a) for a in amps]
    floor = scenegen.quad((-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6))
    ident = np.eye(4, dtype=np.float32).reshape(16)
    ctx = capi.Context(256, 256, stream=side.cuda_stream)
    ctx.set_materials(np.array([pod.make_material()], dtype=pod.MAT_DT))
    ids = [ctx.build_blas(base), ctx.build_blas(floor)]
    nodes0, _ = ctx.read_blas(ids[0], n)
    node_count = len(nodes0)

    def instances(blas_ids):
        out = []
        for k, b in enumerate(blas_ids):
            root = ctx.read_blas(b, n if k == 0 else len(floor))[0][0]
            out.append(capi.instance_init(b, 0, ident, root))
        return np.array(out, dtype=pod.INST_DT)

    ctx.rebuild_tlas(instances(ids))
    rays = scenegen.random_rays(args.rays, seed=3, radius=5.0, target_extent=1.4)
    rays["origin"][:, 1] += 0.56
    ctx.trace_batch(rays[:4096])  # first use: code objects, queues

    say("BLAS refit against rebuild: displaced torus, %d triangles, %d BVH8 nodes (binned-SAH device build)" % (n, node_count))
    say()

    # ---- timing --------------------------------------------------------------------------------------------------------------
    dev = [torch.from_numpy(np.frombuffer(s.tobytes(), dtype=np.uint8).copy()).to("cuda") for s in shapes]
    torch.cuda.synchronize()
    null = None

    def refresh_now():
        capi.check(ctx.L.nxhip_read_tlas(ctx.h, null, 0, null, 0), "nxhip_read_tlas")

    ctx.update_blas_device(ids[0], dev[0].data_ptr(), n)  # first update: the refit plan is made (one read-back of the nodes)
    refresh_now()
    with_refresh, alone = [], []
    for k in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        ctx.update_blas_device(ids[0], dev[k % 3].data_ptr(), n)
        refresh_now()
        e1.record(side)
        e1.synchronize()
        with_refresh.append(e0.elapsed_time(e1))
    for k in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        ctx.update_blas_device(ids[0], dev[k % 3].data_ptr(), n)
        e1.record(side)
        e1.synchronize()
        alone.append(e0.elapsed_time(e1))
    refresh_now()
    host_form = []
    for k in range(5):
        t0 = time.perf_counter()
        ctx.update_blas(ids[0], shapes[k % 3])
        host_form.append((time.perf_counter() - t0) * 1e3)
    refresh_now()
    built, built_wall, rebuilt_ids = [], [], []
    for k in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        t0 = time.perf_counter()
        rebuilt_ids.append(ctx.build_blas(shapes[k % 3]))
        built_wall.append((time.perf_counter() - t0) * 1e3)
        e1.record(side)
        e1.synchronize()
        built.append(e0.elapsed_time(e1))
    copies = []
    scratch = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(np.frombuffer(shapes[0].tobytes(), dtype=np.uint8).copy())  # pageable, as the caller's array is
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scratch.copy_(src)
        torch.cuda.synchronize()
        copies.append((time.perf_counter() - t0) * 1e3)

    med = statistics.median
    refit_ms, alone_ms, build_ms, copy_ms = med(with_refresh), med(alone), med(built), med(copies)
    # bytes the update moves: triangles copied (96 read + 96 written), the intersection stream (index 4 + triangle 96 read, 48
    # written), the refit (per node: 80 read, 64 written, a 32-byte box written and read once by the parent; per triangle: index 4 +
    # the 96-byte record its 36 bytes of positions lie in)
    moved = n * (96 + 96) + n * (4 + 96 + 48) + node_count * (80 + 64 + 32 + 32) + n * (4 + 96)
    say("nxhip_update_blas_device + deferred refresh   median of 20: %8.3f ms   (min %.3f, max %.3f)" % (refit_ms, min(with_refresh), max(with_refresh)))
    say("nxhip_update_blas_device alone                median of 20: %8.3f ms   (min %.3f, max %.3f)" % (alone_ms, min(alone), max(alone)))
    say("  bytes moved by an update: %.1f MB (%.0f B per triangle) -> %.2f TB/s, %.1f %% of the %.1f TB/s HBM peak" % (
        moved / 1e6, moved / n, moved / (alone_ms * 1e-3) / 1e12, 100.0 * moved / (alone_ms * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
    say("nxhip_update_blas (host triangles), wall      median of 5:  %8.3f ms   (the %d MB transfer and a synchronisation included)" % (med(host_form), 96 * n // 1000000))
    say("nxhip_build_blas of the deformed triangles    median of 5:  %8.3f ms by events, %.3f ms wall (host triangles: their transfer included)" % (build_ms, med(built_wall)))
    say("  a transfer of as many bytes from pageable memory, wall:   %8.3f ms   -> the build proper: about %.3f ms" % (copy_ms, build_ms - copy_ms))
    say()
    ratio_call, ratio_proper = build_ms / refit_ms, (build_ms - copy_ms) / refit_ms
    say("rebuild / (refit + refresh): %.1f x against the whole nxhip_build_blas call, %.1f x against the build without its transfer" % (ratio_call, ratio_proper))
    say("bar (refit + refresh <= rebuild / 3): %s against the call, %s against the build proper" % ("met" if ratio_call >= 3 else "MISSED", "met" if ratio_proper >= 3 else "MISSED"))
    say()

    # ---- what the refit does to the tree ------------------------------------------------------------------------------------
    ctx.enable_trace_stats(True)
    say("visits per ray, %d rays towards the mesh (closest hit):" % len(rays))
    say("  amplitude (built at %.2f)   refitted tree: nodes  triangles     rebuilt tree: nodes  triangles     refitted / rebuilt nodes" % base_amp)

    def visits():
        ctx.read_trace_stats(reset=True)
        ctx.trace_batch(rays)
        d = ctx.read_trace_stats(reset=True)[0]  # (closest hit)
        return d["nodes"] / max(1, d["rays"]), d["tris"] / max(1, d["rays"])

    for k, a in enumerate(amps):
        ctx.update_blas_device(ids[0], dev[k].data_ptr(), n)
        ctx.rebuild_tlas(instances(ids))
        rn, rt = visits()
        ctx.rebuild_tlas(instances([rebuilt_ids[k], ids[1]]))
        bn, bt = visits()
        say("  %.2f                        %19.2f %10.2f %23.2f %10.2f %20.3f" % (a, rn, rt, bn, bt, rn / bn))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
