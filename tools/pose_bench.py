"""Skinned meshes: what the fused pose pass costs against the route a caller had before it (nxhip_pose_blas, nx_skin.hip).

  python tools/pose_bench.py [--out profiles/pose_blas.txt]

On a wavy grid skinned with two joints across x — 1 048 352 triangles (m = 724) and 10 082 (m = 71) — in one process, the two routes
alternating, each between two events on the context's stream, median of 20 after a warm-up of both:
  * fused:   nxhip_pose_blas — the palette's transfer, ONE kernel that reads the bind triangle and its skin and writes the triangle and
             its intersection-stream record, then the level-by-level node refit.
  * before:  the palette's transfer (from the same pageable array), a minimal stand-alone skinning kernel
             (tools/pose_bench_kernel.hip, compiled by this tool) writing 96-byte records into a buffer of the caller's, then
             nxhip_update_blas_device: a device copy of the records, the pass that reads every triangle again for the intersection
             stream, the same node refit.
The two halves of the second route are timed on their own as well (the skin kernel with its palette already on the device; the update
of records that are already there), and the bytes each route must move are counted from the shapes.  No threshold: the file says which
route was faster and by how much against the run-to-run spread.
torch provides the events and the device buffers; it must initialise the GPU before the library does, so it is imported first."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nexus_amd import capi, pod  # noqa: E402
from tests import deform_meshes as D  # noqa: E402
from tests import skin_cases as K  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the card's specification
KERNEL_SRC = os.path.join(ROOT, "tools", "pose_bench_kernel.hip")
KERNEL_LIB = os.path.join(ROOT, "nexus_amd", "lib", "pose_bench_kernel.so")


def kernel_lib():
    """the stand-alone skinning kernel as a shared object, compiled when it is missing or older than its source"""
    if not os.path.exists(KERNEL_LIB) or os.path.getmtime(KERNEL_LIB) < os.path.getmtime(KERNEL_SRC):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "--offload-arch=gfx950",
                        KERNEL_SRC, "-o", KERNEL_LIB], check=True)
    lib = C.CDLL(KERNEL_LIB)
    lib.pose_bench_skin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]
    return lib


def packed_skin(corners, joint_count):
    """the 80-byte per-triangle records the library keeps (nx_device.h SkinTri), from normalised corner records"""
    c = pod.normalise_skin_corners(corners, joint_count)
    n = len(c) // 3
    out = np.zeros(n, dtype=np.dtype([("weight", "<f4", (3, 4)), ("joint", "<u2", (3, 4)), ("pad", "<u4", 2)]))
    out["weight"] = c["weight"].reshape(n, 3, 4)
    out["joint"] = c["joint"].reshape(n, 3, 4)
    return out


def device_bytes(a):
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8).copy()).to("cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[724, 71])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="", help="the commit the figures belong to (the tree on the GPU machine is no git repository)")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    torch.cuda.set_device(0)
    side = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(side)
    lib = kernel_lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    say("nxhip_pose_blas (fused) against a stand-alone skinning kernel + nxhip_update_blas_device (before)")
    if args.commit:
        say("commit %s" % args.commit)
    say("%s, %d CUs; times by device events on the context's stream, median of %d, the two routes alternating" % (torch.cuda.get_device_name(0), cus, args.repeats))
    say()
    med = statistics.median
    for m in args.sizes:
        tris = np.ascontiguousarray(D.base_grid(m), dtype=pod.TRI_DT)
        n = len(tris)
        corners = K.two_joint_skin(tris, 0, 2)
        palettes = [K.palette(kind, 2, 2.0, seed) for kind, seed in (("ordinary", 1), ("ordinary", 2), ("mirror", 3))]
        ctx = capi.Context(64, 64, stream=side.cuda_stream)
        ctx.set_materials(np.array([pod.make_material()], dtype=pod.MAT_DT))
        bid = ctx.build_blas(tris)
        nodes, _idx = ctx.read_blas(bid, n)
        ctx.set_blas_skin(bid, corners, 2)
        d_bind, d_skin = device_bytes(tris), device_bytes(packed_skin(corners, 2))
        d_pal = [device_bytes(p) for p in palettes]
        h_pal = [torch.from_numpy(p.copy()) for p in palettes]  # pageable, as the caller's array is
        d_pal_sent = torch.empty(2 * 12, dtype=torch.float32, device="cuda")
        d_out = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
        grid = min((n + 255) // 256, 8 * cus)
        torch.cuda.synchronize()

        def fused(k):
            ctx.pose_blas(bid, palettes[k % 3])

        def before(k):
            d_pal_sent.copy_(h_pal[k % 3].reshape(-1), non_blocking=True)  # (on the context's stream: torch's current one)
            rc = lib.pose_bench_skin(side.cuda_stream, d_bind.data_ptr(), d_skin.data_ptr(), d_pal_sent.data_ptr(), n, d_out.data_ptr(), grid)
            assert rc == 0, rc
            ctx.update_blas_device(bid, d_out.data_ptr(), n)

        def skin_only(k):
            rc = lib.pose_bench_skin(side.cuda_stream, d_bind.data_ptr(), d_skin.data_ptr(), d_pal[k % 3].data_ptr(), n, d_out.data_ptr(), grid)
            assert rc == 0, rc

        def update_only(k):
            ctx.update_blas_device(bid, d_out.data_ptr(), n)

        def timed(route, k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            route(k)
            e1.record(side)
            e1.synchronize()
            return e0.elapsed_time(e1)

        # the two routes give the same triangles and the same tree
        fused(0)
        a_tris, a_nodes = ctx.read_blas_triangles(bid, n), ctx.read_blas(bid, n)[0]
        before(0)
        b_tris, b_nodes = ctx.read_blas_triangles(bid, n), ctx.read_blas(bid, n)[0]
        same = a_tris.tobytes() == b_tris.tobytes() and a_nodes.tobytes() == b_nodes.tobytes()
        for k in range(3):  # warm-up of every shape the timed window uses
            fused(k), before(k)
        t = {"fused": [], "before": [], "skin": [], "update": []}
        for k in range(args.repeats):
            t["fused"].append(timed(fused, k))
            t["before"].append(timed(before, k))
        for k in range(args.repeats):
            t["skin"].append(timed(skin_only, k))
            t["update"].append(timed(update_only, k))
        node_count = len(nodes)
        # bytes each route must move, from the shapes.  The refit both share: per node 80 read, 64 written, a 32-byte box written and
        # read once by the parent; per triangle the index (4) and the 96-byte record its positions lie in.
        refit = node_count * (80 + 64 + 32 + 32) + n * (4 + 96)
        fused_bytes = n * (4 + 96 + 80) + n * (96 + 48) + refit                      # index, bind, skin read; triangle, stream written
        before_bytes = n * (96 + 80) + n * 96 + n * (96 + 96) + n * (4 + 96 + 48) + refit  # skin kernel; device copy; stream pass
        say("wavy grid m = %d: %d triangles, %d BVH8 nodes; the two routes give the same triangles and nodes: %s" % (m, n, node_count, "yes" if same else "NO"))
        for name, label, moved in (("fused", "nxhip_pose_blas (fused)", fused_bytes), ("before", "skin kernel + nxhip_update_blas_device", before_bytes),
                                   ("skin", "  the stand-alone skin kernel alone", n * (96 + 80 + 96)), ("update", "  nxhip_update_blas_device alone", before_bytes - n * (96 + 80 + 96))):
            ms = med(t[name])
            say("  %-42s %9.4f ms  (min %.4f, max %.4f)  %7.1f MB -> %6.3f TB/s, %5.1f %% of the %.0f TB/s HBM peak" % (
                label, ms, min(t[name]), max(t[name]), moved / 1e6, moved / (ms * 1e-3) / 1e12, 100.0 * moved / (ms * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
        f, b = med(t["fused"]), med(t["before"])
        spread = max(max(t["fused"]) - min(t["fused"]), max(t["before"]) - min(t["before"]))
        verdict = "faster" if f < b - spread else "slower" if f > b + spread else "the same within the run-to-run spread"
        say("  fused / before = %.3f (before - fused = %.4f ms, spread %.4f ms): the fused pass is %s" % (f / b, b - f, spread, verdict))
        say("  bytes per triangle without the shared refit: fused %d, before %d" % ((fused_bytes - refit) // n, (before_bytes - refit) // n))
        say()
        ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
