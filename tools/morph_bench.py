"""Morph targets: what nxhip_pose_blas_morph costs by the number of ACTIVE targets, against the route a caller had before it.

  python tools/morph_bench.py [--out profiles/morph_blas.txt]

On the wavy grid of tools/pose_bench.py — 1 048 352 triangles (m = 724) — with 52 morph targets, unskinned and skinned with two joints,
in one process:
  * fused:   nxhip_pose_blas_morph with 0, 1, 4 and 16 of the 52 weights not 0 — the weights compacted on the host, the active list's (and
             the palette's) transfer, ONE kernel that reads the bind triangle, the active targets' 80-byte delta records (and the skin) and
             writes the triangle and its intersection-stream record, then the level-by-level node refit.  Timed between two events on the
             context's stream, and by the host's clock around the call (which ends with the stream's wait).
  * before:  what a caller could do without it: the same blend in numpy on the host, in binary32 — deltas, normalisation, then the joints
             where the mesh is skinned — and nxhip_update_blas of the 96-byte triangles.  Timed by the host's clock around both.
The bytes a pose must move are counted from the rule — read 96 (bind) + 80 per active target (+ 80 skin) and the 4-byte index, written
96 + 48 per triangle; the build keeps no separate shading copy — and set against the time of the kernel's route and the 8 TB/s of HBM; the
node refit both routes share is inside the times and outside the bytes.  No threshold: the file says what was measured.
torch provides the events; it must initialise the GPU before the library does, so it is imported first."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nexus_amd import capi, pod  # noqa: E402
from tests import deform_meshes as D  # noqa: E402
from tests import morph_cases as M  # noqa: E402
from tests import skin_cases as K  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the card's specification
TARGETS = 52


def tiled_deltas(tris, targets):
    """(targets, 3 n) records: four distinct targets of morph_cases.deltas, repeated with a per-target scale (a million triangles x 52
    targets of distinct trigonometry would take the host longer than everything measured here)"""
    base = M.deltas(tris, 4, seed=11)
    d = np.empty((targets, base.shape[1]), dtype=pod.MORPH_CORNER_DT)
    for t in range(targets):
        s = np.float32(0.25 + 0.75 * ((7 * t) % 13) / 12.0)
        d["dPosition"][t] = base["dPosition"][t % 4] * s
        d["dNormal"][t] = base["dNormal"][t % 4] * s
    return d


def host_blend(bind, d, weights, corners, pal):
    """the rule in numpy binary32 over corner arrays -> 96-byte triangles (the route without the kernel)"""
    n = len(bind)
    p, nrm = K.corner_positions(bind).copy(), K.corner_normals(bind).copy()
    act = np.flatnonzero(weights != 0)
    if len(act):
        live = np.any(nrm != 0, axis=1)
        for t in act:
            p += weights[t] * d["dPosition"][t]
            nrm += weights[t] * d["dNormal"][t]
        ln = np.sqrt(np.sum(nrm * nrm, axis=1, dtype=np.float32))
        ok = live & (ln > 0) & np.isfinite(ln)
        nrm = np.where(ok[:, None], nrm / np.where(ok, ln, 1)[:, None], np.float32(0))
    if corners is not None:
        J = pal.reshape(-1, 3, 4)
        Mx = np.einsum("ck,ckrs->crs", corners["weight"], J[corners["joint"]]).astype(np.float32)
        p = np.einsum("crs,cs->cr", Mx[:, :, :3], p) + Mx[:, :, 3]
        m3 = Mx[:, :, :3]
        cof = np.empty_like(m3)
        for r in range(3):
            for s in range(3):
                r1, r2, s1, s2 = (r + 1) % 3, (r + 2) % 3, (s + 1) % 3, (s + 2) % 3
                cof[:, r, s] = m3[:, r1, s1] * m3[:, r2, s2] - m3[:, r1, s2] * m3[:, r2, s1]
        v = np.einsum("crs,cs->cr", cof, nrm)
        v[np.einsum("cs,cs->c", m3[:, 0], cof[:, 0]) < 0] *= -1
        ln = np.sqrt(np.sum(v * v, axis=1))
        ok = (ln > 0) & np.isfinite(ln)
        nrm = np.where(ok[:, None], v / np.where(ok, ln, 1)[:, None], np.float32(0))
    out = bind.copy()
    p, nrm = p.reshape(n, 3, 3), nrm.reshape(n, 3, 3)
    for k in range(3):
        out["pos%d" % k], out["normal%d" % k] = p[:, k], nrm[:, k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=724)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="", help="the commit the figures belong to")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    torch.cuda.set_device(0)
    side = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(side)
    med = statistics.median
    tris = np.ascontiguousarray(D.base_grid(args.size), dtype=pod.TRI_DT)
    n = len(tris)
    d = tiled_deltas(tris, TARGETS)
    corners = K.two_joint_skin(tris, 0, 2)
    stored = pod.normalise_skin_corners(corners, 2)
    pal = K.palette("ordinary", 2, 2.0, 1)
    say("nxhip_pose_blas_morph by active targets (fused) against a numpy blend on the host + nxhip_update_blas (before)")
    if args.commit:
        say("commit %s" % args.commit)
    say("%s, %d CUs; wavy grid m = %d: %d triangles, %d morph targets (%.2f GB of delta records on the device)" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, args.size, n, TARGETS, TARGETS * n * 80 / 1e9))
    say("fused: device events on the context's stream and the host's clock, median of %d; before: the host's clock, median of %d" % (args.repeats, args.host_repeats))
    say()
    ctx = capi.Context(64, 64, stream=side.cuda_stream)
    ctx.set_materials(np.array([pod.make_material()], dtype=pod.MAT_DT))
    bid = ctx.build_blas(tris)
    t0 = time.perf_counter()
    ctx.set_blas_morph(bid, d)
    say("nxhip_set_blas_morph (validation, repacking, %.2f GB to the device), once: %.2f s" % (TARGETS * n * 80 / 1e9, time.perf_counter() - t0))
    say()
    say("%-10s %-7s %10s %19s %10s %10s %8s %7s   %14s %8s" % ("", "active", "events ms", "(min .. max)", "host ms", "MB moved", "TB/s", "% peak", "before host ms", "x fused"))
    for skinned in (False, True):
        if skinned:
            ctx.set_blas_skin(bid, corners, 2)
        for active in (0, 1, 4, 16):
            w = np.zeros(TARGETS, np.float32)
            idx = (np.arange(active) * (TARGETS // max(active, 1)) + 1) % TARGETS  # spread over the 52
            w[idx] = np.linspace(0.2, 0.6, active).astype(np.float32) * np.where(np.arange(active) % 3 == 2, -1, 1)
            p = pal if skinned else None

            def fused():
                ctx.pose_blas_morph(bid, w, p)

            for _ in range(3):
                fused()
            ev, host = [], []
            for _ in range(args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                c0 = time.perf_counter()
                e0.record(side)
                fused()
                e1.record(side)
                e1.synchronize()
                host.append((time.perf_counter() - c0) * 1e3)
                ev.append(e0.elapsed_time(e1))
            got = ctx.read_blas_triangles(bid, n)
            before = []
            for _ in range(args.host_repeats):
                c0 = time.perf_counter()
                blended = host_blend(tris, d, w, stored if skinned else None, pal)
                ctx.update_blas(bid, blended)
                before.append((time.perf_counter() - c0) * 1e3)
            # the two routes agree to binary32 rounding (numpy sums in another order than the kernel: no bit comparison)
            err = float(np.max(np.abs(K.corner_positions(got).astype(np.float64) - K.corner_positions(blended))))
            assert err < 1e-4, err
            moved = n * (4 + 96 + 80 * active + (80 if skinned else 0)) + n * (96 + 48)
            ms = med(ev)
            say("%-10s %-7d %10.4f %19s %10.4f %10.1f %8.3f %7.1f   %14.1f %8.0f" % (
                "skinned" if skinned else "unskinned", active, ms, "(%.4f .. %.4f)" % (min(ev), max(ev)), med(host), moved / 1e6, moved / (ms * 1e-3) / 1e12,
                100.0 * moved / (ms * 1e-3) / HBM_PEAK, med(before), med(before) / med(host)))
    say()
    say("the refit of the BVH8 nodes is inside every time and outside the bytes: the percentages understate the pose kernel's own bandwidth")
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
