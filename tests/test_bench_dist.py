"""bench.py's N > 1 code path over the real RCCL backend, on the one GPU of the box.

The driver's scaling run is `torch.distributed.run --nproc-per-node N bench.py --gpus N` with the "nccl" (= RCCL) backend:
process group with a device id, one explicit torch stream carrying kernels and collective, a zero-copy torch view of the
context's accumulation, `dist.gather` of device tensors, compose on the root.  VERDICT r3: that path had last been executed in
round 1 and rewritten twice since; the 2-rank rehearsal forces gloo.  Here it runs as a fresh child process at world size 1
(NX_BENCH_FORCE_DIST=1: same code, the gather degenerates to a copy) and its image must equal the plain run's byte for byte."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--frames-per-pass", "2", "--passes-in-flight", "2"]], ids=["one-pass", "passes-in-flight"])
def test_bench_through_torchrun_and_rccl_renders_the_plain_image(tmp_path, extra):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("NX_BENCH_BACKEND", None)
    common = ["--steps", "5", "--warmup", "2", "--reps", "2", "--width", "256", "--height", "160", "--no-cpu-baseline", "--no-roofline", "--no-obj-check"] + extra
    plain, rccl = str(tmp_path / "plain.png"), str(tmp_path / "rccl.png")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common + ["--png", plain], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", _free_port(),
           os.path.join(ROOT, "bench.py"), "--gpus", "1"] + common + ["--png", rccl]
    r = subprocess.run(cmd, env=dict(env, NX_BENCH_FORCE_DIST="1"), cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert open(plain, "rb").read() == open(rccl, "rb").read()
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    # the line of a distributed run says how every rank did, not only the slowest
    pr = line["config"]["per_rank"]
    assert pr["backend"] == "nccl" and len(pr["rep_ms_by_rank"]) == 2 and len(pr["median_ms_by_rank"]) == 1 and pr["slowest_rank"] == 0
    assert pr["gather_bytes_per_rank_and_pass"] == 256 * 160 * 16
    assert line["n_gpus"] == 1 and line["steps"] == 5 and line["value"] > 0


@pytest.mark.gpu
def test_a_distributed_bench_line_carries_rank_zeros_roofline(tmp_path):
    """The line of an N > 1 run with --full has the `roofline` block too (rank 0's launches on its own tiles; no collective inside the section, the
    other ranks wait at the closing barrier) — `cpu_baseline` stays an N = 1 figure."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0", NX_BENCH_FORCE_DIST="1")
    env.pop("NX_BENCH_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", _free_port(),
           os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--reps", "2", "--width", "256", "--height", "160", "--no-obj-check", "--full"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    rf = line["roofline"]
    assert rf["kernel"] == "trace_kernel<closest>" and rf["rays_per_launch"] > 0 and rf["avg_launch_ms"] > 0 and "scope" in rf
    # (the fractions need the committed per-ray counters, which are tied to the hash of the device sources they were collected on: a
    #  build whose sources have changed since says so instead of quoting stale figures)
    if rf["frac"] is None:
        assert rf["traffic"] is None and "source" in rf["traffic_source"]
    else:
        assert 0.0 < rf["frac"] < 1.5 and rf["traffic"] > 0
    assert "cpu_baseline" not in line and "per_rank" in line["config"]


@pytest.mark.gpu
def test_a_plain_run_times_the_steps_only_and_dumps_the_same_outputs_every_time(tmp_path):
    """`bench.py --steps K --warmup W` without --full: one timed region of K steps and the headline fields, nothing else measured;
    --dump-outputs writes the accumulation and the RGBA8 image of the last step in image order, the same bits on every run, and
    the RGBA8 image is the one --png shows."""
    runs = []
    for k in (1, 2):
        out, png = tmp_path / ("dump%d" % k), str(tmp_path / ("plain%d.png" % k))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--width", "256", "--height", "160",
                            "--dump-outputs", str(out), "--png", png], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
        runs.append((line, np.load(out / "accumulation.npy"), np.load(out / "rgba8.npy"), open(png, "rb").read()))
        assert not (out / "pixel_index.npy").exists()
    line, acc, rgba, png = runs[0]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and line["warmup"] == 2 and len(line["config"]["rep_ms"]) == 1 and line["config"]["frames_timed"] == 3
    assert abs(line["value"] - 256 * 160 * 3 / (line["ms_per_step"] * 3 * 1e-3) / 1e6) < 1e-2 * line["value"]
    assert not {"roofline", "cpu_baseline"} & set(line) and not {"reference_mode", "obj_round_trip"} & set(line["config"])
    assert acc.dtype == np.float32 and acc.shape == (160, 256, 3) and np.isfinite(acc).all() and acc.max() > 0
    assert rgba.dtype == np.float32 and rgba.shape == (160, 256, 4) and rgba.min() >= 0 and rgba.max() <= 255
    for other in runs[1:]:
        assert np.array_equal(acc.view(np.uint32), other[1].view(np.uint32)) and np.array_equal(rgba, other[2]) and png == other[3]
    from nexus_amd import capi

    shown, _ = capi.decode_image(png)
    assert np.array_equal(shown[::-1].astype(np.float32), rgba)  # (the PNG's first row is the top of the view, the buffers' the bottom)


def test_dump_outputs_writes_whole_images_within_the_budget_and_a_fixed_sample_beyond_it(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    W, H = 40, 30
    rng = np.random.RandomState(3)
    arrays = {"accumulation": rng.rand(W * H, 3).astype(np.float32), "rgba8": rng.randint(0, 256, (W * H, 4)).astype(np.float32)}
    bench.dump_outputs(str(tmp_path / "whole"), arrays, W, H)
    assert np.array_equal(np.load(tmp_path / "whole" / "accumulation.npy"), arrays["accumulation"].reshape(H, W, 3))
    assert np.array_equal(np.load(tmp_path / "whole" / "rgba8.npy"), arrays["rgba8"].reshape(H, W, 4))
    assert not (tmp_path / "whole" / "pixel_index.npy").exists()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 100 * (28 + 8))
    samples = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, W, H)
        idx = np.load(tmp_path / d / "pixel_index.npy")
        assert idx.dtype == np.float64 and len(idx) == 100 and np.all(np.diff(idx) > 0) and idx.max() < W * H
        got = {k: np.load(tmp_path / d / (k + ".npy")) for k in arrays}
        for k, a in arrays.items():
            assert np.array_equal(got[k], a[idx.astype(np.int64)])
        assert sum(v.nbytes for v in got.values()) + idx.nbytes <= bench.DUMP_BUDGET_BYTES
        samples.append(idx)
    assert np.array_equal(samples[0], samples[1])


def test_bench_help_prints_its_options_without_a_gpu():
    """`python bench.py --help`: argparse expands every help string with %-formatting, so a literal per-cent sign in one of them
    is a crash before anything runs (it was: "2 % fewer node visits")."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for option in ("--gpus", "--steps", "--warmup", "--config", "--passes-in-flight", "--full", "--dump-outputs"):
        assert option in r.stdout


def test_the_pass_plan_of_the_drivers_scaling_run():
    """`--steps 20` on N = 1, 2, 4, 8 GPUs: under weak scaling (a step = one frame per GPU) every rank renders its tiles of 20 N frames as
    ONE pass — the path count of the 1-GPU pass —, under strong scaling its tiles of 20 frames; the default 512 steps are passes of
    64 N frames (at most 512), four in flight.  (bench.plan_schedule; no GPU needed.)"""
    sys.path.insert(0, ROOT)
    import bench

    for n in (1, 2, 4, 8):
        cap = min(64 * n, 512)
        assert bench.plan_schedule(20 * n, cap, None, False, 1.0 / n) == (20 * n, 1, 1)  # weak
        assert bench.plan_schedule(20, cap, None, False, 1.0 / n) == (20, 1, 1)          # strong
        S, R, passes = bench.plan_schedule(512 * n, cap, None, False, 1.0 / n)
        assert S == cap and R == 4 and passes == 512 * n // cap
        # the paths of a rank's pass never exceed what the 1-GPU run allocates for its own
        assert S * (1920 * 1080 // n) <= 128 * 1920 * 1080
