"""The numpy restatement of adaptive sampling (tests/adaptive_reference.py) on synthetic radiance: no GPU.

Three blocks of 64 pixels and a partial fourth: constant pixels, pixels of known variance, constant pixels with one NaN pixel among them.
"""
import numpy as np

from tests import adaptive_reference as A

FRAMES = 24


def _synthetic(seed=7):
    rng = np.random.RandomState(seed)
    n = 3 * 64 + 20
    frames = []
    const = rng.uniform(0.1, 2.0, (n, 3)).astype(np.float32)
    for _ in range(FRAMES):
        r = const.copy()
        r[64:128] = rng.normal(0.5, 0.5, (64, 3)).astype(np.float32)  # known variance (negative values are fine for the arithmetic)
        r[130] = np.nan
        frames.append(r)
    return frames, n


def test_constant_pixels_have_no_variance_and_settle_at_the_floor():
    frames, n = _synthetic()
    sim, hist = A.run(frames, threshold=0.05, lum_floor=0.01, min_samples=8, cull=True, interval=4, max_frames=FRAMES)
    const = np.r_[0:64, 192:n]
    assert np.all(sim.m2[const] == 0.0) and np.all(sim.block_max[[0, 3]] == 0.0)
    # decided at frames 4 (below the floor: everything stays), 8 (blocks 0 and 3 settle), ...
    assert hist[0]["active_blocks"] == 4 and hist[0]["active_pixels"] == n
    assert list(hist[1]["flags"]) == [False, True, True, False]
    assert np.all(sim.count[const] == 8), "a culled block takes no further samples"
    assert np.array_equal(hist[1]["active"], np.arange(64, 192))
    assert A.same_bits(sim.acc[const], frames[0][const]), "the mean of equal samples is the sample"
    assert hist[1]["active_pixels"] == 128


def test_welford_agrees_with_the_two_pass_variance():
    frames, n = _synthetic()
    sim, _ = A.run(frames, threshold=0.0, lum_floor=0.01, min_samples=8, cull=False, interval=4, max_frames=FRAMES)
    assert np.all(sim.count == FRAMES), "estimate only: nothing is ever deactivated"
    y = np.stack([A.luminance(f[64:128]) for f in frames]).astype(np.float64)  # the float32 luminances, exactly
    want_var, want_mean = np.var(y, axis=0), np.mean(y, axis=0)
    got_var = sim.m2[64:128].astype(np.float64) / FRAMES
    rel = np.abs(got_var - want_var) / want_var
    print("Welford M2 / n against np.var (float64): largest relative deviation %.3g; mean: %.3g" % (rel.max(), np.max(np.abs(sim.mean[64:128] - want_mean))))
    assert rel.max() <= 1e-5
    assert np.max(np.abs(sim.mean[64:128] - want_mean)) <= 1e-6
    # the error the decision uses, against the textbook formula
    e = A.relative_error(sim.count, sim.mean, sim.m2, 0.01)[64:128]
    want_e = np.sqrt(np.var(y, axis=0, ddof=1) / FRAMES) / np.maximum(want_mean, 0.01)
    assert np.max(np.abs(e - want_e) / want_e) <= 1e-5
    assert np.all(sim.block_max[1] == e.max())


def test_a_nan_pixel_keeps_its_block_alive():
    frames, n = _synthetic()
    sim, hist = A.run(frames, threshold=1e30, lum_floor=0.01, min_samples=8, cull=True, interval=4, max_frames=FRAMES)
    # with a threshold nothing finite exceeds, every block settles at the floor — except the one with the NaN
    assert [h["active_blocks"] for h in hist] == [4] + [1] * 5 and hist[-1]["frames_issued"] == FRAMES
    assert list(sim.flags) == [False, False, True, False]
    assert np.isinf(sim.block_max[2]) and np.all(np.isfinite(sim.block_max[[0, 1, 3]]))
    assert np.all(sim.count[128:192] == FRAMES) and np.all(sim.count[:128] == 8) and np.all(sim.count[192:] == 8)
    assert np.isnan(sim.acc[130]).all() and np.isfinite(sim.acc[np.r_[128:130, 131:192]]).all()


def test_estimate_only_stops_by_the_same_rule_without_culling():
    frames, n = _synthetic()
    frames = [np.where(np.isnan(f), np.float32(1.0), f) for f in frames]
    kw = dict(threshold=0.3, lum_floor=0.01, min_samples=8, interval=4, max_frames=FRAMES)
    culled, hc = A.run(frames, cull=True, **kw)
    plain, hp = A.run(frames, cull=False, **kw)
    assert np.all(plain.count == hp[-1]["frames_issued"])
    assert np.all(culled.count <= plain.count) and culled.count.sum() < plain.count.sum()
    # the partial last block is the last of the active order and keeps its 20 pixels
    assert hc[0]["active_pixels"] == n and len(hc[0]["active"]) == n
    # until the first block is culled the two runs are the same run
    assert A.same_bits(hc[0]["acc"], hp[0]["acc"]) and A.same_bits(hc[0]["stats"], hp[0]["stats"])
