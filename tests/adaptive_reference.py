"""Adaptive sampling restated in numpy (include/nexus_hip.h, "adaptive sampling"; nexus_amd/csrc/device/nx_adaptive.hip).

Every operation is a single binary32 operation on numpy float32 arrays — the build has contraction off and `/` and sqrt are correctly
rounded on both sides — so counts, (meanY, M2), the running mean of the colour, the block decisions and the block maxima are defined
bit for bit.  The simulator takes per-frame FULL-FRAME radiance in the base order of the context (what a plain context's read_radiance
returns, frame by frame: with pixel-keyed random numbers a path's radiance depends on its pixel and frame only) and applies the
bookkeeping to the pixels that are active.
"""
import numpy as np

F = np.float32
BLOCK = 64


def luminance(rgb):
    rgb = np.asarray(rgb, F)
    return (F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]


def relative_error(count, mean, m2, lum_floor):
    """e of every pixel (float32; garbage where count < 2: the callers mask those)"""
    with np.errstate(all="ignore"):
        n = count.astype(F)
        return np.sqrt(m2 / (n * (n - F(1.0)))) / np.fmax(mean, F(lum_floor))  # (fmaxf: a NaN operand gives the other one)


def block_view(per_pixel, fill):
    """(blocks, 64) view of a per-pixel array, the partial last block padded with `fill`"""
    n = len(per_pixel)
    blocks = (n + BLOCK - 1) // BLOCK
    out = np.full(blocks * BLOCK, fill, per_pixel.dtype)
    out[:n] = per_pixel
    return out.reshape(blocks, BLOCK)


class Simulator:
    def __init__(self, pixels, threshold, lum_floor, min_samples, cull, channels=3):
        self.n = int(pixels)
        self.blocks = (self.n + BLOCK - 1) // BLOCK
        self.threshold, self.lum_floor, self.min_samples, self.cull = F(threshold), F(lum_floor), int(min_samples), bool(cull)
        self.count = np.zeros(self.n, np.uint32)
        self.mean = np.zeros(self.n, F)
        self.m2 = np.zeros(self.n, F)
        self.acc = np.zeros((self.n, 3), F)
        self.extra = None                      # optional further buffers folded like the colour, all their components (feature buffers)
        self.flags = np.ones(self.blocks, bool)  # block still active (only ever cleared)
        self.block_max = np.zeros(self.blocks, F)
        self.active = np.arange(self.n, dtype=np.uint32)  # base-local indices the next pass renders, in order

    def fold(self, radiance, extra=None):
        """one frame: `radiance` (n, 3) full-frame values in base order; only the active pixels take part"""
        a = self.active
        if len(a) == 0:
            return
        r = np.asarray(radiance, F).reshape(self.n, 3)[a]
        self.count[a] += 1
        n = self.count[a]
        nf = n.astype(F)
        first = n == 1
        with np.errstate(all="ignore"):
            acc = self.acc[a]
            acc = np.where(first[:, None], r, acc + (r - acc) / nf[:, None])
            self.acc[a] = acc
            y = luminance(r)
            d = y - self.mean[a]
            mean = self.mean[a] + d / nf
            m2 = self.m2[a] + d * (y - mean)
            self.mean[a] = np.where(first, y, mean)
            self.m2[a] = np.where(first, F(0.0), m2)
            if extra is not None:
                if self.extra is None:
                    self.extra = [np.zeros((self.n,) + np.asarray(x).shape[1:], F) for x in extra]
                for buf, x in zip(self.extra, extra):
                    x = np.asarray(x, F)[a]
                    old = buf[a]
                    buf[a] = np.where(first[:, None], x, old + (x - old) / nf[:, None])

    def update(self):
        """the decision: (active pixels, active blocks)"""
        e = relative_error(self.count, self.mean, self.m2, self.lum_floor)
        has = self.count >= 2
        with np.errstate(all="ignore"):
            unsettled = np.where(has, (self.count < self.min_samples) | ~(e <= self.threshold), True)
            shown = np.where(has, np.where(e >= 0, np.abs(e), F(np.inf)), F(0.0)).astype(F)  # NaN counts as +inf; abs: -0 -> +0
        self.block_max = block_view(shown, F(0.0)).max(axis=1)
        self.flags &= block_view(unsettled, False).any(axis=1)
        per_pixel = np.repeat(self.flags, BLOCK)[:self.n]
        if self.cull:
            self.active = np.flatnonzero(per_pixel).astype(np.uint32)
        return int(per_pixel.sum()), int(self.flags.sum())

    def snapshot(self):
        return dict(count=self.count.copy(), stats=np.stack([self.mean, self.m2], axis=1), acc=self.acc.copy(), flags=self.flags.copy(),
                    block_max=self.block_max.copy(), active=self.active.copy(), extra=None if self.extra is None else [x.copy() for x in self.extra])


def run(frames, threshold, lum_floor, min_samples, cull, interval, max_frames, extras=None):
    """nxhip_render_adaptive on recorded radiance: `frames[f]` is the full-frame radiance of frame f + 1.  Returns the simulator and one
    snapshot per interval (with `frames_issued`, `active_pixels`, `active_blocks`)."""
    sim = Simulator(len(frames[0]), threshold, lum_floor, min_samples, cull)
    history, issued, blocks = [], 0, sim.blocks
    while blocks != 0 and issued < max_frames:
        n = min(interval, max_frames - issued)
        for f in range(issued, issued + n):
            sim.fold(frames[f], None if extras is None else extras[f])
        issued += n
        pixels, blocks = sim.update()
        snap = sim.snapshot()
        snap.update(frames_issued=issued, active_pixels=pixels, active_blocks=blocks)
        history.append(snap)
    return sim, history


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
