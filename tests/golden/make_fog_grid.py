"""Writes tests/golden/fog_puff.npy: a 16 x 16 x 16 fog density grid, float32, C order, shape (nz, ny, nx) — a puff that is densest a little
off the centre, lumpy, and exactly 0 outside a radius of 0.95 half-widths, so the corners of the box are empty.  Deterministic; numpy only.

    python tests/golden/make_fog_grid.py"""
import os

import numpy as np

N = 16


def puff(n=N):
    c = (np.arange(n) + 0.5) / n * 2.0 - 1.0  # voxel centres in [-1, 1]
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    r2 = (x - 0.1) ** 2 + (y + 0.05) ** 2 + z ** 2
    body = np.maximum(0.0, 1.0 - r2 / 0.95 ** 2) ** 2
    lumps = 1.0 + 0.35 * np.sin(5.0 * x + 1.0) * np.sin(4.0 * y - 0.5) * np.sin(6.0 * z + 0.3)
    return (1.6 * body * lumps).astype(np.float32)


if __name__ == "__main__":
    grid = puff()
    assert grid.min() == 0.0 and grid[0, 0, 0] == 0.0 and grid[-1, -1, -1] == 0.0 and grid.max() > 1.0
    np.save(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fog_puff.npy"), grid)
