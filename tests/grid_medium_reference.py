"""The density grid's rule (include/nexus_hip.h, nxhip_set_medium_density) restated in numpy: xorshift32 and rng_next, the trilinear lookup,
the majorant bricks, the walk over the bricks in both modes (delta tracking for the free flight, ratio tracking for shadow rays), and the
optical depth of the trilinear field by Gauss-Legendre quadrature.  Every function of the rule takes the number format as `dt`: float64 is
the reference, float32 the same formulas in the device's precision (tests/test_grid_medium_reference.py derives the hooks' bars from the
difference).  The walk is vectorised over rays: one numpy step per iteration of the rule, over the rays still walking."""
import numpy as np

from tests import medium_reference as MR

BRICK = 8
BOUND = 4096


# ---- random numbers (nx_rng.h) ---------------------------------------------------------------------------------------------------------------

def xorshift32(s):
    s = s.astype(np.uint32).copy()
    s ^= s << np.uint32(13)
    s ^= s >> np.uint32(17)
    s ^= s << np.uint32(5)
    return s


def rng_next(s, dt=np.float64):
    """(new state, number in [0, 1) with 23 bits: exact in either format)"""
    s = xorshift32(s)
    return s, ((s >> np.uint32(9)).astype(np.float64) / float(1 << 23)).astype(dt)


def draw_tau(s, dt):
    s, xi = rng_next(s, dt)
    return s, -np.log(dt(1) - xi)


# ---- the grid's constants --------------------------------------------------------------------------------------------------------------------

def scales(box_min, box_max, shape):
    """(vscale, bscale, n, nb) for a grid of numpy shape (nz, ny, nx): formed in binary64, rounded once to binary32, as the host forms them"""
    n = np.array(shape[::-1], dtype=np.int64)
    extent = np.asarray(box_max, np.float32).astype(np.float64) - np.asarray(box_min, np.float32).astype(np.float64)
    return (n / extent).astype(np.float32), (n / (8.0 * extent)).astype(np.float32), n, (n + BRICK - 1) // BRICK


def lookup(grid, box_min, box_max, p, dt=np.float64):
    """rho(p): clamp to edge, three nested a + f * (b - a) lerps along x, then y, then z"""
    vscale, _, n, _ = scales(box_min, box_max, grid.shape)
    p = np.asarray(p, dt).reshape(-1, 3)
    g = grid.astype(dt)
    i0, i1, f = [], [], []
    for k in range(3):
        gk = (p[:, k] - dt(np.float32(box_min[k]))) * dt(vscale[k]) - dt(0.5)
        fl = np.floor(gk)
        f.append(gk - fl)
        i0.append(np.clip(fl, 0, n[k] - 1).astype(np.int64))
        i1.append(np.clip(fl + 1, 0, n[k] - 1).astype(np.int64))

    def lerp(a, b, w):
        return a + w * (b - a)

    def row(z, y):
        return lerp(g[z, y, i0[0]], g[z, y, i1[0]], f[0])

    c0 = lerp(row(i0[2], i0[1]), row(i0[2], i1[1]), f[1])
    c1 = lerp(row(i1[2], i0[1]), row(i1[2], i1[1]), f[1])
    return lerp(c0, c1, f[2])


def bricks(grid):
    """M[bz, by, bx]: the maximum over the voxels [8 b - 1, 8 b + 8] per axis, clamped to the grid — by brute force"""
    nz, ny, nx = grid.shape
    nb = [(m + BRICK - 1) // BRICK for m in (nz, ny, nx)]
    out = np.zeros(nb, dtype=np.float32)
    for bz in range(nb[0]):
        for by in range(nb[1]):
            for bx in range(nb[2]):
                out[bz, by, bx] = grid[max(0, 8 * bz - 1):8 * bz + 9, max(0, 8 * by - 1):8 * by + 9, max(0, 8 * bx - 1):8 * bx + 9].max()
    return out


def brick_of(box_min, box_max, shape, p, dt=np.float64):
    """the brick the walk's start rule gives a point: (n, 3) indices, x first"""
    _, bscale, _, nb = scales(box_min, box_max, shape)
    p = np.asarray(p, dt).reshape(-1, 3)
    u = (p - np.asarray(box_min, np.float32).astype(dt)) * bscale.astype(dt)
    return np.clip(np.floor(u), 0, nb - 1).astype(np.int64)


# ---- the walk --------------------------------------------------------------------------------------------------------------------------------

def walk(grid, box_min, box_max, sigma_t, o, d, t_end, seed, ratio, dt=np.float64, majorants=None):
    """The rule's walk for rays (o[k], d[k]) that end at t_end[k], each from the xorshift32 state seed[k].  ratio False: delta tracking — scatter_t
    is the parameter of the real collision, -1 where there is none.  ratio True: ratio tracking — T.  Also iters and colls (tentative
    collisions), empties (iterations in bricks with M == 0), crosses (the segment rule), bound (the walk hit the iteration bound)."""
    M = (bricks(grid) if majorants is None else majorants).astype(dt)
    _, bscale, _, nb = scales(box_min, box_max, grid.shape)
    bs = bscale.astype(dt)
    bmin = np.asarray(box_min, np.float32).astype(dt)
    o, d = np.asarray(o, dt).reshape(-1, 3), np.asarray(d, dt).reshape(-1, 3)
    sigma = dt(np.float32(sigma_t))
    n = len(o)
    t0, L, crosses = MR.segment(np.asarray(box_min, np.float32), np.asarray(box_max, np.float32), o, d, t_end, dt)
    t1 = t0 + L
    state = np.asarray(seed, np.uint32).copy()
    active = crosses.copy()
    b = np.clip(np.floor(((o + d * t0[:, None]) - bmin) * bs), 0, nb - 1).astype(np.int64)
    fw = d > 0

    def t_next(rays, axes):
        with np.errstate(divide="ignore", invalid="ignore"):
            edge = (b[rays, axes] + fw[rays, axes]).astype(dt) / bs[axes] + bmin[axes]
            tn = (edge - o[rays, axes]) / d[rays, axes]
        return np.where(d[rays, axes] == 0, dt(np.inf), tn)

    everyone = np.arange(n)
    tn = np.stack([t_next(everyone, np.full(n, k)) for k in range(3)], 1)
    t = t0.copy()
    state, tau = draw_tau(state, dt)
    T = np.ones(n, dt)
    scatter_t = np.full(n, dt(-1))
    iters, colls, empties = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for _ in range(BOUND):
        idx = np.nonzero(active)[0]
        if len(idx) == 0:
            break
        iters[idx] += 1
        x, y, z = tn[idx, 0], tn[idx, 1], tn[idx, 2]
        ax = np.where(x <= y, np.where(x <= z, 0, 2), np.where(y <= z, 1, 2))
        tn_ax = tn[idx, ax]
        t_exit = np.minimum(tn_ax, t1[idx])
        Mb = M[b[idx, 2], b[idx, 1], b[idx, 0]]
        empties[idx[Mb == 0]] += 1
        mu = sigma * Mb
        depth = mu * (t_exit - t[idx])
        coll = tau[idx] < depth
        # tentative collisions
        ci = idx[coll]
        if len(ci):
            t[ci] = t[ci] + tau[ci] / mu[coll]
            r = lookup(grid, box_min, box_max, o[ci] + d[ci] * t[ci][:, None], dt)
            colls[ci] += 1
            if ratio:
                T[ci] = T[ci] * np.maximum(dt(0), dt(1) - r / Mb[coll])
                over = T[ci] == 0
            else:
                s, zeta = rng_next(state[ci], dt)
                state[ci] = s
                over = zeta * Mb[coll] < r
                scatter_t[ci[over]] = t[ci[over]]
            active[ci[over]] = False
            on = ci[~over]
            s, fresh = draw_tau(state[on], dt)
            state[on], tau[on] = s, fresh
        # brick steps
        st = ~coll
        si = idx[st]
        if len(si):
            tau[si] = tau[si] - np.maximum(depth[st], dt(0))
            ends = ~(tn_ax[st] < t1[si])
            active[si[ends]] = False
            mv, ax_mv = si[~ends], ax[st][~ends]
            t[mv] = t_exit[st][~ends]
            b[mv, ax_mv] += np.where(fw[mv, ax_mv], 1, -1)
            left = (b[mv, ax_mv] < 0) | (b[mv, ax_mv] >= nb[ax_mv])
            active[mv[left]] = False
            b[mv[left], ax_mv[left]] = np.clip(b[mv[left], ax_mv[left]], 0, nb[ax_mv[left]] - 1)  # (never read again: kept a valid index)
            tn[mv[~left], ax_mv[~left]] = t_next(mv[~left], ax_mv[~left])
    bound = active.copy()
    if ratio:
        T[bound] = 0
    return dict(scatter_t=scatter_t, T=T, iters=iters, colls=colls, crosses=crosses, bound=bound, t0=t0, t1=t1, empties=empties)


def steps_word(w):
    """the hook's word for a walk: iterations | tentative collisions << 16"""
    return (w["iters"] | (w["colls"] << 16)).astype(np.uint32)


# ---- quadrature ------------------------------------------------------------------------------------------------------------------------------

def optical_depth(grid, box_min, box_max, sigma_t, o, d, t_end, panels=256, nodes=8):
    """tau = sigmaT x the integral of rho along the ray's segment in the box, float64: composite Gauss-Legendre (the trilinear field is a cubic
    along a ray between the planes through the voxel centres, with kinks on them; the panels are far finer than the voxels)"""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    t0, L, crosses = MR.segment(np.asarray(box_min, np.float32), np.asarray(box_max, np.float32), o, d, t_end)
    x, w = np.polynomial.legendre.leggauss(nodes)
    edges = np.linspace(0.0, 1.0, panels + 1)
    u = (edges[:-1, None] + (x[None, :] + 1.0) * 0.5 / panels).reshape(-1)  # positions in [0, 1]
    wu = np.tile(w * 0.5 / panels, panels)
    t = t0[:, None] + L[:, None] * u[None, :]
    p = o[:, None, :] + d[:, None, :] * t[:, :, None]
    rho = lookup(grid, box_min, box_max, p.reshape(-1, 3)).reshape(len(o), -1)
    return np.where(crosses, float(np.float32(sigma_t)) * L * (rho * wu[None, :]).sum(1), 0.0)
