"""The float64 statement of the density grid's rule (tests/grid_medium_reference.py) checked against itself and against quadrature, and the
bars of the device tests derived from it: the same formulas in numpy binary32 on the hooks' inputs, worst deviation from float64, times 4 (the
project's convention).  Also the .npy reader of the host layer and the exported symbols.  No GPU."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from nexus_amd import capi, pod
from tests import grid_medium_reference as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(1, 1, 1), (8, 8, 8), (8, 8, 9), (18, 13, 20)]  # numpy order (nz, ny, nx): 1x1x1, 8x8x8, 9x8x8 and 20x13x18 as nx x ny x nz

# ---- the hooks' medium, grid and inputs (tests/test_gpu_grid_medium.py runs the device on exactly these) ----------------------------------

HOOK_N = 20000


def hook_medium():
    return pod.make_medium(box_min=(-1.0, -0.5, -1.5), box_max=(1.0, 1.0, 0.5), sigma_t=5.0, g=0.3, albedo=(0.9, 0.8, 0.7))


def shape_grid(shape, seed=7):
    """a lumpy field in [0, 1.5] with everything under 0.45 cut to 0, and — where the grid has more than one brick along x — the low-x bricks
    of the upper half emptied: bricks with M == 0"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    f = 0.75 + 0.5 * np.sin(0.7 * x + 0.3) * np.cos(0.9 * y - 0.2) + 0.25 * np.sin(1.1 * z) + rng.uniform(-0.1, 0.1, shape)
    f = np.where(f < 0.45, 0.0, f)
    if nx > 9:
        f[nz // 2:, :, :10] = 0.0
    if f.max() == 0.0:
        f[...] = 0.8
    return f.astype(np.float32)


def hook_grid():
    return shape_grid((18, 13, 20))


def puff():
    return np.load(os.path.join(GOLDEN, "fog_puff.npy"))


def hook_inputs():
    """20 000 rays: origins in [-3, 3]^3, a fifth inside the box, some on a face; half aimed at a point of the box, the rest anywhere; one in
    eight with a zero direction component (its origin's component moved into the box's range on half of them, so that some cross); tEnd
    finite or inf; xorshift32 states"""
    rng = np.random.default_rng(20261020)
    m = hook_medium()
    lo, hi = m["boxMin"].astype(np.float64), m["boxMax"].astype(np.float64)
    o = rng.uniform(-3.0, 3.0, (HOOK_N, 3))
    o[::5] = rng.uniform(lo + 0.05, hi - 0.05, (len(o[::5]), 3))
    o[3::40, 0] = lo[0]
    d = rng.normal(size=(HOOK_N, 3))
    aim = rng.uniform(lo, hi, (HOOK_N, 3)) - o
    d[1::2] = aim[1::2]
    axis = rng.integers(0, 3, HOOK_N)
    rows = np.arange(0, HOOK_N, 8)
    d[rows, axis[rows]] = 0.0
    inside = rows[::2]
    o[inside, axis[inside]] = rng.uniform(lo, hi, (HOOK_N, 3))[inside, axis[inside]]
    d = d / np.sqrt((d * d).sum(1))[:, None]
    t_end = rng.uniform(0.2, 8.0, HOOK_N)
    t_end[::3] = np.inf
    seed = rng.integers(1, 1 << 32, HOOK_N, dtype=np.uint64).astype(np.uint32)
    return o.astype(np.float32), d.astype(np.float32), t_end.astype(np.float32), seed


_cache = {}


def track_reference(dt=np.float64):
    """(free flight, ratio tracking): the walks of the hook's rays"""
    key = ("track", dt)
    if key not in _cache:
        m, grid = hook_medium(), hook_grid()
        o, d, t_end, seed = hook_inputs()
        _cache[key] = tuple(G.walk(grid, m["boxMin"], m["boxMax"], m["sigmaT"], o, d, t_end, seed, ratio, dt) for ratio in (False, True))
    return _cache[key]


def decisions(flight, ratio):
    """what tells two walks of a ray apart: the words the hook reports, and whether the flight scattered"""
    return np.stack([G.steps_word(flight), G.steps_word(ratio), (flight["scatter_t"] >= 0).astype(np.uint32)], 1)


def track_bars():
    """(bars, keep, (flight64, ratio64)): absolute bars on scatter t and T; keep = rays whose decision sequences agree between binary32 and float64"""
    ref, f32 = track_reference(np.float64), track_reference(np.float32)
    keep = np.all(decisions(*ref) == decisions(*f32), 1)
    bars = {"scatter_t": 4.0 * float(np.abs(f32[0]["scatter_t"].astype(np.float64) - ref[0]["scatter_t"])[keep].max()),
            "T": 4.0 * float(np.abs(f32[1]["T"].astype(np.float64) - ref[1]["T"])[keep].max())}
    return bars, keep, ref


def lookup_points():
    """20 000 points: most in the box, some on its faces, some outside (clamp to edge)"""
    rng = np.random.default_rng(11)
    m = hook_medium()
    lo, hi = m["boxMin"].astype(np.float64), m["boxMax"].astype(np.float64)
    p = rng.uniform(lo, hi, (HOOK_N, 3))
    p[::50] = rng.uniform(lo - 0.5, hi + 0.5, (len(p[::50]), 3))
    p[7::100, 1] = hi[1]
    return p.astype(np.float32)


def lookup_bar():
    """(bar, float64 lookup): 4 x the worst binary32-against-float64 deviation of the lookup on lookup_points()"""
    m, grid, p = hook_medium(), hook_grid(), lookup_points()
    r64 = G.lookup(grid, m["boxMin"], m["boxMax"], p, np.float64)
    r32 = G.lookup(grid, m["boxMin"], m["boxMax"], p, np.float32)
    return 4.0 * float(np.abs(r32.astype(np.float64) - r64).max()), r64


# ---- tests -----------------------------------------------------------------------------------------------------------------------------------

def _bricks_by_voxel(grid):
    """the definition read the other way round: every voxel raises every brick whose range [8 b - 1, 8 b + 8] holds it"""
    nz, ny, nx = grid.shape
    nb = [(k + 7) // 8 for k in (nz, ny, nx)]
    out = np.zeros(nb, np.float32)

    def owners(i, n):
        return [b for b in range(n) if 8 * b - 1 <= i <= 8 * b + 8]

    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                for bz in owners(z, nb[0]):
                    for by in owners(y, nb[1]):
                        for bx in owners(x, nb[2]):
                            out[bz, by, bx] = max(out[bz, by, bx], grid[z, y, x])
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["1x1x1", "8x8x8", "9x8x8", "20x13x18"])
def test_bricks_by_brute_force_and_majorant_bounds_the_lookup(shape):
    grid = shape_grid(shape)
    M = G.bricks(grid)
    assert M.shape == tuple((k + 7) // 8 for k in shape)
    assert np.array_equal(M, _bricks_by_voxel(grid))
    if shape[2] > 9:
        assert (M == 0).any(), "the hook's grid has empty bricks"
    m = hook_medium()
    rng = np.random.default_rng(3)
    p = rng.uniform(m["boxMin"].astype(np.float64), m["boxMax"].astype(np.float64), (HOOK_N, 3)).astype(np.float32)
    for dt in (np.float64, np.float32):
        rho = G.lookup(grid, m["boxMin"], m["boxMax"], p, dt).astype(np.float64)
        b = G.brick_of(m["boxMin"], m["boxMax"], grid.shape, p, dt)
        top = M[b[:, 2], b[:, 1], b[:, 0]].astype(np.float64)
        assert np.all(rho <= top * (1.0 + 2.0 ** -23)), "a majorant lies under the lookup by more than an ulp"


def test_a_constant_grid_returns_its_constant_exactly():
    m = hook_medium()
    grid = np.full((5, 9, 11), 0.7, np.float32)
    for dt in (np.float64, np.float32):
        assert np.all(G.lookup(grid, m["boxMin"], m["boxMax"], lookup_points(), dt) == dt(np.float32(0.7)))


def test_both_estimators_meet_the_quadrature():
    """three rays through the hook's grid, 20 000 streams each: the mean of the ratio tracking's T, and the share of free flights that pass
    without a real collision, both against exp(-tau) within 4.5 standard errors"""
    m, grid = hook_medium(), hook_grid()
    # (origin, direction, tEnd): through the whole box; from above, ending inside it; from inside the box to a hit inside it
    rays = [((-2.0, 0.3, -0.4), (1.0, 0.02, 0.05), np.inf), ((0.1, 2.0, -1.2), (0.05, -1.0, 0.3), 1.6), ((-0.6, 0.4, 0.2), (0.3, -0.25, -1.0), 0.9)]
    rng = np.random.default_rng(99)
    n = 20000
    for o, d, t_end in rays:
        d = np.array(d) / np.linalg.norm(d)
        O, D, te = np.tile(np.float32(o), (n, 1)), np.tile(d.astype(np.float32), (n, 1)), np.full(n, t_end, np.float32)
        want = np.exp(-G.optical_depth(grid, m["boxMin"], m["boxMax"], m["sigmaT"], O[:1], D[:1], te[:1])[0])
        assert 0.02 < want < 0.9, want
        seed = rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        ratio = G.walk(grid, m["boxMin"], m["boxMax"], m["sigmaT"], O, D, te, seed, True)
        flight = G.walk(grid, m["boxMin"], m["boxMax"], m["sigmaT"], O, D, te, seed, False)
        assert not ratio["bound"].any() and not flight["bound"].any()
        passed = (flight["scatter_t"] < 0).astype(np.float64)
        for what, x in (("ratio tracking", ratio["T"]), ("no real collision", passed)):
            se = x.std(ddof=1) / np.sqrt(n)
            print("%s: %.5f against exp(-tau) = %.5f, standard error %.2g: z = %.2f" % (what, x.mean(), want, se, (x.mean() - want) / se))
            assert abs(x.mean() - want) <= 4.5 * se, what


def test_binary32_takes_the_decisions_of_float64_on_the_hook_inputs():
    bars, keep, (flight, ratio) = track_bars()
    n = len(keep)
    print("decision sequences that differ between binary32 and float64: %d of %d; bars %s" % ((~keep).sum(), n, bars))
    assert (~keep).mean() <= 1e-3
    assert 0.0 < bars["scatter_t"] < 1e-4 and 0.0 < bars["T"] < 1e-4
    crosses = flight["crosses"]
    scat = flight["scatter_t"] >= 0
    M = G.bricks(hook_grid())
    assert (M == 0).any()
    empties = ratio["empties"] > 0  # walked through a brick with M == 0
    print("cross %.3f, scatter %.3f, T < 1 %.3f, through an empty brick %.3f, iterations mean %.1f max %d" % (
        crosses.mean(), scat.mean(), (ratio["T"] < 1).mean(), empties.mean(), flight["iters"][crosses].mean(), flight["iters"].max()))
    assert crosses.mean() > 0.3 and scat.mean() > 0.1 and (crosses & ~scat).mean() > 0.05 and empties.mean() > 0.05
    assert not flight["bound"].any() and not ratio["bound"].any()
    assert np.all(ratio["T"][ratio["colls"] == 0] == 1.0) and np.all(flight["scatter_t"][~crosses] == -1.0)
    o, d, t_end, _ = hook_inputs()
    assert ((d == 0).any(1)).mean() > 0.1 and np.isinf(t_end).mean() > 0.3 and (o[:, 0] == hook_medium()["boxMin"][0]).sum() > 100


# ---- the .npy reader ---------------------------------------------------------------------------------------------------------------------------

def _npy(a, version=None):
    f = io.BytesIO()
    if version is None:
        np.save(f, a)
    else:
        np.lib.format.write_array(f, a, version=version)
    return f.getvalue()


def test_npy_reader_round_trips_numpy_save():
    for shape in ((16, 16, 16), (3, 5, 7), (1, 1, 1)):
        a = np.random.default_rng(1).uniform(0, 2, shape).astype(np.float32)
        for version in (None, (1, 0), (2, 0)):
            got = capi.decode_npy_grid(_npy(a, version))
            assert got.shape == shape and np.array_equal(got.view(np.uint32), a.view(np.uint32))
    with open(os.path.join(GOLDEN, "fog_puff.npy"), "rb") as f:
        got = capi.decode_npy_grid(f.read())
    assert np.array_equal(got, puff()) and got.shape == (16, 16, 16)


def test_npy_reader_refuses_what_is_no_density_grid():
    a = np.ones((4, 5, 6), np.float32)
    bad = {"float64": _npy(a.astype(np.float64)), "Fortran order": _npy(np.asfortranarray(a)), "2-D": _npy(a[0]), "4-D": _npy(a[None]),
           "big-endian": _npy(a.astype(">f4")), "truncated": _npy(a)[:-8], "no file": b"not a numpy file at all", "513": _npy(np.ones((1, 1, 513), np.float32))}
    for what, data in bad.items():
        with pytest.raises(capi.NexusError) as e:
            capi.decode_npy_grid(data)
        print(what, "->", e.value)
        assert len(str(e.value)) > 30, what


def test_the_fixture_is_what_its_generator_writes():
    from tests.golden import make_fog_grid
    g = puff()
    assert g.dtype == np.float32 and g.shape == (16, 16, 16) and np.array_equal(g, make_fog_grid.puff())
    assert g[0, 0, 0] == 0 and g[-1, -1, -1] == 0 and g[0, -1, 0] == 0 and g.max() > 1.0 and os.path.getsize(os.path.join(GOLDEN, "fog_puff.npy")) < 17000


def test_exported_symbols():
    L, H = capi.lib(), capi.host_lib() if hasattr(capi, "host_lib") else capi.lib()
    hip = ["nxhip_set_medium_density", "nxhip_read_medium_majorants", "nxhip_medium_density_batch", "nxhip_medium_track_batch"]
    host = ["nxs_scene_set_medium_density", "nxs_scene_clear_medium_density", "nxs_scene_medium_density", "nxh_decode_npy_grid"]
    for s in hip:
        assert s in capi.HIP_SYMBOLS and hasattr(L, s), s
    for s in host:
        assert s in capi.HOST_SYMBOLS and hasattr(H, s), s
    assert capi.FLAVOR_MEDIUM_GRID == 16384 and capi.API_VERSION == 8, "no struct was added: the version stays"
    for name in ("set_medium_density", "read_medium_majorants", "medium_density_batch", "medium_track_batch"):
        assert callable(getattr(capi.Context, name)), name
    assert callable(capi.Scene.set_medium_density) and callable(capi.Scene.medium_density)
    from nexus_amd import workloads
    assert workloads.Workload.medium_density is None
    # the setter validates before it looks at the device: no context, no GPU
    assert L.nxhip_set_medium_density(None, None, 0, 0, 0) != 0
