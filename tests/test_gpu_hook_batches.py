"""The columnar test hooks' plumbing (nx_hookbatch.h HookBatch, capi._cols / _outs / Context._hook), not their physics: every hook on one
tiny scene.  Each item's result depends on its own inputs only, so one call over 257 items (one more than a 256-thread block) must give,
bit for bit, what a call on item 0 and a call on items 1 .. 256 give — a column copied with a wrong width, stride or count does not.
Then the empty batch, and the two optional columns (env_eval's pdf / texel, fmath's b)."""
import numpy as np
import pytest

from nexus_amd import capi, pod, scenegen, workloads
from tests import metalrough_reference as MR
from tests import oracle_lib as O
from tests import scene_helpers as SH

N = 257
F32, U32, F64 = np.float32, np.uint32, np.float64
MATERIAL = MR.material((0.9, 0.6, 0.3), 0.6, 0.5, diffuse_map=0, emissive=(1.0, 0.8, 0.6), intensity=2.0)  # (emissive: the quad is the light table's mesh light)


def _scene():
    quad = scenegen.quad((-1, 0, -1), (-1, 0, 1), (1, 0, 1), (1, 0, -1))
    for k in range(3):
        quad["texCoord%d" % k][:, 0] = (quad["pos%d" % k][:, 0] + 1.0) / 2.0
        quad["texCoord%d" % k][:, 1] = (quad["pos%d" % k][:, 2] + 1.0) / 2.0
    rs = np.random.RandomState(3)
    base = rs.randint(0, 256, (2, 2, 4)).astype(np.uint8)
    env = rs.randint(1, 256, (2, 4, 4)).astype(np.uint8)
    base[..., 3] = env[..., 3] = 255
    sc = SH.BuiltScene([quad], [(0, 0, workloads.IDENTITY)], materials=np.array([MATERIAL], dtype=pod.MAT_DT), diffuse_maps=[base], hdr_map=env)
    sc.lights = SH.mesh_lights(sc.instances, sc.materials)
    sc.env_sampling, sc.light_sampling = True, pod.LIGHTS_POWER
    sc.medium = pod.make_medium(box_min=(-1, -1, -1), box_max=(1, 1, 1), sigma_t=1.5, g=0.4, albedo=(0.9, 0.8, 0.7))
    sc.medium_density = rs.uniform(0.2, 1.0, (9, 9, 9)).astype(F32)  # (two bricks per axis)
    return sc


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    c = gpu_ctx_factory(16, 16)
    _scene().upload(c)
    c.set_analytic_lights([pod.make_analytic_light(pod.ALIGHT_POINT, position=(0.3, 1.5, 0.2), colour=(1.0, 0.9, 0.8), intensity=5.0)])
    return c


def _unit(rs, *shape):
    """binary32 numbers in [0, 1) (multiples of 2^-23: none rounds up to 1)"""
    return (rs.randint(0, 1 << 23, shape) / float(1 << 23)).astype(F32)


def _dirs(rs, n, upper=False):
    v = rs.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if upper:
        v[:, 2] = np.abs(v[:, 2])
    return v.astype(F32)


def _bsdf_queries(rs, n):
    q = np.zeros(n, dtype=pod.BSDF_QUERY_DT)
    q["wi"], q["wo"] = _dirs(rs, n, True), _dirs(rs, n, True)
    q["rng"] = rs.randint(1, 2 ** 32 - 1, size=n, dtype=np.uint64).astype(U32)
    return (q,)


def _rays(rs, n):
    t_end = rs.uniform(0.1, 6.0, n).astype(F32)
    t_end[::5] = np.inf  # (a miss)
    return rs.uniform(-2, 2, (n, 3)).astype(F32), _dirs(rs, n), t_end


def _hits(rs, n):
    b = rs.uniform(0, 1, (n, 2))
    fold = b.sum(1) > 1
    b[fold] = 1 - b[fold]
    return rs.randint(0, 2, n).astype(U32), b.astype(F32)


def _fmath_pairs(rs, n):
    a, b = rs.uniform(-4, 4, n), rs.uniform(-4, 4, n)
    a[::7], b[3::11] = np.nan, np.inf  # (NaN results: compared as bit patterns)
    return a, b


# name -> (the inputs of n items from a RandomState, the call, the outputs' (dtype, shape after n))
HOOKS = {
    "bsdf_sample": (_bsdf_queries, lambda c, q: (c.bsdf_sample_batch(MATERIAL, q),), [(pod.BSDF_RESULT_DT, ())]),
    "bsdf_eval": (_bsdf_queries, lambda c, q: (c.bsdf_eval_batch(MATERIAL, q),), [(pod.BSDF_RESULT_DT, ())]),
    "tex2d": (lambda rs, n: (rs.uniform(-0.5, 1.5, (n, 2)).astype(F32),), lambda c, uv: (c.tex2d_batch("diffuse", 0, uv),), [(F32, (4,))]),
    "env_sample": (lambda rs, n: (_unit(rs, n, 2),), lambda c, r: c.env_sample_batch(r), [(F32, (3,)), (F32, ()), (U32, ())]),
    "env_eval": (lambda rs, n: (_dirs(rs, n),), lambda c, d: c.env_eval_batch(d), [(F32, (3,)), (F32, ()), (U32, ())]),
    "analytic_light_sample": (lambda rs, n: (rs.uniform(-1, 1, (n, 3)).astype(F32), _unit(rs, n, 2)), lambda c, o, r: c.analytic_light_sample_batch(0, o, r),
                              [(F32, (3,)), (F32, ()), (F32, (3,)), (np.bool_, ())]),
    "medium_segment": (lambda rs, n: _rays(rs, n) + (_unit(rs, n),), lambda c, *a: c.medium_segment_batch(*a), [(F32, ())] * 4),
    "medium_phase": (lambda rs, n: (_dirs(rs, n), _unit(rs, n), _unit(rs, n)), lambda c, *a: c.medium_phase_batch(*a), [(F32, (3,)), (F32, ())]),
    "medium_density": (lambda rs, n: (rs.uniform(-1.5, 1.5, (n, 3)).astype(F32),), lambda c, p: c.medium_density_batch(p), [(F32, ()), (F32, ())]),
    "medium_track": (lambda rs, n: _rays(rs, n) + (rs.randint(1, 2 ** 32 - 1, size=n, dtype=np.uint64).astype(U32),), lambda c, *a: c.medium_track_batch(*a),
                     [(F32, ()), (F32, ()), (U32, (2,))]),
    "shading_frame": (lambda rs, n: _hits(rs, n) + (_dirs(rs, n),), lambda c, t, uv, d: c.shading_frame_batch(0, t, uv, d), [(F32, (3,)), (F32, ()), (np.bool_, ())]),
    "material_inputs": (_hits, lambda c, t, uv: c.material_inputs_batch(0, t, uv), [(F32, (3,)), (F32, ()), (F32, ())]),
    "fmath": (_fmath_pairs, lambda c, a, b: (c.fmath_batch(pod.NXF_OPS["atan2"], a, b),), [(F64, ())]),
    "light_pick": (lambda rs, n: (_unit(rs, n),), lambda c, u: c.light_pick_batch(u), [(U32, ()), (F32, ())]),
}


def _bits(a):
    """the array's bytes, one row per item: NaNs compare as their bit patterns"""
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _check_shapes(name, outs, n):
    specs = HOOKS[name][2]
    assert len(outs) == len(specs), name
    for k, (out, (dtype, tail)) in enumerate(zip(outs, specs)):
        assert out.dtype == dtype and out.shape == (n,) + tail, (name, k, out.dtype, out.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HOOKS))
def test_one_call_equals_two_calls_on_its_parts(ctx, name):
    make, call, _ = HOOKS[name]
    ins = make(np.random.RandomState(17), N)
    whole = call(ctx, *ins)
    _check_shapes(name, whole, N)
    head, tail = call(ctx, *[a[:1] for a in ins]), call(ctx, *[a[1:] for a in ins])
    _check_shapes(name, head, 1)
    for k, (w, h, t) in enumerate(zip(whole, head, tail)):
        assert np.array_equal(_bits(w), _bits(np.concatenate([h, t]))), (name, "output %d" % k, np.flatnonzero((_bits(w) != _bits(np.concatenate([h, t]))).any(1))[:8])
    assert any(_bits(w).any() for w in whole), "%s: every output is all zero bits — nothing was copied back" % name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HOOKS))
def test_an_empty_batch_gives_empty_arrays(ctx, name):
    make, call, _ = HOOKS[name]
    _check_shapes(name, call(ctx, *make(np.random.RandomState(17), 0)), 0)


@pytest.mark.gpu
def test_the_optional_columns(ctx):
    rs = np.random.RandomState(23)
    d = _dirs(rs, N)
    rgb, pdf, texel = ctx.env_eval_batch(d, with_pdf=False)
    assert pdf is None and texel is None
    with_pdf = ctx.env_eval_batch(d, with_pdf=True)
    assert np.array_equal(_bits(rgb), _bits(with_pdf[0])) and with_pdf[1].shape == (N,) and with_pdf[2].shape == (N,)
    # a one-operand op without b: what tests/test_fmath.py asks of the device — the oracle's bits (the two compile one text)
    a = rs.uniform(-30, 30, N)
    got, want = ctx.fmath_batch(pod.NXF_OPS["sin"], a), O.fmath_batch(pod.NXF_OPS["sin"], a)
    assert got.shape == (N,) and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_the_python_column_helpers():
    """capi._cols / _outs alone (pure numpy): a list, a non-contiguous slice and a float64 array come back contiguous with the asked dtype
    and shape; inputs of unequal lengths raise"""
    wide = np.arange(40, dtype=F64).reshape(10, 4)
    a, b, c, none = capi._cols(([[1, 2, 3], [4, 5, 6]], F32, 3), (wide[:2, ::2], F32, 2), (np.array([7.0, 8.0]), U32, 1), (None, F64, 1))
    assert none is None
    for got, dtype, shape, want in ((a, F32, (2, 3), [[1, 2, 3], [4, 5, 6]]), (b, F32, (2, 2), [[0, 2], [4, 6]]), (c, U32, (2,), [7, 8])):
        assert got.dtype == dtype and got.shape == shape and got.flags["C_CONTIGUOUS"] and np.array_equal(got, want)
    assert capi._cols((np.zeros((0, 3)), F32, 3))[0].shape == (0, 3) and capi._cols(([], U32, 1))[0].shape == (0,)
    flat, = capi._cols((np.arange(6.0), F32, 3))  # (a flat array of n x k values is n rows)
    assert flat.shape == (2, 3)
    with pytest.raises(AssertionError, match="equal lengths"):
        capi._cols((np.zeros((3, 3)), F32, 3), (np.zeros(2), F32, 1))
    with pytest.raises(ValueError):
        capi._cols((np.zeros(4), F32, 3))  # (not a whole number of rows)
    x, y, z = capi._outs(5, (F32, 3), (U32, 1), None)
    assert x.dtype == F32 and x.shape == (5, 3) and not x.any() and y.dtype == U32 and y.shape == (5,) and z is None
    assert capi._outs(0, (F32, 4))[0].shape == (0, 4)
