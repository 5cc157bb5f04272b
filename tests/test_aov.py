"""Feature buffers and denoiser, the part that needs no GPU: the tests' own references are pinned (the primary-ray restatement against
the oracle's wavefront, the numpy filter against the invariants of its definition) and the binding declares what the library exports."""
import re
import os

import numpy as np

from nexus_amd import capi, pod
from tests import aov_reference as R
from tests import oracle_lib as O
from tests import scene_helpers as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("nxhip_set_aov", "nxhip_read_aov", "nxhip_read_aov_frame", "nxhip_write_aov", "nxhip_denoise", "nxhip_denoise_defaults",
             "nxhip_read_denoised", "nxhip_read_denoised_rgba8")


def _twin_matches(name, sc, W, H, frames=(1, 2)):
    """The oracle's wavefront on the twin scene (pathLength 1, emission = albedo, intensity 1: its radiance IS the albedo buffer)
    against the restated primary ray traced by the oracle: every pixel, bit for bit."""
    base = R.material_albedo(sc.materials)
    want_of = []
    for f in frames:
        albedo, _depth, hits, _rays = R.primary_features(sc, W, H, f)
        want_of.append((albedo, float((hits["hitDistance"] < pod.MISS_DISTANCE).mean())))
    sc.materials["emissive"] = base
    sc.materials["intensity"] = 1.0
    sc.materials["emissiveMapId"] = -1
    sc.settings["pathLength"] = 1
    sc.settings["backgroundIntensity"] = 0.0
    w = O.Wavefront(sc.oracle(), W * H, None, pod.RNG_PIXEL_KEYED, pod.CONDUCTOR_EXTENDED)
    for f, (albedo, share) in zip(frames, want_of):
        w.render(f, threads=8)
        twin = np.array(w.radiance(), dtype=np.float32).reshape(-1, 3)
        same = np.all(albedo[:, 0:3].view(np.uint32) == twin.view(np.uint32), axis=1)
        print("%s %dx%d frame %d: %d of %d pixels equal bits; hit share %.3f" % (name, W, H, f, same.sum(), len(same), share))
        assert same.all()
        assert 0.05 < share < 0.95  # hits and misses are both exercised
    w.close()


def test_restatement_equals_oracle_twin_cornell():
    _twin_matches("cornell", SH.cornell_scene(160, 160, path_length=4), 160, 160)


def test_restatement_equals_oracle_twin_zoo():
    zoo = SH.material_zoo_scene(96, 64, hdr=False, textures=False)
    zoo.camera["lensRadius"] = 0.0
    _twin_matches("zoo", zoo, 96, 64)


def test_binding_declares_and_library_exports_the_new_calls():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "nexus_hip.h")).read()
    for s in NEW_CALLS:
        assert s in capi.HIP_SYMBOLS, s
        assert hasattr(L, s), s
        assert re.search(r"\b%s\(" % s, header), s
    for m in ("set_aov", "read_aov", "read_aov_frame", "write_aov", "denoise", "read_denoised", "read_denoised_rgba8"):
        assert callable(getattr(capi.Context, m))
    assert capi.API_VERSION == 8 and re.search(r"#define NXHIP_API_VERSION 8\b", header)


def test_denoise_params_layout_and_defaults():
    dt = pod.DENOISE_DT
    assert dt.itemsize == 20 and [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16]
    pod_h = open(os.path.join(ROOT, "include", "nexus_pod.h")).read()
    body = re.search(r"typedef struct nx_denoise_params \{(.*?)\} nx_denoise_params;", pod_h, re.S).group(1)
    assert re.findall(r"\b(iterations|sigma\w+)\b", body) == list(dt.names)
    # the stamp the library computes from the header = the stamp of the binding's mirrors (nx_denoise_params included)
    words = capi.abi_words()
    assert words[-3:] == [20, 4, 16]
    assert capi.lib().nxhip_abi_stamp() == capi.abi_stamp()
    d = capi.denoise_defaults()[0]
    assert {k: float(d[n]) for k, n in zip(("iterations", "sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"), dt.names)} == \
        {k: float(np.float32(v)) for k, v in R.DEFAULTS.items()}


def test_filter_definition_invariants():
    W, H = 61, 37
    colour, albedo, nd = R.synthetic_inputs(W, H, seed=3)
    p = dict(R.DEFAULTS)
    for dtype in (np.float64, np.float32):
        # iterations = 0 is the identity
        assert np.array_equal(R.atrous(colour, albedo, nd, **dict(p, iterations=0), dtype=dtype), colour.astype(dtype))
        # a constant image is a fixed point
        const = np.empty_like(colour)
        const[...] = (0.25, 0.5, 2.0)
        out = R.atrous(const, albedo, nd, **p, dtype=dtype)
        assert np.max(np.abs(out - const)) <= (R.FIXED_POINT_BOUND if dtype == np.float32 else 1e-14) * 2.0
        # a hard normal edge with sigmaNormal 0.05: |dN|^2 = 2 -> exp(-800) = 0 in either precision; left of the edge nothing depends
        # on the colours right of it
        edge = W // 2
        a2 = np.zeros_like(albedo); a2[...] = (0.5, 0.5, 0.5, 1.0)
        n2 = np.zeros_like(nd); n2[..., 3] = 4.0
        n2[:, :edge, 0] = 1.0
        n2[:, edge:, 1] = 1.0
        other = colour.copy()
        other[:, edge:] = np.random.RandomState(9).uniform(0, 50, other[:, edge:].shape)
        q = dict(p, sigma_normal=0.05)
        o1 = R.atrous(colour, a2, n2, **q, dtype=dtype)
        o2 = R.atrous(other, a2, n2, **q, dtype=dtype)
        assert np.array_equal(o1[:, :edge], o2[:, :edge])
        assert not np.array_equal(o1[:, edge:], o2[:, edge:])
    # and the float32 evaluation stays close to the definition
    dev = R.rel_dev(R.atrous(colour, albedo, nd, **p, dtype=np.float32), R.atrous(colour, albedo, nd, **p, dtype=np.float64))
    print("float32 evaluation against float64: %.3g of the largest value" % dev)
    assert dev < 1e-4


def test_running_mean_matches_accumulate_order():
    rng = np.random.RandomState(1)
    frames = [rng.uniform(0, 2, (50, 4)).astype(np.float32) for _ in range(6)]
    a = frames[0].copy()
    for k in range(2, 7):
        a += (frames[k - 1] - a) / np.float32(k)
    assert R.same_bits(R.running_mean32(frames), a)
