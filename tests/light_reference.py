"""numpy restatement of the light table of NXHIP_LIGHTS_POWER (include/nexus_hip.h, nx_lights.hip): float64 weights from instances,
triangles and materials; the table as specified; the pick as searchsorted; the guide (cut-point) construction and its walk.

Nothing here is shared with the device code: weights come from float64 geometry, the cumulative table from numpy's cumsum."""
import numpy as np

from nexus_amd import pod

LUMA = np.array([0.2126, 0.7152, 0.0722])
GUIDE_MAX = 1 << 23  # rng_next's resolution


def srgb_decode(byte):
    """the library's 256-entry table (sRGB -> linear), in float64"""
    x = np.asarray(byte, dtype=np.float64) / 255.0
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def map_mean(rgba8):
    """mean of a map's sRGB-decoded texels, alpha ignored"""
    img = np.asarray(rgba8, dtype=np.uint8).reshape(-1, 4)
    return srgb_decode(img[:, :3]).mean(axis=0)


def light_luminance(material, emissive_maps):
    """Y = intensity x luminance of the emissive factor — or, with an emissive map, of the map's mean texel"""
    rgb = np.asarray(material["emissive"], dtype=np.float64)
    if int(material["emissiveMapId"]) != -1:
        rgb = map_mean(emissive_maps[int(material["emissiveMapId"])])
    return float(material["intensity"]) * float(np.dot(LUMA, rgb))


def world_areas(tris, transform16):
    """float64 world-space areas of TRI_DT triangles under a row-major 4 x 4 matrix"""
    M = np.asarray(transform16, dtype=np.float64).reshape(4, 4)
    p = [np.asarray(tris["pos%d" % k], dtype=np.float64) @ M[:3, :3].T + M[:3, 3] for k in range(3)]
    return 0.5 * np.linalg.norm(np.cross(p[1] - p[0], p[2] - p[0]), axis=1)


def weights(meshes, instances, materials, lights, emissive_maps=()):
    """(w float64[N], entryLight uint32[N], lightBase uint32[L + 1]): entries by light (list order), then by triangle index"""
    w, entry_light, base = [], [], [0]
    for l, light in enumerate(lights):
        if int(light["type"]) == pod.LIGHT_MESH:
            inst = instances[int(light["meshId"])]
            tris = meshes[int(inst["bvhIdx"])]
            wl = world_areas(tris, inst["transform"]) * light_luminance(materials[int(inst["materialId"])], emissive_maps)
            w.append(np.where(np.isfinite(wl) & (wl > 0.0), wl, 0.0))  # negative or not finite: 0
            entry_light.append(np.full(len(tris), l, dtype=np.uint32))
        base.append(base[-1] + (len(w[-1]) if int(light["type"]) == pod.LIGHT_MESH else 0))
    if not w:
        return np.zeros(0), np.zeros(0, np.uint32), np.asarray(base, np.uint32)
    return np.concatenate(w), np.concatenate(entry_light), np.asarray(base, np.uint32)


def scene_weights(scene):
    return weights(scene.meshes, scene.instances, scene.materials, scene.lights, scene.emissive_maps)


def shares(w):
    """float64 probability of every entry"""
    return w / w.sum()


def table(w):
    """cdf float32[N]: inclusive float64 prefix sums / total, rounded to binary32, the last entry exactly 1; None: total 0 (invalid)"""
    total = w.sum()
    if not (np.isfinite(total) and total > 0.0):
        return None
    cdf = (np.cumsum(w) / total).astype(np.float32)
    cdf[-1] = np.float32(1.0)
    return cdf


def probabilities(cdf):
    """P(i) = cdf[i] - cdf[i - 1] in binary32, cdf[-1] = 0: what sampler and MIS lookup both read"""
    return np.diff(np.concatenate([np.zeros(1, np.float32), cdf])).astype(np.float32)


def pick(cdf, u):
    """min(searchsorted(cdf, u, 'right'), N - 1)"""
    return np.minimum(np.searchsorted(cdf, np.asarray(u, np.float32), side="right"), len(cdf) - 1).astype(np.uint32)


def guide_size(n):
    g = 1
    while g < n and g < GUIDE_MAX:
        g <<= 1
    return g


def guide(cdf):
    """guide[k] = the smallest i with cdf[i] > k / G, G = the power of two >= N (k / G is exact in binary32)"""
    G = guide_size(len(cdf))
    cuts = (np.arange(G, dtype=np.float64) / G).astype(np.float32)
    assert np.array_equal(cuts.astype(np.float64) * G, np.arange(G, dtype=np.float64))
    return np.searchsorted(cdf, cuts, side="right").astype(np.uint32)


def guided_pick(cdf, gd, u):
    """the device's walk: k = floor(u G); i = guide[k]; while cdf[i] <= u: i++  —  returns (entry, steps walked)"""
    u = np.asarray(u, np.float32)
    G = np.float32(len(gd))
    prod = u * G
    assert np.array_equal(prod.astype(np.float64), u.astype(np.float64) * len(gd)), "u G is exact in binary32"
    i = gd[prod.astype(np.uint32)].astype(np.int64)
    steps = np.zeros(len(u), np.int64)
    while True:
        go = cdf[i] <= u
        if not go.any():
            return i.astype(np.uint32), steps
        assert np.all(i[go] + 1 < len(cdf)), "cdf[N - 1] = 1 > u ends every walk"
        i = i + go
        steps += go
