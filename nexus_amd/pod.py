"""numpy views of the POD contracts in ``include/nexus_pod.h``.

Byte layouts follow the reference's device PODs (file:line relative to /root/reference/Nexus/src):
``D_BVH8Node`` Cuda/BVH/BVH8.cuh:47-63, ``D_Triangle`` Cuda/Geometry/Triangle.cuh:25-49,
``D_BVHInstance`` Cuda/BVH/BVHInstance.cuh:7-14, ``D_Material`` Cuda/Scene/Material.cuh:5-51,
``D_Light`` Cuda/Scene/Light.cuh:4-33, ``D_Camera`` Cuda/Scene/Camera.cuh:5-15,
``D_RenderSettings`` Cuda/Scene/Scene.cuh:10-17, ``D_Intersection`` Cuda/Geometry/Ray.cuh:5-15.
"""
import numpy as np

NODE_DT = np.dtype(
    [
        ("p", "<f4", 3),
        ("e", "u1", 3),
        ("imask", "u1"),
        ("childBaseIdx", "<u4"),
        ("triangleBaseIdx", "<u4"),
        ("meta", "u1", 8),
        ("qlox", "u1", 8),
        ("qloy", "u1", 8),
        ("qloz", "u1", 8),
        ("qhix", "u1", 8),
        ("qhiy", "u1", 8),
        ("qhiz", "u1", 8),
    ]
)
assert NODE_DT.itemsize == 80

TRI_DT = np.dtype(
    [
        ("pos0", "<f4", 3),
        ("pos1", "<f4", 3),
        ("pos2", "<f4", 3),
        ("normal0", "<f4", 3),
        ("normal1", "<f4", 3),
        ("normal2", "<f4", 3),
        ("texCoord0", "<f4", 2),
        ("texCoord1", "<f4", 2),
        ("texCoord2", "<f4", 2),
    ]
)
assert TRI_DT.itemsize == 96

INST_DT = np.dtype(
    [
        ("bvhIdx", "<u4"),
        ("invTransform", "<f4", 16),
        ("transform", "<f4", 16),
        ("boundsMin", "<f4", 3),
        ("boundsMax", "<f4", 3),
        ("materialId", "<i4"),
    ]
)
assert INST_DT.itemsize == 160

# The 28-byte union is exposed as raw floats: diffuse/dielectric/plastic use u[0:3]=albedo, u[3]=roughness,
# u[4]=ior; conductor uses u[0:3]=ior, u[3:6]=k, u[6]=roughness.
MAT_DT = np.dtype(
    {
        "names": ["u", "emissive", "intensity", "opacity", "diffuseMapId", "emissiveMapId", "type"],
        "formats": [("<f4", 7), ("<f4", 3), "<f4", "<f4", "<i4", "<i4", "i1"],
        "offsets": [0, 28, 40, 44, 48, 52, 56],
        "itemsize": 60,
    }
)

LIGHT_DT = np.dtype(
    {"names": ["meshId", "aux", "type"], "formats": ["<u4", "<u4", "i1"], "offsets": [0, 4, 8], "itemsize": 12}
)

# nx_analytic_light (extension, nxhip_set_analytic_lights): 64 bytes, world space
ALIGHT_DT = np.dtype([("position", "<f4", 3), ("radius", "<f4"), ("direction", "<f4", 3), ("angularRadius", "<f4"), ("colour", "<f4", 3), ("intensity", "<f4"),
                      ("innerConeAngle", "<f4"), ("outerConeAngle", "<f4"), ("type", "<u4"), ("pad_", "<u4")])
assert ALIGHT_DT.itemsize == 64

# nx_material_detail (extension, nxhip_set_material_detail): 16 bytes, index-parallel to the material table; -1 = no map
DETAIL_DT = np.dtype([("normalMapId", "<i4"), ("roughnessMapId", "<i4"), ("normalScale", "<f4"), ("pad_", "<u4")])
assert DETAIL_DT.itemsize == 16
# nx_material_alpha (extension, nxhip_set_material_alpha): 8 bytes, index-parallel to the material table
ALPHA_BLEND, ALPHA_MASK, ALPHA_OPAQUE = 0, 1, 2
ALPHA_DT = np.dtype([("mode", "<u4"), ("cutoff", "<f4")])
assert ALPHA_DT.itemsize == 8
# nx_skin_corner (extension, nxhip_set_blas_skin): 24 bytes — the four joints and weights of one triangle corner
SKIN_CORNER_DT = np.dtype([("joint", "<u2", 4), ("weight", "<f4", 4)])
assert SKIN_CORNER_DT.itemsize == 24
SKIN_MAX_JOINTS = 65536
# nx_morph_corner (extension, nxhip_set_blas_morph): 24 bytes — the position and normal deltas of one triangle corner under one morph target
MORPH_CORNER_DT = np.dtype([("dPosition", "<f4", 3), ("dNormal", "<f4", 3)])
assert MORPH_CORNER_DT.itemsize == 24
MORPH_MAX_TARGETS = 1024

# nx_medium (extension, nxhip_set_medium): 48 bytes — fog, one homogeneous medium in a world-space box
MEDIUM_DT = np.dtype([("boxMin", "<f4", 3), ("sigmaT", "<f4"), ("boxMax", "<f4", 3), ("g", "<f4"), ("albedo", "<f4", 3), ("pad", "<u4")])
assert MEDIUM_DT.itemsize == 48

# nx_sky (extension, nxhip_set_sky): 76 bytes — the procedural sun-and-sky environment (the model is in include/nexus_hip.h)
SKY_DT = np.dtype([("sunDirection", "<f4", 3), ("sunAngularRadius", "<f4"), ("sunIrradiance", "<f4", 3), ("altitude", "<f4"), ("rayleighScale", "<f4"), ("mieScale", "<f4"),
                   ("mieG", "<f4"), ("groundAlbedo", "<f4", 3), ("width", "<u4"), ("height", "<u4"), ("viewSteps", "<u4"), ("lightSteps", "<u4"), ("sunDisc", "<u4")])
assert SKY_DT.itemsize == 76

CAM_DT = np.dtype(
    {
        "names": ["position", "right", "up", "lensRadius", "lowerLeftCorner", "viewportX", "viewportY", "resolution"],
        "formats": [("<f4", 3), ("<f4", 3), ("<f4", 3), "<f4", ("<f4", 3), ("<f4", 3), ("<f4", 3), ("<u4", 2)],
        "offsets": [0, 12, 24, 36, 40, 52, 64, 80],
        "itemsize": 88,
    }
)

SETTINGS_DT = np.dtype(
    {
        "names": ["useMIS", "pathLength", "backgroundColor", "backgroundIntensity"],
        "formats": ["u1", "u1", ("<f4", 3), "<f4"],
        "offsets": [0, 1, 4, 16],
        "itemsize": 20,
    }
)

RAY_DT = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3)])
HIT_DT = np.dtype([("hitDistance", "<f4"), ("u", "<f4"), ("v", "<f4"), ("triIdx", "<u4"), ("instanceIdx", "<u4")])
LOADED_INST_DT = np.dtype([("mesh", "<i4"), ("material", "<i4"), ("position", "<f4", 3), ("rotation", "<f4", 3), ("scale", "<f4", 3)])
assert LOADED_INST_DT.itemsize == 44
# BSDF test hooks (nx_bsdf_query 32 B, nx_bsdf_result 48 B)
BSDF_QUERY_DT = np.dtype([("wi", "<f4", 3), ("rng", "<u4"), ("wo", "<f4", 3), ("pad_", "<u4")])
BSDF_RESULT_DT = np.dtype([("wo", "<f4", 3), ("pdf", "<f4"), ("throughput", "<f4", 3), ("ok", "<u4"), ("rngOut", "<u4"), ("pad_", "<u4", 3)])
assert BSDF_QUERY_DT.itemsize == 32 and BSDF_RESULT_DT.itemsize == 48

# nx_denoise_params (nxhip_denoise): iterations of the a-trous filter and the widths of its edge-stopping terms
DENOISE_DT = np.dtype([("iterations", "<u4"), ("sigmaColor", "<f4"), ("sigmaNormal", "<f4"), ("sigmaAlbedo", "<f4"), ("sigmaDepth", "<f4")])
assert DENOISE_DT.itemsize == 20
ADAPTIVE_DT = np.dtype([("threshold", "<f4"), ("lumFloor", "<f4"), ("minSamples", "<u4"), ("cull", "<u4")])
assert ADAPTIVE_DT.itemsize == 16

MAT_DIFFUSE, MAT_DIELECTRIC, MAT_PLASTIC, MAT_CONDUCTOR = 0, 1, 2, 3
MAT_METALROUGH = 4  # an extension: glTF's metallic-roughness model (include/nexus_hip.h)
LIGHT_POINT, LIGHT_AREA, LIGHT_MESH = 0, 1, 2
ALIGHT_POINT, ALIGHT_SPOT, ALIGHT_DIRECTIONAL = 0, 1, 2  # nx_analytic_light.type
RNG_REFERENCE_SLOT, RNG_PIXEL_KEYED = 0, 1
COMPACT_FAST, COMPACT_ORDERED = 0, 1
CONDUCTOR_REFERENCE, CONDUCTOR_EXTENDED = 0, 1
ORDER_ROWS, ORDER_TILES = 0, 1  # nxhip_set_pixel_order
LIGHTS_UNIFORM, LIGHTS_POWER = 0, 1  # nxhip_set_light_sampling
LIGHT_IMPORTANCE_POWER, LIGHT_IMPORTANCE_POSITION = 0, 1  # nxhip_set_light_importance
SHADOWS_OPAQUE, SHADOWS_TRANSMIT = 0, 1  # nxhip_set_shadow_transmittance
PATH_MAX_LENGTH = 100
# include/nexus_fmath.h NXF_OP_*: the shared transcendental functions, by number (double: 0-6; float, carried in doubles: 7-12)
NXF_OPS = {"sin": 0, "cos": 1, "exp": 2, "log": 3, "pow": 4, "atan2": 5, "asin": 6, "sinf": 7, "cosf": 8, "expf": 9, "logf": 10, "atan2f": 11, "asinf": 12}
MISS_DISTANCE = np.float32(1e30)


def make_triangles(pos, normals=None, uvs=None):
    """pos: (n,3,3) float array of vertex positions -> TRI_DT array (normals default to the face normal)."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    n = pos.shape[0]
    t = np.zeros(n, dtype=TRI_DT)
    t["pos0"], t["pos1"], t["pos2"] = pos[:, 0], pos[:, 1], pos[:, 2]
    if normals is None:
        fn = np.cross(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0])
        ln = np.linalg.norm(fn, axis=1, keepdims=True)
        fn = np.where(ln > 0, fn / np.maximum(ln, 1e-30), np.array([0, 0, 1], np.float32)).astype(np.float32)
        t["normal0"] = t["normal1"] = t["normal2"] = fn
    else:
        normals = np.asarray(normals, dtype=np.float32)
        t["normal0"], t["normal1"], t["normal2"] = normals[:, 0], normals[:, 1], normals[:, 2]
    if uvs is not None:
        uvs = np.asarray(uvs, dtype=np.float32)
        t["texCoord0"], t["texCoord1"], t["texCoord2"] = uvs[:, 0], uvs[:, 1], uvs[:, 2]
    return t


def make_material(type=MAT_DIFFUSE, albedo=(0.8, 0.8, 0.8), roughness=0.0, ior=1.45, emissive=(0, 0, 0), intensity=0.0,
                  opacity=1.0, conductor_ior=None, conductor_k=None, diffuse_map=-1, emissive_map=-1, metallic=None):
    """metallic: NX_MAT_METALROUGH only (byte 20 of the union; default 1, glTF's)"""
    m = np.zeros((), dtype=MAT_DT)
    if type == MAT_CONDUCTOR:
        m["u"][0:3] = conductor_ior if conductor_ior is not None else (0.2, 0.9, 1.1)
        m["u"][3:6] = conductor_k if conductor_k is not None else (3.9, 2.4, 2.2)
        m["u"][6] = roughness
    else:
        m["u"][0:3] = albedo
        m["u"][3] = roughness
        m["u"][4] = ior
        if type == MAT_METALROUGH:
            m["u"][5] = 1.0 if metallic is None else metallic
    m["emissive"] = emissive
    m["intensity"] = intensity
    m["opacity"] = opacity
    m["diffuseMapId"] = diffuse_map
    m["emissiveMapId"] = emissive_map
    m["type"] = type
    return m


def make_material_alpha(mode=ALPHA_BLEND, cutoff=0.5):
    """one nx_material_alpha record: ALPHA_BLEND (the default: a stochastic blend) or ALPHA_MASK with glTF's alphaCutoff"""
    a = np.zeros((), dtype=ALPHA_DT)
    a["mode"] = mode
    a["cutoff"] = cutoff
    return a


def make_skin_corners(joints, weights):
    """nx_skin_corner records from (n, 4) joint indices and (n, 4) weights: corner 3 i + v is vertex v of triangle i"""
    joints, weights = np.asarray(joints), np.asarray(weights, dtype=np.float32)
    if joints.ndim != 2 or joints.shape[1] != 4 or weights.shape != joints.shape:
        raise ValueError("joints and weights must both be (n, 4)")
    if joints.size and (joints.min() < 0 or joints.max() >= SKIN_MAX_JOINTS):
        raise ValueError("a joint index does not fit 16 bits")
    c = np.zeros(len(joints), dtype=SKIN_CORNER_DT)
    c["joint"], c["weight"] = joints, weights
    return c


def make_morph_corners(d_positions, d_normals=None):
    """nx_morph_corner records, (T, 3 n): d_positions (T, 3 n, 3) position deltas of T targets — or (3 n, 3) for one —, d_normals the
    normal deltas of the same shape (None: zeros, a target without NORMAL).  Corner 3 i + v is vertex v of triangle i."""
    dp = np.asarray(d_positions, dtype=np.float32)
    if dp.ndim == 2:
        dp = dp[None]
    if dp.ndim != 3 or dp.shape[2] != 3 or dp.shape[1] % 3 != 0:
        raise ValueError("position deltas must be (targets, 3 n, 3)")
    dn = np.zeros_like(dp) if d_normals is None else np.asarray(d_normals, dtype=np.float32).reshape(dp.shape)
    c = np.zeros(dp.shape[:2], dtype=MORPH_CORNER_DT)
    c["dPosition"], c["dNormal"] = dp, dn
    return c


def normalise_skin_corners(corners, joint_count):
    """the records as nxhip_set_blas_skin stores them, by its rules: weights divided by their binary64 sum and rounded once, the joint
    of a zero weight rewritten to 0.  ValueError for what the call refuses: a joint count outside 1 .. 65536, a weight that is negative
    or not finite, a joint index >= joint_count under a non-zero weight, a corner whose weights sum to 0."""
    c = np.ascontiguousarray(corners, dtype=SKIN_CORNER_DT).copy()
    if not 1 <= int(joint_count) <= SKIN_MAX_JOINTS:
        raise ValueError("the joint count must be 1 .. %d" % SKIN_MAX_JOINTS)
    w = c["weight"].astype(np.float64)
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("a weight is negative or not finite")
    used = w != 0
    if np.any(c["joint"][used] >= joint_count):
        raise ValueError("a joint index is not below the joint count")
    total = w.sum(axis=1)
    if np.any(total <= 0):
        raise ValueError("the weights of corner %d sum to 0" % int(np.flatnonzero(total <= 0)[0]))
    c["weight"] = (w / total[:, None]).astype(np.float32)
    c["joint"][~used] = 0
    return c


def make_material_detail(normal_map=-1, roughness_map=-1, normal_scale=1.0):
    """one nx_material_detail: ids of nxhip_upload_texture kind 3 / 4 (-1: none) and glTF's normalTexture.scale"""
    d = np.zeros((), dtype=DETAIL_DT)
    d["normalMapId"], d["roughnessMapId"], d["normalScale"] = normal_map, roughness_map, normal_scale
    return d


def make_analytic_light(type=ALIGHT_POINT, position=(0, 0, 0), direction=(0, 0, -1), colour=(1, 1, 1), intensity=1.0, radius=0.0, angular_radius=0.0,
                        inner_cone=0.0, outer_cone=np.pi / 4):
    """one nx_analytic_light: a point or sphere (radius), a spot (direction = its axis, cone angles in radians) or a sun (direction = the way
    the light travels, angular_radius = half-angle of its disc)"""
    l = np.zeros((), dtype=ALIGHT_DT)
    l["type"] = type
    l["position"] = position
    l["direction"] = direction
    l["colour"] = colour
    l["intensity"] = intensity
    l["radius"] = radius
    l["angularRadius"] = angular_radius
    if type == ALIGHT_SPOT:
        l["innerConeAngle"], l["outerConeAngle"] = inner_cone, outer_cone
    return l


def make_medium(box_min=(0, 0, 0), box_max=(1, 1, 1), sigma_t=0.0, g=0.0, albedo=(1, 1, 1)):
    """one nx_medium: the world-space box, the grey extinction per world unit (0: no medium), the Henyey-Greenstein asymmetry (forward > 0)
    and the single-scattering albedo per channel"""
    m = np.zeros((), dtype=MEDIUM_DT)
    m["boxMin"], m["boxMax"], m["sigmaT"], m["g"], m["albedo"] = box_min, box_max, sigma_t, g, albedo
    return m


def Sky(**fields):
    """one nx_sky: the values of nxhip_sky_defaults (sun at 45 degrees elevation along +x, 2048 x 1024, steps 64 / 16, no disc) with
    `fields` (names of SKY_DT) replacing them"""
    s = np.zeros((), dtype=SKY_DT)
    s["sunDirection"] = (np.sqrt(0.5), np.sqrt(0.5), 0.0)
    s["sunAngularRadius"], s["sunIrradiance"], s["altitude"] = 0.004675, 1.0, 1.0
    s["rayleighScale"], s["mieScale"], s["mieG"], s["groundAlbedo"] = 1.0, 1.0, 0.8, 0.3
    s["width"], s["height"], s["viewSteps"], s["lightSteps"], s["sunDisc"] = 2048, 1024, 64, 16, 0
    for name, value in fields.items():
        s[name] = value  # (a name SKY_DT does not have is numpy's ValueError)
    return s
