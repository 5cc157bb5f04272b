"""ctypes binding of ``nexus_amd/lib/libnexus_amd.so`` — the C-ABI declared in ``include/nexus_hip.h`` (device
layer) and ``include/nexus_host.h`` (host builders).

The headers are the only place where a function's signature is written down: ``cabi`` reads their prototypes, and ``lib()`` sets
``restype`` and ``argtypes`` of every declared function once, when it loads the library.  Every pointer is a ``c_void_p``.

There is no Python / CPU fallback: if the library is missing or a device call fails, an exception is raised.
"""
import ctypes as C
import os

import numpy as np

from . import cabi, pod
from .cabi import NexusError  # noqa: F401  (the one exception type of the binding)

_HERE = os.path.dirname(os.path.abspath(__file__))
# NEXUS_AMD_LIB: another build of the same library (tools/ab_bench.sh compares kernel variants); still no fallback
LIB_PATH = os.environ.get("NEXUS_AMD_LIB") or os.path.join(_HERE, "lib", "libnexus_amd.so")

# every function include/nexus_hip.h and include/nexus_host.h declare, in their order, and {name: (restype, [argtypes])} of them all
_TABLES = cabi.signatures()
HIP_SYMBOLS = list(_TABLES["nexus_hip.h"])
HOST_SYMBOLS = list(_TABLES["nexus_host.h"])
SIGNATURES = {**_TABLES["nexus_hip.h"], **_TABLES["nexus_host.h"]}


class QueueSizes(C.Structure):
    _fields_ = [(n, C.c_int32 * pod.PATH_MAX_LENGTH) for n in
                ("traceSize", "traceShadowSize", "diffuseSize", "plasticSize", "dielectricSize", "conductorSize")]


class TraceStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("nodes", C.c_uint64), ("tris", C.c_uint64), ("instances", C.c_uint64),
                ("waveIters", C.c_uint64), ("lanesActive", C.c_uint64), ("lanesNode", C.c_uint64), ("lanesPrim", C.c_uint64), ("cycles", C.c_uint64 * 8)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "cycles"}
        d["cycles"] = [int(x) for x in self.cycles]
        return d


class KernelTimes(C.Structure):
    _fields_ = [("ms", C.c_double * 7), ("launches", C.c_uint64 * 7)]


KERNEL_CLASSES = ("generate", "trace", "shadow", "logic", "shade", "accumulate", "thin")

API_VERSION = 8  # NXHIP_API_VERSION of the include/nexus_hip.h these bindings were written against


def abi_words():
    """The list nxhip_header_abi_stamp() hashes (include/nexus_hip.h), from THIS module's mirrors of the C structs: API version
    and the size / key offsets of everything that crosses the boundary."""
    off = lambda dt, name: dt.fields[name][1]  # noqa: E731
    return [
        API_VERSION, pod.PATH_MAX_LENGTH,
        pod.NODE_DT.itemsize, off(pod.NODE_DT, "meta"), pod.TRI_DT.itemsize, off(pod.TRI_DT, "texCoord0"),
        pod.INST_DT.itemsize, off(pod.INST_DT, "transform"), off(pod.INST_DT, "materialId"),
        pod.MAT_DT.itemsize, off(pod.MAT_DT, "emissive"), off(pod.MAT_DT, "type"), pod.LIGHT_DT.itemsize, off(pod.LIGHT_DT, "type"),
        pod.ALIGHT_DT.itemsize, off(pod.ALIGHT_DT, "direction"), off(pod.ALIGHT_DT, "colour"), off(pod.ALIGHT_DT, "innerConeAngle"), off(pod.ALIGHT_DT, "type"),
        pod.DETAIL_DT.itemsize, off(pod.DETAIL_DT, "normalScale"), pod.MEDIUM_DT.itemsize, pod.ALPHA_DT.itemsize, off(pod.ALPHA_DT, "cutoff"),
        pod.SKIN_CORNER_DT.itemsize, off(pod.SKIN_CORNER_DT, "weight"), pod.MORPH_CORNER_DT.itemsize, off(pod.MORPH_CORNER_DT, "dNormal"),
        pod.CAM_DT.itemsize, off(pod.CAM_DT, "resolution"), pod.SETTINGS_DT.itemsize, off(pod.SETTINGS_DT, "backgroundColor"),
        pod.RAY_DT.itemsize, pod.HIT_DT.itemsize, pod.BSDF_QUERY_DT.itemsize, pod.BSDF_RESULT_DT.itemsize, off(pod.BSDF_RESULT_DT, "rngOut"),
        C.sizeof(QueueSizes), C.sizeof(TraceStats), TraceStats.cycles.offset, C.sizeof(KernelTimes), len(KERNEL_CLASSES),
        pod.SKY_DT.itemsize, off(pod.SKY_DT, "altitude"), off(pod.SKY_DT, "groundAlbedo"), off(pod.SKY_DT, "width"), off(pod.SKY_DT, "sunDisc"),
        pod.ADAPTIVE_DT.itemsize, off(pod.ADAPTIVE_DT, "minSamples"), off(pod.ADAPTIVE_DT, "cull"),
        pod.DENOISE_DT.itemsize, off(pod.DENOISE_DT, "sigmaColor"), off(pod.DENOISE_DT, "sigmaDepth"),
    ]


def abi_stamp(words=None):
    """FNV-1a over the little-endian 8-byte words: nxhip_header_abi_stamp() as these bindings would compute it"""
    h = 0xcbf29ce484222325
    for w in (abi_words() if words is None else words):
        for _ in range(8):
            h = ((h ^ (w & 0xff)) * 0x100000001b3) & 0xffffffffffffffff
            w >>= 8
    return h


def _declare(L, names):
    """Give the functions `names` of the library the signatures their prototypes declare."""
    for name in names:
        try:
            fn = getattr(L, name)
        except AttributeError:
            raise NexusError(f"{LIB_PATH} does not export {name}, which the headers declare: rebuild it with `make`") from None
        fn.restype, fn.argtypes = SIGNATURES[name]


def check_library(L, stamp=None):
    """Refuse a library that does not match these bindings — a stale build reached through NEXUS_AMD_LIB, a library linked
    from objects of different source states — with an error instead of a GPU fault in the first launch."""
    if not hasattr(L, "nxhip_check_library"):
        raise NexusError(f"{LIB_PATH} predates the ABI stamp (no nxhip_check_library): rebuild it with `make`")
    _declare(L, ("nxhip_check_library", "nxhip_abi_stamp", "nxhip_last_error"))
    rc = L.nxhip_check_library(abi_stamp() if stamp is None else stamp)
    if rc != 0:
        raise NexusError("%s: %s" % (LIB_PATH, (L.nxhip_last_error() or b"").decode()))


_lib = None


def lib():
    """Load the shared library (once).  Raises NexusError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NexusError(f"{LIB_PATH} is missing: build it with `make` (or __graft_entry__.build()); there is no fallback path")
    L = C.CDLL(LIB_PATH)
    check_library(L)
    _declare(L, SIGNATURES)
    _lib = L
    return L


_F32, _U32 = np.float32, np.uint32  # (the batch hooks' column types)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _cols(*specs):
    """the inputs of a batch hook, one (values, dtype, k) each, as contiguous arrays of `dtype`: (n, k), or (n,) for k == 1 — all of one n.
    (values None: an optional input that is left out, None back)"""
    cols = [None if a is None else np.ascontiguousarray(a, dtype=dt).reshape(-1, *((k,) if k != 1 else ())) for a, dt, k in specs]
    assert len({len(a) for a in cols if a is not None}) <= 1, "the inputs of a batch hook must have equal lengths"
    return cols


def _outs(n, *specs):
    """the outputs of a batch hook for n items, one (dtype, k) each, zeroed: (n, k), or (n,) for k == 1 (a spec of None: None back)"""
    return [None if s is None else np.zeros((n, s[1]) if s[1] != 1 else n, dtype=s[0]) for s in specs]


def check(rc, what=""):
    if rc != 0:
        msg = lib().nxhip_last_error()
        raise NexusError(f"{what} failed (status {rc}): {msg.decode() if msg else ''}")


def _copy_out(addr, count, dtype):
    if count == 0:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(addr)
    return np.frombuffer(buf, dtype=dtype, count=count).copy()


# ---- sun and sky (no context needed) ------------------------------------------------------------------

def sky_defaults():
    """nxhip_sky_defaults: a pod.SKY_DT record"""
    s = np.zeros(1, dtype=pod.SKY_DT)
    check(lib().nxhip_sky_defaults(_ptr(s)), "nxhip_sky_defaults")
    return s[0]


def sky_sun_light(sky):
    """nxhip_sky_sun_light: the sky's sun as a pod.ALIGHT_DT record (NX_ALIGHT_DIRECTIONAL) for Context.set_analytic_lights — an
    alternative to sunDisc = 1, never both"""
    s = np.ascontiguousarray(sky, dtype=pod.SKY_DT).reshape(1)
    out = np.zeros(1, dtype=pod.ALIGHT_DT)
    check(lib().nxhip_sky_sun_light(_ptr(s), _ptr(out)), "nxhip_sky_sun_light")
    return out[0]


# ---- host builders --------------------------------------------------------------------------------

def bvh8_build(tris, threads=0):
    """BVH8Builder(tris).Init().Build() -> (nodes NODE_DT[], triIdx u32[])."""
    tris = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
    h = C.c_void_p()
    rc = lib().nxh_bvh8_build(_ptr(tris), len(tris), threads, C.byref(h))
    if rc != 0:
        raise NexusError(f"nxh_bvh8_build failed ({rc})")
    try:
        nodes = _copy_out(lib().nxh_bvh8_nodes(h), lib().nxh_bvh8_node_count(h), pod.NODE_DT)
        idx = _copy_out(lib().nxh_bvh8_prim_indices(h), lib().nxh_bvh8_prim_count(h), np.uint32)
    finally:
        lib().nxh_bvh8_free(h)
    return nodes, idx


def tlas_build(instances):
    instances = np.ascontiguousarray(instances, dtype=pod.INST_DT)
    h = C.c_void_p()
    rc = lib().nxh_tlas_build(_ptr(instances), len(instances), C.byref(h))
    if rc != 0:
        raise NexusError(f"nxh_tlas_build failed ({rc})")
    try:
        nodes = _copy_out(lib().nxh_bvh8_nodes(h), lib().nxh_bvh8_node_count(h), pod.NODE_DT)
        idx = _copy_out(lib().nxh_bvh8_prim_indices(h), lib().nxh_bvh8_prim_count(h), np.uint32)
    finally:
        lib().nxh_bvh8_free(h)
    return nodes, idx


BVH2_NODE_DT = np.dtype([("aabbMin", "<f4", 3), ("aabbMax", "<f4", 3), ("leftFirst", "<u4"), ("triCount", "<u4")])


def bvh2_build(tris, threads=0):
    tris = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
    nodes = np.zeros(2 * len(tris) - 1, dtype=BVH2_NODE_DT)
    idx = np.zeros(len(tris), dtype=np.uint32)
    rc = lib().nxh_bvh2_build(_ptr(tris), len(tris), threads, _ptr(nodes), _ptr(idx))
    if rc != 0:
        raise NexusError(f"nxh_bvh2_build failed ({rc})")
    return nodes, idx


def mat4_from_trs(pos=(0, 0, 0), rot_deg=(0, 0, 0), scale=(1, 1, 1)):
    out = np.zeros(16, np.float32)
    p, r, s = (np.asarray(x, np.float32) for x in (pos, rot_deg, scale))
    lib().nxh_mat4_from_trs(_ptr(p), _ptr(r), _ptr(s), _ptr(out))
    return out


def mat4_invert(m):
    m = np.ascontiguousarray(m, np.float32)
    out = np.zeros(16, np.float32)
    lib().nxh_mat4_invert(_ptr(m), _ptr(out))
    return out


def instance_init(bvh_idx, material_id, transform, blas_root_node):
    inst = np.zeros(1, dtype=pod.INST_DT)
    t = np.ascontiguousarray(transform, np.float32)
    root = np.ascontiguousarray(blas_root_node, dtype=pod.NODE_DT).reshape(1)
    rc = lib().nxh_instance_init(_ptr(inst), int(bvh_idx), int(material_id), _ptr(t), _ptr(root))
    if rc != 0:
        raise NexusError(f"nxh_instance_init failed ({rc})")
    return inst[0]


def camera_init(position, forward, hfov_deg, width, height, focus_dist=5.0, defocus_deg=0.0):
    cam = np.zeros(1, dtype=pod.CAM_DT)
    p = np.asarray(position, np.float32)
    f = np.asarray(forward, np.float32)
    rc = lib().nxh_camera_init(_ptr(cam), _ptr(p), _ptr(f), hfov_deg, width, height, focus_dist, defocus_deg)
    if rc != 0:
        raise NexusError(f"nxh_camera_init failed ({rc})")
    return cam[0]


# ---- device context -------------------------------------------------------------------------------

def tlas_refit(nodes, inst_idx, instances):
    """In-place-style refit of a TLAS (returns the new node array): same topology, bounds from the instances' current boxes."""
    nodes = np.ascontiguousarray(nodes, dtype=pod.NODE_DT).copy()
    inst_idx = np.ascontiguousarray(inst_idx, dtype=np.uint32)
    instances = np.ascontiguousarray(instances, dtype=pod.INST_DT)
    if lib().nxh_tlas_refit(_ptr(nodes), len(nodes), _ptr(inst_idx), _ptr(instances), len(instances)) != 0:
        raise NexusError("nxh_tlas_refit: malformed TLAS")
    return nodes


def bvh8_refit(nodes, tri_idx, tris):
    """Refit of a BLAS to moved vertices (returns the new node array): same topology, bounds from the triangles' vertex boxes.
    The byte reference of Context.update_blas."""
    nodes = np.ascontiguousarray(nodes, dtype=pod.NODE_DT).copy()
    tri_idx = np.ascontiguousarray(tri_idx, dtype=np.uint32)
    tris = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
    if lib().nxh_bvh8_refit(_ptr(nodes), len(nodes), _ptr(tri_idx), _ptr(tris), len(tris)) != 0:
        raise NexusError("nxh_bvh8_refit: malformed BLAS")
    return nodes


LOAD_METAL_ROUGH = 1  # nxh_load_scene_file_ex: NXH_LOAD_METAL_ROUGH


def load_scene_file(path, metal_rough=False):
    """nexus::OBJLoader::Parse through the C-ABI: (meshes [TRI_DT arrays], materials MAT_DT array, instances LOADED_INST_DT array).
    metal_rough: LoadOptions::metalRough — a .glb's materials as MAT_METALROUGH (off: the reference's PLASTIC)"""
    L = lib()
    h = C.c_void_p()
    if metal_rough:
        rc = L.nxh_load_scene_file_ex(str(path).encode(), LOAD_METAL_ROUGH, C.byref(h))
    else:
        rc = L.nxh_load_scene_file(str(path).encode(), C.byref(h))
    if rc != 0:
        raise NexusError("nxh_load_scene_file: " + L.nxs_last_error().decode())
    try:
        meshes = []
        for m in range(L.nxh_loaded_mesh_count(h)):
            t = np.zeros(L.nxh_loaded_mesh_triangle_count(h, m), dtype=pod.TRI_DT)
            if L.nxh_loaded_mesh_triangles(h, m, _ptr(t)) != 0:
                raise NexusError(L.nxs_last_error().decode())
            meshes.append(t)
        mats = np.zeros(L.nxh_loaded_material_count(h), dtype=pod.MAT_DT)
        if L.nxh_loaded_materials(h, _ptr(mats)) != 0:
            raise NexusError(L.nxs_last_error().decode())
        insts = np.zeros(L.nxh_loaded_instance_count(h), dtype=pod.LOADED_INST_DT)
        if L.nxh_loaded_instances(h, _ptr(insts)) != 0:
            raise NexusError(L.nxs_last_error().decode())
    finally:
        L.nxh_loaded_scene_free(h)
    return meshes, mats, insts


LOAD_ALPHA_MODES = 2  # nxh_load_scene_file_ex: NXH_LOAD_ALPHA_MODES


def load_scene_material_alpha(path, alpha_modes=True):
    """the alpha modes of a .glb's materials as the C++ reader makes them (LoadOptions::alphaModes): pod.ALPHA_DT records, one per material;
    none when the reader is not asked (alpha_modes=False)"""
    L = lib()
    h = C.c_void_p()
    if L.nxh_load_scene_file_ex(str(path).encode(), LOAD_ALPHA_MODES if alpha_modes else 0, C.byref(h)) != 0:
        raise NexusError("nxh_load_scene_file_ex: " + L.nxs_last_error().decode())
    try:
        n = C.c_uint32(0)
        if L.nxh_loaded_material_alpha(h, None, 0, C.byref(n)) != 0:
            raise NexusError(L.nxs_last_error().decode())
        out = np.zeros(n.value, dtype=pod.ALPHA_DT)
        if n.value and L.nxh_loaded_material_alpha(h, _ptr(out), n.value, C.byref(n)) != 0:
            raise NexusError(L.nxs_last_error().decode())
    finally:
        L.nxh_loaded_scene_free(h)
    return out


LOAD_SKINS = 4  # nxh_load_scene_file_ex: NXH_LOAD_SKINS


def load_scene_skins(path, skins=True):
    """the skins of a .glb as the C++ reader makes them (LoadOptions::skins): per loaded mesh its pod.SKIN_CORNER_DT records (None: not
    skinned) and joint count, then the animation count and the reader's warnings -> (corner arrays, joint counts, animations, warnings)"""
    L = lib()
    h = C.c_void_p()
    if L.nxh_load_scene_file_ex(str(path).encode(), LOAD_SKINS if skins else 0, C.byref(h)) != 0:
        raise NexusError("nxh_load_scene_file_ex: " + L.nxs_last_error().decode())
    try:
        corners, joints = [], []
        for m in range(L.nxh_loaded_mesh_count(h)):
            n, j = C.c_uint32(0), C.c_uint32(0)
            if L.nxh_loaded_skin(h, m, None, 0, C.byref(n), C.byref(j)) != 0:
                raise NexusError(L.nxs_last_error().decode())
            out = np.zeros(n.value, dtype=pod.SKIN_CORNER_DT) if n.value else None
            if n.value and L.nxh_loaded_skin(h, m, _ptr(out), n.value, C.byref(n), C.byref(j)) != 0:
                raise NexusError(L.nxs_last_error().decode())
            corners.append(out)
            joints.append(int(j.value))
        warnings = [L.nxh_loaded_warning(h, i).decode() for i in range(L.nxh_loaded_warning_count(h))]
        animations = int(L.nxh_loaded_animation_count(h))
    finally:
        L.nxh_loaded_scene_free(h)
    return corners, joints, animations, warnings


LOAD_MORPHS = 8  # nxh_load_scene_file_ex: NXH_LOAD_MORPHS


def load_scene_morphs(path, skins=False, morphs=True):
    """the morph targets of a .glb as the C++ reader makes them (LoadOptions::morphs, with LoadOptions::skins beside it if asked): per loaded
    mesh its (targets, 3 n) pod.MORPH_CORNER_DT records (None: no targets) and default weights, then the animation count and the reader's
    warnings -> (delta arrays, weight arrays, animations, warnings)"""
    L = lib()
    h = C.c_void_p()
    if L.nxh_load_scene_file_ex(str(path).encode(), (LOAD_MORPHS if morphs else 0) | (LOAD_SKINS if skins else 0), C.byref(h)) != 0:
        raise NexusError("nxh_load_scene_file_ex: " + L.nxs_last_error().decode())
    try:
        deltas, weights = [], []
        for m in range(L.nxh_loaded_mesh_count(h)):
            n, t = C.c_uint32(0), C.c_uint32(0)
            if L.nxh_loaded_morph(h, m, None, 0, C.byref(n), C.byref(t), None) != 0:
                raise NexusError(L.nxs_last_error().decode())
            out = np.zeros((t.value, n.value), dtype=pod.MORPH_CORNER_DT) if t.value else None
            w = np.zeros(t.value, np.float32) if t.value else None
            if t.value and L.nxh_loaded_morph(h, m, _ptr(out), out.size, C.byref(n), C.byref(t), _ptr(w)) != 0:
                raise NexusError(L.nxs_last_error().decode())
            deltas.append(out)
            weights.append(w)
        warnings = [L.nxh_loaded_warning(h, i).decode() for i in range(L.nxh_loaded_warning_count(h))]
        animations = int(L.nxh_loaded_animation_count(h))
    finally:
        L.nxh_loaded_scene_free(h)
    return deltas, weights, animations, warnings


def load_scene_analytic_lights(path):
    """the KHR_lights_punctual lights of a .glb as the C++ reader makes them: pod.ALIGHT_DT records, one per node that carries a light"""
    L = lib()
    h = C.c_void_p()
    if L.nxh_load_scene_file(str(path).encode(), C.byref(h)) != 0:
        raise NexusError("nxh_load_scene_file: " + L.nxs_last_error().decode())
    try:
        lights = np.zeros(L.nxh_loaded_analytic_light_count(h), dtype=pod.ALIGHT_DT)
        if len(lights) and L.nxh_loaded_analytic_lights(h, _ptr(lights)) != 0:
            raise NexusError(L.nxs_last_error().decode())
    finally:
        L.nxh_loaded_scene_free(h)
    return lights


def load_scene_detail(path):
    """The detail maps of a scene file as the C++ reader makes them: (detail textures [(kind "normal" / "roughness", HxWx4 uint8)], normal
    texture index per material, roughness texture index per material, normal scale per material, warnings)."""
    L = lib()
    h = C.c_void_p()
    if L.nxh_load_scene_file(str(path).encode(), C.byref(h)) != 0:
        raise NexusError("nxh_load_scene_file: " + L.nxs_last_error().decode())
    try:
        textures = []
        for i in range(L.nxh_loaded_detail_texture_count(h)):
            w, hh, kind = C.c_uint32(), C.c_uint32(), C.c_int32()
            if L.nxh_loaded_detail_texture_info(h, i, C.byref(w), C.byref(hh), C.byref(kind)) != 0:
                raise NexusError(L.nxs_last_error().decode())
            px = np.zeros((hh.value, w.value, 4), dtype=np.uint8)
            if L.nxh_loaded_detail_texture_pixels(h, i, _ptr(px)) != 0:
                raise NexusError(L.nxs_last_error().decode())
            textures.append(("normal" if kind.value == 3 else "roughness", px))
        n = L.nxh_loaded_material_count(h)
        normal, rough, scale = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        if L.nxh_loaded_material_detail(h, _ptr(normal), _ptr(rough), _ptr(scale)) != 0:
            raise NexusError(L.nxs_last_error().decode())
        warnings = [L.nxh_loaded_warning(h, i).decode() for i in range(L.nxh_loaded_warning_count(h))]
    finally:
        L.nxh_loaded_scene_free(h)
    return textures, normal.tolist(), rough.tolist(), scale.tolist(), warnings


def load_scene_textures(path):
    """The images of a scene file as the C++ reader decodes them: (textures [(kind, HxWx4 uint8)], diffuse texture index
    per material, emissive texture index per material, warnings)."""
    L = lib()
    h = C.c_void_p()
    if L.nxh_load_scene_file(str(path).encode(), C.byref(h)) != 0:
        raise NexusError("nxh_load_scene_file: " + L.nxs_last_error().decode())
    try:
        texs = []
        for i in range(L.nxh_loaded_texture_count(h)):
            w, hh, k = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
            if L.nxh_loaded_texture_info(h, i, C.byref(w), C.byref(hh), C.byref(k)) != 0:
                raise NexusError(L.nxs_last_error().decode())
            px = np.zeros((hh.value, w.value, 4), dtype=np.uint8)
            if L.nxh_loaded_texture_pixels(h, i, _ptr(px)) != 0:
                raise NexusError(L.nxs_last_error().decode())
            texs.append(("emissive" if k.value == 1 else "diffuse", px))
        n = L.nxh_loaded_material_count(h)
        dt, et = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        if L.nxh_loaded_material_textures(h, _ptr(dt), _ptr(et)) != 0:
            raise NexusError(L.nxs_last_error().decode())
        warns = [L.nxh_loaded_warning(h, i).decode() for i in range(L.nxh_loaded_warning_count(h))]
    finally:
        L.nxh_loaded_scene_free(h)
    return texs, dt, et, warns


def decode_png(data):
    """nexus::IMGLoader::LoadIMG through the C-ABI: (HxWx4 uint8, channels of the file)"""
    L = lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    w, h, ch = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    if L.nxh_decode_png(_ptr(buf), len(buf), C.byref(w), C.byref(h), C.byref(ch), None, 0) != 0:
        raise NexusError("nxh_decode_png: " + L.nxs_last_error().decode())
    out = np.zeros((h.value, w.value, 4), dtype=np.uint8)
    if L.nxh_decode_png(_ptr(buf), len(buf), C.byref(w), C.byref(h), C.byref(ch), _ptr(out), out.size) != 0:
        raise NexusError("nxh_decode_png: " + L.nxs_last_error().decode())
    return out, int(ch.value)


def decode_npy_grid(data):
    """IMGLoader::LoadNPYGrid on a .npy file in memory: the fog density grid it holds, float32 of shape (nz, ny, nx)."""
    L = lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    dims = (C.c_uint32 * 3)()
    if L.nxh_decode_npy_grid(_ptr(buf), len(buf), dims, None, 0) != 0:
        raise NexusError("nxh_decode_npy_grid: " + L.nxs_last_error().decode())
    out = np.zeros((dims[2], dims[1], dims[0]), dtype=np.float32)
    if L.nxh_decode_npy_grid(_ptr(buf), len(buf), dims, _ptr(out), out.size) != 0:
        raise NexusError("nxh_decode_npy_grid: " + L.nxs_last_error().decode())
    return out


def decode_hdr_float(data):
    """IMGLoader::LoadHDRFloat on a Radiance .hdr file in memory: HxWx3 float32 of linear radiance."""
    L = lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    w, h = C.c_uint32(0), C.c_uint32(0)
    if L.nxh_decode_hdr_float(_ptr(buf), len(buf), C.byref(w), C.byref(h), None, 0) != 0:
        raise NexusError("nxh_decode_hdr_float: " + L.nxs_last_error().decode())
    out = np.zeros((h.value, w.value, 3), dtype=np.float32)
    if L.nxh_decode_hdr_float(_ptr(buf), len(buf), C.byref(w), C.byref(h), _ptr(out), out.size) != 0:
        raise NexusError("nxh_decode_hdr_float: " + L.nxs_last_error().decode())
    return out


def decode_image(data):
    """IMGLoader::LoadIMG on an image file in memory — PNG, JPEG or Radiance .hdr by its signature: (HxWx4 uint8, channels)."""
    return decode_png(data)


FLAVOR_IDENTITY, FLAVOR_NO_MAPS = 256, 512  # Context.debug_pass_flavor: the specialised kernel instances of a pass graph
FLAVOR_ANALYTIC = 1024  # ... and the instances of a context with analytic lights (set_analytic_lights)
FLAVOR_DETAIL = 4096  # ... and the DETAIL instances of the material kernels: some material names a normal or a roughness map (set_material_detail)
TEXTURE_KINDS = {"diffuse": 0, "emissive": 1, "hdr": 2, "normal": 3, "roughness": 4}  # nxhip_upload_texture / nxhip_tex2d_batch
FLAVOR_MEDIUM = 8192  # ... and the medium's two launches per bounce: a medium with sigmaT > 0 is set (set_medium)
FLAVOR_MEDIUM_GRID = 16384  # ... and their GRID instances: a medium with sigmaT > 0 and a density grid are set (set_medium_density)
FLAVOR_METAL = 32768  # ... and the METAL instances of the material launch and the tail kernel: some material is a MAT_METALROUGH (set_materials)
FLAVOR_ALPHA_TEST = 65536  # ... and the ALPHA_TEST instances of the trace kernels: some material of the alpha table is pod.ALPHA_MASK (set_material_alpha)
FLAVOR_SOLID = 131072  # ... and the SOLID instances of the material launches: some material is pod.ALPHA_MASK or pod.ALPHA_OPAQUE (set_material_alpha)
FLAVOR_LIGHT_TREE = 262144  # ... and the TREE instances of the material launch and the medium's scatter kernel: LIGHTS_POWER with LIGHT_IMPORTANCE_POSITION under the SCAN pipeline
FLAVOR_TRANSMIT = 2048  # ... and the any-hit TRANSMIT instance: SHADOWS_TRANSMIT over a table with a see-through material (set_shadow_transmittance)


class Context:
    """One ``nxhip_ctx`` (one GPU).  Thin 1:1 wrapper of the C-ABI; raises NexusError on any failure."""

    adaptive = False     # set_adaptive
    _pass_paths = None   # adaptive: paths of the pass render_frame issued last (what read_radiance returns)

    def __init__(self, width, height, device=0, stream=None):
        self.L = lib()
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        check(self.L.nxhip_create(device, self.width, self.height, C.c_void_p(stream) if stream else None, C.byref(h)), "nxhip_create")
        self.h = h
        self.local_count = self.width * self.height
        self.frames_per_pass = 1

    def close(self):
        if getattr(self, "h", None):
            self.L.nxhip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # scene
    def upload_blas(self, nodes, tris, tri_idx):
        nodes = np.ascontiguousarray(nodes, dtype=pod.NODE_DT)
        tris = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
        tri_idx = np.ascontiguousarray(tri_idx, dtype=np.uint32)
        bid = C.c_int32(-1)
        check(self.L.nxhip_upload_blas(self.h, _ptr(nodes), len(nodes), _ptr(tris), len(tris), _ptr(tri_idx), C.byref(bid)), "nxhip_upload_blas")
        return bid.value

    def clear_blas(self):
        check(self.L.nxhip_clear_blas(self.h), "nxhip_clear_blas")

    def set_tlas(self, nodes, inst_idx, instances):
        nodes = np.ascontiguousarray(nodes, dtype=pod.NODE_DT)
        inst_idx = np.ascontiguousarray(inst_idx, dtype=np.uint32)
        instances = np.ascontiguousarray(instances, dtype=pod.INST_DT)
        check(self.L.nxhip_set_tlas(self.h, _ptr(nodes), len(nodes), _ptr(inst_idx), _ptr(instances), len(instances)), "nxhip_set_tlas")

    def set_materials(self, materials):
        materials = np.ascontiguousarray(materials, dtype=pod.MAT_DT)
        check(self.L.nxhip_set_materials(self.h, _ptr(materials), len(materials)), "nxhip_set_materials")

    def set_lights(self, lights):
        lights = np.ascontiguousarray(lights, dtype=pod.LIGHT_DT)
        check(self.L.nxhip_set_lights(self.h, _ptr(lights) if len(lights) else None, len(lights)), "nxhip_set_lights")

    def set_analytic_lights(self, lights):
        """point, sphere, spot and sun lights (pod.ALIGHT_DT records, pod.make_analytic_light); an empty list removes them
        (nxhip_set_analytic_lights: the sampling rule is in include/nexus_hip.h)"""
        lights = np.ascontiguousarray(lights, dtype=pod.ALIGHT_DT).reshape(-1)
        check(self.L.nxhip_set_analytic_lights(self.h, _ptr(lights) if len(lights) else None, len(lights)), "nxhip_set_analytic_lights")

    def set_material_alpha(self, alphas):
        """how the materials' alpha is read: pod.ALPHA_DT records (pod.make_material_alpha), one per material of the table; an empty
        list removes the table: every material is a stochastic blend again (nxhip_set_material_alpha: the rule is in include/nexus_hip.h)"""
        alphas = np.ascontiguousarray(alphas, dtype=pod.ALPHA_DT)
        check(self.L.nxhip_set_material_alpha(self.h, _ptr(alphas) if len(alphas) else None, len(alphas)), "nxhip_set_material_alpha")

    def set_material_detail(self, details):
        """the materials' detail maps: pod.DETAIL_DT records (pod.make_material_detail), one per material of the table; an empty list
        removes the table (nxhip_set_material_detail: the shading rule is in include/nexus_hip.h)"""
        details = np.ascontiguousarray(details, dtype=pod.DETAIL_DT).reshape(-1)
        check(self.L.nxhip_set_material_detail(self.h, _ptr(details) if len(details) else None, len(details)), "nxhip_set_material_detail")

    def set_medium(self, medium):
        """fog: one homogeneous medium in a world-space box (a pod.MEDIUM_DT record, pod.make_medium); None removes it
        (nxhip_set_medium: the rule is in include/nexus_hip.h)"""
        if medium is None:
            check(self.L.nxhip_set_medium(self.h, None), "nxhip_set_medium")
            return
        m = np.ascontiguousarray(medium, dtype=pod.MEDIUM_DT).reshape(1)
        check(self.L.nxhip_set_medium(self.h, _ptr(m)), "nxhip_set_medium")

    def set_medium_density(self, rho):
        """fog density grid: a float32 array of shape (nz, ny, nx) over the medium's box — the extinction at p becomes sigmaT x rho(p), a
        trilinear lookup; None removes it (nxhip_set_medium_density: the rule is in include/nexus_hip.h)"""
        if rho is None:
            check(self.L.nxhip_set_medium_density(self.h, None, 0, 0, 0), "nxhip_set_medium_density")
            return
        r = np.ascontiguousarray(rho, dtype=np.float32)
        assert r.ndim == 3, "a density grid has the shape (nz, ny, nx)"
        nz, ny, nx = r.shape
        check(self.L.nxhip_set_medium_density(self.h, _ptr(r), nx, ny, nz), "nxhip_set_medium_density")

    def read_medium_majorants(self):
        """the majorant bricks the device built from the density grid — a test hook: float32[nbz, nby, nbx]"""
        nb = (C.c_uint32 * 3)()
        check(self.L.nxhip_read_medium_majorants(self.h, None, 0, nb), "nxhip_read_medium_majorants")
        out = np.zeros((nb[2], nb[1], nb[0]), dtype=np.float32)
        check(self.L.nxhip_read_medium_majorants(self.h, _ptr(out), out.size, nb), "nxhip_read_medium_majorants")
        return out

    def medium_density_batch(self, points):
        """the density grid's lookup at points[k], and the majorant of the brick the walk would start in there — a test hook:
        (rho float32[n], majorant float32[n])"""
        p, = _cols((points, _F32, 3))
        rho, maj = _outs(len(p), (_F32, 1), (_F32, 1))
        self._hook("nxhip_medium_density_batch", p, len(p), rho, maj)
        return rho, maj

    def medium_track_batch(self, origin, direction, t_end, seed):
        """the walk through the density grid for rays (origin[k], direction[k]) that end at t_end[k] (inf: a miss), in both modes, each from
        the xorshift32 state seed[k] != 0 — a test hook: (scatter_t float32[n], -1 where the free flight meets no real collision;
        transmittance float32[n] of the ratio tracking; steps uint32[n, 2]: iterations | tentative collisions << 16 of the two walks)"""
        o, d, te, sd = _cols((origin, _F32, 3), (direction, _F32, 3), (t_end, _F32, 1), (seed, _U32, 1))
        st, tr, steps = _outs(len(o), (_F32, 1), (_F32, 1), (_U32, 2))
        self._hook("nxhip_medium_track_batch", o, d, te, sd, len(o), st, tr, steps)
        return st, tr, steps

    def medium_segment_batch(self, origin, direction, t_end, xi):
        """the medium's segment rule, transmittance and free flight for rays (origin[k], direction[k]) that end at t_end[k] (inf: a miss) with
        the random number xi[k] in [0, 1) — a test hook: (t0, length, transmittance, scatter_t) float32[n] each; scatter_t is -1 where the
        flight does not scatter"""
        o, d, te, x = _cols((origin, _F32, 3), (direction, _F32, 3), (t_end, _F32, 1), (xi, _F32, 1))
        out = _outs(len(o), *[(_F32, 1)] * 4)
        self._hook("nxhip_medium_segment_batch", o, d, te, x, len(o), *out)
        return tuple(out)

    def medium_phase_batch(self, dir_in, xi1, xi2):
        """the continuation the medium's scatter kernel draws about the direction of travel dir_in[k] from (xi1[k], xi2[k]) in [0, 1)^2 — a test
        hook: (direction float32[n, 3], pdf float32[n])"""
        d, a, b = _cols((dir_in, _F32, 3), (xi1, _F32, 1), (xi2, _F32, 1))
        out, pdf = _outs(len(d), (_F32, 3), (_F32, 1))
        self._hook("nxhip_medium_phase_batch", d, a, b, len(d), out, pdf)
        return out, pdf

    def shading_frame_batch(self, instance, tri_idx, hit_uv, ray_dir):
        """what the material kernels hand their sampling code for hits on triangles tri_idx[k] of `instance` at barycentrics hit_uv[k],
        reached along ray_dir[k] — a test hook: (shading normal float32[n, 3], roughness float32[n], fell_back bool[n])"""
        t, uv, d = _cols((tri_idx, _U32, 1), (hit_uv, _F32, 2), (ray_dir, _F32, 3))
        normal, roughness, fell = _outs(len(t), (_F32, 3), (_F32, 1), (_U32, 1))
        self._hook("nxhip_shading_frame_batch", int(instance), t, uv, d, len(t), normal, roughness, fell)
        return normal, roughness, fell != 0

    def material_inputs_batch(self, instance, tri_idx, hit_uv):
        """base colour, roughness and metalness the BSDF of an NX_MAT_METALROUGH material receives for hits on triangles tri_idx[k] of
        `instance` at barycentrics hit_uv[k] — a test hook: (c float32[n, 3], r float32[n], m float32[n])"""
        t, uv = _cols((tri_idx, _U32, 1), (hit_uv, _F32, 2))
        out, = _outs(len(t), (_F32, 5))
        self._hook("nxhip_material_inputs_batch", int(instance), t, uv, len(t), out)
        return out[:, :3].copy(), out[:, 3].copy(), out[:, 4].copy()

    def analytic_light_sample_batch(self, light_index, origins, r):
        """the light sample's draw for analytic light `light_index` from every origin[k] with the random pair r[k] in [0, 1)^2 — a test hook:
        (direction float32[n, 3], tmax float32[n], factor float32[n, 3], ok bool[n])"""
        o, r = _cols((origins, _F32, 3), (r, _F32, 2))
        direction, tmax, factor, ok = _outs(len(o), (_F32, 3), (_F32, 1), (_F32, 3), (_U32, 1))
        self._hook("nxhip_analytic_light_sample_batch", int(light_index), o, r, len(o), direction, tmax, factor, ok)
        return direction, tmax, factor, ok != 0

    def upload_texture(self, kind, rgba8):
        img = np.ascontiguousarray(rgba8, dtype=np.uint8)
        assert img.ndim == 3 and img.shape[2] == 4
        tid = C.c_int32(-1)
        check(self.L.nxhip_upload_texture(self.h, TEXTURE_KINDS[kind], _ptr(img), img.shape[1], img.shape[0], C.byref(tid)),
              "nxhip_upload_texture")
        return tid.value

    def upload_env_float(self, rgb):
        """the environment map as linear float radiance: H x W x 3 float32, row 0 the top row (nxhip_upload_env_float)"""
        img = np.ascontiguousarray(rgb, dtype=np.float32)
        assert img.ndim == 3 and img.shape[2] == 3
        check(self.L.nxhip_upload_env_float(self.h, _ptr(img), img.shape[1], img.shape[0]), "nxhip_upload_env_float")

    def set_sky(self, sky):
        """the environment generated on the device from the sun-and-sky model (a pod.SKY_DT record, pod.Sky / capi.sky_defaults):
        installed as a float map (nxhip_set_sky: the model is in include/nexus_hip.h)"""
        s = np.ascontiguousarray(sky, dtype=pod.SKY_DT).reshape(1)
        check(self.L.nxhip_set_sky(self.h, _ptr(s)), "nxhip_set_sky")

    def sky_radiance(self, sky, dirs):
        """the sky term alone (ground included, no disc) along every unit direction dirs[k]: float32[n, 3] — a test hook over the device
        function the map kernel calls (nxhip_sky_radiance_batch)"""
        s = np.ascontiguousarray(sky, dtype=pod.SKY_DT).reshape(1)
        d, = _cols((dirs, _F32, 3))
        rgb, = _outs(len(d), (_F32, 3))
        self._hook("nxhip_sky_radiance_batch", s, d, len(d), rgb)
        return rgb

    def read_env_float(self):
        """the float environment map as it is stored: H x W x 3 float32"""
        w, h = C.c_uint32(0), C.c_uint32(0)
        check(self.L.nxhip_read_env_float(self.h, None, 0, C.byref(w), C.byref(h)), "nxhip_read_env_float")
        out = np.zeros((h.value, w.value, 3), dtype=np.float32)
        check(self.L.nxhip_read_env_float(self.h, _ptr(out), w.value * h.value, C.byref(w), C.byref(h)), "nxhip_read_env_float")
        return out

    def read_env_guides(self):
        """the cut points of the environment sampler's cdf inversion: (marginal uint32[65], rows uint32[H, 65])"""
        w, h = C.c_uint32(0), C.c_uint32(0)
        check(self.L.nxhip_read_env_tables(self.h, None, None, None, 0, C.byref(w), C.byref(h)), "nxhip_read_env_tables")
        marginal, rows = np.zeros(65, np.uint32), np.zeros((h.value, 65), np.uint32)
        check(self.L.nxhip_read_env_guides(self.h, _ptr(marginal), _ptr(rows), h.value), "nxhip_read_env_guides")
        return marginal, rows

    def clear_textures(self):
        check(self.L.nxhip_clear_textures(self.h), "nxhip_clear_textures")

    def set_camera(self, cam):
        cam = np.ascontiguousarray(cam, dtype=pod.CAM_DT).reshape(1)
        check(self.L.nxhip_set_camera(self.h, _ptr(cam)), "nxhip_set_camera")

    def set_render_settings(self, st):
        st = np.ascontiguousarray(st, dtype=pod.SETTINGS_DT).reshape(1)
        check(self.L.nxhip_set_render_settings(self.h, _ptr(st)), "nxhip_set_render_settings")

    def set_modes(self, rng_mode=pod.RNG_REFERENCE_SLOT, compact_mode=pod.COMPACT_FAST, conductor_mode=pod.CONDUCTOR_REFERENCE):
        check(self.L.nxhip_set_modes(self.h, rng_mode, compact_mode, conductor_mode), "nxhip_set_modes")

    def set_pixel_map(self, pixel_map):
        if pixel_map is None:
            check(self.L.nxhip_set_pixel_map(self.h, None, 0), "nxhip_set_pixel_map")
            self.local_count = self.width * self.height
        else:
            pm = np.ascontiguousarray(pixel_map, dtype=np.uint32)
            check(self.L.nxhip_set_pixel_map(self.h, _ptr(pm), len(pm)), "nxhip_set_pixel_map")
            self.local_count = len(pm)

    def set_pixel_order(self, order):
        """nxhip_set_pixel_order: ORDER_ROWS (0, the reference's) or ORDER_TILES (1: 8 x 8 pixel tiles) over the full frame"""
        check(self.L.nxhip_set_pixel_order(self.h, int(order)), "nxhip_set_pixel_order")
        self.local_count = self.width * self.height

    def build_blas(self, tris):
        """BLAS built on the device (binned SAH + SAH-DP collapse by default, see set_device_builder); returns the BLAS id"""
        t = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
        bid = C.c_int32(-1)
        check(self.L.nxhip_build_blas(self.h, _ptr(t), len(t), C.byref(bid)), "nxhip_build_blas")
        return int(bid.value)

    def build_blas_batch(self, meshes):
        """the BLASes of several meshes in one device build (nxhip_build_blas_batch); returns their ids (consecutive)"""
        arrays = [np.ascontiguousarray(m, dtype=pod.TRI_DT) for m in meshes]
        ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
        counts = np.array([len(a) for a in arrays], dtype=np.uint32)
        ids = np.full(len(arrays), -1, dtype=np.int32)
        check(self.L.nxhip_build_blas_batch(self.h, ptrs, _ptr(counts), len(arrays), _ptr(ids)), "nxhip_build_blas_batch")
        return [int(i) for i in ids]

    def read_blas_batch(self, first_id, tri_counts):
        """nodes and primitive index lists of consecutive BLAS ids: [(nodes, idx), ...]"""
        count = len(tri_counts)
        node_counts = np.zeros(count, dtype=np.uint32)
        check(self.L.nxhip_read_blas_batch(self.h, first_id, count, None, 0, _ptr(node_counts), None, 0), "nxhip_read_blas_batch")
        nodes = np.zeros(int(node_counts.sum()), dtype=pod.NODE_DT)
        idx = np.zeros(int(np.sum(tri_counts)), dtype=np.uint32)
        check(self.L.nxhip_read_blas_batch(self.h, first_id, count, _ptr(nodes), len(nodes), _ptr(node_counts), _ptr(idx), len(idx)), "nxhip_read_blas_batch")
        out, na, pa = [], 0, 0
        for k in range(count):
            out.append((nodes[na:na + int(node_counts[k])], idx[pa:pa + int(tri_counts[k])]))
            na += int(node_counts[k])
            pa += int(tri_counts[k])
        return out

    def read_blas(self, blas_id, tri_count):
        n = C.c_uint32(0)
        check(self.L.nxhip_read_blas(self.h, blas_id, None, 0, None, 0, C.byref(n)), "nxhip_read_blas")
        nodes = np.zeros(n.value, dtype=pod.NODE_DT)
        idx = np.zeros(tri_count, dtype=np.uint32)
        check(self.L.nxhip_read_blas(self.h, blas_id, _ptr(nodes), n.value, _ptr(idx), tri_count, C.byref(n)), "nxhip_read_blas")
        return nodes, idx

    def set_device_builder(self, clustering_radius=-1):
        """device BLAS / TLAS builders: -1 (NXHIP_BUILDER_SAH, the default) = top-down binned SAH, 0 = radix tree (LBVH),
        > 0 = clustering (PLOC) with this search radius"""
        check(self.L.nxhip_set_device_builder(self.h, int(clustering_radius)), "nxhip_set_device_builder")

    def release_queues(self):
        """PathTracer::FreeDeviceBuffers: queue / path-state buffers back to the allocator until the next render"""
        check(self.L.nxhip_release_queues(self.h), "nxhip_release_queues")

    def rebuild_tlas(self, instances):
        """build the TLAS on the device (the BLAS builder over the instances' boxes) and install it; returns (nodes, instance index list)"""
        instances = np.ascontiguousarray(instances, dtype=pod.INST_DT)
        check(self.L.nxhip_rebuild_tlas(self.h, _ptr(instances), len(instances)), "nxhip_rebuild_tlas")
        n = C.c_uint32(0)
        idx = np.zeros(len(instances), dtype=np.uint32)
        check(self.L.nxhip_read_tlas_index(self.h, _ptr(idx), len(idx), C.byref(n)), "nxhip_read_tlas_index")
        nodes, _ = self.read_tlas(n.value, len(instances))
        return nodes, idx

    def debug_write_blas_node(self, blas_id, node_idx, node):
        """test hook: overwrite one node of an uploaded BLAS without the upload checks"""
        node = np.ascontiguousarray(node, dtype=pod.NODE_DT).reshape(1)
        check(self.L.nxhip_debug_write_blas_node(self.h, blas_id, node_idx, _ptr(node)), "nxhip_debug_write_blas_node")

    def debug_set_scan_epoch(self, epoch):
        """test hook: passes begun since the ordered compaction's status words were last cleared (wraps at 2^20)"""
        check(self.L.nxhip_debug_set_scan_epoch(self.h, int(epoch)), "nxhip_debug_set_scan_epoch")

    def debug_keep_binary_tree(self, on=True):
        """test hook: single device builds (build_blas, rebuild_tlas) keep their binary tree and cost table for debug_read_binary_tree"""
        check(self.L.nxhip_debug_keep_binary_tree(self.h, 1 if on else 0), "nxhip_debug_keep_binary_tree")

    def debug_read_binary_tree(self):
        """the binary tree of the last single device build (include/nexus_hip.h): a dict of n, prim_cost, builder, left / right / count
        int32[n - 1], parent int32[2n - 1], box float32[2n - 1, 2, 3], leaf_order uint32[n] and the cost table cost float32[n - 1, 7],
        decision / left_count / right_count int8[n - 1, 7]; n == 0 (empty arrays) after a build of at most 8 primitives"""
        n, cost, builder = C.c_uint32(0), C.c_float(0.0), C.c_int32(0)
        rc = self.L.nxhip_debug_read_binary_tree(self.h, 0, C.byref(n), C.byref(cost), C.byref(builder), None, None, None, None, None, None, None)
        if n.value == 0:
            check(rc, "nxhip_debug_read_binary_tree")
        m = int(n.value)
        inner, nodes = max(m - 1, 0), max(2 * m - 1, 0)
        left, right, count = (np.zeros(inner, np.int32) for _ in range(3))
        parent = np.zeros(nodes, np.int32)
        box = np.zeros((nodes, 2, 3), np.float32)
        order = np.zeros(m, np.uint32)
        table = np.zeros((inner, 7), dtype=np.dtype([("cost", "<f4"), ("decision", "i1"), ("leftCount", "i1"), ("rightCount", "i1"), ("pad", "i1")]))
        if m:
            check(self.L.nxhip_debug_read_binary_tree(self.h, m, C.byref(n), C.byref(cost), C.byref(builder), _ptr(left), _ptr(right), _ptr(parent), _ptr(count),
                                                      _ptr(box), _ptr(order), _ptr(table)), "nxhip_debug_read_binary_tree")
        return {"n": m, "prim_cost": float(cost.value), "builder": int(builder.value), "left": left, "right": right, "count": count, "parent": parent,
                "box": box, "leaf_order": order, "cost": np.ascontiguousarray(table["cost"]), "decision": np.ascontiguousarray(table["decision"]),
                "left_count": np.ascontiguousarray(table["leftCount"]), "right_count": np.ascontiguousarray(table["rightCount"])}

    def set_instance_transforms(self, instance_ids, transforms16):
        """move existing instances on the device (inverse, bounds, traversal records, TLAS refit): no scene re-upload"""
        ids = np.ascontiguousarray(instance_ids, dtype=np.uint32)
        m = np.ascontiguousarray(transforms16, dtype=np.float32).reshape(len(ids), 16)
        check(self.L.nxhip_set_instance_transforms(self.h, _ptr(ids), _ptr(m), len(ids)), "nxhip_set_instance_transforms")

    def update_blas(self, blas_id, tris):
        """new vertices for an existing BLAS (same triangles, same order): triangles, intersection stream and nodes are redone
        on the device; instances and the TLAS follow before the next render / ray batch / read_tlas"""
        t = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
        check(self.L.nxhip_update_blas(self.h, int(blas_id), _ptr(t), len(t)), "nxhip_update_blas")

    def update_blas_device(self, blas_id, ptr, count):
        """update_blas from `count` 96-byte triangle records in device memory (e.g. a torch tensor's data_ptr()); asynchronous"""
        check(self.L.nxhip_update_blas_device(self.h, int(blas_id), C.c_void_p(int(ptr)) if ptr else None, int(count)), "nxhip_update_blas_device")

    def set_blas_skin(self, blas_id, corners, joint_count):
        """the skin of a BLAS (3 nx_skin_corner records per triangle; None removes it): its current triangles become the bind pose
        every pose_blas starts from"""
        if corners is None:
            check(self.L.nxhip_set_blas_skin(self.h, int(blas_id), None, 0, 0), "nxhip_set_blas_skin")
            return
        s = np.ascontiguousarray(corners, dtype=pod.SKIN_CORNER_DT)
        check(self.L.nxhip_set_blas_skin(self.h, int(blas_id), _ptr(s), len(s), int(joint_count)), "nxhip_set_blas_skin")

    def set_blas_morph(self, blas_id, deltas):
        """the morph targets of a BLAS: (T, 3 n) nx_morph_corner records (pod.make_morph_corners), target-major; None removes them.  The
        bind copy is shared with the skin (include/nexus_hip.h: whichever is set first takes it)"""
        if deltas is None:
            check(self.L.nxhip_set_blas_morph(self.h, int(blas_id), None, 0, 0), "nxhip_set_blas_morph")
            return
        d = np.ascontiguousarray(deltas, dtype=pod.MORPH_CORNER_DT)
        if d.ndim != 2:
            raise ValueError("morph deltas must be (targets, 3 x triangles) records")
        check(self.L.nxhip_set_blas_morph(self.h, int(blas_id), _ptr(d), d.shape[1], d.shape[0]), "nxhip_set_blas_morph")

    def pose_blas_morph(self, blas_id, weights, palette=None):
        """pose a morphed BLAS: one weight per target, and on a skinned BLAS the (jointCount, 12) palette of pose_blas; deltas first, then
        joints, in one pass, and the refit behind it.  Weights do not persist."""
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        if palette is None:
            check(self.L.nxhip_pose_blas_morph(self.h, int(blas_id), _ptr(w), len(w), None, 0), "nxhip_pose_blas_morph")
            return
        m = np.ascontiguousarray(palette, dtype=np.float32).reshape(-1, 12)
        check(self.L.nxhip_pose_blas_morph(self.h, int(blas_id), _ptr(w), len(w), _ptr(m), len(m)), "nxhip_pose_blas_morph")

    def pose_blas(self, blas_id, joint_matrices):
        """pose a skinned BLAS: (jointCount, 12) row-major 3 x 4 object-space matrices; triangles, intersection stream and nodes are
        redone on the device, instances and the TLAS follow as after update_blas"""
        m = np.ascontiguousarray(joint_matrices, dtype=np.float32)
        m = m.reshape(-1, 12)
        check(self.L.nxhip_pose_blas(self.h, int(blas_id), _ptr(m), len(m)), "nxhip_pose_blas")

    def read_blas_triangles(self, blas_id, tri_count):
        """the BLAS's current 96-byte triangles"""
        t = np.zeros(int(tri_count), dtype=pod.TRI_DT)
        check(self.L.nxhip_read_blas_triangles(self.h, int(blas_id), _ptr(t), len(t)), "nxhip_read_blas_triangles")
        return t

    def read_blas_bounds(self, blas_id):
        """(lo, hi) of the box the BLAS's root node encodes after the last build, refit or pose"""
        lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
        check(self.L.nxhip_read_blas_bounds(self.h, int(blas_id), _ptr(lo), _ptr(hi)), "nxhip_read_blas_bounds")
        return lo, hi

    def read_tlas(self, node_count, instance_count):
        nodes = np.zeros(node_count, dtype=pod.NODE_DT)
        insts = np.zeros(instance_count, dtype=pod.INST_DT)
        check(self.L.nxhip_read_tlas(self.h, _ptr(nodes), node_count, _ptr(insts), instance_count), "nxhip_read_tlas")
        return nodes, insts

    # ---- native multi-GPU tile split (RCCL inside the library; bench.py's N > 1 path uses torch.distributed instead)
    def mgpu_init(self, world, rank, unique_id, tile_rows):
        uid = np.frombuffer(bytes(unique_id), dtype=np.uint8).copy()
        assert len(uid) == 128
        check(self.L.nxhip_mgpu_init(self.h, world, rank, _ptr(uid), tile_rows), "nxhip_mgpu_init")
        n = C.c_uint32(0)
        check(self.L.nxhip_tile_pixel_map(self.width, self.height, world, rank, tile_rows, 1, None, C.byref(n)), "nxhip_tile_pixel_map")
        self.local_count = int(n.value)

    def mgpu_gather(self):
        check(self.L.nxhip_mgpu_gather(self.h), "nxhip_mgpu_gather")

    def mgpu_read_rgba8(self):
        out = np.zeros(self.width * self.height, dtype=np.uint32)
        check(self.L.nxhip_mgpu_read_rgba8(self.h, _ptr(out)), "nxhip_mgpu_read_rgba8")
        return out

    def mgpu_read_accumulation(self):
        out = np.zeros((self.width * self.height, 3), dtype=np.float32)
        check(self.L.nxhip_mgpu_read_accumulation(self.h, _ptr(out)), "nxhip_mgpu_read_accumulation")
        return out

    def mgpu_shutdown(self):
        check(self.L.nxhip_mgpu_shutdown(self.h), "nxhip_mgpu_shutdown")

    def resize(self, width, height):
        check(self.L.nxhip_resize(self.h, width, height), "nxhip_resize")
        self.width, self.height = int(width), int(height)
        self.local_count = self.width * self.height

    # rendering
    def reset_frame_number(self):
        check(self.L.nxhip_reset_frame_number(self.h), "nxhip_reset_frame_number")

    def set_frame_number(self, f):
        check(self.L.nxhip_set_frame_number(self.h, f), "nxhip_set_frame_number")

    def frame_number(self):
        return int(self.L.nxhip_frame_number(self.h))

    def render_frame(self):
        if self.adaptive:  # the pass renders the active set as it is now
            active = self.active_count()
            if active:  # (no active pixel: nothing is rendered and the last pass stays the last pass)
                self._pass_paths = active * self.frames_per_pass
        check(self.L.nxhip_render_frame(self.h), "nxhip_render_frame")

    def accumulate(self):
        check(self.L.nxhip_accumulate(self.h), "nxhip_accumulate")

    def accumulate_external(self, dev_ptr, count, first_frame, pixel_map_dev_ptr=None, slices=1, slice_stride=None):
        check(self.L.nxhip_accumulate_external(self.h, C.c_void_p(dev_ptr), count, slices, slice_stride if slice_stride is not None else count,
                                               first_frame, C.c_void_p(pixel_map_dev_ptr) if pixel_map_dev_ptr else None), "nxhip_accumulate_external")

    def compose_tiles(self, src_accum_dev_ptr, count, pixel_map_dev_ptr, dst_accum_dev_ptr, dst_rgba8_dev_ptr=None):
        check(self.L.nxhip_compose_tiles(self.h, C.c_void_p(src_accum_dev_ptr), count, C.c_void_p(pixel_map_dev_ptr) if pixel_map_dev_ptr else None,
                                         C.c_void_p(dst_accum_dev_ptr), C.c_void_p(dst_rgba8_dev_ptr) if dst_rgba8_dev_ptr else None), "nxhip_compose_tiles")

    def set_env_sampling(self, on=True):
        check(self.L.nxhip_set_env_sampling(self.h, 1 if on else 0), "nxhip_set_env_sampling")

    def read_env_tables(self):
        """the environment sampler's tables as uploaded: (marginalCdf float32[H], rowCdf float32[H, W], density float32[H, W])"""
        w, h = C.c_uint32(0), C.c_uint32(0)
        check(self.L.nxhip_read_env_tables(self.h, None, None, None, 0, C.byref(w), C.byref(h)), "nxhip_read_env_tables")
        n = w.value * h.value
        marginal, row, density = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        check(self.L.nxhip_read_env_tables(self.h, _ptr(marginal), _ptr(row), _ptr(density), n, C.byref(w), C.byref(h)), "nxhip_read_env_tables")
        return marginal[:h.value].copy(), row.reshape(h.value, w.value), density.reshape(h.value, w.value)

    def env_sample_batch(self, r):
        """the environment sampler's draw for every pair r[k] in [0, 1)^2: (direction float32[n, 3], pdf float32[n], texel uint32[n] —
        y * W + x that the cdf inversion picked)"""
        r, = _cols((r, _F32, 2))
        direction, pdf, texel = _outs(len(r), (_F32, 3), (_F32, 1), (_U32, 1))
        self._hook("nxhip_env_sample_batch", r, len(r), direction, pdf, texel)
        return direction, pdf, texel

    def env_eval_batch(self, directions, with_pdf=True):
        """the background for every direction, and (with_pdf, sampler on) the sampler's pdf there and the texel the direction's map
        coordinates fall in: (rgb float32[n, 3], pdf float32[n] or None, texel uint32[n] or None)"""
        d, = _cols((directions, _F32, 3))
        rgb, pdf, texel = _outs(len(d), (_F32, 3), (_F32, 1) if with_pdf else None, (_U32, 1) if with_pdf else None)
        self._hook("nxhip_env_eval_batch", d, len(d), rgb, pdf, texel)
        return rgb, pdf, texel

    def set_light_sampling(self, mode):
        """LIGHTS_UNIFORM (0, the reference's rule) or LIGHTS_POWER (1): the light sample picks among the mesh lights' triangles in
        proportion to area x emitted luminance, from a table built on the device (include/nexus_hip.h)"""
        check(self.L.nxhip_set_light_sampling(self.h, int(mode)), "nxhip_set_light_sampling")

    def set_light_importance(self, importance):
        """LIGHT_IMPORTANCE_POWER (0, the default) or LIGHT_IMPORTANCE_POSITION (1): in LIGHTS_POWER mode the light sample descends a
        bounding hierarchy over the table's entries with probabilities that depend on the shading point (nxhip_set_light_importance);
        remembered, and without effect, in LIGHTS_UNIFORM"""
        check(self.L.nxhip_set_light_importance(self.h, int(importance)), "nxhip_set_light_importance")

    def set_shadow_transmittance(self, mode):
        """SHADOWS_OPAQUE (0, the reference's rule: a shadow ray ends at the first triangle) or SHADOWS_TRANSMIT (1): every crossing
        multiplies the ray's transmittance by 1 - opacity x alpha(uv) (nxhip_set_shadow_transmittance; deterministic, same expectation as
        the paths' own pass-through)"""
        check(self.L.nxhip_set_shadow_transmittance(self.h, int(mode)), "nxhip_set_shadow_transmittance")

    def read_light_table(self, light_count):
        """the light table of LIGHTS_POWER (brought up to date first): (cdf float32[N], entryLight uint32[N], lightBase uint32[light_count + 1])"""
        n = C.c_uint32(0)
        base = np.zeros(int(light_count) + 1, dtype=np.uint32)
        check(self.L.nxhip_read_light_table(self.h, None, None, 0, _ptr(base), C.byref(n)), "nxhip_read_light_table")
        cdf = np.zeros(n.value, dtype=np.float32)
        light = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            check(self.L.nxhip_read_light_table(self.h, _ptr(cdf), _ptr(light), n.value, _ptr(base), C.byref(n)), "nxhip_read_light_table")
        return cdf, light, base

    def light_pick_batch(self, u):
        """the device's pick for every u in [0, 1): (entry uint32[], prob float32[]) — the table's walk and its P(entry)"""
        u, = _cols((u, _F32, 1))
        entry, prob = _outs(len(u), (_U32, 1), (_F32, 1))
        self._hook("nxhip_light_pick_batch", u, len(u), entry, prob)
        return entry, prob

    def read_light_tree(self):
        """the light tree of LIGHTS_POWER with LIGHT_IMPORTANCE_POSITION (brought up to date first): (nodes float32[2G, 8] — lo xyz, w,
        hi xyz, entry bits; node 0 unused —, order uint32[N]); G = len(nodes) // 2"""
        g, n = C.c_uint32(0), C.c_uint32(0)
        check(self.L.nxhip_read_light_tree(self.h, None, None, 0, C.byref(g), C.byref(n)), "nxhip_read_light_tree")
        nodes = np.zeros((2 * g.value, 8), dtype=np.float32)
        order = np.zeros(n.value, dtype=np.uint32)
        check(self.L.nxhip_read_light_tree(self.h, _ptr(nodes), _ptr(order), 2 * g.value, C.byref(g), C.byref(n)), "nxhip_read_light_tree")
        return nodes, order

    def light_tree_pick_batch(self, points, u):
        """the device's descent from every point with its u in [0, 1): (entry uint32[] — 0xffffffff: no sample —, prob float32[])"""
        p, u = _cols((points, _F32, 3), (u, _F32, 1))
        entry, prob = _outs(len(u), (_U32, 1), (_F32, 1))
        self._hook("nxhip_light_tree_pick_batch", p, u, len(u), entry, prob)
        return entry, prob

    def light_tree_prob_batch(self, points, entry):
        """the probability the descent from every point has of its entry: float32[]"""
        p, e = _cols((points, _F32, 3), (entry, _U32, 1))
        prob, = _outs(len(e), (_F32, 1))
        self._hook("nxhip_light_tree_prob_batch", p, e, len(e), prob)
        return prob

    def set_entry_points(self, on=True):
        """primary rays start from the state their run's first node steps provably share (include/nexus_hip.h)"""
        check(self.L.nxhip_set_entry_points(self.h, 1 if on else 0), "nxhip_set_entry_points")

    def debug_thin_counts_of_pass(self, bounce):
        """rays the trace launches of level `bounce` of the last pass handed to the thin kernel: (closest-hit, any-hit)"""
        c = (C.c_int32 * 2)()
        check(self.L.nxhip_debug_thin_counts_of_pass(self.h, bounce, c), "nxhip_debug_thin_counts_of_pass")
        return int(c[0]), int(c[1])

    def debug_ended_rays_of_pass(self, bounce):
        """continuation rays the material launch of `bounce` of the last pass did not queue: their roulette draw was lost already (include/nexus_hip.h)"""
        n = C.c_int32(0)
        check(self.L.nxhip_debug_ended_rays_of_pass(self.h, bounce, C.byref(n)), "nxhip_debug_ended_rays_of_pass")
        return int(n.value)

    def debug_set_requeue(self, on=True):
        """test hook: the trace kernels hand the same rays out again and again (include/nexus_hip.h)"""
        check(self.L.nxhip_debug_set_requeue(self.h, 1 if on else 0), "nxhip_debug_set_requeue")

    def sync_timeout(self, timeout_ms):
        """nxhip_sync with a wall-clock limit; raises NexusError (code NXHIP_ERR_TIMEOUT = 6, the context is dead afterwards) when it expires"""
        check(self.L.nxhip_sync_timeout(self.h, int(timeout_ms)), "nxhip_sync_timeout")

    def debug_set_thin(self, lanes=16, iters=16, in_hooks=False, any_time=False):
        """the thin kernel's hand-over rule, and whether the ray-batch hooks use it too (a test hook: include/nexus_hip.h);
        any_time: hand over after `iters` iterations of every stretch between two refill points, dry queue or not"""
        check(self.L.nxhip_debug_set_thin(self.h, lanes, iters, (1 if in_hooks else 0) | (2 if any_time else 0)), "nxhip_debug_set_thin")

    def debug_set_thin_pool(self, slots=0):
        """how many items a thin wave's pool may hold before a round puts items back (0: the product's limit; a test hook)"""
        check(self.L.nxhip_debug_set_thin_pool(self.h, int(slots)), "nxhip_debug_set_thin_pool")

    def debug_thin_counts(self):
        """rays the last ray-batch hook call handed to the thin kernel: (closest-hit, any-hit)"""
        out = (C.c_int32 * 2)()
        check(self.L.nxhip_debug_thin_counts(self.h, out), "nxhip_debug_thin_counts")
        return int(out[0]), int(out[1])

    def debug_entry_walks(self):
        """entry-state walks the context has launched since it was created (include/nexus_hip.h): a table is reused until an input changes"""
        n = C.c_uint64(0)
        check(self.L.nxhip_debug_entry_walks(self.h, C.byref(n)), "nxhip_debug_entry_walks")
        return int(n.value)

    def debug_read_primary_rays(self, capacity=None):
        """the primary rays of the last pass as the generate kernel left them, in path order (path k = slice x local_count + local pixel):
        (origin float32[n, 3], direction float32[n, 3], path_index uint32[n]) — a test hook: include/nexus_hip.h.  Needs pathLength 1 and one
        pass in flight; `capacity`: the size of the arrays handed over (None: the pass's own path count)."""
        n = C.c_uint32(0)
        if capacity is None:
            rc = self.L.nxhip_debug_read_primary_rays(self.h, None, None, None, 0, C.byref(n))
            if n.value == 0:
                check(rc, "nxhip_debug_read_primary_rays")
            capacity = n.value
        origin = np.zeros((capacity, 3), np.float32)
        direction = np.zeros((capacity, 3), np.float32)
        index = np.zeros(capacity, np.uint32)
        check(self.L.nxhip_debug_read_primary_rays(self.h, _ptr(origin), _ptr(direction), _ptr(index), capacity, C.byref(n)), "nxhip_debug_read_primary_rays")
        return origin[:n.value], direction[:n.value], index[:n.value]

    def debug_pass_flavor(self, force_general=None):
        """flavor bits of the graph the last pass replayed (FLAVOR_IDENTITY: trace instances without the transform path, FLAVOR_NO_MAPS:
        map-free material launch); force_general: the bits whose specialised instances later passes must not use (None: unchanged) —
        a test hook: include/nexus_hip.h"""
        f = C.c_uint32(0)
        check(self.L.nxhip_debug_pass_flavor(self.h, 0xffffffff if force_general is None else int(force_general), C.byref(f)), "nxhip_debug_pass_flavor")
        return int(f.value)

    PASS_INSTANCE_WORDS = ("scan", "tail", "tail_bounce", "medium", "logic", "primary", "closest", "any_hit")
    NO_INSTANCE = 0xFFFFFFFF
    MEDIUM_GRID_FORM = 0x10000

    def debug_pass_instances(self):
        """the instance sets (nx_variants.h) the last pass's launches were looked up by, as recorded when its graph was built: a dict over
        PASS_INSTANCE_WORDS plus "medium_grid" (bool, None without a medium); None for a family the pass did not launch — a test hook:
        include/nexus_hip.h"""
        out = (C.c_uint32 * 8)()
        check(self.L.nxhip_debug_pass_instances(self.h, out), "nxhip_debug_pass_instances")
        got = {k: (None if int(v) == self.NO_INSTANCE else int(v)) for k, v in zip(self.PASS_INSTANCE_WORDS, out)}
        got["medium_grid"] = None if got["medium"] is None else bool(got["medium"] & self.MEDIUM_GRID_FORM)
        if got["medium"] is not None:
            got["medium"] &= ~self.MEDIUM_GRID_FORM
        return got

    def read_entry_states(self):
        """(runs, 40) int32: the entry states of the last pass; column 19 = node steps saved, 16 = stack entries, 18 = instance record,
        31 = instance record of the triangle the walk consumed (-1: none), 35 = triangles it skipped, 38 / 39 = the run's hit-distance
        bounds after the consumed triangle (float32 bits)"""
        n = C.c_uint32(0)
        check(self.L.nxhip_read_entry_states(self.h, None, 0, C.byref(n)), "nxhip_read_entry_states")
        out = np.zeros((n.value, 40), np.int32)
        if n.value:
            check(self.L.nxhip_read_entry_states(self.h, _ptr(out), n.value, C.byref(n)), "nxhip_read_entry_states")
        return out

    TAIL_AUTO = 0xFFFFFFFF

    def set_tail_bounce(self, bounce):
        """0 = off, 2 .. pathLength = from that bounce on, Context.TAIL_AUTO = the default rule (include/nexus_hip.h)"""
        check(self.L.nxhip_set_tail_bounce(self.h, bounce), "nxhip_set_tail_bounce")

    def set_passes_in_flight(self, passes):
        check(self.L.nxhip_set_passes_in_flight(self.h, passes), "nxhip_set_passes_in_flight")

    def set_queue_budget(self, queues):
        """hardware queues the library may count on when it shapes R passes in flight: 0 = read GPU_MAX_HW_QUEUES again (else 4),
        1 .. 32 = this many (include/nexus_hip.h)"""
        check(self.L.nxhip_set_queue_budget(self.h, int(queues)), "nxhip_set_queue_budget")

    def queue_budget(self):
        """(budget, chained, graph_instances): the resolved budget, whether a pass issued now replays the chain shape, the largest
        number of pass-graph instances a slot holds"""
        q, ch, g = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(self.L.nxhip_get_queue_budget(self.h, C.byref(q), C.byref(ch), C.byref(g)), "nxhip_get_queue_budget")
        return int(q.value), bool(ch.value), int(g.value)

    def debug_last_graph(self):
        """(nodes, edges, fan_out) of the pass graph the last pass replayed, as the runtime holds it; fan_out 1: a chain (a test hook)"""
        n, e, f = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(self.L.nxhip_debug_last_graph(self.h, C.byref(n), C.byref(e), C.byref(f)), "nxhip_debug_last_graph")
        return int(n.value), int(e.value), int(f.value)

    def debug_resident_slots(self):
        """(resident, trace_blocks, slot_of_last_pass): the slots a pass issued now shares the chip among, the workgroups of its
        closest-hit launches, and which of the slots the last pass rendered in (a test hook)"""
        r, b, s = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(self.L.nxhip_debug_resident_slots(self.h, C.byref(r), C.byref(b), C.byref(s)), "nxhip_debug_resident_slots")
        return int(r.value), int(b.value), int(s.value)

    def set_frames_per_pass(self, frames):
        check(self.L.nxhip_set_frames_per_pass(self.h, frames), "nxhip_set_frames_per_pass")
        self.frames_per_pass = int(frames)

    def write_accumulation(self, accumulation, frame_number):
        a = np.ascontiguousarray(accumulation, dtype=np.float32).reshape(-1, 3)
        assert len(a) == self.local_count
        check(self.L.nxhip_write_accumulation(self.h, _ptr(a), int(frame_number)), "nxhip_write_accumulation")

    # ---- feature buffers and the denoiser (include/nexus_hip.h) ----
    def set_aov(self, on=True):
        """Feature buffers of the camera ray's hit (albedo + coverage, shading normal + depth), accumulated like the colour"""
        check(self.L.nxhip_set_aov(self.h, 1 if on else 0), "nxhip_set_aov")

    def read_aov(self):
        """(albedo, normalDepth): the accumulated feature buffers, (local_count, 4) float32 each, in the order of read_accumulation"""
        a = np.zeros((self.local_count, 4), np.float32)
        n = np.zeros((self.local_count, 4), np.float32)
        check(self.L.nxhip_read_aov(self.h, _ptr(a), _ptr(n)), "nxhip_read_aov")
        return a, n

    def read_aov_frame(self):
        """(albedo, normalDepth) of the pass rendered last: (local_count * frames_per_pass, 4) float32 each, frame slices in turn"""
        a = np.zeros((self._last_pass_paths(), 4), np.float32)
        n = np.zeros((self._last_pass_paths(), 4), np.float32)
        check(self.L.nxhip_read_aov_frame(self.h, _ptr(a), _ptr(n)), "nxhip_read_aov_frame")
        return a, n

    def write_aov(self, albedo=None, normal_depth=None):
        """Load accumulated feature buffers (the twin of write_accumulation); None leaves a buffer as it is"""
        bufs = []
        for b in (albedo, normal_depth):
            if b is not None:
                b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 4)
                assert len(b) == self.local_count
            bufs.append(b)
        check(self.L.nxhip_write_aov(self.h, _ptr(bufs[0]) if bufs[0] is not None else None, _ptr(bufs[1]) if bufs[1] is not None else None), "nxhip_write_aov")

    def denoise(self, iterations=None, sigma_color=None, sigma_normal=None, sigma_albedo=None, sigma_depth=None):
        """Edge-avoiding a-trous filter over the accumulated colour, guided by the accumulated feature buffers; None = the
        library's default for that parameter.  The result is a separate image: read_denoised / read_denoised_rgba8."""
        p = denoise_defaults()
        for name, v in (("iterations", iterations), ("sigmaColor", sigma_color), ("sigmaNormal", sigma_normal), ("sigmaAlbedo", sigma_albedo), ("sigmaDepth", sigma_depth)):
            if v is not None:
                p[name] = v
        check(self.L.nxhip_denoise(self.h, _ptr(p)), "nxhip_denoise")

    def read_denoised(self):
        out = np.zeros((self.width * self.height, 3), np.float32)
        check(self.L.nxhip_read_denoised(self.h, _ptr(out)), "nxhip_read_denoised")
        return out

    def read_denoised_rgba8(self):
        out = np.zeros(self.width * self.height, np.uint32)
        check(self.L.nxhip_read_denoised_rgba8(self.h, _ptr(out)), "nxhip_read_denoised_rgba8")
        return out

    # ---- adaptive sampling (include/nexus_hip.h) ----
    def set_adaptive(self, threshold=None, lum_floor=None, min_samples=None, cull=None, on=True):
        """Per-pixel noise statistics, the per-block stop rule and (cull) the device-built active set; None = the library's
        default for that parameter.  on=False: off, buffers released, base set restored."""
        if not on:
            check(self.L.nxhip_set_adaptive(self.h, None), "nxhip_set_adaptive")
            self.adaptive = False
            return
        p = adaptive_defaults()
        for name, v in (("threshold", threshold), ("lumFloor", lum_floor), ("minSamples", min_samples), ("cull", cull)):
            if v is not None:
                p[name] = v
        check(self.L.nxhip_set_adaptive(self.h, _ptr(p)), "nxhip_set_adaptive")
        self.adaptive = True
        self._pass_paths = None

    def adaptive_update(self):
        """Folds pending passes, decides, rebuilds the active set, synchronises: (active pixels, active blocks)"""
        px, bl = C.c_uint32(0), C.c_uint32(0)
        check(self.L.nxhip_adaptive_update(self.h, C.byref(px), C.byref(bl)), "nxhip_adaptive_update")
        return px.value, bl.value

    def render_adaptive(self, max_frames, interval):
        """{render interval frames, accumulate, update} until no block is active or max_frames: (frames issued, active pixels)"""
        fr, px = C.c_uint32(0), C.c_uint32(0)
        self._pass_paths = None
        check(self.L.nxhip_render_adaptive(self.h, int(max_frames), int(interval), C.byref(fr), C.byref(px)), "nxhip_render_adaptive")
        return fr.value, px.value

    def read_sample_counts(self):
        out = np.zeros(self.local_count, np.uint32)
        check(self.L.nxhip_read_sample_counts(self.h, _ptr(out)), "nxhip_read_sample_counts")
        return out

    def read_noise_stats(self):
        """(local_count, 2) float32: Welford's (meanY, M2) of the luminance, base order"""
        out = np.zeros((self.local_count, 2), np.float32)
        check(self.L.nxhip_read_noise_stats(self.h, _ptr(out)), "nxhip_read_noise_stats")
        return out

    def read_block_noise(self):
        """(largest relative standard error per block, active flag per block) as of the last adaptive_update"""
        n = C.c_uint32(0)
        check(self.L.nxhip_read_block_noise(self.h, None, None, 0, C.byref(n)), "nxhip_read_block_noise")
        bmax, active = np.zeros(n.value, np.float32), np.zeros(n.value, np.uint8)
        check(self.L.nxhip_read_block_noise(self.h, _ptr(bmax), _ptr(active), n.value, C.byref(n)), "nxhip_read_block_noise")
        return bmax, active

    def active_count(self):
        n = C.c_uint32(0)
        check(self.L.nxhip_read_active_map(self.h, None, 0, C.byref(n)), "nxhip_read_active_map")
        return n.value

    def read_active_map(self):
        """base-local index of every path of a frame slice of the next pass, in order"""
        out = np.zeros(max(self.active_count(), 1), np.uint32)
        n = C.c_uint32(0)
        check(self.L.nxhip_read_active_map(self.h, _ptr(out), len(out), C.byref(n)), "nxhip_read_active_map")
        return out[:n.value]

    def bind_radiance(self, dev_ptr, capacity):
        check(self.L.nxhip_bind_radiance(self.h, C.c_void_p(dev_ptr) if dev_ptr else None, capacity), "nxhip_bind_radiance")

    def read_full_accumulation(self):
        out = np.zeros((self.width * self.height, 3), np.float32)
        check(self.L.nxhip_read_full_accumulation(self.h, _ptr(out)), "nxhip_read_full_accumulation")
        return out

    def read_full_rgba8(self):
        out = np.zeros(self.width * self.height, np.uint32)
        check(self.L.nxhip_read_full_rgba8(self.h, _ptr(out)), "nxhip_read_full_rgba8")
        return out

    def render(self, frames):
        check(self.L.nxhip_render(self.h, frames), "nxhip_render")

    def sync(self):
        check(self.L.nxhip_sync(self.h), "nxhip_sync")

    def read_radiance(self):
        out = np.zeros((self._last_pass_paths(), 3), np.float32)
        check(self.L.nxhip_read_radiance(self.h, _ptr(out)), "nxhip_read_radiance")
        return out

    def _last_pass_paths(self):
        if not self.adaptive:
            return self.local_count * self.frames_per_pass
        if self._pass_paths is None:
            raise NexusError("adaptive sampling: the per-path values are those of the last render_frame pass; none has been issued since "
                             "set_adaptive / render_adaptive (whose passes pack a number of frames this wrapper does not know)")
        return self._pass_paths

    def read_accumulation(self):
        out = np.zeros((self.local_count, 3), np.float32)
        check(self.L.nxhip_read_accumulation(self.h, _ptr(out)), "nxhip_read_accumulation")
        return out

    def read_rgba8(self):
        out = np.zeros(self.local_count, np.uint32)
        check(self.L.nxhip_read_rgba8(self.h, _ptr(out)), "nxhip_read_rgba8")
        return out

    def radiance_device_ptr(self):
        return self.L.nxhip_radiance_device_ptr(self.h)

    def accumulation_device_ptr(self):
        return self.L.nxhip_accumulation_device_ptr(self.h)

    def read_queue_sizes(self):
        q = QueueSizes()
        check(self.L.nxhip_read_queue_sizes(self.h, C.byref(q)), "nxhip_read_queue_sizes")
        return {n: np.array(getattr(q, n)[:], dtype=np.int32) for n, _ in QueueSizes._fields_}

    def read_material_queue_sizes(self, material_type):
        """items the material step shaded as `material_type` (pod.MAT_*, MAT_METALROUGH included) per bounce slot: int32[PATH_MAX_LENGTH]"""
        out = np.zeros(pod.PATH_MAX_LENGTH, dtype=np.int32)
        check(self.L.nxhip_read_material_queue_sizes(self.h, int(material_type), _ptr(out)), "nxhip_read_material_queue_sizes")
        return out

    def set_pixel_query(self, x, y):
        check(self.L.nxhip_set_pixel_query(self.h, x, y), "nxhip_set_pixel_query")

    def get_selected_instance(self):
        v = C.c_int32(0)
        check(self.L.nxhip_get_selected_instance(self.h, C.byref(v)), "nxhip_get_selected_instance")
        return v.value

    # hooks
    def trace_batch(self, rays):
        rays = np.ascontiguousarray(rays, dtype=pod.RAY_DT)
        hits = np.zeros(len(rays), dtype=pod.HIT_DT)
        check(self.L.nxhip_trace_batch(self.h, _ptr(rays), len(rays), _ptr(hits)), "nxhip_trace_batch")
        return hits

    def trace_shadow_batch(self, rays, tmax):
        rays = np.ascontiguousarray(rays, dtype=pod.RAY_DT)
        tmax = np.ascontiguousarray(tmax, dtype=np.float32)
        occ = np.zeros(len(rays), dtype=np.uint8)
        check(self.L.nxhip_trace_shadow_batch(self.h, _ptr(rays), _ptr(tmax), len(rays), _ptr(occ)), "nxhip_trace_shadow_batch")
        return occ

    def trace_transmittance_batch(self, rays, tmax):
        """the rays' transmittance T (float32; 0 = occluded) through the any-hit TRANSMIT instance, whatever the context's mode"""
        rays = np.ascontiguousarray(rays, dtype=pod.RAY_DT)
        tmax = np.ascontiguousarray(tmax, dtype=np.float32)
        out = np.zeros(len(rays), dtype=np.float32)
        check(self.L.nxhip_trace_transmittance_batch(self.h, _ptr(rays), _ptr(tmax), len(rays), _ptr(out)), "nxhip_trace_transmittance_batch")
        return out

    def _hook(self, name, *args):
        """the library's `name` on this context; arrays go as their addresses, None as a null pointer"""
        check(getattr(self.L, name)(self.h, *[_ptr(a) if isinstance(a, np.ndarray) else a for a in args]), name)

    def _bsdf_batch(self, name, material, queries):
        mat = np.ascontiguousarray(material, dtype=pod.MAT_DT).reshape(1)
        q, = _cols((queries, pod.BSDF_QUERY_DT, 1))
        out, = _outs(len(q), (pod.BSDF_RESULT_DT, 1))
        self._hook(name, mat, q, len(q), out)
        return out

    def bsdf_sample_batch(self, material, queries):
        return self._bsdf_batch("nxhip_bsdf_sample_batch", material, queries)

    def bsdf_eval_batch(self, material, queries):
        return self._bsdf_batch("nxhip_bsdf_eval_batch", material, queries)

    def tex2d_batch(self, kind, texture_id, uv):
        uv, = _cols((uv, _F32, 2))
        out, = _outs(len(uv), (_F32, 4))
        self._hook("nxhip_tex2d_batch", TEXTURE_KINDS[kind], int(texture_id), uv, len(uv), out)
        return out

    def fmath_batch(self, op, a, b=None):
        """include/nexus_fmath.h on the device: out[i] = nxf_apply(op, a[i], b[i]) (op: pod.NXF_OP_*)"""
        a, b = _cols((a, np.float64, 1), (b, np.float64, 1))
        out, = _outs(len(a), (np.float64, 1))
        self._hook("nxhip_fmath_batch", int(op), a, b, len(a), out)
        return out

    def enable_trace_stats(self, on=True):
        check(self.L.nxhip_enable_trace_stats(self.h, 1 if on else 0), "nxhip_enable_trace_stats")

    def read_trace_stats(self, reset=False):
        a, b = TraceStats(), TraceStats()
        check(self.L.nxhip_read_trace_stats(self.h, C.byref(a), C.byref(b), 1 if reset else 0), "nxhip_read_trace_stats")
        return a.as_dict(), b.as_dict()

    def enable_kernel_timing(self, on=True, in_graph=False, last_replay_only=False):
        """on: hipEvent pair per kernel launch; in_graph: keep the hipGraph (and its trace || shadow overlap) and time with
        event-record nodes inside it, otherwise launch kernel by kernel; last_replay_only (with in_graph): no sync between
        replays, read_kernel_times returns the last replay of the series"""
        mode = 0 if not on else (3 if (in_graph and last_replay_only) else 2 if in_graph else 1)
        check(self.L.nxhip_enable_kernel_timing(self.h, mode), "nxhip_enable_kernel_timing")

    def read_graph_timeline(self):
        """the kernels of the last timed replay (enable_kernel_timing(in_graph=True)) in graph order:
        [(class name, start ms since the replay's first kernel, duration ms), ...]"""
        n = C.c_uint32(0)
        check(self.L.nxhip_read_graph_timeline(self.h, None, None, None, 0, C.byref(n)), "nxhip_read_graph_timeline")
        k = np.zeros(n.value, np.int32)
        s = np.zeros(n.value, np.float32)
        d = np.zeros(n.value, np.float32)
        if n.value:
            check(self.L.nxhip_read_graph_timeline(self.h, _ptr(k), _ptr(s), _ptr(d), n.value, C.byref(n)), "nxhip_read_graph_timeline")
        return [(KERNEL_CLASSES[int(k[i])], float(s[i]), float(d[i])) for i in range(n.value)]

    def read_kernel_times(self, reset=False):
        t = KernelTimes()
        check(self.L.nxhip_read_kernel_times(self.h, C.byref(t), 1 if reset else 0), "nxhip_read_kernel_times")
        return {k: {"ms": t.ms[i], "launches": int(t.launches[i])} for i, k in enumerate(KERNEL_CLASSES)}


def denoise_defaults():
    """nxhip_denoise_defaults as a pod.DENOISE_DT record"""
    p = np.zeros(1, pod.DENOISE_DT)
    check(lib().nxhip_denoise_defaults(_ptr(p)), "nxhip_denoise_defaults")
    return p


def adaptive_defaults():
    """nxhip_adaptive_defaults as a pod.ADAPTIVE_DT record"""
    p = np.zeros(1, pod.ADAPTIVE_DT)
    check(lib().nxhip_adaptive_defaults(_ptr(p)), "nxhip_adaptive_defaults")
    return p


def tile_pixel_map(width, height, world, rank, tile_rows, tiled=True):
    """the library's own tile split (nxhip_tile_pixel_map); no GPU needed"""
    n = C.c_uint32(0)
    check(lib().nxhip_tile_pixel_map(width, height, world, rank, tile_rows, 1 if tiled else 0, None, C.byref(n)), "nxhip_tile_pixel_map")
    out = np.zeros(n.value, dtype=np.uint32)
    check(lib().nxhip_tile_pixel_map(width, height, world, rank, tile_rows, 1 if tiled else 0, _ptr(out), C.byref(n)), "nxhip_tile_pixel_map")
    return out


def mgpu_unique_id():
    uid = np.zeros(128, dtype=np.uint8)
    check(lib().nxhip_mgpu_unique_id(_ptr(uid)), "nxhip_mgpu_unique_id")
    return uid.tobytes()


def device_count():
    return int(lib().nxhip_device_count())


def queue_budget_from_text(text):
    """nxhip_queue_budget_from_text: the queue budget a value of GPU_MAX_HW_QUEUES resolves to (None: not set); no device needed"""
    L = lib()
    return int(L.nxhip_queue_budget_from_text(None if text is None else str(text).encode()))


def resident_slots_for(passes, budget):
    """nxhip_resident_slots_for: of `passes` in flight, the slots the library keeps resident under a queue budget; no device needed"""
    return int(lib().nxhip_resident_slots_for(int(passes), int(budget)))


# ---- C++ Scene / PathTracer facade (include/nexus/Scene.h, PathTracer.h) -------------------------------

def _scheck(rc, what):
    if rc != 0:
        msg = lib().nxs_last_error()
        raise NexusError(f"{what} failed: {msg.decode() if msg else ''}")


class Scene:
    """nexus::Scene + its AssetManager, driven with the reference's call sequence."""

    def __init__(self, width, height):
        self.L = lib()
        h = C.c_void_p()
        _scheck(self.L.nxs_scene_create(width, height, C.byref(h)), "nxs_scene_create")
        self.h = h
        self.width, self.height = width, height

    def close(self):
        if getattr(self, "h", None):
            self.L.nxs_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_material(self, mat):
        m = np.ascontiguousarray(mat, dtype=pod.MAT_DT).reshape(1)
        i = C.c_int32(-1)
        _scheck(self.L.nxs_scene_add_material(self.h, _ptr(m), C.byref(i)), "nxs_scene_add_material")
        return i.value

    def add_texture(self, kind, rgba8):
        img = np.ascontiguousarray(rgba8, dtype=np.uint8)
        i = C.c_int32(-1)
        _scheck(self.L.nxs_scene_add_texture(self.h, TEXTURE_KINDS[kind], _ptr(img), img.shape[1], img.shape[0], C.byref(i)), "nxs_scene_add_texture")
        return i.value

    def set_hdr_map(self, rgba8):
        img = np.ascontiguousarray(rgba8, dtype=np.uint8)
        _scheck(self.L.nxs_scene_set_hdr_map(self.h, _ptr(img), img.shape[1], img.shape[0]), "nxs_scene_set_hdr_map")

    def set_hdr_map_float(self, rgb):
        """Scene::AddHDRMapFloat: H x W x 3 float32 of linear radiance"""
        img = np.ascontiguousarray(rgb, dtype=np.float32)
        _scheck(self.L.nxs_scene_set_hdr_map_float(self.h, _ptr(img), img.shape[1], img.shape[0]), "nxs_scene_set_hdr_map_float")

    def set_sky(self, sky):
        """Scene::SetSky (a pod.SKY_DT record, pod.Sky); None: Scene::ClearSky"""
        if sky is None:
            _scheck(self.L.nxs_scene_clear_sky(self.h), "nxs_scene_clear_sky")
            return
        s = np.ascontiguousarray(sky, dtype=pod.SKY_DT).reshape(1)
        _scheck(self.L.nxs_scene_set_sky(self.h, _ptr(s)), "nxs_scene_set_sky")

    def add_hdr_map_file_float(self, path, file_name):
        """Scene::AddHDRMapFloat(filePath, fileName): a Radiance .hdr file as linear float radiance"""
        _scheck(self.L.nxs_scene_add_hdr_map_file_float(self.h, path.encode(), file_name.encode()), "nxs_scene_add_hdr_map_file_float")

    def add_mesh(self, tris, material_id=-1):
        t = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
        i = C.c_int32(-1)
        _scheck(self.L.nxs_scene_add_mesh(self.h, _ptr(t), len(t), material_id, C.byref(i)), "nxs_scene_add_mesh")
        return i.value

    def update_mesh(self, mesh_id, tris):
        """AssetManager::UpdateMeshTriangles: the mesh's triangles, in the same order, at new positions (a deforming mesh)"""
        t = np.ascontiguousarray(tris, dtype=pod.TRI_DT)
        _scheck(self.L.nxs_scene_update_mesh(self.h, mesh_id, _ptr(t), len(t)), "nxs_scene_update_mesh")

    def set_instance_transform(self, instance_id, position, rotation_deg, scale):
        p, r, sc = (np.asarray(x, np.float32) for x in (position, rotation_deg, scale))
        _scheck(self.L.nxs_scene_set_instance_transform(self.h, instance_id, _ptr(p), _ptr(r), _ptr(sc)), "nxs_scene_set_instance_transform")

    def assign_material(self, instance_id, material_id):
        _scheck(self.L.nxs_scene_assign_material(self.h, instance_id, material_id), "nxs_scene_assign_material")

    def set_tlas_refit(self, enable=True):
        _scheck(self.L.nxs_scene_set_tlas_refit(self.h, 1 if enable else 0), "nxs_scene_set_tlas_refit")

    def set_device_tlas(self, enable=True):
        """the TLAS is built (nxhip_rebuild_tlas) and refitted on the device; update() runs no host TLAS builder"""
        _scheck(self.L.nxs_scene_set_device_tlas(self.h, 1 if enable else 0), "nxs_scene_set_device_tlas")

    def load_file(self, path, file_name):
        """Scene::CreateMeshInstanceFromFile: materials, meshes (one BVH8 each) and instances of a .glb / .obj"""
        _scheck(self.L.nxs_scene_load_file(self.h, str(path).encode(), str(file_name).encode()), "nxs_scene_load_file")

    def set_metal_rough(self, on=True):
        """Scene::SetMetalRoughMaterials: the files loaded from here on read a .glb's materials as MAT_METALROUGH (off by default)"""
        _scheck(self.L.nxs_scene_set_metal_rough(self.h, 1 if on else 0), "nxs_scene_set_metal_rough")

    def set_material_alpha_modes(self, on=True):
        """Scene::SetMaterialAlphaModes: the files loaded from here on carry their materials' glTF alphaMode / alphaCutoff to the device (off by default)"""
        _scheck(self.L.nxs_scene_set_material_alpha_modes(self.h, 1 if on else 0), "nxs_scene_set_material_alpha_modes")

    def set_skins(self, on=True):
        """Scene::SetSkins: the files loaded from here on keep their glTF skins, joint animations and node tree (off by default)"""
        _scheck(self.L.nxs_scene_set_skins(self.h, 1 if on else 0), "nxs_scene_set_skins")

    def set_morphs(self, on=True):
        """Scene::SetMorphs: the files loaded from here on keep their glTF morph targets and weights animations (off by default)"""
        _scheck(self.L.nxs_scene_set_morphs(self.h, 1 if on else 0), "nxs_scene_set_morphs")

    def mesh_target_count(self, mesh_id):
        """morph targets of the mesh; 0: it has none"""
        return int(self.L.nxs_scene_mesh_target_count(self.h, int(mesh_id)))

    def morph_weights(self, mesh_id, animation=None, t=0.0):
        """Scene::MorphWeights: (targets,) float32 — the file's defaults, or the weights channel of animation `animation` at time t; the twin of
        nexus_amd.animation.morph_weights"""
        n = C.c_uint32(0)
        a = -1 if animation is None else int(animation)
        _scheck(self.L.nxs_scene_morph_weights(self.h, int(mesh_id), a, float(t), None, 0, C.byref(n)), "nxs_scene_morph_weights")
        out = np.zeros(n.value, np.float32)
        _scheck(self.L.nxs_scene_morph_weights(self.h, int(mesh_id), a, float(t), _ptr(out), n.value, C.byref(n)), "nxs_scene_morph_weights")
        return out

    def mesh_count(self):
        return int(self.L.nxs_scene_mesh_count(self.h))

    def animation_count(self):
        return int(self.L.nxs_scene_animation_count(self.h))

    def mesh_joint_count(self, mesh_id):
        """joints of the mesh's skin; 0: the mesh is not skinned"""
        return int(self.L.nxs_scene_mesh_joint_count(self.h, int(mesh_id)))

    def joint_palette(self, mesh_id, animation=None, t=0.0):
        """Scene::JointPalette: (joints, 12) float32 — the pose of animation `animation` (None: the rest pose) at time t, evaluated in binary64
        on the host; the twin of nexus_amd.animation.joint_palette"""
        n = C.c_uint32(0)
        a = -1 if animation is None else int(animation)
        _scheck(self.L.nxs_scene_joint_palette(self.h, int(mesh_id), a, float(t), None, 0, C.byref(n)), "nxs_scene_joint_palette")
        out = np.zeros((n.value, 12), np.float32)
        _scheck(self.L.nxs_scene_joint_palette(self.h, int(mesh_id), a, float(t), _ptr(out), n.value, C.byref(n)), "nxs_scene_joint_palette")
        return out

    def material_alphas(self):
        """AssetManager::GetMaterialAlphas: pod.ALPHA_DT records, one per material (empty: no material has a mode)"""
        n = C.c_uint32(0)
        _scheck(self.L.nxs_scene_material_alphas(self.h, None, 0, C.byref(n)), "nxs_scene_material_alphas")
        out = np.zeros(n.value, dtype=pod.ALPHA_DT)
        if n.value:
            _scheck(self.L.nxs_scene_material_alphas(self.h, _ptr(out), n.value, C.byref(n)), "nxs_scene_material_alphas")
        return out

    def create_instance(self, mesh_id, material_id, position=(0, 0, 0), rotation_deg=(0, 0, 0), scale=(1, 1, 1)):
        p, r, s = (np.asarray(x, np.float32) for x in (position, rotation_deg, scale))
        i = C.c_int32(-1)
        _scheck(self.L.nxs_scene_create_instance(self.h, mesh_id, material_id, _ptr(p), _ptr(r), _ptr(s), C.byref(i)), "nxs_scene_create_instance")
        return i.value

    def set_camera(self, position, forward, hfov_deg, focus_dist=5.0, defocus_deg=0.0):
        p, f = np.asarray(position, np.float32), np.asarray(forward, np.float32)
        _scheck(self.L.nxs_scene_set_camera(self.h, _ptr(p), _ptr(f), hfov_deg, focus_dist, defocus_deg), "nxs_scene_set_camera")

    def set_render_settings(self, st):
        st = np.ascontiguousarray(st, dtype=pod.SETTINGS_DT).reshape(1)
        _scheck(self.L.nxs_scene_set_render_settings(self.h, _ptr(st)), "nxs_scene_set_render_settings")

    def update(self):
        _scheck(self.L.nxs_scene_update(self.h), "nxs_scene_update")

    def light_count(self):
        return int(self.L.nxs_scene_light_count(self.h))

    def add_analytic_light(self, light):
        """Scene::AddAnalyticLight: a pod.ALIGHT_DT record (pod.make_analytic_light); returns its index"""
        l = np.ascontiguousarray(light, dtype=pod.ALIGHT_DT).reshape(1)
        i = C.c_uint32(0)
        _scheck(self.L.nxs_scene_add_analytic_light(self.h, _ptr(l), C.byref(i)), "nxs_scene_add_analytic_light")
        return int(i.value)

    def set_material_detail(self, material_id, detail):
        """AssetManager::SetMaterialDetail: a pod.DETAIL_DT record (pod.make_material_detail) with ids of add_texture("normal" / "roughness", ...)"""
        d = np.ascontiguousarray(detail, dtype=pod.DETAIL_DT).reshape(1)
        _scheck(self.L.nxs_scene_set_material_detail(self.h, int(material_id), _ptr(d)), "nxs_scene_set_material_detail")

    def clear_material_details(self):
        """AssetManager::ClearMaterialDetails: no material has detail maps any more (what nexus_render --no-detail-maps does)"""
        _scheck(self.L.nxs_scene_clear_material_details(self.h), "nxs_scene_clear_material_details")

    def material_details(self):
        """AssetManager::GetMaterialDetails: pod.DETAIL_DT records, one per material, or none at all"""
        out = np.zeros(int(self.L.nxs_scene_material_detail_count(self.h)), dtype=pod.DETAIL_DT)
        _scheck(self.L.nxs_scene_material_details(self.h, _ptr(out) if len(out) else None, len(out)), "nxs_scene_material_details")
        return out

    def remove_analytic_light(self, index):
        _scheck(self.L.nxs_scene_remove_analytic_light(self.h, int(index)), "nxs_scene_remove_analytic_light")

    def analytic_lights(self):
        """Scene::GetAnalyticLights: the records as the scene holds them (added by hand or read from a .glb's KHR_lights_punctual)"""
        out = np.zeros(int(self.L.nxs_scene_analytic_light_count(self.h)), dtype=pod.ALIGHT_DT)
        _scheck(self.L.nxs_scene_analytic_lights(self.h, _ptr(out) if len(out) else None, len(out)), "nxs_scene_analytic_lights")
        return out

    def set_medium(self, medium):
        """Scene::SetMedium (a pod.MEDIUM_DT record, pod.make_medium); None: Scene::ClearMedium"""
        if medium is None:
            _scheck(self.L.nxs_scene_clear_medium(self.h), "nxs_scene_clear_medium")
            return
        m = np.ascontiguousarray(medium, dtype=pod.MEDIUM_DT).reshape(1)
        _scheck(self.L.nxs_scene_set_medium(self.h, _ptr(m)), "nxs_scene_set_medium")

    def set_medium_density(self, rho):
        """Scene::SetMediumDensity (float32 of shape (nz, ny, nx)); None: Scene::ClearMediumDensity"""
        if rho is None:
            _scheck(self.L.nxs_scene_clear_medium_density(self.h), "nxs_scene_clear_medium_density")
            return
        r = np.ascontiguousarray(rho, dtype=np.float32)
        assert r.ndim == 3, "a density grid has the shape (nz, ny, nx)"
        _scheck(self.L.nxs_scene_set_medium_density(self.h, _ptr(r), r.shape[2], r.shape[1], r.shape[0]), "nxs_scene_set_medium_density")

    def medium_density(self):
        """Scene::GetMediumDensity: float32 of shape (nz, ny, nx), or None"""
        dims = (C.c_uint32 * 3)()
        _scheck(self.L.nxs_scene_medium_density(self.h, dims, None, 0), "nxs_scene_medium_density")
        if dims[0] == 0:
            return None
        out = np.zeros((dims[2], dims[1], dims[0]), dtype=np.float32)
        _scheck(self.L.nxs_scene_medium_density(self.h, dims, _ptr(out), out.size), "nxs_scene_medium_density")
        return out

    def medium(self):
        """Scene::GetMedium: the record, or None"""
        out = np.zeros(1, dtype=pod.MEDIUM_DT)
        has = C.c_int(0)
        _scheck(self.L.nxs_scene_medium(self.h, _ptr(out), C.byref(has)), "nxs_scene_medium")
        return out[0] if has.value else None

    def instance_count(self):
        return int(self.L.nxs_scene_instance_count(self.h))


def write_png(path, rgba8, width, height, flip=True):
    px = np.ascontiguousarray(rgba8, dtype=np.uint32)
    L = lib()
    _scheck(L.nxh_write_png(str(path).encode(), _ptr(px), width, height, 1 if flip else 0), "nxh_write_png")


def write_exr(path, rgb, width, height, flip=True):
    px = np.ascontiguousarray(rgb, dtype=np.float32)
    L = lib()
    _scheck(L.nxh_write_exr(str(path).encode(), _ptr(px), width, height, 1 if flip else 0), "nxh_write_exr")


class Renderer:
    """nexus::Renderer: the reference's frame driver (Renderer::Render / SaveScreenshot) without its window."""

    def __init__(self, width, height, scene, device=0):
        self.L = lib()
        L = self.L
        h = C.c_void_p()
        _scheck(L.nxs_renderer_create(width, height, scene.h, device, C.byref(h)), "nxs_renderer_create")
        self.h = h
        self.width, self.height = width, height

    def close(self):
        if getattr(self, "h", None):
            self.L.nxs_renderer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_modes(self, rng_mode, compact_mode, conductor_mode):
        _scheck(self.L.nxs_renderer_set_modes(self.h, rng_mode, compact_mode, conductor_mode), "nxs_renderer_set_modes")

    def render(self, scene, delta_time=0.0):
        _scheck(self.L.nxs_renderer_render(self.h, scene.h, delta_time), "nxs_renderer_render")

    def reset(self):
        _scheck(self.L.nxs_renderer_reset(self.h), "nxs_renderer_reset")

    def save_screenshot(self, path):
        _scheck(self.L.nxs_renderer_save_screenshot(self.h, str(path).encode()), "nxs_renderer_save_screenshot")

    def save_exr(self, path):
        _scheck(self.L.nxs_renderer_save_exr(self.h, str(path).encode()), "nxs_renderer_save_exr")

    def set_denoise(self, on=True):
        """Renderer::SetDenoise: feature buffers on, accumulation restarted; save_screenshot then writes the filtered image"""
        _scheck(self.L.nxs_renderer_set_denoise(self.h, 1 if on else 0), "nxs_renderer_set_denoise")

    def save_denoised_exr(self, path):
        _scheck(self.L.nxs_renderer_save_denoised_exr(self.h, str(path).encode()), "nxs_renderer_save_denoised_exr")

    def save_feature_exr(self, path):
        """<stem>.albedo.exr, <stem>.normal.exr, <stem>.depth.exr beside each other"""
        _scheck(self.L.nxs_renderer_save_feature_exr(self.h, str(path).encode()), "nxs_renderer_save_feature_exr")

    def set_adaptive(self, params=None):
        """Renderer::SetAdaptive: a pod.ADAPTIVE_DT record (adaptive_defaults()), None = off; starts the accumulation over"""
        p = None if params is None else np.ascontiguousarray(params, dtype=pod.ADAPTIVE_DT).reshape(1)
        _scheck(self.L.nxs_renderer_set_adaptive(self.h, _ptr(p) if p is not None else None), "nxs_renderer_set_adaptive")

    def render_adaptive(self, scene, max_frames, interval):
        """Renderer::RenderAdaptive: the frames issued"""
        frames = C.c_uint32(0)
        _scheck(self.L.nxs_renderer_render_adaptive(self.h, scene.h, int(max_frames), int(interval), C.byref(frames)), "nxs_renderer_render_adaptive")
        return frames.value

    def save_sample_count_exr(self, path):
        _scheck(self.L.nxs_renderer_save_sample_count_exr(self.h, str(path).encode()), "nxs_renderer_save_sample_count_exr")

    def device_context(self):
        """the renderer's nxhip_ctx wrapped as a Context that does not own it (read-backs; do not close)"""
        ctx = Context.__new__(Context)
        ctx.L = lib()
        ctx.h = C.c_void_p(self.L.nxs_renderer_device_context(self.h))
        ctx.width, ctx.height = self.width, self.height
        ctx.local_count = self.width * self.height
        ctx.frames_per_pass = 1
        ctx.close = lambda: None  # (the renderer owns it)
        return ctx

    def frame_number(self):
        return int(self.L.nxs_renderer_frame_number(self.h))

    def megasamples_per_second(self):
        return float(self.L.nxs_renderer_megasamples_per_second(self.h))

    def read_accumulation(self):
        out = np.zeros((self.width * self.height, 3), dtype=np.float32)
        check(lib().nxhip_read_accumulation(C.c_void_p(self.L.nxs_renderer_device_context(self.h)), _ptr(out)), "nxhip_read_accumulation")
        return out

    def read_pixels(self):
        out = np.zeros(self.width * self.height, dtype=np.uint32)
        check(lib().nxhip_read_rgba8(C.c_void_p(self.L.nxs_renderer_device_context(self.h)), _ptr(out)), "nxhip_read_rgba8")
        return out


class PathTracer:
    """nexus::PathTracer: Render(scene) = one frame through the device layer + accumulate."""

    def __init__(self, width, height, device=0):
        self.L = lib()
        h = C.c_void_p()
        _scheck(self.L.nxs_pathtracer_create(width, height, device, C.byref(h)), "nxs_pathtracer_create")
        self.h = h
        self.width, self.height = width, height

    def close(self):
        if getattr(self, "h", None):
            self.L.nxs_pathtracer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_modes(self, rng_mode, compact_mode, conductor_mode):
        _scheck(self.L.nxs_pathtracer_set_modes(self.h, rng_mode, compact_mode, conductor_mode), "nxs_pathtracer_set_modes")

    def set_frames_per_pass(self, frames):
        _scheck(self.L.nxs_pathtracer_set_frames_per_pass(self.h, frames), "nxs_pathtracer_set_frames_per_pass")

    def set_passes_in_flight(self, passes):
        _scheck(self.L.nxs_pathtracer_set_passes_in_flight(self.h, passes), "nxs_pathtracer_set_passes_in_flight")

    def set_pixel_order(self, order):
        _scheck(self.L.nxs_pathtracer_set_pixel_order(self.h, int(order)), "nxs_pathtracer_set_pixel_order")

    def set_entry_points(self, on=True):
        _scheck(self.L.nxs_pathtracer_set_entry_points(self.h, 1 if on else 0), "nxs_pathtracer_set_entry_points")

    def set_shadow_transmittance(self, mode):
        """PathTracer::SetShadowTransmittance: pod.SHADOWS_OPAQUE (the reference's rule) or pod.SHADOWS_TRANSMIT (opacity and texture alpha attenuate shadow rays)"""
        _scheck(self.L.nxs_pathtracer_set_shadow_transmittance(self.h, int(mode)), "nxs_pathtracer_set_shadow_transmittance")

    def set_light_sampling(self, mode):
        """PathTracer::SetLightSampling: pod.LIGHTS_UNIFORM (the reference's rule) or pod.LIGHTS_POWER (area x emitted luminance)"""
        _scheck(self.L.nxs_pathtracer_set_light_sampling(self.h, int(mode)), "nxs_pathtracer_set_light_sampling")

    def set_light_importance(self, importance):
        """PathTracer::SetLightImportance: pod.LIGHT_IMPORTANCE_POWER (the default) or pod.LIGHT_IMPORTANCE_POSITION (the light tree)"""
        _scheck(self.L.nxs_pathtracer_set_light_importance(self.h, int(importance)), "nxs_pathtracer_set_light_importance")

    def read_accumulation(self):
        """the running mean over the frames rendered so far, (pixels, 3) float32, from this path tracer's device context"""
        out = np.zeros((self.width * self.height, 3), np.float32)
        check(self.L.nxhip_read_accumulation(self.L.nxs_pathtracer_device_context(self.h), _ptr(out)), "nxhip_read_accumulation")
        return out

    def set_feature_buffers(self, on=True):
        """PathTracer::SetFeatureBuffers: albedo / normal / depth of the camera ray's hit, accumulated like the colour"""
        _scheck(self.L.nxs_pathtracer_set_feature_buffers(self.h, 1 if on else 0), "nxs_pathtracer_set_feature_buffers")

    def set_adaptive(self, params=None):
        """PathTracer::SetAdaptive: a pod.ADAPTIVE_DT record (adaptive_defaults()), None = off"""
        p = None if params is None else np.ascontiguousarray(params, dtype=pod.ADAPTIVE_DT).reshape(1)
        _scheck(self.L.nxs_pathtracer_set_adaptive(self.h, _ptr(p) if p is not None else None), "nxs_pathtracer_set_adaptive")

    def set_device_blas_build(self, scene, enable=True):
        """PathTracer::SetDeviceBlasBuild: meshes added to `scene` from now on are built into BVH8s on the GPU"""
        _scheck(self.L.nxs_pathtracer_set_device_blas_build(self.h, scene.h, 1 if enable else 0), "nxs_pathtracer_set_device_blas_build")

    def pose_mesh(self, scene, mesh_id, palette):
        """PathTracer::PoseMesh: pose a skinned mesh on the device with a (joints, 12) palette — before scene.update()"""
        m = np.ascontiguousarray(palette, dtype=np.float32).reshape(-1, 12)
        _scheck(self.L.nxs_pathtracer_pose_mesh(self.h, scene.h, int(mesh_id), _ptr(m), len(m)), "nxs_pathtracer_pose_mesh")

    def pose_mesh_morph(self, scene, mesh_id, weights, palette=None):
        """the PathTracer::PoseMesh overload that takes weights: one per morph target, and the (joints, 12) palette where the mesh is skinned —
        before scene.update()"""
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        m = None if palette is None else np.ascontiguousarray(palette, dtype=np.float32).reshape(-1, 12)
        _scheck(self.L.nxs_pathtracer_pose_mesh_morph(self.h, scene.h, int(mesh_id), _ptr(w), len(w), None if m is None else _ptr(m), 0 if m is None else len(m)),
                "nxs_pathtracer_pose_mesh_morph")

    def update_device_scene(self, scene):
        _scheck(self.L.nxs_pathtracer_update_device_scene(self.h, scene.h), "nxs_pathtracer_update_device_scene")

    def render(self, scene):
        _scheck(self.L.nxs_pathtracer_render(self.h, scene.h), "nxs_pathtracer_render")

    def reset_frame_number(self):
        _scheck(self.L.nxs_pathtracer_reset_frame_number(self.h), "nxs_pathtracer_reset_frame_number")

    def frame_number(self):
        return int(self.L.nxs_pathtracer_frame_number(self.h))

    def read_pixels(self):
        out = np.zeros(self.width * self.height, np.uint32)
        _scheck(self.L.nxs_pathtracer_read_pixels(self.h, _ptr(out)), "nxs_pathtracer_read_pixels")
        return out

    def read_radiance(self):
        out = np.zeros((self.width * self.height, 3), np.float32)
        check(self.L.nxhip_read_radiance(self.L.nxs_pathtracer_device_context(self.h), _ptr(out)), "nxhip_read_radiance")
        return out

    def read_blas(self, blas_id, tri_count):
        """nodes and primitive index list of BLAS `blas_id` of this path tracer's device context"""
        ctx = self.L.nxs_pathtracer_device_context(self.h)
        n = C.c_uint32(0)
        check(self.L.nxhip_read_blas(ctx, blas_id, None, 0, None, 0, C.byref(n)), "nxhip_read_blas")
        nodes = np.zeros(n.value, dtype=pod.NODE_DT)
        idx = np.zeros(tri_count, dtype=np.uint32)
        check(self.L.nxhip_read_blas(ctx, blas_id, _ptr(nodes), n.value, _ptr(idx), tri_count, C.byref(n)), "nxhip_read_blas")
        return nodes, idx
