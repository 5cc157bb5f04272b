"""nexus_amd/cabi.py: ctypes signatures from C prototypes — every accepted form, and a refusal for everything else (no library needed)."""
import ctypes as C

import pytest

from nexus_amd import cabi

HEADER = """
/* a header (with parentheses; and a semicolon) in its comment: int nxhip_not_this(int); */
#ifndef X_H
#define X_H
#define NXHIP_LONG_MACRO(a) \\
    nxhip_not_this_either(a);
#ifdef __cplusplus
extern "C" {
#endif
typedef struct nxhip_ctx nxhip_ctx;
struct nxs_scene;
enum { NXHIP_OK = 0, NXHIP_ERR = 1 };
typedef struct nxhip_sizes {
    int32_t traceSize[8]; /* int nxhip_nor_this(void); */
} nxhip_sizes;
const char *nxhip_last_error(void);
int nxhip_device_count();
int nxhip_create(int device, uint32_t width, uint32_t height, const nx_settings *settings, /* (may be NULL); */
                 nxhip_ctx **out);
void nxhip_destroy(nxhip_ctx *ctx);
void nxh_mat4_from_trs(const float pos[3], const float rotDeg[3], const float scale[3], float out16[16]);
int nxhip_build_batch(nxhip_ctx *ctx, const nx_triangle *const *tris, const uint32_t *counts, uint32_t n, int32_t ids[2]);
int nxs_scene_load_file(nxs_scene *s, const char *path, const char *fileName); // trailing (comment);
int nxh_decode(const uint8_t *data, size_t size, uint64_t seed, float scale, double t, int32_t kind /* 0 (diffuse); 1 */, char *dst);
struct nxhip_ctx *nxs_renderer_device_context(nxs_renderer *r);
const uint32_t *nxh_prim_indices(const nxh_bvh8 *b);
uint32_t nxh_count(const nxh_bvh8 *b);
uint64_t nxhip_abi_stamp(void);
double nxs_rate(const nxs_renderer *r);
static inline uint64_t nxhip_abi_mix(uint64_t h, uint64_t v)
{
    for (int i = 0; i < 8; ++i) { h ^= v & 0xff; }
    return h;
}
static inline int nxhip_header_check(void)
{
    return nxhip_check_library(nxhip_abi_mix(nxhip_abi_stamp(), 1));
}
int nxhip_check_library(uint64_t stamp);
#ifdef __cplusplus
}
#endif
#endif
"""

vp, cp, u32 = C.c_void_p, C.c_char_p, C.c_uint32


def test_every_accepted_form():
    assert cabi.parse(HEADER) == {
        "nxhip_last_error": (cp, []),
        "nxhip_device_count": (C.c_int, []),
        "nxhip_create": (C.c_int, [C.c_int, u32, u32, vp, vp]),  # a prototype over two lines
        "nxhip_destroy": (None, [vp]),
        "nxh_mat4_from_trs": (None, [vp, vp, vp, vp]),  # arrays
        "nxhip_build_batch": (C.c_int, [vp, vp, vp, u32, vp]),  # const T* const*
        "nxs_scene_load_file": (C.c_int, [vp, cp, cp]),
        "nxh_decode": (C.c_int, [vp, C.c_size_t, C.c_uint64, C.c_float, C.c_double, C.c_int32, vp]),  # (a char* that is not const: a buffer)
        "nxs_renderer_device_context": (vp, [vp]),
        "nxh_prim_indices": (vp, [vp]),
        "nxh_count": (u32, [vp]),
        "nxhip_abi_stamp": (C.c_uint64, []),
        "nxs_rate": (C.c_double, [vp]),
        "nxhip_check_library": (C.c_int, [C.c_uint64]),
    }
    assert list(cabi.parse(HEADER))[:3] == ["nxhip_last_error", "nxhip_device_count", "nxhip_create"], "in the header's order"


@pytest.mark.parametrize("proto, what", [
    ("int nxhip_wait(nxhip_ctx *ctx, long timeout);", "long timeout"),  # a scalar type the table does not know
    ("long nxhip_ticks(void);", "long"),
    ("int nxhip_set_camera(nxhip_ctx *ctx, nx_camera cam);", "nx_camera cam"),  # a struct by value
    ("int nxhip_set_camera2(nxhip_ctx *ctx, struct nx_camera cam);", "struct nx_camera cam"),
    ("nx_camera nxhip_get_camera(nxhip_ctx *ctx);", "nx_camera"),
    ("int nxhip_on_frame(nxhip_ctx *ctx, void (*callback)(int frame));", None),  # a function pointer
    ("int nxhip_log(const char *format, ...);", None),  # variadic
    ("int nxhip_unsigned(unsigned int n);", "unsigned int n"),
    ("int nxhip_defined_here(int a) { return a; }", None),  # an exported function with a body
    ("int helper(int a);", None),  # not one of the three prefixes
    ("extern int nxhip_counter;", None),  # a variable
])
def test_what_it_cannot_classify_is_refused_with_the_prototype(proto, what):
    with pytest.raises(cabi.NexusError) as e:
        cabi.parse("typedef struct nxhip_ctx nxhip_ctx;\n" + proto + "\nint nxhip_sync(nxhip_ctx *ctx);\n")
    msg = str(e.value)
    assert " ".join(proto.rstrip(";").split("{")[0].split()) in msg, msg
    assert what is None or "'%s'" % what in msg, msg


def test_unbalanced_braces_are_refused():
    with pytest.raises(cabi.NexusError, match="unbalanced"):
        cabi.parse("int nxhip_sync(nxhip_ctx *ctx);\n}\n")
    with pytest.raises(cabi.NexusError, match="ends inside"):
        cabi.parse('extern "C" {\nint nxhip_sync(nxhip_ctx *ctx)')


def test_a_missing_header_is_an_error_that_names_its_path(tmp_path):
    with pytest.raises(cabi.NexusError) as e:
        cabi.signatures(str(tmp_path))
    assert str(tmp_path / "nexus_hip.h") in str(e.value)


def test_the_real_headers():
    tables = cabi.signatures()
    assert list(tables) == ["nexus_hip.h", "nexus_host.h"]
    assert all(n.startswith("nxhip_") for n in tables["nexus_hip.h"]) and len(tables["nexus_hip.h"]) >= 140
    assert all(n.startswith(("nxh_", "nxs_")) for n in tables["nexus_host.h"]) and len(tables["nexus_host.h"]) >= 124
    assert "nxhip_header_abi_stamp" not in tables["nexus_hip.h"] and "nxhip_abi_mix" not in tables["nexus_hip.h"]
    assert tables["nexus_hip.h"]["nxhip_get_queue_budget"] == (C.c_int, [vp, vp, vp, vp])
    assert tables["nexus_host.h"]["nxs_scene_medium_density"] == (C.c_int, [vp, vp, vp, C.c_size_t])
