/*
 * nexus_pod.h — plain-old-data contracts shared by the host classes, the HIP device layer and the
 * test oracle.  Plain C (also valid C++ / HIP).  Byte layouts are identical to the reference's device
 * PODs so that buffers built by either side are interchangeable and fixtures are raw bytes.
 *
 * Reference layouts followed (all paths relative to /root/reference/Nexus/src):
 *   nx_bvh8_node     80 B  Cuda/BVH/BVH8.cuh:47-63, Geometry/BVH/BVH8.h:24-49
 *   nx_triangle      96 B  Cuda/Geometry/Triangle.cuh:25-49
 *   nx_mat4          64 B  Math/Mat4.h:24 (row major)
 *   nx_bvh_instance 160 B  Cuda/BVH/BVHInstance.cuh:7-14
 *   nx_material      60 B  Cuda/Scene/Material.cuh:5-51
 *   nx_light         12 B  Cuda/Scene/Light.cuh:4-33
 *   (nx_analytic_light 64 B: an extension, no reference layout)
 *   (nx_material_detail 16 B: an extension, no reference layout)
 *   (nx_medium 48 B: an extension, no reference layout)
 *   (nx_sky 76 B: an extension, no reference layout)
 *   nx_camera        88 B  Cuda/Scene/Camera.cuh:5-15
 *   nx_render_settings 20 B Cuda/Scene/Scene.cuh:10-17, Renderer/RenderSettings.h:4-10
 */
#ifndef NEXUS_POD_H
#define NEXUS_POD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
#define NX_STATIC_ASSERT(c, m) static_assert(c, m)
#else
#define NX_STATIC_ASSERT(c, m) _Static_assert(c, m)
#endif

#define NX_ALIGN(n) __attribute__((aligned(n)))

/* Ylitie et al. 2017 compressed wide BVH node. */
typedef struct NX_ALIGN(16) nx_bvh8_node {
    float p[3];               /* origin of the local quantisation grid */
    uint8_t e[3];             /* biased exponents of the grid scale per axis */
    uint8_t imask;            /* bit i set: child slot i is an internal node */
    uint32_t childBaseIdx;    /* index of the first internal child */
    uint32_t triangleBaseIdx; /* index of the first leaf primitive in the index list */
    uint8_t meta[8];          /* per slot: inner 001|24+slot, leaf unary count|offset, empty 0 */
    uint8_t qlox[8], qloy[8], qloz[8];
    uint8_t qhix[8], qhiy[8], qhiz[8];
} nx_bvh8_node;
NX_STATIC_ASSERT(sizeof(nx_bvh8_node) == 80, "nx_bvh8_node must be 80 bytes");

typedef struct NX_ALIGN(8) nx_triangle {
    float pos0[3], pos1[3], pos2[3];
    float normal0[3], normal1[3], normal2[3];
    float texCoord0[2], texCoord1[2], texCoord2[2];
} nx_triangle;
NX_STATIC_ASSERT(sizeof(nx_triangle) == 96, "nx_triangle must be 96 bytes");

typedef struct nx_mat4 {
    float cell[16]; /* row major */
} nx_mat4;

typedef struct nx_bvh_instance {
    uint32_t bvhIdx;
    nx_mat4 invTransform;
    nx_mat4 transform;
    float boundsMin[3], boundsMax[3];
    int32_t materialId;
} nx_bvh_instance;
NX_STATIC_ASSERT(sizeof(nx_bvh_instance) == 160, "nx_bvh_instance must be 160 bytes");

/* NX_MAT_METALROUGH: an extension — glTF's metallic-roughness model in one BSDF (the rule is stated in full in include/nexus_hip.h,
 * nxhip_set_materials).  The four types in front of it are the reference's. */
enum { NX_MAT_DIFFUSE = 0, NX_MAT_DIELECTRIC = 1, NX_MAT_PLASTIC = 2, NX_MAT_CONDUCTOR = 3, NX_MAT_METALROUGH = 4 };

typedef struct nx_material {
    union {
        struct { float albedo[3]; } diffuse;
        struct { float albedo[3]; float roughness; float ior; } dielectric;
        struct { float albedo[3]; float roughness; float ior; } plastic;
        struct { float ior[3]; float k[3]; float roughness; } conductor;
        struct { float albedo[3]; float roughness; float ior; float metallic; } metalrough; /* = plastic's fields + metallic at byte 20 */
    };
    float emissive[3];
    float intensity;
    float opacity;
    int32_t diffuseMapId;
    int32_t emissiveMapId;
    int8_t type;
} nx_material;
NX_STATIC_ASSERT(sizeof(nx_material) == 60, "nx_material must be 60 bytes");
NX_STATIC_ASSERT(offsetof(nx_material, metalrough.metallic) == 20 && offsetof(nx_material, emissive) == 28, "the metalrough view fits the 28-byte union");

enum { NX_LIGHT_POINT = 0, NX_LIGHT_AREA = 1, NX_LIGHT_MESH = 2 };

typedef struct nx_light {
    union {
        struct { uint32_t radius; uint32_t intensity; } point;
        struct { uint32_t intensity; } area;
        struct { uint32_t meshId; } mesh; /* index of the mesh instance == index into the instance array */
    };
    int8_t type;
} nx_light;
NX_STATIC_ASSERT(sizeof(nx_light) == 12, "nx_light must be 12 bytes");

/* Extension: an analytic light (nxhip_set_analytic_lights; the sampling rule is stated in full in include/nexus_hip.h).  The 12-byte
 * nx_light above carries no position, so its NX_LIGHT_POINT can never be placed; this record can.  World space.  Radiometric RGB
 * throughout: no 683 lm/W enters anywhere.  glTF's `range` has no counterpart and is ignored by the loaders. */
enum { NX_ALIGHT_POINT = 0, NX_ALIGHT_SPOT = 1, NX_ALIGHT_DIRECTIONAL = 2 };
typedef struct NX_ALIGN(16) nx_analytic_light {
    float position[3];  float radius;         /* POINT, SPOT: centre; sphere radius, 0 = a point            */
    float direction[3]; float angularRadius;  /* SPOT: axis, away from the light.  DIRECTIONAL: the way the  */
                                              /* light travels; half-angle of the disc in radians, 0 = delta */
    float colour[3];    float intensity;      /* POINT, SPOT: colour x intensity = radiant intensity per sr  */
                                              /* DIRECTIONAL: irradiance of a surface facing the light       */
    float innerConeAngle, outerConeAngle;     /* SPOT, radians, 0 <= inner < outer <= pi/2                   */
    uint32_t type, pad_;
} nx_analytic_light;
NX_STATIC_ASSERT(sizeof(nx_analytic_light) == 64, "nx_analytic_light must be 64 bytes");

/* Extension: the detail maps of one material (nxhip_set_material_detail; the shading rule is stated in full in include/nexus_hip.h).
 * A table of these runs index-parallel to the material table: the 60-byte nx_material keeps the reference's layout.  Ids are those
 * nxhip_upload_texture returned for kind 3 (normal) and kind 4 (roughness); -1 = none. */
typedef struct nx_material_detail {
    int32_t normalMapId, roughnessMapId;
    float normalScale;  /* glTF normalTexture.scale: multiplies the x and y of the decoded normal */
    uint32_t pad_;
} nx_material_detail;
NX_STATIC_ASSERT(sizeof(nx_material_detail) == 16, "nx_material_detail must be 16 bytes");

/* Extension: how the alpha of one material is read (nxhip_set_material_alpha; the rule is stated in full in include/nexus_hip.h).  A table
 * of these runs index-parallel to the material table, like nx_material_detail: the 60-byte nx_material keeps the reference's layout. */
enum { NX_ALPHA_BLEND = 0, NX_ALPHA_MASK = 1, NX_ALPHA_OPAQUE = 2 };
typedef struct nx_material_alpha {
    uint32_t mode;  /* NX_ALPHA_* */
    float cutoff;   /* NX_ALPHA_MASK: a crossing with opacity x alpha below it does not exist (glTF alphaCutoff, default 0.5) */
} nx_material_alpha;
NX_STATIC_ASSERT(sizeof(nx_material_alpha) == 8, "nx_material_alpha must be 8 bytes");

/* Extension: the skin of one triangle corner (nxhip_set_blas_skin; the blending rule is stated in full in include/nexus_hip.h): up to four
 * joints and their weights, as glTF's JOINTS_0 / WEIGHTS_0 of the corner's vertex.  Corner 3 i + v is vertex v of triangle i. */
typedef struct nx_skin_corner {
    uint16_t joint[4];
    float weight[4];
} nx_skin_corner;
NX_STATIC_ASSERT(sizeof(nx_skin_corner) == 24 && offsetof(nx_skin_corner, weight) == 8, "nx_skin_corner must be 24 bytes");

/* Extension: the deltas of one triangle corner under one morph target (nxhip_set_blas_morph; the rule is stated in full in include/nexus_hip.h):
 * glTF's target POSITION and NORMAL of the corner's vertex (a target without NORMAL: zeros).  Corner 3 i + v is vertex v of triangle i. */
typedef struct nx_morph_corner {
    float dPosition[3];
    float dNormal[3];
} nx_morph_corner;
NX_STATIC_ASSERT(sizeof(nx_morph_corner) == 24 && offsetof(nx_morph_corner, dNormal) == 12, "nx_morph_corner must be 24 bytes");

/* Extension: one homogeneous participating medium ("fog") per context, confined to a world-space axis-aligned box (nxhip_set_medium; the
 * rule is stated in full in include/nexus_hip.h). */
typedef struct nx_medium {
    float boxMin[3]; float sigmaT;   /* extinction per world unit, grey; 0 = no medium                        */
    float boxMax[3]; float g;        /* Henyey-Greenstein asymmetry, forward > 0, |g| <= 0.99                 */
    float albedo[3]; uint32_t pad;   /* single-scattering albedo sigma_s / sigma_t per channel, each in [0, 1] */
} nx_medium;
NX_STATIC_ASSERT(sizeof(nx_medium) == 48, "nx_medium must be 48 bytes");

/* Extension: a procedural sun-and-sky environment (nxhip_set_sky; the model is stated in full in include/nexus_hip.h).  Up is +y;
 * lengths in metres, angles in radians; radiometric RGB, as for the analytic lights. */
typedef struct nx_sky {
    float sunDirection[3];       /* TOWARDS the sun, any non-zero length (normalised on the host in binary64)  */
    float sunAngularRadius;      /* alpha: half-angle of the sun's disc, [0, pi/2)                              */
    float sunIrradiance[3];      /* of a surface facing the sun at the top of the atmosphere                    */
    float altitude;              /* of the observer above the ground, [1, 50000]                                */
    float rayleighScale, mieScale, mieG;  /* multipliers of betaR and betaM (>= 0); Cornette-Shanks g, |g| < 1 */
    float groundAlbedo[3];       /* Lambertian planet below the horizon, each in [0, 1]                         */
    uint32_t width, height;      /* of the generated latitude-longitude map (nxhip_upload_env_float's limits)   */
    uint32_t viewSteps, lightSteps;  /* quadrature segments per view ray / per light ray, each in [1, 1024]    */
    uint32_t sunDisc;            /* 1: the sun's disc is baked into the map; 0: sky and ground only             */
} nx_sky;
NX_STATIC_ASSERT(sizeof(nx_sky) == 76 && offsetof(nx_sky, width) == 56, "nx_sky must be 76 bytes");

typedef struct NX_ALIGN(8) nx_camera {
    float position[3];
    float right[3];
    float up[3];
    float lensRadius;
    float lowerLeftCorner[3];
    float viewportX[3];
    float viewportY[3];
    uint32_t pad_;
    uint32_t resolution[2];
} nx_camera;
NX_STATIC_ASSERT(sizeof(nx_camera) == 88, "nx_camera must be 88 bytes");

typedef struct nx_render_settings {
    uint8_t useMIS;
    uint8_t pathLength;
    uint8_t pad_[2];
    float backgroundColor[3];
    float backgroundIntensity;
} nx_render_settings;
NX_STATIC_ASSERT(sizeof(nx_render_settings) == 20, "nx_render_settings must be 20 bytes");

/* A ray as handed to the batch-trace test hook: origin, direction (not necessarily unit). */
typedef struct nx_ray {
    float origin[3];
    float direction[3];
} nx_ray;

/* Hit record == the reference's D_Intersection (Cuda/Geometry/Ray.cuh:5-15). Miss: hitDistance == 1e30f. */
typedef struct nx_hit {
    float hitDistance;
    float u, v;
    uint32_t triIdx;
    uint32_t instanceIdx;
} nx_hit;

/* RGBA8 image, row 0 first, as uploaded to a reference texture (Assets/Texture.cpp:10-39). */
typedef struct nx_texture_desc {
    uint32_t width, height;
    const uint8_t *rgba8;
} nx_texture_desc;

/* query / result of the BSDF test hooks (nxhip_bsdf_sample_batch, nxhip_bsdf_eval_batch) */
typedef struct nx_bsdf_query {
    float wi[3];
    uint32_t rng;
    float wo[3];
    uint32_t pad_;
} nx_bsdf_query;
typedef struct nx_bsdf_result {
    float wo[3];
    float pdf;
    float throughput[3];
    uint32_t ok;      /* the BSDF's return value (false: sample rejected / invalid pdf) */
    uint32_t rngOut;  /* xorshift state after the call (sample only) */
    uint32_t pad_[3];
} nx_bsdf_result;
NX_STATIC_ASSERT(sizeof(nx_bsdf_query) == 32, "nx_bsdf_query must be 32 bytes");
NX_STATIC_ASSERT(sizeof(nx_bsdf_result) == 48, "nx_bsdf_result must be 48 bytes");


/* Parameters of nxhip_denoise (include/nexus_hip.h): iterations of the a-trous filter (0 .. 6, step 2^i) and the widths of its four
 * edge-stopping terms — colour (halved every iteration), shading normal, albedo + coverage, depth relative to the centre's. */
typedef struct nx_denoise_params {
    uint32_t iterations;
    float sigmaColor, sigmaNormal, sigmaAlbedo, sigmaDepth;
} nx_denoise_params;
NX_STATIC_ASSERT(sizeof(nx_denoise_params) == 20, "nx_denoise_params must be 20 bytes");

/* Parameters of nxhip_set_adaptive (include/nexus_hip.h): a pixel is settled when it has at least minSamples samples and the relative
 * standard error of its mean luminance, sqrt(M2 / (n (n - 1))) / max(meanY, lumFloor), is at most threshold.  cull != 0: blocks of 64
 * paths whose pixels are all settled are no longer rendered; cull == 0: estimate only. */
typedef struct nx_adaptive_params {
    float threshold;
    float lumFloor;
    uint32_t minSamples;
    uint32_t cull;
} nx_adaptive_params;
NX_STATIC_ASSERT(sizeof(nx_adaptive_params) == 16, "nx_adaptive_params must be 16 bytes");

/* How Logic/Shade seed their RNG.  REFERENCE_SLOT mirrors Cuda/Random.cuh:79-82 + PathTracer.cu:143,326
 * (seed by queue slot, no bounce term).  PIXEL_KEYED seeds by (global pixel, bounce, frame): the image
 * then does not depend on queue slot order, so it is reproducible under racing compaction and under a
 * multi-GPU tile split. */
enum { NX_RNG_REFERENCE_SLOT = 0, NX_RNG_PIXEL_KEYED = 1 };

/* Queue compaction: ORDERED reproduces the reference's serial slot order (ascending thread index,
 * material kernels in graph order); FAST uses wave-aggregated atomics. */
enum { NX_COMPACT_FAST = 0, NX_COMPACT_ORDERED = 1 };

/* Conductor handling.  REFERENCE: the reference's ConductorMaterialKernel body is commented out
 * (PathTracer.cu:475-478) so conductor hits end the path.  EXTENDED: shade them (beyond the reference). */
enum { NX_CONDUCTOR_REFERENCE = 0, NX_CONDUCTOR_EXTENDED = 1 };

#define NX_PATH_MAX_LENGTH 100 /* Cuda/PathTracer/PathTracer.cuh:15 */
#define NX_MISS_DISTANCE 1e30f

#endif /* NEXUS_POD_H */
