// pose_bench_kernel.hip — the route a caller had BEFORE nxhip_pose_blas, for tools/pose_bench.py to time against it: a minimal
// stand-alone skinning kernel that writes 96-byte triangle records into a buffer of the caller's, which then go through
// nxhip_update_blas_device (a device copy, the strided shading copy, the intersection-stream pass and the node refit).
// One lane per triangle in id order — the coalesced walk, which this route is free to take because it writes no leaf-ordered
// stream —, the blending rule of include/nexus_hip.h in the fused kernel's operation order, the palette read from global memory.
// Not part of the library: tools/pose_bench.py compiles it into a small shared object of its own.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

struct Tri {
    float v[24];  // nx_triangle: pos0 pos1 pos2 normal0 normal1 normal2 texCoord0..2
};
struct Skin {  // the library's SkinTri: weights of corner v in chunk v, the twelve joint indices behind them
    float weight[3][4];
    uint16_t joint[3][4];
    uint32_t pad[2];
};
static_assert(sizeof(Tri) == 96 && sizeof(Skin) == 80, "record layouts");

__global__ void __launch_bounds__(256) skin_kernel(const Tri* __restrict__ bind, const Skin* __restrict__ skin, const float4* __restrict__ palette, const uint32_t n, Tri* __restrict__ out)
{
    for (uint32_t id = blockIdx.x * blockDim.x + threadIdx.x; id < n; id += gridDim.x * blockDim.x) {
        Tri t = bind[id];
        const Skin s = skin[id];
        for (int c = 0; c < 3; c++) {
            float m[3][4];
            for (int r = 0; r < 3; r++) {
                const float4 a = palette[3u * s.joint[c][0] + r], b = palette[3u * s.joint[c][1] + r], d = palette[3u * s.joint[c][2] + r], e = palette[3u * s.joint[c][3] + r];
                const float w0 = s.weight[c][0], w1 = s.weight[c][1], w2 = s.weight[c][2], w3 = s.weight[c][3];
                m[r][0] = ((w0 * a.x + w1 * b.x) + w2 * d.x) + w3 * e.x;
                m[r][1] = ((w0 * a.y + w1 * b.y) + w2 * d.y) + w3 * e.y;
                m[r][2] = ((w0 * a.z + w1 * b.z) + w2 * d.z) + w3 * e.z;
                m[r][3] = ((w0 * a.w + w1 * b.w) + w2 * d.w) + w3 * e.w;
            }
            float* p = t.v + 3 * c;
            float* nr = t.v + 9 + 3 * c;
            const float q[3] = {p[0], p[1], p[2]};
            for (int r = 0; r < 3; r++) p[r] = m[r][0] * q[0] + m[r][1] * q[1] + m[r][2] * q[2] + m[r][3];
            if (nr[0] == 0.0f && nr[1] == 0.0f && nr[2] == 0.0f) continue;
            const float k[3][3] = {
                {m[1][1] * m[2][2] - m[1][2] * m[2][1], m[1][2] * m[2][0] - m[1][0] * m[2][2], m[1][0] * m[2][1] - m[1][1] * m[2][0]},
                {m[0][2] * m[2][1] - m[0][1] * m[2][2], m[0][0] * m[2][2] - m[0][2] * m[2][0], m[0][1] * m[2][0] - m[0][0] * m[2][1]},
                {m[0][1] * m[1][2] - m[0][2] * m[1][1], m[0][2] * m[1][0] - m[0][0] * m[1][2], m[0][0] * m[1][1] - m[0][1] * m[1][0]}};
            const float det = m[0][0] * k[0][0] + m[0][1] * k[0][1] + m[0][2] * k[0][2];
            float v[3];
            for (int r = 0; r < 3; r++) {
                v[r] = k[r][0] * nr[0] + k[r][1] * nr[1] + k[r][2] * nr[2];
                if (det < 0.0f) v[r] = -v[r];
            }
            const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            const bool ok = len > 0.0f && len < __uint_as_float(0x7f800000u);
            for (int r = 0; r < 3; r++) nr[r] = ok ? v[r] / len : 0.0f;
        }
        out[id] = t;
    }
}

}  // namespace

// launches on `stream`; returns the HIP status of the launch
extern "C" int pose_bench_skin(void* stream, const void* bind, const void* skin, const void* palette, uint32_t n, void* out, int grid)
{
    skin_kernel<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(static_cast<const Tri*>(bind), static_cast<const Skin*>(skin), static_cast<const float4*>(palette), n, static_cast<Tri*>(out));
    return static_cast<int>(hipGetLastError());
}
