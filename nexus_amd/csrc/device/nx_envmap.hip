// nx_envmap.hip — the sampler tables of a FLOAT environment map (nxhip_upload_env_float), built on the device.
//
// The tables have the layout and meaning of the 8-bit map's (nxhip_scene.hip build_env_tables: marginal cdf over rows, conditional cdf
// per row, density = pdf per solid angle x cos(latitude), cut-point guides), so env_invert / env_pdf / cdf_find read either.  What differs
// is the texel weight.  The lookup is bilinear (nx_texture.h tex2d_float): a bright texel bleeds half a texel into its neighbours, and
// with "luminance of the texel's own value" as weight the neighbours' pdf knows nothing of it — value / pdf is then bounded by
// sun / sky, 10^6 for a float sun instead of the 8-bit maps' 255, a heavy tail no frame count meets.  So the weight is the integral of
// the FILTERED luminance over the texel's footprint, which for bilinear filtering is the 3 x 3 kernel k = (1/8, 3/4, 1/8) per axis:
//   Lf(x, y) = sum over dy, dx in {-1, 0, 1} of k[dy] k[dx] lum(x + dx, y + dy)      (neighbours wrap on both axes, as the lookup's do)
//   weight(x, y) = Lf(x, y) x sin(pi (y + 1/2) / H) + 1e-6                           (lum = 0.2126 R + 0.7152 G + 0.0722 B, linear)
// All of it in binary64:
//   env_row_kernel<false>   one workgroup per row: the row's inclusive scan of the weights, chunk after chunk of kEnvBlock texels with
//                           the running sum carried from chunk to chunk; only the row's sum is kept
//   env_marginal_kernel     one workgroup: the scan over the row sums, the marginal cdf (binary32, rounded once, last entry exactly 1)
//                           and its guide
//   env_row_kernel<true>    the same scan again — the same additions in the same order, so the same sums — now that the row's sum and
//                           the total are known: row cdf = binary32(prefix / row sum), last entry exactly 1; density =
//                           binary32(weight / total x W x H / (2 pi^2)); then the row's guide
// Scanning twice instead of keeping W x H binary64 prefixes: a 2^27-texel map would need a gigabyte of scratch for them.
// Nothing comes back to the host during a build.
//
// What this shape is slow for: one workgroup walks a whole row chunk by chunk, so the build has H workgroups and W / 256 serial steps
// each, and every weight is computed twice (nine 16-byte loads each time, most of them cache hits).  Latitude-longitude maps have
// W = 2 H and fill the device (4096 x 2048: 2048 workgroups, 16 steps, 0.17 ms — profiles/r15_env_float.txt).  A map that is wide and
// flat, which nxhip_upload_env_float accepts — 32768 x 2 — runs on two workgroups of 128 steps; it is still correct, and a scan that
// splits a row over workgroups (a carry through memory) is what such a shape would need.
#include "nx_host.h"
#include "nx_texture.h"

namespace nxd {

namespace {

constexpr int kEnvBlock = 256;

__device__ __forceinline__ double env_lum(const float4 t) { return (0.2126 * (double)t.x + 0.7152 * (double)t.y) + 0.0722 * (double)t.z; }

__device__ double env_weight(const float4* __restrict__ texels, const int W, const int H, const int x, const int y, const double sinTheta)
{
    const double k[3] = {0.125, 0.75, 0.125};
    double Lf = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const size_t row = (size_t)wrapi(y + dy, H) * (size_t)W;
        double acc = 0.0;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) acc += k[dx + 1] * env_lum(texels[row + (size_t)wrapi(x + dx, W)]);
        Lf += k[dy + 1] * acc;
    }
    return Lf * sinTheta + 1e-6;
}

// Inclusive scan of one value per thread over the workgroup (Hillis-Steele through LDS: a fixed order of additions).  Every thread of
// the workgroup calls it; s is [2][kEnvBlock].  The caller synchronises before the next call (s[0] is read last and written first).
__device__ double block_scan(double v, double (*s)[kEnvBlock])
{
    const int t = (int)threadIdx.x;
    int cur = 0;
    s[0][t] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < kEnvBlock; off <<= 1) {
        double x = s[cur][t];
        if (t >= off) x += s[cur][t - off];
        s[cur ^ 1][t] = x;
        cur ^= 1;
        __syncthreads();
    }
    return s[cur][t];  // (cur == 0: eight steps)
}

// first index of cdf[0 .. n - 1] whose value exceeds bound, n - 1 when none does (the host's make_guide rule)
__device__ uint32_t first_above(const float* cdf, const uint32_t n, const float bound)
{
    uint32_t lo = 0, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (cdf[mid] > bound) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

template <bool kWrite>
__global__ void __launch_bounds__(kEnvBlock) env_row_kernel(const float4* __restrict__ texels, const uint32_t W, const uint32_t H, double* rowSum, const double* marginalPrefix,
                                                            float* rowCdf, float* __restrict__ density, uint32_t* __restrict__ rowGuide)
{
    __shared__ double s[2][kEnvBlock];
    const double pi = 3.14159265358979323846;
    const uint32_t y = blockIdx.x;  // (grid = H)
    const double sinTheta = sin(pi * ((double)y + 0.5) / (double)H);
    const double sum = kWrite ? rowSum[y] : 0.0, total = kWrite ? marginalPrefix[H - 1u] : 0.0;
    double carry = 0.0;
    for (uint32_t base = 0; base < W; base += kEnvBlock) {
        const uint32_t x = base + threadIdx.x;
        const double w = x < W ? env_weight(texels, (int)W, (int)H, (int)x, (int)y, sinTheta) : 0.0;
        const double prefix = carry + block_scan(w, s);
        carry += s[0][kEnvBlock - 1];
        if (kWrite && x < W) {
            const size_t i = (size_t)y * W + x;
            rowCdf[i] = x == W - 1u ? 1.0f : (float)(prefix / sum);
            density[i] = (float)(w / total * (double)W * (double)H / (2.0 * pi * pi));
        }
        __syncthreads();
    }
    if (!kWrite) {
        if (threadIdx.x == 0) rowSum[y] = carry;
        return;
    }
    // the row's cdf is complete (this workgroup wrote all of it; the barrier above orders the stores): its guide
    __threadfence_block();
    if (threadIdx.x <= (unsigned)kEnvGuide)
        rowGuide[(size_t)y * (size_t)(kEnvGuide + 1) + threadIdx.x] = first_above(rowCdf + (size_t)y * W, W, (float)threadIdx.x / (float)kEnvGuide);
}

__global__ void __launch_bounds__(kEnvBlock) env_marginal_kernel(const double* __restrict__ rowSum, const uint32_t H, double* marginalPrefix, float* marginalCdf,
                                                                 uint32_t* __restrict__ marginalGuide)
{
    __shared__ double s[2][kEnvBlock];
    double carry = 0.0;
    for (uint32_t base = 0; base < H; base += kEnvBlock) {
        const uint32_t y = base + threadIdx.x;
        const double prefix = carry + block_scan(y < H ? rowSum[y] : 0.0, s);
        carry += s[0][kEnvBlock - 1];
        if (y < H) marginalPrefix[y] = prefix;
        __syncthreads();
    }
    const double total = carry;  // (every thread holds the same: positive, the floor alone makes it so)
    for (uint32_t y = threadIdx.x; y < H; y += kEnvBlock) marginalCdf[y] = y == H - 1u ? 1.0f : (float)(marginalPrefix[y] / total);  // (its own stores)
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x <= (unsigned)kEnvGuide) marginalGuide[threadIdx.x] = first_above(marginalCdf, H, (float)threadIdx.x / (float)kEnvGuide);
}

}  // namespace

// temp: 2 x height doubles (row sums, their prefix sums); width, height >= 1
int env_float_tables_build(hipStream_t st, const float4* texels, uint32_t width, uint32_t height, double* temp, float* marginalCdf, float* rowCdf, float* density,
                           uint32_t* marginalGuide, uint32_t* rowGuide)
{
    double* rowSum = temp;
    double* marginalPrefix = temp + height;
    env_row_kernel<false><<<height, kEnvBlock, 0, st>>>(texels, width, height, rowSum, nullptr, nullptr, nullptr, nullptr);
    NX_HIP(hipGetLastError());
    env_marginal_kernel<<<1, kEnvBlock, 0, st>>>(rowSum, height, marginalPrefix, marginalCdf, marginalGuide);
    NX_HIP(hipGetLastError());
    env_row_kernel<true><<<height, kEnvBlock, 0, st>>>(texels, width, height, rowSum, marginalPrefix, rowCdf, density, rowGuide);
    NX_HIP(hipGetLastError());
    return NXHIP_OK;
}

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_envmap() { return layout_stamp(); }

}  // namespace nxd
