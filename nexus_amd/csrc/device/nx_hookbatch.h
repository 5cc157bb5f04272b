// nx_hookbatch.h — the columnar test hooks' plumbing (nxhip_hooks.hip, nxhip_features.hip): `count` items as flat host arrays in, one
// wide kernel over them, flat host arrays out.  A hook states each column once — element type and elements per item — and calls run.
#pragma once

#include <vector>

#include "nx_host.h"

namespace nxd {

struct HookBatch {
    nxhip_ctx* c;
    size_t count;
    int rc = NXHIP_OK;  // the first column that failed (its error string is set); run returns it before anything is launched
    struct Out { void* host; const void* dev; size_t bytes; };
    std::vector<DevBuf> bufs;  // freed with the batch, on every path
    std::vector<Out> outs;     // what run copies back, in the order stated
    HookBatch(nxhip_ctx* ctx, uint32_t n) : c(ctx), count(n) {}

    // `width` elements per item, copied in (synchronously); host == nullptr: no column, a null device pointer
    template <class T> T* in(const T* host, size_t width)
    {
        T* d = column(host, width);
        if (d && !hip_ok(hipMemcpy(d, host, count * width * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy(column in)", __FILE__, __LINE__)) rc = NXHIP_ERR_HIP;
        return rc == NXHIP_OK ? d : nullptr;
    }
    // `width` elements per item, copied back to `host` by run; host == nullptr: no column, a null device pointer
    template <class T> T* out(T* host, size_t width)
    {
        T* d = column(host, width);
        if (d) outs.push_back({host, d, count * width * sizeof(T)});
        return d;
    }
    // the kernel over c->wideBlocks x kWideBlock on the context's stream, the wait, the outputs (typed as launch_untimed is)
    template <class... A> int run(Kernel<A...> k, std::common_type_t<A>... args)
    {
        NX_TRY(rc);
        NX_HIP(launch_untimed(k, c->wideBlocks, kWideBlock, c->stream, args...));
        NX_SYNC_ALL(c);
        for (const Out& o : outs) NX_HIP(hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
        return NXHIP_OK;
    }

private:
    template <class T> T* column(const T* host, size_t width)
    {
        if (!host || rc != NXHIP_OK) return nullptr;
        bufs.emplace_back();
        if (!bufs.back().alloc(count * width * sizeof(T))) rc = NXHIP_ERR_HIP;  // (DevBuf::alloc has set the error string)
        return rc == NXHIP_OK ? bufs.back().template as<T>() : nullptr;
    }
};

// ---- the hooks' argument checks ------------------------------------------------------------------------
// (written so that a NaN fails; +-inf is not finite)
inline bool all_finite(const float* x, size_t n)
{
    for (size_t k = 0; k < n; k++)
        if (!(x[k] >= -3.0e38f && x[k] <= 3.0e38f)) return false;
    return true;
}
inline bool all_unit(const float* x, size_t n)  // every x in [0, 1)
{
    for (size_t k = 0; k < n; k++)
        if (!(x[k] >= 0.0f && x[k] < 1.0f)) return false;
    return true;
}

}  // namespace nxd
