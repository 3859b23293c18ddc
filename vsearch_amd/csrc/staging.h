// staging.h -- the pointer convention of the small list kernels (vs_topk_collapse, vs_group_filter, vs_mmr_select_csr): the buffers of a call are
// all host pointers (staged on the device, copied back, the call blocks) or all device pointers on the call's device (only enqueued).
#pragma once
#include "common.h"
#include "new_index.h"

#include <algorithm>

namespace vs {

inline int device_ok(const void* p, int device, const char* what) {
    hipPointerAttribute_t attr;
    VS_HIP(hipPointerGetAttributes(&attr, p));
    if (attr.device != device) return fail(VS_EINVAL, "%s lives on device %d, the call runs on device %d", what, attr.device, device);
    return VS_OK;
}

// the buffers of a call are all host or all device pointers (NULL ones aside) -> *dev; device ones must live on `device`
inline int pointers_kind(const void* const* ptrs, const char* const* names, int n, int device, bool* dev) {
    const void* first = nullptr;
    for (int i = 0; i < n && !first; ++i) first = ptrs[i];
    *dev = is_device_ptr(first);
    for (int i = 0; i < n; ++i) {
        if (!ptrs[i]) continue;
        if (is_device_ptr(ptrs[i]) != *dev) return fail(VS_EINVAL, "%s: the buffers of a call must all be host or all be device pointers", names[i]);
        if (*dev) VS_TRY(device_ok(ptrs[i], device, names[i]));
    }
    return VS_OK;
}

// a host buffer's copy on the device (the pointer itself for a device buffer)
struct Staged {
    DevBuf buf;
    void* host = nullptr;
    size_t bytes = 0;
    template <class T>
    int in(const T* src, size_t n, bool dev, bool copy, hipStream_t s, T** out) {
        *out = const_cast<T*>(src);
        if (dev || !src) return VS_OK;
        bytes = n * sizeof(T);
        host = const_cast<T*>(src);
        VS_TRY(buf.alloc(std::max<size_t>(bytes, 4)));
        if (copy && bytes) VS_HIP(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, s));
        *out = buf.as<T>();
        return VS_OK;
    }
    int back(hipStream_t s) {
        if (host && bytes) VS_HIP(hipMemcpyAsync(host, buf.p, bytes, hipMemcpyDeviceToHost, s));
        return VS_OK;
    }
};

}  // namespace vs
