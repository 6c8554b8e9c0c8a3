// hpdct_residency.hpp -- residency caps by dynamic-LDS reservation (round 3):
// the device attributes the caps read and the reservation that leaves room for
// at most k workgroups per CU, and the one launch helper every launcher uses.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace hpdct {

// The cap is set by reserving dynamic LDS the kernel does not use: a
// workgroup that holds more than 1/(k+1) of the CU's LDS leaves room for at
// most k.  The LDS size is the device's own
// (hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, 160 KiB on gfx950 per
// MI355X_MICROARCH.md), so the caps keep their meaning on a part with another
// LDS size.
constexpr size_t kLdsPerCUDefault = 160u * 1024u;

// A device attribute of the current device, cached per thread and device.
template <hipDeviceAttribute_t kAttr>
inline int device_attr(int fallback) {
    static thread_local int cached_dev = -1;
    static thread_local int cached = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fallback;
    if (dev != cached_dev) {
        int v = 0;
        cached = hipDeviceGetAttribute(&v, kAttr, dev) == hipSuccess && v > 0 ? v : fallback;
        cached_dev = dev;
    }
    return cached;
}
inline uint32_t device_cus() {
    return static_cast<uint32_t>(device_attr<hipDeviceAttributeMultiprocessorCount>(256));
}
inline size_t device_lds_per_cu() {
    return static_cast<size_t>(
        device_attr<hipDeviceAttributeMaxSharedMemoryPerMultiprocessor>(static_cast<int>(kLdsPerCUDefault)));
}

// dynamic LDS bytes for at most `wgs` resident workgroups per CU of a kernel
// that has `static_bytes` of its own (0 when no reservation is needed)
inline size_t residency_cap_lds(size_t static_bytes, uint32_t wgs) {
    if (wgs == 0) return 0;
    const size_t per = (device_lds_per_cu() / wgs) & ~static_cast<size_t>(511);
    return per > static_bytes ? per - static_bytes : 0;
}

// Every launch of the library: kKern on (grid, block) with at most cap_wgs
// resident workgroups per CU (0: the hardware's default, no reservation).  The
// kernel's static LDS is queried once per kernel and process.
template <auto kKern, typename... Args>
hipError_t launch_capped(dim3 grid, dim3 block, uint32_t cap_wgs, hipStream_t s, const Args&... args) {
    size_t dyn = 0;
    if (cap_wgs != 0) {
        static const size_t st = [] {
            hipFuncAttributes a{};
            const auto* k = reinterpret_cast<const void*>(kKern);
            return hipFuncGetAttributes(&a, k) == hipSuccess ? a.sharedSizeBytes : size_t(0);
        }();
        dyn = residency_cap_lds(st, cap_wgs);
    }
    hipLaunchKernelGGL(kKern, grid, block, dyn, s, args...);
    return hipGetLastError();
}

}  // namespace hpdct
