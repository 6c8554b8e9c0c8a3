// hpdct_fill_hash.hpp -- hpdct_fill_hash_u8's kernel: one library unit (hpdct_fwd_u8.hip) and tools.
#pragma once

#include "hpdct_kernels_impl.hpp"

namespace hpdct {

// Synthetic frame generator (config C4): 16 pixels per lane.
__device__ __forceinline__ uint32_t hash_px(uint64_t seed, uint64_t idx) {
    uint64_t z = seed + (idx + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<uint32_t>((z ^ (z >> 31)) & 255u);
}

[[maybe_unused]] static __global__ __launch_bounds__(kBlockThreads) void fill_hash_kernel(uint8_t* __restrict__ out, uint64_t n,
                                                                         uint64_t seed, uint64_t first) {
    const uint64_t i0 = (static_cast<uint64_t>(blockIdx.x) * kBlockThreads + threadIdx.x) * 16u;
    if (i0 >= n) return;
    if (i0 + 16 <= n) {
        uint32_t w[4];
        unroll<4>([&](auto k) {
            uint32_t acc = 0;
            unroll<4>([&](auto b) { acc |= hash_px(seed, first + i0 + k * 4 + b) << (8 * b); });
            w[k] = acc;
        });
        *reinterpret_cast<uint4*>(out + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (uint64_t i = i0; i < n; ++i) out[i] = static_cast<uint8_t>(hash_px(seed, first + i));
    }
}

inline hipError_t launch_fill_hash_impl(uint8_t* out, uint64_t n, uint64_t seed, uint64_t first, hipStream_t s) {
    const uint64_t lanes = (n + 15) / 16;
    const dim3 grid(static_cast<uint32_t>((lanes + kBlockThreads - 1) / kBlockThreads));
    hipLaunchKernelGGL(fill_hash_kernel, grid, dim3(kBlockThreads), 0, s, out, n, seed, first);
    return hipGetLastError();
}

}  // namespace hpdct
