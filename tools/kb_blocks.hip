// kb_blocks.hip -- A/B of the int16 block forward kernel's store paths
// (csrc/hpdct_blocks.hpp): direct (eight 16-B stores per lane at a 128-B
// stride) against staged (kBlkStaged: the set's 8 KiB through LDS, 1 KiB
// contiguous per store instruction), 256-thread workgroups and one-wave
// workgroups under a residency cap, alternated in one process.  The default
// JPEG table (the per-position quotient forms), zig-zag order.  Rotating buffer
// sets whose inputs total >= 1 GiB, every variant checked byte for byte
// against the first, median of batch averages.  The library launches the
// variant marked "product" (policy::kBlocksFwdVar); the other is reachable
// from here only.
//   kb_blocks [height=8192] [width=8192] [iters=48] [rounds=3]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "hpdct_blocks.hpp"
#include "hpdct_launch.hpp"

using namespace hpdct;

int hpdct::mapping_mode() { return 0; }

#define CK(x)                                                                        \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                      \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(2);                                                                 \
        }                                                                            \
    } while (0)

typedef void (*Fn)(const uint8_t*, int16_t*, const TileGrid&, const QParams&, hipStream_t);

constexpr unsigned kJ = kVarFastDiv | kVarJpegQ;
constexpr unsigned kDirect = kVarNT | kJ, kStaged = kVarNT | kBlkStaged | kJ;

// kThreads-thread workgroups, at most kCap resident per CU (0: no cap)
template <unsigned kBase, uint32_t kThreads, uint32_t kCap>
void run(const uint8_t* in, int16_t* out, const TileGrid& g, const QParams& qp, hipStream_t s) {
    constexpr unsigned kV = with_block<kThreads>(kBase);
    (void)launch_capped<fdct_blocks_kernel<false, kV>>(dim3(policy::wgs_for(policy::tile_waves(g), kThreads)),
                                                       dim3(kThreads), kCap, s, in, out, g, qp);
}

struct V {
    std::string name;
    Fn fn;
    unsigned var;
};

int main(int argc, char** argv) {
    const uint32_t H = argc > 1 ? atoi(argv[1]) : 8192, W = argc > 2 ? atoi(argv[2]) : 8192;
    const int iters = argc > 3 ? atoi(argv[3]) : 48;
    const int rounds = argc > 4 ? atoi(argv[4]) : 3;
    if (H == 0 || W == 0 || H % 8 || W % 8) {
        fprintf(stderr, "height and width must be positive multiples of 8\n");
        return 2;
    }
    const uint64_t n = (uint64_t)H * W;
    const int nsets = std::max<int>(2, (int)(((1ull << 30) + n - 1) / n));
    TileGrid g{(H / 8) * (W / 8), W / 8, W};
    QParams qp;
    for (int i = 0; i < 64; ++i) qp.q.v[i] = tables::kQ[i], qp.r.v[i] = 1.0f / tables::kQ[i];

    std::vector<V> vars = {
        {"direct  b256", run<kDirect, 256, 0>, with_block<256>(kDirect)},
        {"staged  b256", run<kStaged, 256, 0>, with_block<256>(kStaged)},
        {"direct  b64 cap 20 w/cu", run<kDirect, 64, 20>, with_block<64>(kDirect)},
        {"staged  b64 cap 16 w/cu", run<kStaged, 64, 16>, with_block<64>(kStaged)},
        {"direct  b256 again", run<kDirect, 256, 0>, with_block<256>(kDirect)},
        {"staged  b256 again", run<kStaged, 256, 0>, with_block<256>(kStaged)},
    };
    for (auto& v : vars)
        if (v.var == (policy::kBlocksFwdVar | kJ)) v.name += " (product)";

    std::vector<uint8_t*> in(nsets);
    std::vector<int16_t*> out(nsets);
    std::vector<uint8_t> h(n);
    srand(42);
    for (uint64_t i = 0; i < n; ++i) h[i] = (uint8_t)(rand() % 256);
    for (int k = 0; k < nsets; ++k) {
        CK(hipMalloc(&in[k], n));
        CK(hipMalloc(&out[k], n * 2));
        CK(hipMemcpy(in[k], h.data(), n, hipMemcpyHostToDevice));
    }
    // correctness: every variant byte for byte against the first
    std::vector<int16_t> first(n), got(n);
    for (size_t v = 0; v < vars.size(); ++v) {
        CK(hipMemset(out[0], 0xa5, n * 2));
        vars[v].fn(in[0], out[0], g, qp, 0);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(v ? got.data() : first.data(), out[0], n * 2, hipMemcpyDeviceToHost));
        const bool same = v == 0 || memcmp(got.data(), first.data(), n * 2) == 0;
        printf("check %-32s %s\n", vars[v].name.c_str(), same ? "equal" : "MISMATCH");
        if (!same) return 1;
    }
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    // clocks up: 20000 back-to-back launches (most of a second at 8192^2)
    for (int w = 0; w < 20000; ++w) vars[0].fn(in[w % nsets], out[w % nsets], g, qp, 0);
    CK(hipDeviceSynchronize());
    std::vector<std::vector<float>> us(vars.size());
    for (int r = 0; r < rounds; ++r)
        for (size_t v = 0; v < vars.size(); ++v) {
            for (int w = 0; w < nsets; ++w) vars[v].fn(in[w % nsets], out[w % nsets], g, qp, 0);
            for (int i = 0; i < iters; i += nsets) {
                CK(hipEventRecord(a, 0));
                for (int k = 0; k < nsets; ++k) vars[v].fn(in[k], out[k], g, qp, 0);
                CK(hipEventRecord(b, 0));
                CK(hipEventSynchronize(b));
                float ms = 0;
                CK(hipEventElapsedTime(&ms, a, b));
                us[v].push_back(ms * 1e3f / nsets);
            }
        }
    printf("%u x %u, %d sets\n%-32s %10s %10s %10s %8s\n", H, W, nsets, "variant", "median_us", "min_us", "max_us",
           "frac8T");
    for (size_t v = 0; v < vars.size(); ++v) {
        auto t = us[v];
        std::sort(t.begin(), t.end());
        const double med = t[t.size() / 2];
        printf("%-32s %10.2f %10.2f %10.2f %8.3f\n", vars[v].name.c_str(), med, t[0], t.back(),
               3.0 * n / (med * 1e-6) / 8e12);
    }
    return 0;
}
