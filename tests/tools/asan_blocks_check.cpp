// asan_blocks_check.cpp -- drives the validation paths of hpdct_forward_blocks /
// hpdct_inverse_blocks and hpdct_zigzag_order under ASan + UBSan, CPU only: a
// stand-alone program linked with the sanitised host sources of the C ABI (g++; asan.mk's HOST) and the
// library's kernel objects, as tests/tools/asan.mk links asan_host_check.  No
// kernel is launched: every call here fails its checks (or touches host
// memory only).  Built and run by tests/test_blocks_host.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "hpdct.h"

namespace {
int g_bad = 0;
void expect(const char* what, int got, int want, const char* text = nullptr) {
    const bool ok = got == want && (!text || std::strstr(hpdct_last_error_string(), text));
    if (!ok) {
        ++g_bad;
        std::printf("MISMATCH %s: status %d (expected %d), last error \"%s\"\n", what, got, want,
                    hpdct_last_error_string());
    }
}
}  // namespace

int main() {
    // never dereferenced: validation fails first
    const auto A = reinterpret_cast<uint8_t*>(uintptr_t(1) << 20);
    const auto B = reinterpret_cast<int16_t*>(uintptr_t(1) << 30);
    auto at = [](auto* p, intptr_t bytes) {
        return reinterpret_cast<decltype(p)>(reinterpret_cast<uintptr_t>(p) + bytes);
    };
    expect("fwd null image", hpdct_forward_blocks(nullptr, B, 8, 8, 0, nullptr), 1);
    expect("fwd null blocks", hpdct_forward_blocks(A, nullptr, 8, 8, 0, nullptr), 1);
    expect("fwd 12x8", hpdct_forward_blocks(A, B, 12, 8, 0, nullptr), 1, "multiples of 8");
    expect("fwd 8x20", hpdct_forward_blocks(A, B, 8, 20, 0, nullptr), 1, "multiples of 8");
    expect("fwd huge", hpdct_forward_blocks(A, B, int64_t(1) << 23, int64_t(1) << 23, 0, nullptr), 1, "too large");
    expect("fwd blocks + 8", hpdct_forward_blocks(A, at(B, 8), 8, 8, 0, nullptr), 1, "aligned");
    expect("fwd overlap", hpdct_forward_blocks(A, reinterpret_cast<int16_t*>(at(A, 32)), 8, 8, 0, nullptr), 1,
           "overlap");
    expect("fwd flag 0x80", hpdct_forward_blocks(A, B, 8, 8, 0x80u, nullptr), 2);
    expect("inv null", hpdct_inverse_blocks(nullptr, A, HPDCT_U8, 8, 8, 0, nullptr), 1);
    expect("inv 8x20", hpdct_inverse_blocks(B, A, HPDCT_F32, 8, 20, 0, nullptr), 1, "multiples of 8");
    expect("inv I8 out", hpdct_inverse_blocks(B, A, HPDCT_I8, 8, 8, 0, nullptr), 2);
    expect("inv fp32 pixels + 8", hpdct_inverse_blocks(B, at(A, 8), HPDCT_F32, 8, 8, 0, nullptr), 1, "aligned");
    expect("inv overlap", hpdct_inverse_blocks(B, at(reinterpret_cast<uint8_t*>(B), 64), HPDCT_U8, 8, 8, 0, nullptr), 1,
           "overlap");
    expect("inv flag 0x80", hpdct_inverse_blocks(B, A, HPDCT_U8, 8, 8, HPDCT_BLOCKS_NATURAL | 0x80u, nullptr), 2);
    // the shared overlap check, 8x8: 64 bytes of uint8 pixels (8-byte units), 128 of blocks (16-byte units).
    // The later buffer starts one unit before the earlier one's end, either way round; TOP's extent would wrap.
    const auto A16 = reinterpret_cast<int16_t*>(A);
    const auto B8 = reinterpret_cast<uint8_t*>(B);
    const uintptr_t top = (~uintptr_t(0) - 50) & ~uintptr_t(15);
    expect("fwd blocks at image end - 16", hpdct_forward_blocks(A, at(A16, 48), 8, 8, 0, nullptr), 1, "overlap");
    expect("fwd image at blocks end - 8", hpdct_forward_blocks(at(B8, 120), B, 8, 8, 0, nullptr), 1, "overlap");
    expect("fwd image wraps", hpdct_forward_blocks(reinterpret_cast<uint8_t*>(top), B, 8, 8, 0, nullptr), 1, "wrap");
    expect("fwd blocks wrap", hpdct_forward_blocks(A, reinterpret_cast<int16_t*>(top), 8, 8, 0, nullptr), 1, "wrap");
    expect("inv pixels at blocks end - 8", hpdct_inverse_blocks(B, at(B8, 120), HPDCT_U8, 8, 8, 0, nullptr), 1,
           "overlap");
    expect("inv blocks at pixels end - 16", hpdct_inverse_blocks(at(A16, 48), A, HPDCT_U8, 8, 8, 0, nullptr), 1,
           "overlap");
    expect("inv pixels wrap", hpdct_inverse_blocks(B, reinterpret_cast<uint8_t*>(top), HPDCT_F32, 8, 8, 0, nullptr), 1,
           "wrap");

    // the range rule: 1/64 everywhere can give |q| = 65536
    float q[64];
    for (float& v : q) v = 1.0f / 64.0f;
    expect("set 1/64 table", hpdct_set_quant_table(q), 0);
    expect("fwd range", hpdct_forward_blocks(A, B, 8, 8, 0, nullptr), 3, "int16");
    // blocks right behind the image (and the image right behind the blocks) are no overlap: under a table of
    // 0.001 the call gets as far as the range rule
    for (float& v : q) v = 0.001f;
    expect("set 0.001 table", hpdct_set_quant_table(q), 0);
    expect("fwd blocks at image end", hpdct_forward_blocks(A, at(A16, 64), 8, 8, 0, nullptr), 3, "int16");
    expect("fwd image at blocks end", hpdct_forward_blocks(at(B8, 128), B, 8, 8, 0, nullptr), 3, "int16");
    expect("restore table", hpdct_set_quant_table(nullptr), 0);
    // a huge finite table is legal (the inverses take their full-chain kernels under it): the skip criterion
    // is computed when the table is set, and a call is still judged by its arguments first
    for (float& v : q) v = 2e34f;
    q[5] = -3.0e38f;
    expect("set huge table", hpdct_set_quant_table(q), 0);
    expect("inv null under the huge table", hpdct_inverse_blocks(nullptr, A, HPDCT_U8, 8, 8, 0, nullptr), 1);
    expect("inv 8x20 under the huge table", hpdct_inverse_blocks(B, A, HPDCT_F32, 8, 20, 0, nullptr), 1,
           "multiples of 8");
    expect("restore table", hpdct_set_quant_table(nullptr), 0);

    // exactly 64 bytes on the heap: a write past them is an ASan report
    std::unique_ptr<uint8_t[]> z(new uint8_t[64]);
    hpdct_zigzag_order(z.get());
    hpdct_zigzag_order(nullptr);
    bool seen[64] = {};
    for (int n = 0; n < 64; ++n) {
        if (z[n] >= 64 || seen[z[n]]) ++g_bad;
        else seen[z[n]] = true;
    }
    if (z[0] != 0 || z[1] != 1 || z[2] != 8 || z[63] != 63) ++g_bad;

    if (g_bad != 0) {
        std::printf("asan_blocks_check: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("asan_blocks_check: ok\n");
    return 0;
}
