// asan_rgb_check.cpp -- drives the validation paths of hpdct_forward_rgb_blocks /
// hpdct_inverse_rgb_blocks and hpdct_default_chroma_quant_table under ASan +
// UBSan, CPU only: a stand-alone program linked with the sanitised
// the C ABI's host sources (g++; asan.mk's HOST) and the library's kernel objects, as asan_blocks_check.cpp
// is.  No kernel is launched: every call here fails its checks (or touches host
// memory only).  Built and run by tests/test_rgb_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
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
    // never dereferenced: validation fails first.  Far apart, 16-byte aligned.
    const auto RGB = reinterpret_cast<uint8_t*>(uintptr_t(1) << 20);
    const auto Y = reinterpret_cast<int16_t*>(uintptr_t(1) << 30);
    const auto CB = reinterpret_cast<int16_t*>(uintptr_t(1) << 31);
    const auto CR = reinterpret_cast<int16_t*>(uintptr_t(1) << 32);
    auto at = [](auto* p, intptr_t bytes) {
        return reinterpret_cast<decltype(p)>(reinterpret_cast<uintptr_t>(p) + bytes);
    };
    const auto S444 = HPDCT_SUBSAMPLING_444, S420 = HPDCT_SUBSAMPLING_420;
    auto fwd = [&](const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, int64_t h, int64_t w, int sub,
                   const float* ql, const float* qc, unsigned flags) {
        return hpdct_forward_rgb_blocks(rgb, y, cb, cr, h, w, static_cast<hpdct_subsampling>(sub), ql, qc, flags,
                                        nullptr);
    };
    auto inv = [&](const int16_t* y, const int16_t* cb, const int16_t* cr, uint8_t* rgb, int64_t h, int64_t w, int sub,
                   const float* ql, const float* qc, unsigned flags) {
        return hpdct_inverse_rgb_blocks(y, cb, cr, rgb, h, w, static_cast<hpdct_subsampling>(sub), ql, qc, flags,
                                        nullptr);
    };
    expect("fwd null rgb", fwd(nullptr, Y, CB, CR, 16, 16, S420, nullptr, nullptr, 0), 1, "null");
    expect("fwd null y", fwd(RGB, nullptr, CB, CR, 16, 16, S420, nullptr, nullptr, 0), 1, "null");
    expect("fwd null cb", fwd(RGB, Y, nullptr, CR, 16, 16, S420, nullptr, nullptr, 0), 1, "null");
    expect("fwd null cr", fwd(RGB, Y, CB, nullptr, 16, 16, S420, nullptr, nullptr, 0), 1, "null");
    expect("fwd 8x8 420", fwd(RGB, Y, CB, CR, 8, 8, S420, nullptr, nullptr, 0), 1, "multiples of 16");
    expect("fwd 16x24 420", fwd(RGB, Y, CB, CR, 16, 24, S420, nullptr, nullptr, 0), 1, "multiples of 16");
    expect("fwd 12x8 444", fwd(RGB, Y, CB, CR, 12, 8, S444, nullptr, nullptr, 0), 1, "multiples of 8");
    expect("fwd 0x16", fwd(RGB, Y, CB, CR, 0, 16, S420, nullptr, nullptr, 0), 1, "multiples of 16");
    expect("fwd huge", fwd(RGB, Y, CB, CR, int64_t(1) << 23, int64_t(1) << 23, S444, nullptr, nullptr, 0), 1,
           "too large");
    expect("fwd enum 2", fwd(RGB, Y, CB, CR, 16, 16, 2, nullptr, nullptr, 0), 1, "subsampling");
    expect("fwd enum -1", fwd(RGB, Y, CB, CR, 16, 16, -1, nullptr, nullptr, 0), 1, "subsampling");
    expect("fwd flag 0x80", fwd(RGB, Y, CB, CR, 16, 16, S420, nullptr, nullptr, 0x80u), 2);
    expect("fwd rgb + 8", fwd(at(RGB, 8), Y, CB, CR, 16, 16, S420, nullptr, nullptr, 0), 1, "aligned");
    expect("fwd cr + 8", fwd(RGB, Y, CB, at(CR, 8), 16, 16, S420, nullptr, nullptr, 0), 1, "aligned");
    // 16x16: rgb 768 bytes, y 512, cb and cr 128 (4:2:0) or 512 (4:4:4)
    expect("fwd y in rgb", fwd(RGB, reinterpret_cast<int16_t*>(at(RGB, 752)), CB, CR, 16, 16, S420, nullptr, nullptr, 0),
           1, "overlap");
    expect("fwd cb = cr", fwd(RGB, Y, CB, CB, 16, 16, S420, nullptr, nullptr, 0), 1, "overlap");
    expect("fwd cr in cb 444", fwd(RGB, Y, CB, at(CB, 128), 16, 16, S444, nullptr, nullptr, 0), 1, "overlap");
    expect("fwd cb in y", fwd(RGB, Y, at(Y, 496), CR, 16, 16, S420, nullptr, nullptr, 0), 1, "overlap");
    // the other way round: rgb starts one 16-byte unit before y's end; and a buffer whose extent would wrap
    const uintptr_t top = (~uintptr_t(0) - 50) & ~uintptr_t(15);
    expect("fwd rgb in y", fwd(at(reinterpret_cast<uint8_t*>(Y), 496), Y, CB, CR, 16, 16, S420, nullptr, nullptr, 0), 1,
           "overlap");
    expect("fwd rgb wraps", fwd(reinterpret_cast<uint8_t*>(top), Y, CB, CR, 16, 16, S420, nullptr, nullptr, 0), 1,
           "wrap");
    expect("fwd cr wraps", fwd(RGB, Y, CB, reinterpret_cast<int16_t*>(top), 16, 16, S420, nullptr, nullptr, 0), 1,
           "wrap");
    expect("inv null", inv(Y, CB, CR, nullptr, 16, 16, S420, nullptr, nullptr, 0), 1, "null");
    expect("inv 8x8 420", inv(Y, CB, CR, RGB, 8, 8, S420, nullptr, nullptr, 0), 1, "multiples of 16");
    expect("inv enum 7", inv(Y, CB, CR, RGB, 16, 16, 7, nullptr, nullptr, 0), 1, "subsampling");
    expect("inv flag", inv(Y, CB, CR, RGB, 16, 16, S444, nullptr, nullptr, HPDCT_BLOCKS_NATURAL | 0x2u), 2);
    expect("inv y + 2", inv(at(Y, 2), CB, CR, RGB, 16, 16, S444, nullptr, nullptr, 0), 1, "aligned");
    expect("inv rgb in y", inv(Y, CB, CR, at(reinterpret_cast<uint8_t*>(Y), 256), 16, 16, S444, nullptr, nullptr, 0), 1,
           "overlap");

    // tables: exactly 64 floats on the heap, so a read past them is an ASan report
    std::unique_ptr<float[]> good(new float[64]), bad(new float[64]);
    hpdct_default_chroma_quant_table(good.get());
    hpdct_default_chroma_quant_table(nullptr);
    if (good[0] != 17.0f || good[1] != 18.0f || good[8] != 18.0f || good[18] != 56.0f || good[63] != 99.0f) ++g_bad;
    for (int i = 0; i < 64; ++i) bad[i] = good[i];
    bad[63] = std::numeric_limits<float>::quiet_NaN();
    expect("fwd NaN chroma", fwd(RGB, Y, CB, CR, 16, 16, S420, good.get(), bad.get(), 0), 1, "chroma");
    // cr right behind the 128 bytes of cb is no overlap for 4:2:0: the call gets as far as the tables
    expect("fwd cr after cb 420", fwd(RGB, Y, CB, at(CB, 128), 16, 16, S420, nullptr, bad.get(), 0), 1, "chroma");
    expect("inv NaN luma", inv(Y, CB, CR, RGB, 16, 16, S420, bad.get(), good.get(), 0), 1, "luma");
    bad[63] = 0.0f;
    expect("fwd zero luma", fwd(RGB, Y, CB, CR, 16, 16, S444, bad.get(), nullptr, 0), 1, "luma");
    bad[63] = std::numeric_limits<float>::infinity();
    expect("fwd inf chroma", fwd(RGB, Y, CB, CR, 16, 16, S444, nullptr, bad.get(), 0), 1, "chroma");
    for (int i = 0; i < 64; ++i) bad[i] = 1.0f / 64.0f;  // |q| up to 65536
    expect("fwd range luma", fwd(RGB, Y, CB, CR, 16, 16, S420, bad.get(), nullptr, 0), 3, "luma");
    expect("fwd range chroma", fwd(RGB, Y, CB, CR, 16, 16, S420, nullptr, bad.get(), 0), 3, "chroma");
    expect("inv range chroma", inv(Y, CB, CR, RGB, 16, 16, S420, good.get(), bad.get(), 0), 3, "int16");
    // arguments are judged before the tables
    expect("fwd flag before range", fwd(RGB, Y, CB, CR, 16, 16, S420, bad.get(), nullptr, 0x80u), 2);
    // the library-owned luma table is under the same rule
    expect("set 1/64 table", hpdct_set_quant_table(bad.get()), 0);
    expect("fwd range library table", fwd(RGB, Y, CB, CR, 16, 16, S420, nullptr, nullptr, 0), 3, "luma");
    // y right behind the 768 bytes of rgb, and rgb right behind the 512 of y, are no overlap: under a library
    // table of 0.001 the call gets as far as the range rule
    for (int i = 0; i < 64; ++i) bad[i] = 0.001f;
    expect("set 0.001 table", hpdct_set_quant_table(bad.get()), 0);
    expect("fwd y at rgb end", fwd(RGB, reinterpret_cast<int16_t*>(at(RGB, 768)), CB, CR, 16, 16, S420, nullptr,
                                   nullptr, 0), 3, "luma");
    expect("fwd rgb at y end", fwd(at(reinterpret_cast<uint8_t*>(Y), 512), Y, CB, CR, 16, 16, S420, nullptr, nullptr, 0),
           3, "luma");
    expect("restore table", hpdct_set_quant_table(nullptr), 0);

    if (g_bad != 0) {
        std::printf("asan_rgb_check: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("asan_rgb_check: ok\n");
    return 0;
}
