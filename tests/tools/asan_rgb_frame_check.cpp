// asan_rgb_frame_check.cpp -- drives the validation paths of
// hpdct_rgb_frame_geometry, hpdct_forward_rgb_frame and hpdct_inverse_rgb_frame
// under ASan + UBSan, CPU only: a stand-alone program linked with the sanitised
// the C ABI's host sources (g++; asan.mk's HOST) and the library's kernel objects, as asan_rgb_check.cpp
// is.  No kernel is launched: every device call here fails its checks first.
// Built and run by tests/test_rgb_frame_host.py.
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
void expect_geometry(const char* what, int64_t h, int64_t w, hpdct_subsampling sub, int64_t hp, int64_t wp,
                     int64_t yb, int64_t cb) {
    // each on the heap: a write past an output is an ASan report
    std::unique_ptr<int64_t> o[4];
    for (auto& p : o) p.reset(new int64_t(-1));
    const int st = hpdct_rgb_frame_geometry(h, w, sub, o[0].get(), o[1].get(), o[2].get(), o[3].get());
    if (st != 0 || *o[0] != hp || *o[1] != wp || *o[2] != yb || *o[3] != cb) {
        ++g_bad;
        std::printf("MISMATCH geometry %s: status %d, %lld x %lld, %lld + 2 x %lld blocks\n", what, st,
                    static_cast<long long>(*o[0]), static_cast<long long>(*o[1]), static_cast<long long>(*o[2]),
                    static_cast<long long>(*o[3]));
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
    auto fwd = [&](const uint8_t* rgb, int64_t pitch, int16_t* y, int16_t* cb, int16_t* cr, int64_t h, int64_t w,
                   int sub, const float* ql, const float* qc, unsigned flags) {
        return hpdct_forward_rgb_frame(rgb, pitch, y, cb, cr, h, w, static_cast<hpdct_subsampling>(sub), ql, qc, flags,
                                       nullptr);
    };
    auto inv = [&](const int16_t* y, const int16_t* cb, const int16_t* cr, uint8_t* rgb, int64_t pitch, int64_t h,
                   int64_t w, int sub, const float* ql, const float* qc, unsigned flags) {
        return hpdct_inverse_rgb_frame(y, cb, cr, rgb, pitch, h, w, static_cast<hpdct_subsampling>(sub), ql, qc, flags,
                                       nullptr);
    };

    expect_geometry("1x1 444", 1, 1, S444, 8, 8, 1, 1);
    expect_geometry("1x1 420", 1, 1, S420, 16, 16, 4, 1);
    expect_geometry("1080x1920 444", 1080, 1920, S444, 1080, 1920, 135 * 240, 135 * 240);
    expect_geometry("1080x1920 420", 1080, 1920, S420, 1088, 1920, 136 * 240, 68 * 120);
    expect_geometry("667x1000 444", 667, 1000, S444, 672, 1000, 84 * 125, 84 * 125);
    expect_geometry("667x1000 420", 667, 1000, S420, 672, 1008, 84 * 126, 42 * 63);
    expect("geometry null outputs", hpdct_rgb_frame_geometry(13, 515, S444, nullptr, nullptr, nullptr, nullptr), 0);
    expect("geometry 0x16", hpdct_rgb_frame_geometry(0, 16, S420, nullptr, nullptr, nullptr, nullptr), 1, "positive");
    expect("geometry enum", hpdct_rgb_frame_geometry(16, 16, static_cast<hpdct_subsampling>(2), nullptr, nullptr,
                                                     nullptr, nullptr), 1, "subsampling");
    // 8 x (2^35 - 15): one tile row of 2^32 - 1 tiles for 4:4:4, 2^32 after padding to whole MCUs for 4:2:0
    const int64_t wide = (int64_t(1) << 35) - 15;
    expect_geometry("8 x (2^35 - 15) 444", 8, wide, S444, 8, (int64_t(1) << 35) - 8, (int64_t(1) << 32) - 1,
                    (int64_t(1) << 32) - 1);
    expect("geometry padded limit", hpdct_rgb_frame_geometry(8, wide, S420, nullptr, nullptr, nullptr, nullptr), 1,
           "too large");
    expect("geometry int64 max", hpdct_rgb_frame_geometry(std::numeric_limits<int64_t>::max(),
                                                          std::numeric_limits<int64_t>::max(), S420, nullptr, nullptr,
                                                          nullptr, nullptr), 1, "too large");

    // tables: exactly 64 floats on the heap, so a read past them is an ASan report
    std::unique_ptr<float[]> good(new float[64]), bad(new float[64]);
    hpdct_default_chroma_quant_table(good.get());
    for (int i = 0; i < 64; ++i) bad[i] = good[i];
    bad[63] = std::numeric_limits<float>::quiet_NaN();
    // a call that passes every pointer check gets as far as this chroma table
    const float* nanq = bad.get();

    expect("fwd null rgb", fwd(nullptr, 51, Y, CB, CR, 15, 17, S420, nullptr, nullptr, 0), 1, "null");
    expect("fwd null y", fwd(RGB, 51, nullptr, CB, CR, 15, 17, S420, nullptr, nullptr, 0), 1, "null");
    expect("fwd null cb", fwd(RGB, 51, Y, nullptr, CR, 15, 17, S420, nullptr, nullptr, 0), 1, "null");
    expect("fwd null cr", fwd(RGB, 51, Y, CB, nullptr, 15, 17, S420, nullptr, nullptr, 0), 1, "null");
    expect("fwd 0x17", fwd(RGB, 51, Y, CB, CR, 0, 17, S420, nullptr, nullptr, 0), 1, "positive");
    expect("fwd 15x-1", fwd(RGB, 51, Y, CB, CR, 15, -1, S444, nullptr, nullptr, 0), 1, "positive");
    expect("fwd pitch 3w - 1", fwd(RGB, 50, Y, CB, CR, 15, 17, S420, nullptr, nullptr, 0), 1, "pitch_bytes");
    expect("fwd pitch 0", fwd(RGB, 0, Y, CB, CR, 15, 17, S420, nullptr, nullptr, 0), 1, "pitch_bytes");
    expect("fwd pitch negative", fwd(RGB, -64, Y, CB, CR, 15, 17, S420, nullptr, nullptr, 0), 1, "pitch_bytes");
    expect("fwd huge", fwd(RGB, int64_t(3) << 23, Y, CB, CR, int64_t(1) << 23, int64_t(1) << 23, S444, nullptr, nullptr,
                           0), 1, "too large");
    expect("fwd padded limit", fwd(RGB, 3 * wide, Y, CB, CR, 8, wide, S420, nullptr, nullptr, 0), 1, "too large");
    expect("fwd pitch overflow", fwd(RGB, std::numeric_limits<int64_t>::max() / 4, Y, CB, CR, 15, 17, S420, nullptr,
                                     nullptr, 0), 1, "too large");
    expect("fwd enum 2", fwd(RGB, 51, Y, CB, CR, 15, 17, 2, nullptr, nullptr, 0), 1, "subsampling");
    expect("fwd flag 0x80", fwd(RGB, 51, Y, CB, CR, 15, 17, S420, nullptr, nullptr, 0x80u), 2);
    expect("fwd y + 8", fwd(RGB, 51, at(Y, 8), CB, CR, 15, 17, S420, nullptr, nullptr, 0), 1, "aligned");
    expect("fwd cr + 2", fwd(RGB, 51, Y, CB, at(CR, 2), 15, 17, S420, nullptr, nullptr, 0), 1, "aligned");
    // 15x17 4:2:0 pads to 16x32: y 1024 bytes, cb and cr 256 each; dense rgb extent 14 * 51 + 51 = 765
    expect("fwd y right behind rgb", fwd(at(RGB, 3), 51, reinterpret_cast<int16_t*>(at(RGB, 768)), CB, CR, 15, 17, S420,
                                         nullptr, nanq, 0), 1, "chroma");                     // no overlap: the tables
    expect("fwd y in rgb", fwd(at(RGB, 4), 51, reinterpret_cast<int16_t*>(at(RGB, 768)), CB, CR, 15, 17, S420, nullptr,
                               nullptr, 0), 1, "overlap");
    // the same pointers overlap only through the pitch: extent 14 * 64 + 51 = 947
    expect("fwd y in pitched rgb", fwd(RGB, 64, reinterpret_cast<int16_t*>(at(RGB, 768)), CB, CR, 15, 17, S420, nullptr,
                                       nullptr, 0), 1, "overlap");
    expect("fwd y behind pitched rgb", fwd(RGB, 64, reinterpret_cast<int16_t*>(at(RGB, 960)), CB, CR, 15, 17, S420,
                                           nullptr, nanq, 0), 1, "chroma");
    // the block arrays have the padded sizes: cb 256 bytes (a 15x17 plane of its own would need less)
    expect("fwd cr in padded cb", fwd(RGB, 51, Y, CB, at(CB, 240), 15, 17, S420, nullptr, nullptr, 0), 1, "overlap");
    expect("fwd cr behind padded cb", fwd(RGB, 51, Y, CB, at(CB, 256), 15, 17, S420, nullptr, nanq, 0), 1, "chroma");
    expect("fwd cb in padded y", fwd(RGB, 51, Y, at(Y, 1008), CR, 15, 17, S420, nullptr, nullptr, 0), 1, "overlap");
    expect("fwd cr in cb 444", fwd(RGB, 51, Y, CB, at(CB, 256), 15, 17, S444, nullptr, nullptr, 0), 1, "overlap");
    // d_rgb has no alignment rule
    expect("fwd rgb + 1", fwd(at(RGB, 1), 51, Y, CB, CR, 15, 17, S420, nullptr, nanq, 0), 1, "chroma");

    expect("inv null", inv(Y, CB, CR, nullptr, 51, 15, 17, S420, nullptr, nullptr, 0), 1, "null");
    expect("inv pitch 3w - 1", inv(Y, CB, CR, RGB, 50, 15, 17, S444, nullptr, nullptr, 0), 1, "pitch_bytes");
    expect("inv 0 rows", inv(Y, CB, CR, RGB, 51, 0, 17, S444, nullptr, nullptr, 0), 1, "positive");
    expect("inv enum 7", inv(Y, CB, CR, RGB, 51, 15, 17, 7, nullptr, nullptr, 0), 1, "subsampling");
    expect("inv flag", inv(Y, CB, CR, RGB, 51, 15, 17, S444, nullptr, nullptr, HPDCT_BLOCKS_NATURAL | 0x2u), 2);
    expect("inv y + 2", inv(at(Y, 2), CB, CR, RGB, 51, 15, 17, S444, nullptr, nullptr, 0), 1, "aligned");
    expect("inv pitched rgb over y", inv(Y, CB, CR, at(reinterpret_cast<uint8_t*>(Y), -900), 64, 15, 17, S444, nullptr,
                                         nullptr, 0), 1, "overlap");
    expect("inv dense rgb before y", inv(Y, CB, CR, at(reinterpret_cast<uint8_t*>(Y), -900), 51, 15, 17, S444, nullptr,
                                         nanq, 0), 1, "chroma");
    expect("inv padded limit", inv(Y, CB, CR, RGB, 3 * wide, 8, wide, S420, nullptr, nullptr, 0), 1, "too large");

    // tables
    expect("fwd NaN chroma", fwd(RGB, 51, Y, CB, CR, 15, 17, S420, good.get(), bad.get(), 0), 1, "chroma");
    expect("inv NaN luma", inv(Y, CB, CR, RGB, 51, 15, 17, S420, bad.get(), good.get(), 0), 1, "luma");
    bad[63] = 0.0f;
    expect("fwd zero luma", fwd(RGB, 51, Y, CB, CR, 15, 17, S444, bad.get(), nullptr, 0), 1, "luma");
    for (int i = 0; i < 64; ++i) bad[i] = 1.0f / 64.0f;  // |q| up to 65536
    expect("fwd range luma", fwd(RGB, 51, Y, CB, CR, 15, 17, S420, bad.get(), nullptr, 0), 3, "luma");
    expect("inv range chroma", inv(Y, CB, CR, RGB, 51, 15, 17, S420, good.get(), bad.get(), 0), 3, "int16");
    // arguments are judged before the tables
    expect("fwd pitch before range", fwd(RGB, 50, Y, CB, CR, 15, 17, S420, bad.get(), nullptr, 0), 1, "pitch_bytes");
    expect("set 1/64 table", hpdct_set_quant_table(bad.get()), 0);
    expect("fwd range library table", fwd(RGB, 51, Y, CB, CR, 15, 17, S420, nullptr, nullptr, 0), 3, "luma");
    expect("restore table", hpdct_set_quant_table(nullptr), 0);

    if (g_bad != 0) {
        std::printf("asan_rgb_frame_check: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("asan_rgb_frame_check: ok\n");
    return 0;
}
