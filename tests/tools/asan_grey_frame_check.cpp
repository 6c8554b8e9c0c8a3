// asan_grey_frame_check.cpp -- drives the validation paths of
// hpdct_grey_frame_geometry, hpdct_forward_grey_frame and hpdct_inverse_grey_frame
// under ASan + UBSan, CPU only: a stand-alone program linked with the C ABI's
// host sources (g++; asan.mk's HOST) and the library's kernel objects, as
// asan_rgb_frame_check.cpp is.  No kernel is launched: every device call here
// fails its checks first.  Built and run by tests/test_grey_frame_host.py.
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
void expect_geometry(const char* what, int64_t h, int64_t w, int64_t hp, int64_t wp, int64_t blocks) {
    // each on the heap: a write past an output is an ASan report
    std::unique_ptr<int64_t> o[3];
    for (auto& p : o) p.reset(new int64_t(-1));
    const int st = hpdct_grey_frame_geometry(h, w, o[0].get(), o[1].get(), o[2].get());
    if (st != 0 || *o[0] != hp || *o[1] != wp || *o[2] != blocks) {
        ++g_bad;
        std::printf("MISMATCH geometry %s: status %d, %lld x %lld, %lld blocks\n", what, st,
                    static_cast<long long>(*o[0]), static_cast<long long>(*o[1]), static_cast<long long>(*o[2]));
    }
}
}  // namespace

int main() {
    // never dereferenced: validation fails first.  Far apart, 16-byte aligned.
    const auto IMG = reinterpret_cast<uint8_t*>(uintptr_t(1) << 20);
    const auto BLK = reinterpret_cast<int16_t*>(uintptr_t(1) << 30);
    auto at = [](auto* p, intptr_t bytes) {
        return reinterpret_cast<decltype(p)>(reinterpret_cast<uintptr_t>(p) + bytes);
    };
    auto fwd = [&](const uint8_t* img, int64_t pitch, int16_t* blk, int64_t h, int64_t w, const float* q,
                   unsigned flags) { return hpdct_forward_grey_frame(img, pitch, blk, h, w, q, flags, nullptr); };
    auto inv = [&](const int16_t* blk, uint8_t* img, int64_t pitch, int64_t h, int64_t w, const float* q,
                   unsigned flags) { return hpdct_inverse_grey_frame(blk, img, pitch, h, w, q, flags, nullptr); };

    expect_geometry("1x1", 1, 1, 8, 8, 1);
    expect_geometry("7x9", 7, 9, 8, 16, 2);
    expect_geometry("8x8", 8, 8, 8, 8, 1);
    expect_geometry("1080x1920", 1080, 1920, 1080, 1920, 135 * 240);
    expect("geometry null outputs", hpdct_grey_frame_geometry(13, 515, nullptr, nullptr, nullptr), 0);
    expect("geometry 0x16", hpdct_grey_frame_geometry(0, 16, nullptr, nullptr, nullptr), 1, "positive");
    // 8 x (2^35 - 15): one tile row of 2^32 - 1 tiles; one pixel more pads to 2^32
    const int64_t wide = (int64_t(1) << 35) - 15;
    expect_geometry("8 x (2^35 - 15)", 8, wide, 8, (int64_t(1) << 35) - 8, (int64_t(1) << 32) - 1);
    expect("geometry padded limit", hpdct_grey_frame_geometry(8, wide + 8, nullptr, nullptr, nullptr), 1, "too large");
    expect("geometry 9 rows at the limit", hpdct_grey_frame_geometry(9, wide, nullptr, nullptr, nullptr), 1, "too large");
    expect("geometry int64 max", hpdct_grey_frame_geometry(std::numeric_limits<int64_t>::max(),
                                                           std::numeric_limits<int64_t>::max(), nullptr, nullptr,
                                                           nullptr), 1, "too large");

    // tables: exactly 64 floats on the heap, so a read past them is an ASan report
    std::unique_ptr<float[]> good(new float[64]), bad(new float[64]);
    hpdct_default_quant_table(good.get());
    for (int i = 0; i < 64; ++i) bad[i] = good[i];
    bad[63] = std::numeric_limits<float>::quiet_NaN();
    // a call that passes every argument check gets as far as this table
    const float* nanq = bad.get();

    // a 15x17 frame pads to 16x24: 6 blocks, 768 bytes; dense extent 14 * 17 + 17 = 255
    expect("fwd reaches the table", fwd(IMG, 17, BLK, 15, 17, nanq, 0), 1, "finite");
    expect("fwd null image", fwd(nullptr, 17, BLK, 15, 17, nullptr, 0), 1, "null");
    expect("fwd null blocks", fwd(IMG, 17, nullptr, 15, 17, nullptr, 0), 1, "null");
    expect("fwd 0x17", fwd(IMG, 17, BLK, 0, 17, nullptr, 0), 1, "positive");
    expect("fwd 15x-1", fwd(IMG, 17, BLK, 15, -1, nullptr, 0), 1, "positive");
    expect("fwd pitch w - 1", fwd(IMG, 16, BLK, 15, 17, nullptr, 0), 1, "pitch_bytes");
    expect("fwd pitch 0", fwd(IMG, 0, BLK, 15, 17, nullptr, 0), 1, "pitch_bytes");
    expect("fwd pitch negative", fwd(IMG, -64, BLK, 15, 17, nullptr, 0), 1, "pitch_bytes");
    expect("fwd huge", fwd(IMG, int64_t(1) << 23, BLK, int64_t(1) << 23, int64_t(1) << 23, nullptr, 0), 1, "too large");
    expect("fwd padded limit", fwd(IMG, wide + 8, BLK, 8, wide + 8, nullptr, 0), 1, "too large");
    expect("fwd pitch overflow", fwd(IMG, std::numeric_limits<int64_t>::max() / 4, BLK, 15, 17, nullptr, 0), 1,
           "too large");
    expect("fwd flag 0x80", fwd(IMG, 17, BLK, 15, 17, nullptr, 0x80u), 2);
    expect("fwd blocks + 8", fwd(IMG, 17, at(BLK, 8), 15, 17, nullptr, 0), 1, "aligned");
    expect("fwd blocks + 2", fwd(IMG, 17, at(BLK, 2), 15, 17, nullptr, 0), 1, "aligned");
    // the image has no alignment rule
    expect("fwd image + 1", fwd(at(IMG, 1), 17, BLK, 15, 17, nanq, 0), 1, "finite");
    expect("fwd image + 4", fwd(at(IMG, 4), 17, BLK, 15, 17, nanq, 0), 1, "finite");
    // overlap: the dense extent ends at 255, the pitched one (pitch 64) at 14 * 64 + 17 = 913
    expect("fwd blocks right behind the image", fwd(at(IMG, 1), 17, reinterpret_cast<int16_t*>(at(IMG, 256)), 15, 17,
                                                    nanq, 0), 1, "finite");
    expect("fwd blocks in the image", fwd(at(IMG, 2), 17, reinterpret_cast<int16_t*>(at(IMG, 256)), 15, 17, nullptr, 0),
           1, "overlap");
    expect("fwd blocks in the pitched image", fwd(IMG, 64, reinterpret_cast<int16_t*>(at(IMG, 256)), 15, 17, nullptr,
                                                  0), 1, "overlap");
    expect("fwd blocks in the last pitched row", fwd(IMG, 64, reinterpret_cast<int16_t*>(at(IMG, 912)), 15, 17, nullptr,
                                                     0), 1, "overlap");
    expect("fwd blocks behind the pitched image", fwd(IMG, 64, reinterpret_cast<int16_t*>(at(IMG, 928)), 15, 17, nanq,
                                                      0), 1, "finite");
    // the block array has the padded frame's size: 768 bytes (15 x 17 int16 would be 510)
    expect("fwd image in the padded blocks", fwd(reinterpret_cast<uint8_t*>(at(BLK, 767)), 17, BLK, 15, 17, nullptr, 0),
           1, "overlap");
    expect("fwd image behind the padded blocks", fwd(reinterpret_cast<uint8_t*>(at(BLK, 768)), 17, BLK, 15, 17, nanq, 0),
           1, "finite");
    expect("fwd extent wraps", fwd(reinterpret_cast<uint8_t*>(~uintptr_t(0) - 100), 17, BLK, 15, 17, nullptr, 0), 1,
           "wrap");

    expect("inv reaches the table", inv(BLK, IMG, 17, 15, 17, nanq, 0), 1, "finite");
    expect("inv null", inv(BLK, nullptr, 17, 15, 17, nullptr, 0), 1, "null");
    expect("inv pitch w - 1", inv(BLK, IMG, 16, 15, 17, nullptr, 0), 1, "pitch_bytes");
    expect("inv 0 rows", inv(BLK, IMG, 17, 0, 17, nullptr, 0), 1, "positive");
    expect("inv flag", inv(BLK, IMG, 17, 15, 17, nullptr, HPDCT_BLOCKS_NATURAL | 0x2u), 2);
    expect("inv blocks + 2", inv(at(BLK, 2), IMG, 17, 15, 17, nullptr, 0), 1, "aligned");
    expect("inv pitched image over the blocks", inv(BLK, at(reinterpret_cast<uint8_t*>(BLK), -900), 64, 15, 17, nullptr,
                                                    0), 1, "overlap");
    expect("inv dense image before the blocks", inv(BLK, at(reinterpret_cast<uint8_t*>(BLK), -900), 17, 15, 17, nanq, 0),
           1, "finite");
    expect("inv padded limit", inv(BLK, IMG, wide + 8, 8, wide + 8, nullptr, 0), 1, "too large");

    // tables
    bad[63] = 0.0f;
    expect("fwd zero entry", fwd(IMG, 17, BLK, 15, 17, bad.get(), 0), 1, "non-zero");
    bad[63] = std::numeric_limits<float>::infinity();
    expect("inv infinite entry", inv(BLK, IMG, 17, 15, 17, bad.get(), 0), 1, "finite");
    for (int i = 0; i < 64; ++i) bad[i] = 1.0f / 64.0f;  // |q| up to 65536
    expect("fwd range", fwd(IMG, 17, BLK, 15, 17, bad.get(), 0), 3, "int16");
    expect("inv range", inv(BLK, IMG, 17, 15, 17, bad.get(), 0), 3, "int16");
    // arguments are judged before the table
    expect("fwd pitch before range", fwd(IMG, 16, BLK, 15, 17, bad.get(), 0), 1, "pitch_bytes");
    expect("set 1/64 table", hpdct_set_quant_table(bad.get()), 0);
    expect("fwd range library table", fwd(IMG, 17, BLK, 15, 17, nullptr, 0), 3, "int16");
    expect("inv NULL passes a per-call table by", inv(BLK, IMG, 16, 15, 17, good.get(), 0), 1, "pitch_bytes");
    expect("restore table", hpdct_set_quant_table(nullptr), 0);

    if (g_bad != 0) {
        std::printf("asan_grey_frame_check: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("asan_grey_frame_check: ok\n");
    return 0;
}
