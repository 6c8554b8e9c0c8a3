// asan_dct_frames_check.cpp -- drives the argument paths HPDCT_FRAME_DCT adds to
// the four frame calls, and hpdct_dct_transform, under ASan + UBSan, CPU only: a
// stand-alone program linked with the C ABI's host sources (g++; asan.mk's HOST)
// and the library's kernel objects, as asan_grey_frame_check.cpp is.  No kernel
// is launched: every device call here fails its checks first.  Built and run by
// tests/test_dct_frames_host.py.
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
    const auto IMG = reinterpret_cast<uint8_t*>(uintptr_t(1) << 20);
    const auto Y = reinterpret_cast<int16_t*>(uintptr_t(1) << 30);
    const auto CB = reinterpret_cast<int16_t*>(uintptr_t(1) << 31);
    const auto CR = reinterpret_cast<int16_t*>(uintptr_t(1) << 32);
    constexpr unsigned kDct = HPDCT_FRAME_DCT, kNat = HPDCT_BLOCKS_NATURAL;
    static_assert(kDct == 0x100u, "the flag's value is part of the ABI");

    // the matrix: exactly 64 floats on the heap, so a write past them is an ASan report
    std::unique_ptr<float[]> t(new float[64]);
    hpdct_dct_transform(t.get());
    hpdct_dct_transform(nullptr);
    const double pi = std::acos(-1.0);
    for (int v = 0; v < 8; ++v)
        for (int i = 0; i < 8; ++i) {
            const double x = v == 0 ? std::sqrt(1.0 / 8.0) : 0.5 * std::cos((2 * i + 1) * v * pi / 16.0);
            if (t[8 * v + i] != static_cast<float>(x)) {
                ++g_bad;
                std::printf("MISMATCH dct_transform[%d][%d]: %.9g (expected %.9g)\n", v, i, t[8 * v + i],
                            static_cast<float>(x));
            }
        }

    std::unique_ptr<float[]> good(new float[64]), bad(new float[64]);
    hpdct_default_quant_table(good.get());
    for (int i = 0; i < 64; ++i) bad[i] = good[i];
    bad[63] = std::numeric_limits<float>::quiet_NaN();
    const float* nanq = bad.get();  // a call that passes every argument check gets as far as this table

    auto gfwd = [&](const float* q, unsigned flags, int64_t pitch = 17) {
        return hpdct_forward_grey_frame(IMG, pitch, Y, 15, 17, q, flags, nullptr);
    };
    auto ginv = [&](const float* q, unsigned flags, int64_t pitch = 17) {
        return hpdct_inverse_grey_frame(Y, IMG, pitch, 15, 17, q, flags, nullptr);
    };
    auto cfwd = [&](hpdct_subsampling sub, const float* ql, const float* qc, unsigned flags, int64_t pitch = 51) {
        return hpdct_forward_rgb_frame(IMG, pitch, Y, CB, CR, 15, 17, sub, ql, qc, flags, nullptr);
    };
    auto cinv = [&](hpdct_subsampling sub, const float* ql, const float* qc, unsigned flags, int64_t pitch = 51) {
        return hpdct_inverse_rgb_frame(Y, CB, CR, IMG, pitch, 15, 17, sub, ql, qc, flags, nullptr);
    };
    const hpdct_subsampling subs[2] = {HPDCT_SUBSAMPLING_444, HPDCT_SUBSAMPLING_420};

    // the flag alone and with the block order: past every argument check, as far as the table
    for (unsigned f : {kDct, kDct | kNat}) {
        expect("grey fwd takes the flag", gfwd(nanq, f), 1, "finite");
        expect("grey inv takes the flag", ginv(nanq, f), 1, "finite");
        for (hpdct_subsampling s : subs) {
            expect("rgb fwd takes the flag", cfwd(s, nanq, nullptr, f), 1, "finite");
            expect("rgb inv takes the flag", cinv(s, nullptr, nanq, f), 1, "finite");
        }
    }
    // with any other bit: refused
    for (unsigned f : {kDct | 0x2u, kDct | 0x80u, kDct | 0x200u, 0x200u, ~0u}) {
        expect("grey fwd other bits", gfwd(nullptr, f), 2, "flag");
        expect("grey inv other bits", ginv(nullptr, f), 2, "flag");
        for (hpdct_subsampling s : subs) {
            expect("rgb fwd other bits", cfwd(s, nullptr, nullptr, f), 2, "flag");
            expect("rgb inv other bits", cinv(s, nullptr, nullptr, f), 2, "flag");
        }
    }
    // the other checks come first, as without the flag
    expect("grey fwd pitch", gfwd(nullptr, kDct, 16), 1, "pitch_bytes");
    expect("grey inv pitch", ginv(nullptr, kDct, 16), 1, "pitch_bytes");
    expect("rgb fwd pitch", cfwd(HPDCT_SUBSAMPLING_420, nullptr, nullptr, kDct, 50), 1, "pitch_bytes");
    expect("rgb inv pitch", cinv(HPDCT_SUBSAMPLING_444, nullptr, nullptr, kDct, 50), 1, "pitch_bytes");
    expect("grey fwd null", hpdct_forward_grey_frame(nullptr, 17, Y, 15, 17, nullptr, kDct, nullptr), 1, "null");
    expect("rgb inv null", hpdct_inverse_rgb_frame(Y, nullptr, CR, IMG, 51, 15, 17, HPDCT_SUBSAMPLING_420, nullptr,
                                                   nullptr, kDct, nullptr), 1, "null");

    // the range rule under the DCT's row norms: 1/64 gives |q| up to 65536 under either matrix
    for (int i = 0; i < 64; ++i) bad[i] = 1.0f / 64.0f;
    expect("grey fwd range", gfwd(bad.get(), kDct), 3, "int16");
    expect("grey inv range", ginv(bad.get(), kDct), 3, "int16");
    expect("rgb fwd luma range", cfwd(HPDCT_SUBSAMPLING_420, bad.get(), nullptr, kDct), 3, "luma");
    expect("rgb inv chroma range", cinv(HPDCT_SUBSAMPLING_444, nullptr, bad.get(), kDct), 3, "chroma");
    expect("set 1/64 table", hpdct_set_quant_table(bad.get()), 0);
    expect("grey fwd range library table", gfwd(nullptr, kDct), 3, "int16");
    expect("rgb fwd range library table", cfwd(HPDCT_SUBSAMPLING_420, nullptr, nullptr, kDct | kNat), 3, "luma");
    expect("restore table", hpdct_set_quant_table(nullptr), 0);
    // Between the two rules: HpApprDCT's rows 3 and 7 have L1 norm 1.414 against the DCT's 2.563, so an entry at
    // position (7, 7) that the unflagged range rule takes (128 * 2 / Q <= 32767) fails the DCT's (128 * 6.57 / Q)
    for (int i = 0; i < 64; ++i) bad[i] = good[i];
    bad[63] = 0.02f;
    // (without the flag that table passes and the call would launch, so only the flagged calls are made here)
    expect("grey fwd (7,7) table under the flag", gfwd(bad.get(), kDct), 3, "int16");
    expect("grey inv (7,7) table under the flag", ginv(bad.get(), kDct | kNat), 3, "int16");

    // every other entry point keeps refusing the bit
    expect("forward_blocks", hpdct_forward_blocks(IMG, Y, 16, 32, kDct, nullptr), 2, "flag");
    expect("inverse_blocks", hpdct_inverse_blocks(Y, IMG, HPDCT_U8, 16, 32, kDct, nullptr), 2, "flag");
    expect("forward_rgb_blocks", hpdct_forward_rgb_blocks(IMG, Y, CB, CR, 16, 32, HPDCT_SUBSAMPLING_420, nullptr,
                                                          nullptr, kDct, nullptr), 2, "flag");
    expect("inverse_rgb_blocks", hpdct_inverse_rgb_blocks(Y, CB, CR, IMG, 16, 32, HPDCT_SUBSAMPLING_444, nullptr,
                                                          nullptr, kDct | kNat, nullptr), 2, "flag");
    expect("forward", hpdct_forward(IMG, HPDCT_U8, Y, HPDCT_F32, 16, 32, nullptr, kDct, nullptr), 2);
    expect("inverse", hpdct_inverse(Y, HPDCT_F32, IMG, HPDCT_F32, 16, 32, nullptr, kDct, nullptr), 2);

    if (g_bad != 0) {
        std::printf("asan_dct_frames_check: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("asan_dct_frames_check: ok\n");
    return 0;
}
