// policy_dct_check.cpp -- pins what the four frame calls launch under
// HPDCT_FRAME_DCT (csrc/hpdct_policy.hpp: GreyCall::dct, RgbCall::dct), after
// policy_grey_frame_check.cpp.  For every combination of clip, quotient mode,
// full_chain and subsampling with the DCT selected:
//   - the chosen variant never carries kVarJpegQ (the per-position quotient
//     forms are proven under HpApprDCT's bounds only);
//   - the inverse does not depend on full_chain (the matrix has no zero to skip)
//     and never carries kVarFullChain;
//   - the launch shape (family, workgroup size, cap, grid) equals the HpApprDCT
//     row's for the same call;
//   - the variant is the HpApprDCT row's with kFrameDct, the clip bit as there,
//     and nothing else: what the hpdct_dct_*.hip units hold.
// Host code only (g++); run by tests/test_dct_frames_host.py.
#include <cstdio>

#include "hpdct_policy.hpp"

using namespace hpdct;
using namespace hpdct::policy;

namespace {

int g_bad = 0;
int g_rows = 0;

void bad(const char* what, const Choice& got, const Choice& plain) {
    ++g_bad;
    std::printf("MISMATCH %s: var 0x%08x block %u cap %u grid %u x %u (HpApprDCT row: var 0x%08x block %u cap %u "
                "grid %u x %u)\n",
                what, got.var, got.block, got.cap_wgs, got.grid_x, got.grid_y, plain.var, plain.block, plain.cap_wgs,
                plain.grid_x, plain.grid_y);
}
bool same_shape(const Choice& a, const Choice& b) {
    return a.family == b.family && a.block == b.block && a.cap_wgs == b.cap_wgs && a.grid_x == b.grid_x &&
           a.grid_y == b.grid_y;
}
// what every DCT row must satisfy against the HpApprDCT row of the same call
void check(const char* what, const Choice& got, const Choice& plain, unsigned clip_bit, bool clip) {
    ++g_rows;
    if ((got.var & kVarJpegQ) != 0u || (got.var & kVarFullChain) != 0u || (got.var & kFrameDct) == 0u ||
        (got.var & clip_bit) != (clip ? clip_bit : 0u) || (plain.var & kFrameDct) != 0u || !same_shape(got, plain) ||
        block_of(got.var) != got.block)
        bad(what, got, plain);
}

}  // namespace

int main() {
    const uint32_t tiles[] = {1u, 2u, 64u, 65u, 130u, 32400u, 1u << 20, 0xffffffffu};
    for (uint32_t n : tiles)
        for (int clip = 0; clip <= 1; ++clip)
            for (int full = 0; full <= 1; ++full) {
                for (int q = 0; q <= 2; ++q) {
                    GreyCall c;
                    c.tiles = n, c.qmode = q, c.clip = clip != 0, c.full_chain = full != 0;
                    GreyCall d = c;
                    d.dct = true;
                    const Choice got = forward_grey(d);
                    check("grey forward", got, forward_grey(c), kGreyClip, c.clip);
                    // IEEE division for qmode 0, the 3-op quotient for 1 and for 2
                    if ((got.var & kVarFastDiv) != (q != 0 ? kVarFastDiv : 0u)) bad("grey forward quotient", got, got);
                    if (got.var != (kGreyFwdDctVar | (q != 0 ? kVarFastDiv : 0u) | (c.clip ? kGreyClip : 0u)))
                        bad("grey forward variant", got, got);
                }
                GreyCall c;
                c.tiles = n, c.clip = clip != 0, c.full_chain = full != 0;
                GreyCall d = c, e = c;
                d.dct = true;
                e.dct = true, e.full_chain = !c.full_chain;
                const Choice got = inverse_grey(d), other = inverse_grey(e);
                check("grey inverse", got, inverse_grey(c), kGreyClip, c.clip);
                if (got.var != (kGreyInvDctVar | (c.clip ? kGreyClip : 0u))) bad("grey inverse variant", got, got);
                if (got.var != other.var || !same_shape(got, other)) bad("grey inverse reads full_chain", got, other);
            }
    for (uint32_t n : tiles)
        for (int s420 = 0; s420 <= 1; ++s420)
            for (int clip = 0; clip <= 1; ++clip)
                for (int full = 0; full <= 1; ++full) {
                    const unsigned sub = s420 ? kRgb420 : 0u;
                    for (int ql = 0; ql <= 2; ++ql)
                        for (int qc = 0; qc <= 1; ++qc) {
                            RgbCall c;
                            c.units = n, c.s420 = s420 != 0, c.qmode_luma = ql, c.qmode_chroma = qc;
                            c.clip = clip != 0, c.full_chain = full != 0;
                            RgbCall d = c;
                            d.dct = true;
                            const Choice got = forward_rgb(d);
                            check("rgb forward", got, forward_rgb(c), kRgbClip, c.clip);
                            const bool fast = ql != 0 && qc != 0;
                            if (got.var != (kRgbFwdDctVar | sub | (fast ? kVarFastDiv | kRgbChromaFastDiv : 0u) |
                                             (c.clip ? kRgbClip : 0u)))
                                bad("rgb forward variant", got, got);
                        }
                    RgbCall c;
                    c.units = n, c.s420 = s420 != 0, c.clip = clip != 0, c.full_chain = full != 0;
                    RgbCall d = c, e = c;
                    d.dct = true;
                    e.dct = true, e.full_chain = !c.full_chain;
                    const Choice got = inverse_rgb(d), other = inverse_rgb(e);
                    check("rgb inverse", got, inverse_rgb(c), kRgbClip, c.clip);
                    if (got.var != (kRgbInvDctVar | sub | (c.clip ? kRgbClip : 0u))) bad("rgb inverse variant", got, got);
                    if (got.var != other.var || !same_shape(got, other)) bad("rgb inverse reads full_chain", got, other);
                }
    if (g_bad != 0) {
        std::printf("policy_dct_check: %d of %d rows differ\n", g_bad, g_rows);
        return 1;
    }
    std::printf("policy_dct_check: ok (%d rows)\n", g_rows);
    return 0;
}
