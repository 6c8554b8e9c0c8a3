// hpdct_huffman.hpp -- Huffman tables as the caller's data: the
// judgement of a DHT's contents, the blob the *_tables calls read
// (unscan::HuffBlob), and the optimal table of T.81 K.2.  Plain C++, host only,
// no allocation: hpdct_api_jpeg.cpp and tests/tools/asan_huffman_check.cpp include it.
#pragma once

#include <stdint.h>
#include <string.h>

#include "hpdct.h"
#include "hpdct_unscan.hpp"

namespace hpdct {
namespace huff {

inline const char* kind_name(int kind) {
    return kind == 0 ? "DC luma" : kind == 1 ? "AC luma" : kind == 2 ? "DC chroma" : "AC chroma";
}

// Why hpdct_huffman_prepare refuses s as table `kind`, or nullptr if it does not.
inline const char* defect(const hpdct_huffman_spec& s, int kind) {
    if (s.nvals > 256) return "nvals is above 256";
    int sum = 0;
    for (int i = 0; i < 16; ++i) sum += s.bits[i];
    if (s.nvals != sum) return "nvals is not the sum of bits";
    // the lengths assigned canonically: the next code of length l is `code`, and 2^l of them exist
    uint32_t code = 0;
    for (int len = 1; len <= 16; ++len) {
        code += s.bits[len - 1];
        if (code > (1u << len)) return "the code is over-subscribed";
        code <<= 1;
    }
    bool seen[256] = {};
    for (int i = 0; i < s.nvals; ++i) {
        if (seen[s.vals[i]]) return "a symbol appears twice";
        seen[s.vals[i]] = true;
        if ((kind & 1) == 0 && s.vals[i] > 15u) return "a DC symbol is above 15";
    }
    return nullptr;
}

// Annex K's table `kind`, the definition of hpdct_scan.hpp (its unused vals are 0)
inline hpdct_huffman_spec annex_k(int kind) { return scan::spec_of(kind); }
inline bool same_table(const hpdct_huffman_spec& a, const hpdct_huffman_spec& b) {
    return a.nvals == b.nvals && memcmp(a.bits, b.bits, 16) == 0 &&
           memcmp(a.vals, b.vals, static_cast<size_t>(a.nvals < 0 ? 0 : a.nvals)) == 0;
}

// The blob of four specs that passed defect(), by the builders that fill the Annex K constants: scan::fill_codes
// and unscan::fill_decode.  A symbol without a code has the entry 0 (length 0); a lookup slot no code of 8 bits
// or fewer covers is 0.
inline void fill_blob(const hpdct_huffman_spec specs[4], unscan::HuffBlob& b) {
    memset(&b, 0, sizeof(b));
    for (int kind = 0; kind < 4; ++kind) {
        scan::fill_codes(specs[kind], (kind & 1) ? b.code.ac[kind >> 1] : b.code.dc[kind >> 1]);
        unscan::fill_decode(specs[kind], b.dec, kind);
    }
}

// T.81 K.2 (figures K.1 - K.4), as hpdct_huffman_optimal documents it.
inline void optimal(const uint64_t counts[256], hpdct_huffman_spec& out) {
    constexpr int kN = 257;  // the symbols and the pseudo-symbol 256
    uint64_t freq[kN];
    int codesize[kN], others[kN];
    // a tree of 257 leaves is at most 256 deep; one more so that bits[i - 2] .. bits[i] below never leave it
    int bits[kN + 2] = {};
    for (int i = 0; i < 256; ++i) freq[i] = counts[i];
    freq[256] = 1;
    for (int i = 0; i < kN; ++i) codesize[i] = 0, others[i] = -1;
    for (;;) {
        // figure K.1: the least non-zero count, then the next; on ties the larger index
        int v1 = -1, v2 = -1;
        for (int i = 0; i < kN; ++i)
            if (freq[i] != 0u && (v1 < 0 || freq[i] <= freq[v1])) v1 = i;
        for (int i = 0; i < kN; ++i)
            if (freq[i] != 0u && i != v1 && (v2 < 0 || freq[i] <= freq[v2])) v2 = i;
        if (v2 < 0) break;
        freq[v1] += freq[v2], freq[v2] = 0;
        for (++codesize[v1]; others[v1] >= 0;) v1 = others[v1], ++codesize[v1];
        others[v1] = v2;
        for (++codesize[v2]; others[v2] >= 0;) v2 = others[v2], ++codesize[v2];
    }
    memset(&out, 0, sizeof(out));
    int longest = 0, real = 0;
    for (int i = 0; i < kN; ++i)
        if (codesize[i] != 0) ++bits[codesize[i]], longest = codesize[i] > longest ? codesize[i] : longest;
    for (int i = 0; i < 256; ++i) real += codesize[i] != 0;
    if (real == 0) return;  // all counts zero: the pseudo-symbol alone, no code
    // figure K.3: no length above 16
    for (int i = longest; i > 16; --i) {
        while (bits[i] > 0) {
            // a tree with a code of more than 16 bits has a shorter non-empty length (Kraft: codes of 17 bits
            // or more alone cannot fill the code space that 257 leaves take), so j stops above 0
            int j = i - 2;
            while (bits[j] == 0) --j;
            bits[i] -= 2, bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1;
        }
    }
    int i = 16;
    while (bits[i] == 0) --i;
    --bits[i];  // the pseudo-symbol leaves the longest length
    for (int l = 1; l <= 16; ++l) out.bits[l - 1] = static_cast<uint8_t>(bits[l]);
    // figure K.4: by length of the tree, then by symbol value
    int k = 0;
    for (int l = 1; l <= longest; ++l)
        for (int s = 0; s < 256; ++s)
            if (codesize[s] == l) out.vals[k++] = static_cast<uint8_t>(s);
    out.nvals = k;
}

}  // namespace huff
}  // namespace hpdct
