// hpdct_scan_hist.hpp -- the statistics pass of the entropy coder
// (hpdct_scan_histogram): counts[kind][s] = how often hpdct_encode_scan emits
// symbol s of table kind (0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma) for
// the same blocks, geometry and flags.
//
// A block's symbols depend on the block and on the DC of its predecessor alone,
// and scan_locate names that predecessor directly: the pass is parallel over
// BLOCKS (one lane per block, a grid-stride loop), not over intervals, so
// restart_interval = 0 costs what any other interval costs.  A lane stages its
// block as the coder does (scan_stage below) and walks the non-zero mask as scan_walk
// does, counting where the coder puts a code.  The counts go to a 4 x 256 uint32
// histogram of the workgroup in LDS; the EOB, which nearly every block has, is
// counted by ballot, one LDS add per wave and step.  At the end the non-zero
// bins are added to the result with 64-bit integer atomics: order-independent,
// so the result is exact and does not depend on scheduling.  A bin of a
// workgroup holds at most 64 symbols of each of its blocks; a workgroup takes at
// most max(256, 2^32 / kScanHistMaxWgs) = 2^21 blocks, so it stays below 2^27.
// Kernel and launcher, for hpdct_scan.hip alone (it includes this file last).
#pragma once

#include "hpdct_scan.hpp"
#include "hpdct_launch.hpp"

namespace hpdct {

// The coder's staging of a block, a copy of the text in scan_code_body (hpdct_scan.hpp), which stays as the
// coder had it before this pass existed; a change there belongs here too.  Loads the block at blk
// (eight 16-byte loads) into my_blk, the lane's own 32
// dwords of LDS: element n of the staged block = zig-zag coefficient n (natural
// blocks are permuted here).  Returns the mask of its non-zero AC coefficients
// (bit n: coefficient n); dc0: its DC.
template <bool kNatural>
__device__ inline uint64_t scan_stage(const int16_t* blk, uint32_t* my_blk, int& dc0) {
    uint32_t v[32];
    const uint4* p = reinterpret_cast<const uint4*>(blk);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint4 t = p[q];
        v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
    }
    dc0 = static_cast<int16_t>(v[0] & 0xffffu);
    uint64_t nz = 0;
    unroll<32>([&](auto w) {
        uint32_t d = v[w];
        if constexpr (kNatural) {
            constexpr int e0 = zigzag::kOrder[2 * w], e1 = zigzag::kOrder[2 * w + 1];
            const uint32_t lo = (v[e0 >> 1] >> (16 * (e0 & 1))) & 0xffffu;
            const uint32_t hi = (v[e1 >> 1] >> (16 * (e1 & 1))) & 0xffffu;
            d = lo | (hi << 16);
        }
        my_blk[w] = d;
        nz |= static_cast<uint64_t>((d & 0xffffu) != 0u) << (2 * w);
        nz |= static_cast<uint64_t>((d >> 16) != 0u) << (2 * w + 1);
    });
    return nz & ~1ull;  // the DC is coded as a difference
}

template <unsigned kVar>
__global__ __launch_bounds__(256) void scan_hist_kernel(const int16_t* __restrict__ y, const int16_t* __restrict__ cb,
                                                        const int16_t* __restrict__ cr, const scan::ScanGrid g,
                                                        const uint64_t nblk,
                                                        unsigned long long* __restrict__ counts) {
    constexpr bool kNatural = (kVar & kScanNatural) != 0u;
    __shared__ uint32_t s_hist[4u * 256u];
    __shared__ uint32_t s_blk[256u * scan::kBlkStride];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t i = tid; i < 1024u; i += 256u) s_hist[i] = 0u;
    __syncthreads();
    uint32_t* const my_blk = s_blk + tid * scan::kBlkStride;
    const int16_t* c16 = reinterpret_cast<const int16_t*>(my_blk);
    const uint64_t stride = 256ull * gridDim.x;
    // the bound is the workgroup's: every lane of a wave takes every turn (the ballots below)
    for (uint64_t base = 256ull * blockIdx.x; base < nblk; base += stride) {
        const uint64_t jg = base + tid;  // the block's place in the scan
        bool eob = false;
        uint32_t chroma = 0;
        if (jg < nblk) {
            const uint64_t m = jg / g.bpm, m0 = m / g.per_interval * g.per_interval;
            const ScanBlockRef r = scan_locate(y, cb, cr, g, m0, (m - m0) * g.bpm + jg % g.bpm);
            chroma = r.chroma;
            int dc0;
            uint64_t nz = scan_stage<kNatural>(r.blk, my_blk, dc0);
            const int dc = dc0 - (r.prev ? static_cast<int>(*r.prev) : 0);
            uint32_t* const dch = s_hist + 512u * chroma;
            uint32_t* const ach = dch + 256u;
            {
                const uint32_t a = static_cast<uint32_t>(dc < 0 ? -dc : dc);
                uint32_t cat = 32u - static_cast<uint32_t>(__clz(a));  // __clz(0) = 32
                if (cat > scan::kMaxDcCat) cat = scan::kMaxDcCat;
                atomicAdd(&dch[cat], 1u);
            }
            uint32_t prev = 0;
            while (nz != 0ull) {  // at most 63 turns
                const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(nz));
                nz &= nz - 1ull;
                const uint32_t run = k - prev - 1u;
                prev = k;
                const int c = c16[k];
                if (run >= 16u) atomicAdd(&ach[0xf0], run >> 4);  // a ZRL per 16 zeros
                const uint32_t a = static_cast<uint32_t>(c < 0 ? -c : c);
                uint32_t cat = 32u - static_cast<uint32_t>(__clz(a));
                if (cat > scan::kMaxAcCat) cat = scan::kMaxAcCat;
                atomicAdd(&ach[((run & 15u) << 4) | cat], 1u);
            }
            eob = prev != 63u;  // unless coefficient 63 is non-zero
        }
        const uint32_t eob_l = static_cast<uint32_t>(__popcll(__ballot(eob && chroma == 0u)));
        const uint32_t eob_c = static_cast<uint32_t>(__popcll(__ballot(eob && chroma != 0u)));
        if (lane == 0u) {
            if (eob_l != 0u) atomicAdd(&s_hist[256u], eob_l);
            if (eob_c != 0u) atomicAdd(&s_hist[768u], eob_c);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < 1024u; i += 256u) {
        const uint32_t v = s_hist[i];
        if (v != 0u) atomicAdd(&counts[i], static_cast<unsigned long long>(v));  // integer: order-independent
    }
}

hipError_t launch_scan_hist(const int16_t* y, const int16_t* cb, const int16_t* cr, const scan::ScanGrid& g,
                            bool natural, uint64_t* counts, hipStream_t s) {
    if (hipError_t e = hipMemsetAsync(counts, 0, 4u * 256u * sizeof(uint64_t), s)) return e;
    const uint64_t nblk = static_cast<uint64_t>(g.nmcu) * g.bpm;
    const policy::Choice c = policy::scan_hist(nblk, natural);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
    return policy::with_bit<kScanNatural, true>(c.var, [&](auto kN) {
        constexpr unsigned kV = with_block<256>(decltype(kN)::value | kScanHist);
        return launch_choice<kV, scan_hist_kernel<kV>>(c, s, y, cb, cr, g, nblk, out);
    });
}

}  // namespace hpdct
