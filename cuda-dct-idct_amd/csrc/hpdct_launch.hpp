// hpdct_launch.hpp -- the launchers of the forward, inverse and frame-list
// kernels: they ask hpdct_policy.hpp what to launch and instantiate it.
// Included by the explicit-instantiation units (hpdct_fwd_*.hip,
// hpdct_inv*.hip, hpdct_frames.hip) and tools.
#pragma once

#include "hpdct.h"
#include "hpdct_kernels_impl.hpp"
#include "hpdct_octet.hpp"
#include "hpdct_duo.hpp"
#include "hpdct_policy.hpp"
#include "hpdct_residency.hpp"

namespace hpdct {

template <typename T>
constexpr policy::Elem kElem =
    std::is_same_v<T, float> ? policy::Elem::kF32 : std::is_same_v<T, int8_t> ? policy::Elem::kI8 : policy::Elem::kU8;
template <typename TIn, typename TOut>
constexpr unsigned kProdVar = policy::prod_var(kElem<TOut>);
template <typename TOut>
constexpr unsigned kOctVar = policy::oct_var(kElem<TOut>);
using policy::kDuoVar;

// workgroups of a tile-per-lane launch (one 64-tile set per wave)
inline dim3 grid_for(const TileGrid& g, uint32_t block = kBlockThreads) {
    return dim3(policy::wgs_for(policy::tile_waves(g), block));
}

// kKern, the kernel of variant kV, as the policy chose it.  A choice of
// another variant means the caller holds no kernel for it: an error.  The
// launchers below list the workgroup sizes and forms each element type is built
// with: a change of hpdct_policy.hpp that asks for others must change them too.
template <unsigned kV, auto kKern, typename... Args>
hipError_t launch_choice(const policy::Choice& c, hipStream_t s, const Args&... args) {
    if (c.var != kV) return hipErrorInvalidDeviceFunction;
    return launch_capped<kKern>(dim3(c.grid_x, c.grid_y), dim3(c.block), c.cap_wgs, s, args...);
}

template <typename TIn, typename TOut, bool kQuant, bool kBuiltinT, bool kWriteback>
hipError_t launch_fdct_impl(const TIn* img, TOut* out, float* shifted, const TileGrid& g, const float* t_dev,
                            const QParams& q, float shift, int qmode, bool row_first, hipStream_t s) {
    using policy::Family;
    constexpr bool kF32 = std::is_same_v<TIn, float> && std::is_same_v<TOut, float>;
    constexpr bool kU8F32 = std::is_same_v<TIn, uint8_t> && std::is_same_v<TOut, float>;
    constexpr bool kU8I8 = std::is_same_v<TIn, uint8_t> && std::is_same_v<TOut, int8_t>;
    // the kernels this instantiation holds (policy::forward asks for no others)
    constexpr bool kFastDivOk = std::is_same_v<TIn, uint8_t> && kQuant && kBuiltinT && !kWriteback;
    constexpr bool kStraddleOk = kU8F32 && kBuiltinT;
    policy::Call pc;
    pc.g = g, pc.in = kElem<TIn>, pc.out = kElem<TOut>, pc.quant = kQuant, pc.builtin_t = kBuiltinT;
    pc.writeback = kWriteback, pc.row_first = row_first, pc.shift128 = shift == 128.0f, pc.qmode = qmode;
    pc.cus = device_cus(), pc.mapping = mapping_mode();
    const policy::Choice c = policy::forward(pc);
    switch (c.family) {
        case Family::kDuoFwdU8:
            if constexpr (kFastDivOk && kU8F32) return launch_fdct_duo_u8(img, out, g, q, c, s);
            break;
        case Family::kRowFirstDuo:
            if constexpr (kF32)
                return policy::with_block_size<64, 256>(c.block, [&](auto kB) {
                    constexpr unsigned kV = with_block<decltype(kB)::value>(kDuoVar);
                    return launch_choice<kV, rowfirst_duo_kernel<false, kQuant, kBuiltinT, kWriteback, kV>>(
                        c, s, img, out, shifted, g, t_dev, q.q, shift);
                });
            break;
        case Family::kDuo:
            if constexpr (kF32)
                return policy::with_bit<kVarFastDivChecked, kQuant>(c.var, [&](auto kQ) {
                    // one-wave (capped) workgroups with the checked quotient only
                    constexpr unsigned kD = kDuoVar | decltype(kQ)::value;
                    return policy::with_block_size<(kD != kDuoVar ? 64u : 256u), 256>(c.block, [&](auto kB) {
                        constexpr unsigned kV = with_block<decltype(kB)::value>(kD);
                        return launch_choice<kV, fdct_duo_kernel<kQuant, kBuiltinT, kWriteback, kV>>(
                            c, s, img, out, shifted, g, t_dev, q, shift);
                    });
                });
            break;
        case Family::kOctet:
            return policy::with_bit<kVarFastDiv, kFastDivOk>(c.var, [&](auto kQ) {
                constexpr unsigned kV = kOctVar<TOut> | decltype(kQ)::value;
                return launch_choice<kV, fdct_octet_kernel<TIn, TOut, kQuant, kBuiltinT, kWriteback, kV>>(
                    c, s, img, out, shifted, g, t_dev, q, shift);
            });
        case Family::kTile:
            return policy::with_bit<kVarRowFirst, kF32>(c.var, [&](auto kR) {
                return policy::with_quotient<kFastDivOk>(c.var, [&](auto kQ) {
                    return policy::with_bit<kVarStraddle, kStraddleOk>(c.var, [&](auto kS) {
                        constexpr unsigned kQv = decltype(kQ)::value;
                        constexpr unsigned kV0 = kProdVar<TIn, TOut> | decltype(kR)::value | kQv | decltype(kS)::value;
                        // uint8 -> fp32: 1024-thread or one-wave workgroups; uint8 ->
                        // int8 with the JPEG forms: one-wave; else the variant's own
                        constexpr uint32_t kSmall = kU8F32 || (kU8I8 && (kQv & kVarJpegQ) != 0u) ? 64u : kBlock<kV0>;
                        return policy::with_block_size<(kU8F32 ? 1024u : kSmall), kSmall>(c.block, [&](auto kB) {
                            constexpr uint32_t kT = decltype(kB)::value;
                            constexpr unsigned kV =
                                with_block<kT>(kV0) | (kU8F32 && kT == 64u ? policy::kF32OneWaveForm : 0u);
                            return launch_choice<kV, fdct_kernel<TIn, TOut, kQuant, kBuiltinT, kWriteback, kV>>(
                                c, s, img, out, shifted, g, t_dev, q, shift);
                        });
                    });
                });
            });
        default: break;
    }
    return hipErrorInvalidDeviceFunction;
}

template <typename TIn, typename TOut, bool kDequant, bool kBuiltinT>
hipError_t launch_idct_impl(const TIn* coef, TOut* out, float* dq_out, const TileGrid& g, const float* t_dev,
                            const Mat64& q, float shift, bool row_first, bool full_chain, hipStream_t s) {
    using policy::Family;
    constexpr bool kF32 = std::is_same_v<TIn, float> && std::is_same_v<TOut, float>;
    constexpr bool kU8Out = std::is_same_v<TOut, uint8_t>;
    constexpr bool kDuoIn = std::is_same_v<TIn, float> && (kF32 || kU8Out);
    constexpr bool kStraddleOk = std::is_same_v<TIn, int8_t> && std::is_same_v<TOut, float> && kBuiltinT;
    // the full-chain variants exist where zero terms are skipped at all: int8 in, dequantised, built-in T
    constexpr bool kFullOk = std::is_same_v<TIn, int8_t> && kDequant && kBuiltinT;
    policy::Call pc;
    pc.g = g, pc.in = kElem<TIn>, pc.out = kElem<TOut>;
    pc.quant = kDequant, pc.builtin_t = kBuiltinT, pc.wb_dequant = dq_out != nullptr, pc.row_first = row_first;
    pc.cus = device_cus(), pc.mapping = mapping_mode(), pc.full_chain = full_chain;
    const policy::Choice c = policy::inverse(pc);
    if constexpr (kFullOk) {
        if ((c.var & kVarFullChain) != 0u) {
            constexpr unsigned kV = policy::kInvFullVar;
            if (c.family == Family::kOctet)
                return launch_choice<kV, idct_octet_kernel<TIn, TOut, kDequant, kBuiltinT, kV>>(c, s, coef, out, dq_out,
                                                                                                g, t_dev, q, shift);
            if (c.family == Family::kTile)
                return launch_choice<kV, idct_kernel<TIn, TOut, kDequant, kBuiltinT, kV>>(c, s, coef, out, dq_out, g,
                                                                                          t_dev, q, shift);
            return hipErrorInvalidDeviceFunction;
        }
    }
    switch (c.family) {
        case Family::kRowFirstDuo:
            if constexpr (kF32)
                return policy::with_block_size<64, 256>(c.block, [&](auto kB) {
                    constexpr unsigned kV = with_block<decltype(kB)::value>(kDuoVar);
                    if constexpr (kDequant) {
                        if (dq_out)
                            return launch_choice<kV, rowfirst_duo_kernel<true, kDequant, kBuiltinT, true, kV>>(
                                c, s, coef, out, dq_out, g, t_dev, q, shift);
                    }
                    return launch_choice<kV, rowfirst_duo_kernel<true, kDequant, kBuiltinT, false, kV>>(
                        c, s, coef, out, static_cast<float*>(nullptr), g, t_dev, q, shift);
                });
            break;
        case Family::kDuo:
            if constexpr (kDuoIn)
                return policy::with_bit<kVarWbDequant, kDequant>(c.var, [&](auto kW) {
                    constexpr unsigned kD = (kU8Out ? with_block<512>(kDuoVar) : kDuoVar) | decltype(kW)::value;
                    // fp32 pixels: one-wave workgroups when capped
                    return policy::with_block_size<(kF32 ? 64u : kBlock<kD>), kBlock<kD>>(c.block, [&](auto kB) {
                        constexpr unsigned kV = with_block<decltype(kB)::value>(kD);
                        return launch_choice<kV, idct_duo_kernel<kDequant, kBuiltinT, kV, TOut>>(
                            c, s, coef, out, dq_out, g, t_dev, q, shift);
                    });
                });
            break;
        case Family::kOctet:
            return policy::with_bit<kVarWbDequant, kF32 && kDequant>(c.var, [&](auto kW) {
                constexpr unsigned kV = kOctVar<TOut> | decltype(kW)::value;
                return launch_choice<kV, idct_octet_kernel<TIn, TOut, kDequant, kBuiltinT, kV>>(
                    c, s, coef, out, dq_out, g, t_dev, q, shift);
            });
        case Family::kTile:
            return policy::with_bit<kVarRowFirst, kF32>(c.var, [&](auto kR) {
                return policy::with_bit<kVarWbDequant, kF32 && kDequant>(c.var, [&](auto kW) {
                    return policy::with_bit<kVarStraddle, kStraddleOk>(c.var, [&](auto kS) {
                        constexpr unsigned kV =
                            kProdVar<TIn, TOut> | decltype(kR)::value | decltype(kW)::value | decltype(kS)::value;
                        return launch_choice<kV, idct_kernel<TIn, TOut, kDequant, kBuiltinT, kV>>(
                            c, s, coef, out, dq_out, g, t_dev, q, shift);
                    });
                });
            });
        default: break;
    }
    return hipErrorInvalidDeviceFunction;
}

// Frame lists: the tile kernel's product variant per frame; grid (workgroups
// per frame, frames).
template <typename TOut>
hipError_t launch_fdct_frames_impl(const FrameTable<TOut>& ft, int n, const TileGrid& g, const QParams& q, int qmode,
                                   hipStream_t s) {
    constexpr bool kF32Out = std::is_same_v<TOut, float>;
    policy::Call pc;
    pc.g = g, pc.frames = static_cast<uint32_t>(n), pc.out = kElem<TOut>, pc.qmode = qmode;
    pc.cus = device_cus(), pc.mapping = mapping_mode();
    const policy::Choice c = policy::forward_frames(pc);
    if (c.family == policy::Family::kDuoFwdU8) {
        if constexpr (kF32Out) return launch_fdct_duo_u8_frames(ft, g, q, c, s);
        return hipErrorInvalidDeviceFunction;
    }
    return policy::with_quotient<true>(c.var, [&](auto kQ) {
        return policy::with_bit<kVarStraddle, kF32Out>(c.var, [&](auto kS) {
            constexpr unsigned kV0 = kProdVar<uint8_t, TOut> | decltype(kQ)::value | decltype(kS)::value;
            // fp32: one-wave workgroups with the packed transform when capped
            return policy::with_block_size<(kF32Out ? 64u : kBlock<kV0>), kBlock<kV0>>(c.block, [&](auto kB) {
                constexpr uint32_t kT = decltype(kB)::value;
                constexpr unsigned kV = with_block<kT>(kV0) | (kF32Out && kT == 64u ? kVarPacked : 0u);
                return launch_choice<kV, fdct_frames_kernel<TOut, kV>>(c, s, ft, g, q);
            });
        });
    });
}

}  // namespace hpdct
