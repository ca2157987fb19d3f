// Device primitives shared by every kernel of the packed linear layer (cq_linear.hip and, through
// cq_linear_tile.h, cq_linear_bwd.hip and cq_linear_dequant.hip): the vector types, the masked
// 8-element row loader and the magic-number expansion of packed 2/4-bit codes to fp16.
//
// Everything sits in an unnamed namespace and is force-inlined: each including file compiles its
// own copy into its own kernels.
#pragma once

#include "cq_common.h"

namespace cq {
namespace {

using h8 = __attribute__((ext_vector_type(8))) _Float16;
using h4 = __attribute__((ext_vector_type(4))) _Float16;
using h2 = __attribute__((ext_vector_type(2))) _Float16;
using f4 = __attribute__((ext_vector_type(4))) float;
using u4 = __attribute__((ext_vector_type(4))) uint32_t;
using u2 = __attribute__((ext_vector_type(2))) uint32_t;

// elements k .. k + 7 of a row, zero at and beyond lim (lim = 0: nothing is read)
__device__ __forceinline__ h8 ld8(const _Float16* row, int64_t k, int64_t lim, bool al) {
    if (al && k + 8 <= lim) return *reinterpret_cast<const h8*>(row + k);
    h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (k < lim) {  // a ragged end or an unaligned row: element by element
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k + j < lim) v[j] = row[k + j];
    }
    return v;
}

// fp16 magic numbers: 0x6400 | f is 1024 + f for a 10-bit field f, so a code field left where
// it sits in the word (f = code << sh) becomes 1024 + (code << sh); one multiply by 2^-sh and
// one subtraction of (1024 >> sh) + k, both exact in fp16, give code - k.
__device__ __forceinline__ uint32_t pair(uint32_t uu, uint32_t mask) { return (uu & mask) | 0x64006400u; }
__device__ __forceinline__ uint32_t scale_off(uint32_t p, h2 sc, h2 off) {
    const h2 v = __builtin_bit_cast(h2, p) * sc + off;
    return __builtin_bit_cast(uint32_t, v);
}

// 8 consecutive codes (offset-binary, MSB-first) as fp16: 2-bit from the low (hi = 0) or high 16
// bits of `word`, 4-bit from all of it
template <int BITS>
__device__ __forceinline__ h8 expand(uint32_t word, int hi) {
    u4 o;
    if constexpr (BITS == 2) {
        // both halves hold the fragment's two bytes
        uint32_t uu = hi ? ((word >> 16) | (word & 0xffff0000u)) : ((word & 0xffffu) | (word << 16));
        const h2 sa = {(_Float16)(1.0f / 64), (_Float16)(1.0f / 16)}, oa = {(_Float16)-17.0f, (_Float16)-65.0f};
        const h2 sb = {(_Float16)0.25f, (_Float16)1.0f}, ob = {(_Float16)-257.0f, (_Float16)-1025.0f};
        o[0] = scale_off(pair(uu, 0x003000C0u), sa, oa);
        o[1] = scale_off(pair(uu, 0x0003000Cu), sb, ob);
        uu >>= 8;
        o[2] = scale_off(pair(uu, 0x003000C0u), sa, oa);
        o[3] = scale_off(pair(uu, 0x0003000Cu), sb, ob);
    } else {
        const uint32_t u0 = (word & 0xffffu) | (word << 16), u1 = (word >> 16) | (word & 0xffff0000u);
        const h2 sa = {(_Float16)(1.0f / 16), (_Float16)1.0f}, oa = {(_Float16)-71.0f, (_Float16)-1031.0f};
        o[0] = scale_off(pair(u0, 0x000F00F0u), sa, oa);
        o[1] = scale_off(pair(u0 >> 8, 0x000F00F0u), sa, oa);
        o[2] = scale_off(pair(u1, 0x000F00F0u), sa, oa);
        o[3] = scale_off(pair(u1 >> 8, 0x000F00F0u), sa, oa);
    }
    return __builtin_bit_cast(h8, o);
}

}  // namespace
}  // namespace cq
