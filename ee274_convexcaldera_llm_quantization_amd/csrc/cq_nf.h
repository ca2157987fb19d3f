// NF4 / NF2 level tables of the packed linear kernels (cq_linear.hip, cq_linear_bwd.hip): the one
// definition of the integer levels I = D level of the codebook contract (include/caldera_hip.h),
// their byte-indexed LDS table and its lookup.  tests/test_linear_codebook_host.py holds these
// integers against the NF quantiser's levels (cq_codebook.hip) and against _lib.NF_LEVELS.
#pragma once

#include "cq_common.h"

namespace cq {

using nf_h8 = __attribute__((ext_vector_type(8))) _Float16;
using nf_h2 = __attribute__((ext_vector_type(2))) _Float16;
using nf_u4 = __attribute__((ext_vector_type(4))) uint32_t;
using nf_u2 = __attribute__((ext_vector_type(2))) uint32_t;

// NF levels as integers: 1000 level (NF4), the hi plane of 10000 level (NF2: 8165 = 8164 + 1,
// 3333 = 3332 + 1; the lo plane is the level's sign).  All exact in fp16.
static __constant__ short kNF4I[16] = {-1334, -1000, -784, -617, -476, -347, -226, -112,
                                       0,     112,   226,  347,  476,  617,  784,  1000};
static __constant__ short kNF2Hi[4] = {-8164, -3332, 3332, 8164};
constexpr float kNF4D = 1000.f, kNF2D = 10000.f;

__device__ __forceinline__ uint32_t nf_h2bits(int a, int b) {
    const nf_h2 v = {(_Float16)(float)a, (_Float16)(float)b};
    return __builtin_bit_cast(uint32_t, v);
}

// the LDS table of one byte's indices (MSB-first): NF4 256 x 2 fp16, NF2 256 x 4 fp16 (hi plane);
// the caller puts a barrier between this and the first lookup
template <int BITS>
__device__ __forceinline__ void fill_nf_table(uint32_t* tab, int tid, int nthreads) {
    for (int e = tid; e < 256; e += nthreads) {
        if constexpr (BITS == 4) {
            tab[e] = nf_h2bits(kNF4I[e >> 4], kNF4I[e & 15]);
        } else {
            tab[2 * e] = nf_h2bits(kNF2Hi[e >> 6], kNF2Hi[(e >> 4) & 3]);
            tab[2 * e + 1] = nf_h2bits(kNF2Hi[(e >> 2) & 3], kNF2Hi[e & 3]);
        }
    }
}

// 8 consecutive level indices (MSB-first) as their fp16 integer levels (NF2: the hi plane) through
// the table: 2-bit from the low (hi = 0) or high 16 bits of `word`, 4-bit from all of it
template <int BITS>
__device__ __forceinline__ nf_h8 expand_nf(const uint32_t* tab, uint32_t word, int hi) {
    nf_u4 o;
    if constexpr (BITS == 4) {
        o[0] = tab[word & 0xffu];
        o[1] = tab[(word >> 8) & 0xffu];
        o[2] = tab[(word >> 16) & 0xffu];
        o[3] = tab[word >> 24];
    } else {
        const uint32_t half = hi ? word >> 16 : word & 0xffffu;
        const nf_u2 a = reinterpret_cast<const nf_u2*>(tab)[half & 0xffu];
        const nf_u2 b = reinterpret_cast<const nf_u2*>(tab)[half >> 8];
        o[0] = a[0], o[1] = a[1], o[2] = b[0], o[3] = b[1];
    }
    return __builtin_bit_cast(nf_h8, o);
}

// NF2's lo plane from the hi plane: +-1 with the level's sign (where the hi plane is a padded 0
// this gives +1, which only ever meets a zero of the other operand)
__device__ __forceinline__ nf_h8 nf2_lo(const nf_h8 hi) {
    nf_u4 v = __builtin_bit_cast(nf_u4, hi);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (v[i] & 0x80008000u) | 0x3C003C00u;
    return __builtin_bit_cast(nf_h8, v);
}

}  // namespace cq
