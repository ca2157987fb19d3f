// Device helpers shared by the kernels that contract over the ROWS of a packed-layer operand
// (cq_linear_bwd.hip: dx = dy W; cq_linear_dequant.hip: W itself, R's rows against L): the
// masked row-piece loader and the LDS image of a 32-row x 128-column chunk that is written
// row-wise, codes expanded by cq_codes.h on the way in, and read back with ds_read_b64_tr_b16.
//
// LDS image of a chunk: 8 blocks of 16 columns, each 32 rows of 32 bytes, block stride 1040
// bytes.  Row i sits at position prow(i) = i with bits 2 and 3 swapped, so the two 4-row blocks
// that a 32-lane half reads (rows 8g + 4h .. + 3 of lane groups g = 0, 1 resp. 2, 3) are 8
// consecutive 32-byte rows: 64 distinct banks, conflict-free.  The 16 bytes past each block
// spread a wave's 16-byte writes over all banks.
//
// Everything sits in an unnamed namespace and is force-inlined: each including file compiles its
// own copy into its own kernels.
#pragma once

#include "cq_codes.h"
#include "cq_common.h"
#include "cq_nf.h"

namespace cq {
namespace {

constexpr int kBlocks = 8;           // 16-column blocks per workgroup: 128 columns
constexpr int kCols = kBlocks * 16;
constexpr int kChunkRows = 32;            // weight rows per chunk: one MFMA k step
constexpr int kBlockBytes = kChunkRows * 32 + 16;
constexpr int kImageBytes = kBlocks * kBlockBytes;

// a weight operand whose rows are contracted: W = 2 / 4 packed codes (stride in bytes), 16 = fp16
// (stride in elements).  Rows >= rows and, for fp16, columns >= cols are not read and count as 0;
// a code piece that starts inside cols lies inside the 16-byte padded row.
struct Src {
    const void* base; int64_t stride; int al;
    int64_t rows, cols;
};

// what one thread holds of a chunk: 16 consecutive columns of one row, as loaded
struct Raw { u4 a, b; };

// FULL: the piece lies inside the operand and, for fp16, takes aligned 16-byte loads (the caller
// knows): no branch
template <int W, bool FULL>
__device__ __forceinline__ Raw fetch(const Src& s, int64_t row, int64_t col) {
    Raw w;
    w.a = w.b = u4{0u, 0u, 0u, 0u};
    if constexpr (FULL && W == 16) {
        const u4* p = reinterpret_cast<const u4*>(reinterpret_cast<const _Float16*>(s.base) + row * s.stride + col);
        w.a = p[0], w.b = p[1];
    } else if constexpr (FULL) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(s.base) + row * s.stride + col * W / 8;
        if constexpr (W == 2) {
            w.a[0] = *reinterpret_cast<const uint32_t*>(p);
        } else {
            const u2 v = *reinterpret_cast<const u2*>(p);
            w.a[0] = v[0], w.a[1] = v[1];
        }
        w.b[0] = 1u;
    } else if constexpr (W == 16) {
        const _Float16* p = reinterpret_cast<const _Float16*>(s.base) + (row < s.rows ? row : 0) * s.stride;
        const int64_t lim = row < s.rows ? s.cols : 0;
        w.a = __builtin_bit_cast(u4, ld8(p, col, lim, s.al));
        w.b = __builtin_bit_cast(u4, ld8(p, col + 8, lim, s.al));
    } else if (row < s.rows && col < s.cols) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(s.base) + row * s.stride + col * W / 8;
        if constexpr (W == 2) {
            w.a[0] = *reinterpret_cast<const uint32_t*>(p);
        } else {
            const u2 v = *reinterpret_cast<const u2*>(p);
            w.a[0] = v[0], w.a[1] = v[1];
        }
        w.b[0] = 1u;  // loaded: all-zero bits are code -k, not 0
    }
    return w;
}

// position of row i in a block: bits 2 and 3 swapped
__device__ __forceinline__ int prow(int i) { return (i & 0x13) | ((i & 4) << 1) | ((i & 8) >> 1); }

// nftab: the level table when the codes are level indices (NF), else unused
template <int W, bool NF>
__device__ __forceinline__ void to_lds(const Raw& w, unsigned char* image, int row, int block, const uint32_t* nftab) {
    h8 lo, hi;
    if constexpr (W == 16) {
        lo = __builtin_bit_cast(h8, w.a), hi = __builtin_bit_cast(h8, w.b);
    } else if constexpr (NF) {
        lo = expand_nf<W>(nftab, w.a[0], 0);
        hi = W == 2 ? expand_nf<W>(nftab, w.a[0], 1) : expand_nf<W>(nftab, w.a[1], 0);
        if (!w.b[0]) lo = hi = h8{0, 0, 0, 0, 0, 0, 0, 0};
    } else {
        lo = expand<W>(w.a[0], 0), hi = W == 2 ? expand<W>(w.a[0], 1) : expand<W>(w.a[1], 0);
        if (!w.b[0]) lo = hi = h8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    h8* dst = reinterpret_cast<h8*>(image + block * kBlockBytes + prow(row) * 32);
    dst[0] = lo, dst[1] = hi;
}

// rows r .. r + 3 of the block at column (lane & 15), from the addresses of the 16-lane group
__device__ __forceinline__ h4 tr_read(const unsigned char* p) {
    typedef __fp16 raw4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
    return __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) raw4*)(p)));
}

}  // namespace
}  // namespace cq
