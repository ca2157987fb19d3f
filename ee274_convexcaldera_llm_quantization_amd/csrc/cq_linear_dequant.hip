// Packed linear layer, materialise (cq_linear_dequant): the dense weight W = gs (Q + L R) of one
// compressed layer from its packed form, for callers that want the tuned dense GEMM at long
// prefill or a plain nn.Linear back.
//
//   W[i, j] = gs * (qs * V(code[i, j]) + fscale * sum_q lam[i, q] rho[q, j])        i < m, j < n
//
// The kernel is write-bound (33.6 MB out against 6.3 MB in at 4096^2, 2-bit, r = 128), so the tile
// is laid out for the stores.  Each 16 x 16 v_mfma_f32_16x16x32_f16 tile is computed TRANSPOSED,
// D = rho^T lam^T: the A fragment is 8 consecutive q at one column j, the B fragment 8 consecutive
// q of one L row, and D's rows run along j, so a lane ends up with 4 consecutive columns of one W
// row: one 8-byte (fp16 / bf16) or 16-byte (fp32) store.
//   - The B fragment is contiguous in memory: 16 bytes of an fp16 L row, 4 / 2 bytes of L codes
//     expanded with the backward's magic numbers.  It comes straight from global memory.
//   - The A fragment is a strided gather in R (r x n, row-major along j): the workgroup stages R in
//     chunks of 32 rows x 128 columns through the LDS image of cq_linear_tile.h (row loads, codes
//     expanded on the way in, rows >= r written as zeros) and reads it back with
//     ds_read_b64_tr_b16, exactly as cq_linear_bwd.hip reads its operands.  Two images form a
//     ring; one barrier per chunk.
// A workgroup of 4 waves owns kTileRows = 128 rows x 128 columns; a wave owns kRT = 2 tiles of 16
// rows x all 128 columns (64 accumulator registers).  Rows past m take part in every step (the
// barriers and the transposed reads need all lanes) with a zero L and are not stored.
//
// The Q term is not an MFMA operand: after the factor product the lane decodes the 4 codes under
// its 4 outputs -- 2 bytes at 4-bit, 1 byte at 2-bit, loaded before the product so the latency
// hides under it -- with expand<BITS> (uniform) or the LDS level table of cq_nf.h (NF; NF2's level
// is hi + sign, exact in fp32), and finishes each output in fp32:
//
//   f = fscale * acc          (not made when neither factor is coded: f = acc)
//   t = fma(qs, V, f)
//   w = gs * t                then one rounding to fp16 / bf16 (nearest even) where asked
#include <cmath>
#include <cstdio>

#include "cq_linear_host.h"
#include "cq_linear_tile.h"

namespace cq {
namespace {

constexpr int kWaves = 4;                       // waves per workgroup, each with its own rows
constexpr int kRT = 2;                          // 16-row tiles per wave
constexpr int kTileRows = kWaves * kRT * 16;    // 128 rows x kCols = 128 columns per workgroup

struct DqP {
    int64_t m, n, r;
    const uint8_t* codes; int64_t code_stride;
    const void* L; int64_t lstride; int l_al;   // fp16: elements, codes: bytes
    Src R;
    float qs, gs, fscale;
    void* w; int64_t ldw; int w_al;             // w_al: every 4-column piece of every row is aligned to its store
};

// 8 consecutive q of L row i from q0 on: fp16 elements (zero at q >= r) or expanded codes (a piece
// that starts inside r lies inside the 16-byte padded row; what it holds at q >= r meets R's zero rows)
template <int WL>
__device__ __forceinline__ h8 load_l(const DqP& p, int64_t i, int64_t q0) {
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (WL == 16) {
        const _Float16* row = reinterpret_cast<const _Float16*>(p.L) + (i < p.m ? i : 0) * p.lstride;
        return ld8(row, q0, i < p.m ? p.r : 0, p.l_al);
    } else {
        if (i >= p.m || q0 >= p.r) return zero;
        const uint8_t* row = reinterpret_cast<const uint8_t*>(p.L) + i * p.lstride;
        if constexpr (WL == 4) return expand<4>(*reinterpret_cast<const uint32_t*>(row + q0 / 2), 0);
        return expand<2>(*reinterpret_cast<const uint16_t*>(row + q0 / 4), 0);
    }
}

// the 4 codes at columns j .. j + 3 (j a multiple of 4) of a code row: 2 bytes at 4-bit, 1 at 2-bit
template <int BITS>
__device__ __forceinline__ uint32_t load_codes(const uint8_t* row, int64_t j) {
    if constexpr (BITS == 4) return *reinterpret_cast<const uint16_t*>(row + j / 2);
    return row[j / 4];
}

// their values V as fp32: u - k (uniform) or the integer level I[idx] (NF)
template <int BITS, bool NF>
__device__ __forceinline__ f4 code_values(uint32_t c, const uint32_t* nftab) {
    h8 v;
    if constexpr (NF) {
        // a byte's levels: the table entry of that byte (NF2: the hi plane, the level is hi + sign)
        v = expand_nf<BITS>(nftab, c, 0);
        if constexpr (BITS == 2) {
            const h8 lo = nf2_lo(v);
            return f4{(float)v[0] + (float)lo[0], (float)v[1] + (float)lo[1], (float)v[2] + (float)lo[2],
                      (float)v[3] + (float)lo[3]};
        }
    } else {
        v = expand<BITS>(c, 0);
    }
    return f4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

__device__ __forceinline__ uint16_t bf16_bits(float v) {
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);  // NaN stays NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                     // nearest even
}

// 4 consecutive outputs of one row, the first `cnt` of them inside n
template <int DT>
__device__ __forceinline__ void store4(const DqP& p, int64_t i, int64_t j, f4 v, int cnt) {
    if constexpr (DT == CQ_F32) {
        float* dst = reinterpret_cast<float*>(p.w) + i * p.ldw + j;
        if (cnt == 4 && p.w_al) {
            *reinterpret_cast<f4*>(dst) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cnt) dst[e] = v[e];
        }
    } else {
        uint16_t h[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (DT == CQ_F16) h[e] = __builtin_bit_cast(uint16_t, (_Float16)v[e]);
            else h[e] = bf16_bits(v[e]);
        }
        uint16_t* dst = reinterpret_cast<uint16_t*>(p.w) + i * p.ldw + j;
        if (cnt == 4 && p.w_al) {
            *reinterpret_cast<u2*>(dst) = u2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cnt) dst[e] = h[e];
        }
    }
}

// BITS / NF: the layer's codes; WL / WR: L and R as fp16 (16) or codes (2 / 4); DT: the output type
template <int BITS, bool NF, int WL, int WR, int DT>
__global__ __launch_bounds__(kWaves * 64) void linear_dequant_kernel(const DqP p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][kImageBytes];
    const uint32_t* nftab = nullptr;
    if constexpr (NF) {  // complete before the first lookup: the barriers of the chunk loop or the one below
        __shared__ uint32_t tab[BITS == 4 ? 256 : 512];
        fill_nf_table<BITS>(tab, threadIdx.x, kWaves * 64);
        nftab = tab;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * kTileRows + wave * (kRT * 16);
    const int64_t col0 = (int64_t)blockIdx.y * kCols;

    // the codes under the lane's outputs: row row0 + 16 rt + li, columns col0 + 16 b + 4 g ... + 3
    uint32_t qc[kRT][kBlocks];
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt) {
        const int64_t i = row0 + rt * 16 + li;
#pragma unroll
        for (int b = 0; b < kBlocks; ++b) {
            const int64_t j = col0 + b * 16 + g * 4;
            qc[rt][b] = i < p.m && j < p.n ? load_codes<BITS>(p.codes + i * p.code_stride, j) : 0u;
        }
    }

    f4 acc[kRT][kBlocks];
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int b = 0; b < kBlocks; ++b) acc[rt][b] = f4{0.f, 0.f, 0.f, 0.f};

    const int64_t nchunks = (p.r + kChunkRows - 1) / kChunkRows;
    if (nchunks > 0) {  // uniform
        const int frow = tid >> 3, fblock = tid & 7;  // the thread's piece of a chunk of R
        const int64_t fcol = col0 + fblock * 16;
        // transposed read: lane 4 q + p of group g supplies row 8 g + 4 h + q, columns 4 p ... + 3
        const int roff = (((li >> 2) | ((g & 1) << 2) | ((g >> 1) << 4)) * 32) + (li & 3) * 8;
        Raw w = fetch<WR, false>(p.R, frow, fcol);
        to_lds<WR, false>(w, lds[0], frow, fblock, nullptr);
        if (nchunks > 1) w = fetch<WR, false>(p.R, kChunkRows + frow, fcol);
        h8 lf[kRT], ln[kRT];
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) lf[rt] = load_l<WL>(p, row0 + rt * 16 + li, g * 8);
        __syncthreads();
        for (int64_t c = 0; c < nchunks; ++c) {  // ascending q
            const unsigned char* cur = lds[c & 1];
            if (c + 1 < nchunks) {
                to_lds<WR, false>(w, lds[(c + 1) & 1], frow, fblock, nullptr);
                if (c + 2 < nchunks) w = fetch<WR, false>(p.R, (c + 2) * kChunkRows + frow, fcol);
#pragma unroll
                for (int rt = 0; rt < kRT; ++rt) ln[rt] = load_l<WL>(p, row0 + rt * 16 + li, (c + 1) * kChunkRows + g * 8);
            }
#pragma unroll
            for (int b = 0; b < kBlocks; ++b) {
                const h4 a0 = tr_read(cur + b * kBlockBytes + roff), a1 = tr_read(cur + b * kBlockBytes + roff + 256);
                const h8 af = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
#pragma unroll
                for (int rt = 0; rt < kRT; ++rt)
                    acc[rt][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, lf[rt], acc[rt][b], 0, 0, 0);
            }
            if (c + 1 < nchunks) {
#pragma unroll
                for (int rt = 0; rt < kRT; ++rt) lf[rt] = ln[rt];
            }
            __syncthreads();  // the image of chunk c is free for chunk c + 2, that of c + 1 complete
        }
    } else if constexpr (NF) {
        __syncthreads();  // the level table
    }

    // D tile (transposed): W row = lane & 15, columns 4 (lane >> 4) + register
    constexpr bool kScaled = WL != 16 || WR != 16;
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt) {
        const int64_t i = row0 + rt * 16 + li;
        if (i >= p.m) continue;
#pragma unroll
        for (int b = 0; b < kBlocks; ++b) {
            const int64_t j = col0 + b * 16 + g * 4;
            if (j >= p.n) continue;
            const f4 v = code_values<BITS, NF>(qc[rt][b], nftab);
            f4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float f = kScaled ? p.fscale * acc[rt][b][e] : acc[rt][b][e];
                o[e] = p.gs * __builtin_fmaf(p.qs, v[e], f);
            }
            const int64_t left = p.n - j;
            store4<DT>(p, i, j, o, left >= 4 ? 4 : (int)left);
        }
    }
}

int validate(const cq_linear_dequant_args* a, const char* who) {
    CQ_REQUIRE(a != nullptr, "%s: null args", who);
    CQ_REQUIRE(a->bits == 2 || a->bits == 4, "%s: bits %d not in {2, 4}", who, a->bits);
    if (int st = validate_format(who, a->q_format, a->qscale)) return st;
    if (int st = validate_factor_bits(who, a->l_bits, a->r_bits)) return st;
    CQ_REQUIRE(a->m >= 0 && a->n >= 0 && a->r >= 0, "%s: bad shape m=%lld n=%lld r=%lld", who, (long long)a->m,
               (long long)a->n, (long long)a->r);
    if (int st = validate_rank(who, a->r)) return st;
    CQ_REQUIRE(a->m <= ((int64_t)1 << 31) && a->n <= (int64_t)65535 * kCols, "%s: shape too large", who);
    CQ_REQUIRE(a->w_dtype == CQ_F32 || a->w_dtype == CQ_F16 || a->w_dtype == CQ_BF16,
               "%s: w dtype %d not fp32 / fp16 / bf16", who, a->w_dtype);
    CQ_REQUIRE(a->ldw >= a->n, "%s: leading dimension ldw %lld smaller than the row %lld", who, (long long)a->ldw,
               (long long)a->n);
    if (a->m == 0 || a->n == 0) return CQ_OK;
    const bool lcoded = a->r > 0 && coded(a->l_bits), rcoded = a->r > 0 && coded(a->r_bits);
    CQ_REQUIRE(a->codes && a->w, "%s: null codes / w", who);
    if (int st = validate_operands(a, who, lcoded, rcoded)) return st;
    // a coded factor's fp16 pointer and leading dimension are not looked at
    if (int st = validate_fp16_pointers(who, nullptr, lcoded || a->r == 0 ? nullptr : a->L,
                                        rcoded || a->r == 0 ? nullptr : a->R))
        return st;
    CQ_REQUIRE(!misaligned(a->w, a->w_dtype == CQ_F32 ? 3 : 1), "%s: misaligned w pointer", who);
    CQ_REQUIRE(a->r == 0 || ((lcoded || a->ldl >= a->r) && (rcoded || a->ldr >= a->n)),
               "%s: leading dimension smaller than the row", who);
    return CQ_OK;
}

template <int BITS, bool NF, int WL, int WR>
void launch_dt(const DqP& p, int w_dtype, hipStream_t s) {
    const dim3 grid((unsigned)ceil_div(p.m, kTileRows), (unsigned)ceil_div(p.n, kCols)), block(kWaves * 64);
    if (w_dtype == CQ_F32) hipLaunchKernelGGL((linear_dequant_kernel<BITS, NF, WL, WR, CQ_F32>), grid, block, 0, s, p);
    else if (w_dtype == CQ_F16) hipLaunchKernelGGL((linear_dequant_kernel<BITS, NF, WL, WR, CQ_F16>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((linear_dequant_kernel<BITS, NF, WL, WR, CQ_BF16>), grid, block, 0, s, p);
}

template <int BITS, bool NF, int WL>
void launch_r(const DqP& p, int r_bits, int w_dtype, hipStream_t s) {
    if (r_bits == 2) launch_dt<BITS, NF, WL, 2>(p, w_dtype, s);
    else if (r_bits == 4) launch_dt<BITS, NF, WL, 4>(p, w_dtype, s);
    else launch_dt<BITS, NF, WL, 16>(p, w_dtype, s);
}

template <int BITS, bool NF>
void launch_l(const DqP& p, int l_bits, int r_bits, int w_dtype, hipStream_t s) {
    if (l_bits == 2) launch_r<BITS, NF, 2>(p, r_bits, w_dtype, s);
    else if (l_bits == 4) launch_r<BITS, NF, 4>(p, r_bits, w_dtype, s);
    else launch_r<BITS, NF, 16>(p, r_bits, w_dtype, s);
}

}  // namespace
}  // namespace cq

using namespace cq;

extern "C" int cq_linear_dequant(const cq_linear_dequant_args* a, void* stream) {
    const char* who = "cq_linear_dequant";
    if (int st = validate(a, who)) return st;
    if (a->m == 0 || a->n == 0) return CQ_OK;
    const bool nf = a->q_format == CQ_QFMT_NF;
    const bool lcoded = a->r > 0 && coded(a->l_bits), rcoded = a->r > 0 && coded(a->r_bits);
    DqP p{};
    p.m = a->m, p.n = a->n, p.r = a->r;
    p.codes = a->codes, p.code_stride = a->code_stride;
    if (lcoded) p.L = a->L_codes, p.lstride = a->l_code_stride, p.l_al = 1;
    else p.L = a->L, p.lstride = a->ldl, p.l_al = a->r > 0 && al16(a->L, a->ldl);
    if (rcoded) p.R = Src{a->R_codes, a->r_code_stride, 1, a->r, a->n};
    else p.R = Src{a->R, a->ldr, a->r > 0 && al16(a->R, a->ldr), a->r, a->n};
    p.qs = code_scale(a->qscale, a->bits, nf);
    p.gs = a->gscale;
    p.fscale = factor_scale(a, lcoded, rcoded);
    p.w = a->w, p.ldw = a->ldw;
    // a lane's 4 columns start at a multiple of 4: one store when every row does too
    const uintptr_t piece = a->w_dtype == CQ_F32 ? 16 : 8;
    p.w_al = (reinterpret_cast<uintptr_t>(a->w) & (piece - 1)) == 0 && a->ldw % 4 == 0;
    const int l_bits = lcoded ? a->l_bits : 16, r_bits = rcoded ? a->r_bits : 16;
    hipStream_t s = as_stream(stream);
    if (nf) {
        if (a->bits == 2) launch_l<2, true>(p, l_bits, r_bits, a->w_dtype, s);
        else launch_l<4, true>(p, l_bits, r_bits, a->w_dtype, s);
    } else {
        if (a->bits == 2) launch_l<2, false>(p, l_bits, r_bits, a->w_dtype, s);
        else launch_l<4, false>(p, l_bits, r_bits, a->w_dtype, s);
    }
    return check_launch(who);
}
