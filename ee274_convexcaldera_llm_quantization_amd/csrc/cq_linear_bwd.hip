// Packed linear layer, input gradient (cq_linear_backward_input): dx = dy (gs (Q + L R)) straight
// from the 2/4-bit codes and the fp16 factors, never forming the dense weight or its transpose.
//
//   dx[t, j] = gs * ((s / k) * sum_i dy[t, i] c[i, j] + sum_q u[t, q] R[q, j])
//   u[t, q]  = sum_i dy[t, i] L[i, q]
//
// All three products contract over the ROWS of their weight operand (codes, L, R), which are
// stored row-major along the other index, so the v_mfma_f32_16x16x32_f16 B fragment -- 8
// consecutive rows at one column -- is a strided gather in memory.  The transposition is done on
// chip: a workgroup takes a chunk of 32 weight rows x 128 columns with row loads (4 / 8 bytes of
// codes or 32 bytes of fp16 per thread), expands codes with the forward's magic numbers, writes
// the fp16 [row][column] tile to LDS and reads it back with ds_read_b64_tr_b16.  Rows past the
// operand's end are written as zeros (pad, don't mask: the transposed read needs every lane).
//
// LDS image of a chunk: 8 blocks of 16 columns, each 32 rows of 32 bytes, block stride 1040
// bytes.  Row i sits at position prow(i) = i with bits 2 and 3 swapped, so the two 4-row blocks
// that a 32-lane half reads (rows 8g + 4h .. + 3 of lane groups g = 0, 1 resp. 2, 3) are 8
// consecutive 32-byte rows: 64 distinct banks, conflict-free.  The 16 bytes past each block
// spread a wave's 16-byte writes over all banks.  Two images form a ring: chunk c + 1 is
// expanded and written, and chunk c + 2 loaded, under the MFMAs of chunk c; one barrier per chunk.
//
// Two launches of the same kernel: u = dy L (skipped for r = 0; writes the fp32 u_out and the
// split fp16 halves), then codes, scaled by s / k in the accumulator, + the halves times R +
// epilogue.  A wave owns TT tiles of 16 tokens x all 128 columns of its workgroup; tokens are the
// A rows, read from memory with the forward's masked loader.  One dispatch branch: the summation
// order of an output does not depend on the token count.
//
// Factor codes (cq_linear_packed_backward_input): L and / or R as packed 2/4-bit codes with one
// scale each, in the inference layout of the layer's own codes.  Both are contracted over their rows
// like the Q codes, so they take the same chunk walk: W = 2 / 4 in the u product (rows m, columns
// r), and a second width for the main kernel's R stage (rows r, columns n).  u~ = uscale * sum_i dy
// lam with uscale the fp32 product of the coded factors' scale / k, applied once to the complete
// fp32 sum in the u epilogue before the split; a 16-column piece of L codes that straddles r expands
// whatever the tail holds, so that epilogue writes zero halves for q >= r, and R's rows >= r are
// written to LDS as zeros like any row past an operand's end.  cq_linear_backward_input is this path
// with fp16 factors and uscale = 1.
//
// Codebook Q (cq_linear_codebook_backward_input, CQ_QFMT_NF): the layer's codes are NF4 / NF2 level
// indices, the Q term (s / D) * sum_i dy[t, i] I[idx[i, j]] (cq_linear.hip's header).  The chunk walk
// is the same; `to_lds` expands a piece through the byte-indexed LDS level table of cq_nf.h (shared with the forward) instead
// of the magic numbers.  NF2: the image holds the hi plane; the lo plane (+-1, the level's sign) is
// made from the transposed fragment in registers and multiplied into the same accumulator after
// it.  A zero row past the operand's end becomes +1 there and meets dy's zero.
#include <cmath>
#include <cstdio>
#include <type_traits>

#include "cq_common.h"
#include "cq_linear_host.h"
#include "cq_nf.h"
// the chunk image, its loaders and the code expansion: shared with cq_linear_dequant.hip
#include "cq_linear_tile.h"

namespace cq {
namespace {

constexpr int kWaves = 4;            // waves per workgroup, each with its own tokens
constexpr int kRows = 32;            // weight rows per chunk: one MFMA k step
static_assert(kRows == kChunkRows, "the chunk image of cq_linear_tile.h");
constexpr int kTilesMain = 2;        // 16-token tiles per wave: codes + R
constexpr int kTilesU = 1;           // ... the u product (r / 128 column tiles only: more workgroups)

// acc[tt][b] += A (tokens x rows of s) * s[:, col0 + 16 b ...] over all rows of s in chunks of 32.
// load_a(c, tt, a, full): the NA A fragments (rows 32 c + 8 g ... + 7 of the lane's token) that are
// multiplied, in order, with the same B fragment.  Every thread of the workgroup takes every
// step (the barriers and the transposed reads need all lanes).
//
// The masked loaders branch per lane, and at the join of that control flow the compiler waits for
// all loads in flight -- in front of the MFMAs of the chunk before the one they are for.  So the
// chunks whose prefetches need no mask (afull: all the workgroup's tokens exist and their rows are
// aligned; the tile's 128 columns inside the operand; whole chunks of rows) run in a loop of their
// own, compiled without the masks (full = true_type); the masked loop takes the rest.
// NF: s holds NF level indices, expanded through nftab (W = 2: two planes per B fragment).
template <int W, int TT, int NA, bool NF, class LoadA>
__device__ __forceinline__ void product(f4 (&acc)[TT][kBlocks], unsigned char (*lds)[kImageBytes], const Src& s,
                                        int64_t col0, bool afull, LoadA load_a, const uint32_t* nftab = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int li = lane & 15, g = lane >> 4;
    const int frow = tid >> 3, fblock = tid & 7;  // the thread's piece of a chunk
    const int64_t fcol = col0 + fblock * 16;
    // transposed read: lane 4 q + p of group g supplies row 8 g + 4 h + q, columns 4 p ... + 3
    const int roff = (((li >> 2) | ((g & 1) << 2) | ((g >> 1) << 4)) * 32) + (li & 3) * 8;
    const int64_t nchunks = (s.rows + kRows - 1) / kRows;
    const bool tile_full = afull && (W == 16 ? s.al && col0 + kCols <= s.cols : col0 + kCols - 16 < s.cols);
    const int64_t nfull = tile_full ? s.rows / kRows : 0;  // whole chunks of a tile without masks

    Raw w = fetch<W, false>(s, frow, fcol);
    to_lds<W, NF>(w, lds[0], frow, fblock, nftab);
    if (nchunks > 1) w = fetch<W, false>(s, kRows + frow, fcol);
    h8 a[TT][NA], an[TT][NA];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) load_a(0, tt, a[tt], std::false_type{});
    __syncthreads();
    // chunks [cb, ce); full: chunks c + 1 and c + 2 exist and need no mask
    auto run = [&](auto full, int64_t cb, int64_t ce) {
        constexpr bool FULL = decltype(full)::value;
        for (int64_t c = cb; c < ce; ++c) {
            const unsigned char* cur = lds[c & 1];
            if (FULL || c + 1 < nchunks) {
                to_lds<W, NF>(w, lds[(c + 1) & 1], frow, fblock, nftab);
                if (FULL || c + 2 < nchunks) w = fetch<W, FULL>(s, (c + 2) * kRows + frow, fcol);
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) load_a(c + 1, tt, an[tt], full);
            }
#pragma unroll
            for (int b = 0; b < kBlocks; ++b) {
                const h4 b0 = tr_read(cur + b * kBlockBytes + roff), b1 = tr_read(cur + b * kBlockBytes + roff + 256);
                const h8 bf = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
                for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                    for (int ia = 0; ia < NA; ++ia)
                        acc[tt][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[tt][ia], bf, acc[tt][b], 0, 0, 0);
                if constexpr (NF && W == 2) {
                    const h8 bl = nf2_lo(bf);
#pragma unroll
                    for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                        for (int ia = 0; ia < NA; ++ia)
                            acc[tt][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[tt][ia], bl, acc[tt][b], 0, 0, 0);
                }
            }
            if (FULL || c + 1 < nchunks) {
#pragma unroll
                for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                    for (int ia = 0; ia < NA; ++ia) a[tt][ia] = an[tt][ia];
            }
            __syncthreads();  // the image of chunk c is free for chunk c + 2, that of c + 1 complete
        }
    };
    const int64_t cmid = nfull > 2 ? nfull - 2 : 0;
    run(std::true_type{}, 0, cmid);
    run(std::false_type{}, cmid, nchunks);
}

struct BwdP {
    const _Float16* dy; int64_t lddy; int dy_al;
    int64_t T, m, n, r, r32;
    Src w;                                   // u product: L; else the codes
    Src R;
    _Float16* uh; _Float16* ul;              // [T][r32] halves of u: written by the u product, read by the other
    float* u_out; int64_t ldu;
    float sk, gs;
    float uscale;                            // on the complete u sum, before it is split (1 without factor codes)
    void* dx; int dx_f16; int64_t lddx;
};

// UK: the u product (W: L's rows, fp16 or codes), else codes (W = 2 / 4) + R (WR: fp16 or codes) +
// epilogue; QF: the layer's codes are uniform codes or NF level indices
template <int W, int QF, int WR, bool UK, int TT>
__global__ __launch_bounds__(kWaves * 64) void linear_bwd_kernel(const BwdP p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][kImageBytes];
    constexpr bool NF = QF == CQ_QFMT_NF;
    static_assert(!NF || (!UK && W != 16), "only the layer's own codes are level indices");
    const uint32_t* nftab = nullptr;
    if constexpr (NF) {  // complete before the first chunk is expanded
        __shared__ uint32_t tab[W == 4 ? 256 : 512];
        fill_nf_table<W>(tab, threadIdx.x, kWaves * 64);
        __syncthreads();
        nftab = tab;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int64_t tok0 = ((int64_t)blockIdx.x * kWaves + wave) * (TT * 16);
    const int64_t col0 = (int64_t)blockIdx.y * kCols;

    f4 acc[TT][kBlocks];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
#pragma unroll
        for (int b = 0; b < kBlocks; ++b) acc[tt][b] = f4{0.f, 0.f, 0.f, 0.f};

    // all of the workgroup's tokens exist (uniform)
    const bool tokfull = ((int64_t)blockIdx.x + 1) * (kWaves * TT * 16) <= p.T;
    // dy columns >= m and rows >= T are not read; full: a whole chunk of an existing, aligned row
    auto load_dy = [&](int64_t c, int tt, h8 (&a)[1], auto full) {
        const int64_t t = tok0 + tt * 16 + li;
        if constexpr (decltype(full)::value)
            a[0] = *reinterpret_cast<const h8*>(p.dy + t * p.lddy + c * kRows + g * 8);
        else
            a[0] = ld8(p.dy + (t < p.T ? t : 0) * p.lddy, c * kRows + g * 8, t < p.T ? p.m : 0, p.dy_al);
    };
    product<W, TT, 1, NF>(acc, lds, p.w, col0, tokfull && p.dy_al, load_dy, nftab);

    if constexpr (!UK) {
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int b = 0; b < kBlocks; ++b) acc[tt][b] = acc[tt][b] * p.sk;  // s / k once per output
        if (p.r > 0) {  // uniform
            // u as split halves, lo first as the forward's L product takes z; rows >= T read as zero
            auto load_u = [&](int64_t c, int tt, h8 (&a)[2], auto full) {
                const int64_t t = tok0 + tt * 16 + li;
                const int64_t o = (t < p.T ? t : 0) * p.r32;
                if constexpr (decltype(full)::value) {
                    a[0] = *reinterpret_cast<const h8*>(p.ul + o + c * kRows + g * 8);
                    a[1] = *reinterpret_cast<const h8*>(p.uh + o + c * kRows + g * 8);
                } else {
                    a[0] = ld8(p.ul + o, c * kRows + g * 8, t < p.T ? p.r32 : 0, true);
                    a[1] = ld8(p.uh + o, c * kRows + g * 8, t < p.T ? p.r32 : 0, true);
                }
            };
            product<WR, TT, 2, false>(acc, lds, p.R, col0, tokfull, load_u);
        }
    }

    // D tile: column = lane & 15, row (token) = 4 (lane >> 4) + register
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
#pragma unroll
        for (int b = 0; b < kBlocks; ++b) {
            const int64_t j = col0 + b * 16 + li;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t t = tok0 + tt * 16 + g * 4 + e;
                if (t >= p.T) continue;
                if constexpr (UK) {
                    float v = acc[tt][b][e] * p.uscale;  // once, on the complete sum
                    // a piece of L codes that straddles r has expanded the row's tail
                    if constexpr (W != 16) v = j < p.r ? v : 0.f;
                    if (j < p.r && p.u_out) p.u_out[t * p.ldu + j] = v;
                    if (j < p.r32) {  // columns r .. r32 are zero: fp16 L is not read there
                        const _Float16 hi = (_Float16)v;
                        p.uh[t * p.r32 + j] = hi;
                        p.ul[t * p.r32 + j] = (_Float16)(v - (float)hi);
                    }
                } else if (j < p.n) {
                    const float v = p.gs * acc[tt][b][e];
                    if (p.dx_f16) reinterpret_cast<_Float16*>(p.dx)[t * p.lddx + j] = (_Float16)v;
                    else reinterpret_cast<float*>(p.dx)[t * p.lddx + j] = v;
                }
            }
        }
    }
}

// the halves of u: a function of tokens and r alone
size_t workspace_bytes(int64_t tokens, int64_t r) {
    if (r <= 0 || tokens <= 0) return 0;
    return (size_t)(2 * tokens * r32_of(r)) * sizeof(uint16_t);
}

int validate(const cq_linear_packed_backward_args* a, const char* who) {
    CQ_REQUIRE(a != nullptr, "%s: null args", who);
    CQ_REQUIRE(a->bits == 2 || a->bits == 4, "%s: bits %d not in {2, 4}", who, a->bits);
    if (int st = validate_factor_bits(who, a->l_bits, a->r_bits)) return st;
    const bool lcoded = a->r > 0 && coded(a->l_bits), rcoded = a->r > 0 && coded(a->r_bits);
    CQ_REQUIRE(a->tokens >= 0 && a->m > 0 && a->n > 0 && a->r >= 0, "%s: bad shape tokens=%lld m=%lld n=%lld r=%lld", who,
               (long long)a->tokens, (long long)a->m, (long long)a->n, (long long)a->r);
    if (int st = validate_rank(who, a->r)) return st;
    CQ_REQUIRE(a->tokens <= ((int64_t)1 << 31) && a->n <= (int64_t)65535 * kCols, "%s: shape too large", who);
    CQ_REQUIRE(a->dx_dtype == CQ_F32 || a->dx_dtype == CQ_F16, "%s: dx dtype %d not fp32 / fp16", who, a->dx_dtype);
    CQ_REQUIRE(a->dy && a->codes && a->dx, "%s: null dy / codes / dx", who);
    if (int st = validate_operands(a, who, lcoded, rcoded)) return st;
    // a coded factor's fp16 pointer and leading dimension are not looked at
    if (int st = validate_fp16_pointers(who, a->dy, lcoded ? nullptr : a->L, rcoded ? nullptr : a->R)) return st;
    CQ_REQUIRE(!misaligned(a->dx, a->dx_dtype == CQ_F16 ? 1 : 3) && !misaligned(a->u_out, 3),
               "%s: misaligned dx / u_out pointer", who);
    CQ_REQUIRE(a->lddy >= a->m && a->lddx >= a->n &&
                   (a->r == 0 || ((lcoded || a->ldl >= a->r) && (rcoded || a->ldr >= a->n) &&
                                  (a->u_out == nullptr || a->ldu >= a->r))),
               "%s: leading dimension smaller than the row", who);
    return CQ_OK;
}

// cq_linear_backward_args is the leading part of cq_linear_packed_backward_args: the same layer
// with fp16 factors
cq_linear_packed_backward_args with_fp16_factors(const cq_linear_backward_args* a) {
    cq_linear_packed_backward_args b{};
    b.dy = a->dy, b.lddy = a->lddy;
    b.tokens = a->tokens, b.m = a->m, b.n = a->n, b.r = a->r;
    b.bits = a->bits;
    b.codes = a->codes, b.code_stride = a->code_stride;
    b.qscale = a->qscale, b.gscale = a->gscale;
    b.L = a->L, b.ldl = a->ldl;
    b.R = a->R, b.ldr = a->ldr;
    b.dx = a->dx, b.dx_dtype = a->dx_dtype, b.lddx = a->lddx;
    b.u_out = a->u_out, b.ldu = a->ldu;
    b.l_bits = b.r_bits = 16;
    return b;
}

template <int W, int QF, int WR, bool UK, int TT>
void launch(const BwdP& p, int64_t cols, hipStream_t s) {
    const dim3 grid((unsigned)ceil_div(p.T, kWaves * TT * 16), (unsigned)ceil_div(cols, kCols));
    hipLaunchKernelGGL((linear_bwd_kernel<W, QF, WR, UK, TT>), grid, dim3(kWaves * 64), 0, s, p);
}

template <int W, int QF>
void launch_main(const BwdP& p, int r_bits, hipStream_t s) {
    if (r_bits == 2) launch<W, QF, 2, false, kTilesMain>(p, p.n, s);
    else if (r_bits == 4) launch<W, QF, 4, false, kTilesMain>(p, p.n, s);
    else launch<W, QF, 16, false, kTilesMain>(p, p.n, s);
}

int backward(const cq_linear_packed_backward_args* a, int q_format, void* ws, size_t ws_bytes, void* stream,
             const char* who) {
    if (int st = validate(a, who)) return st;
    if (int st = validate_format(who, q_format, a->qscale)) return st;
    const bool nf = q_format == CQ_QFMT_NF;
    // this entry reports a workspace that is too small as CQ_EINVAL
    if (int st = check_workspace(workspace_bytes(a->tokens, a->r), ws, ws_bytes, who, CQ_EINVAL)) return st;
    if (a->tokens == 0) return CQ_OK;
    const bool lcoded = a->r > 0 && coded(a->l_bits), rcoded = a->r > 0 && coded(a->r_bits);
    hipStream_t s = as_stream(stream);
    BwdP p{};
    p.dy = reinterpret_cast<const _Float16*>(a->dy);
    p.lddy = a->lddy;
    p.dy_al = al16(a->dy, a->lddy);
    p.T = a->tokens, p.m = a->m, p.n = a->n, p.r = a->r;
    p.r32 = r32_of(a->r);
    p.uh = reinterpret_cast<_Float16*>(ws);
    p.ul = p.uh ? p.uh + a->tokens * p.r32 : nullptr;
    p.uscale = factor_scale(a, lcoded, rcoded);
    if (a->r > 0) {  // u~ = uscale dy lam: fp32 to u_out, split halves to the workspace
        BwdP u = p;
        u.u_out = a->u_out;
        u.ldu = a->ldu;
        if (lcoded) {
            u.w = Src{a->L_codes, a->l_code_stride, 1, a->m, a->r};
            if (a->l_bits == 2) launch<2, CQ_QFMT_UNIFORM, 16, true, kTilesU>(u, p.r32, s);
            else launch<4, CQ_QFMT_UNIFORM, 16, true, kTilesU>(u, p.r32, s);
        } else {
            u.w = Src{a->L, a->ldl, al16(a->L, a->ldl), a->m, a->r};
            launch<16, CQ_QFMT_UNIFORM, 16, true, kTilesU>(u, p.r32, s);
        }
        char what[64];
        snprintf(what, sizeof what, "%s (u)", who);
        if (int st = check_launch(what)) return st;
    }
    p.w = Src{a->codes, a->code_stride, 1, a->m, a->n};
    if (rcoded) p.R = Src{a->R_codes, a->r_code_stride, 1, a->r, a->n};
    else p.R = Src{a->R, a->ldr, a->r > 0 && al16(a->R, a->ldr), a->r, a->n};
    p.sk = code_scale(a->qscale, a->bits, nf);
    p.gs = a->gscale;
    p.dx = a->dx;
    p.dx_f16 = a->dx_dtype == CQ_F16;
    p.lddx = a->lddx;
    const int r_bits = rcoded ? a->r_bits : 16;
    if (nf) {
        if (a->bits == 2) launch_main<2, CQ_QFMT_NF>(p, r_bits, s);
        else launch_main<4, CQ_QFMT_NF>(p, r_bits, s);
    } else {
        if (a->bits == 2) launch_main<2, CQ_QFMT_UNIFORM>(p, r_bits, s);
        else launch_main<4, CQ_QFMT_UNIFORM>(p, r_bits, s);
    }
    return check_launch(who);
}

}  // namespace
}  // namespace cq

using namespace cq;

extern "C" size_t cq_linear_backward_workspace(const cq_linear_backward_args* a) {
    return a == nullptr ? 0 : workspace_bytes(a->tokens, a->r);
}

extern "C" size_t cq_linear_packed_backward_workspace(const cq_linear_packed_backward_args* a) {
    return a == nullptr ? 0 : workspace_bytes(a->tokens, a->r);
}

extern "C" int cq_linear_backward_input(const cq_linear_backward_args* a, void* ws, size_t ws_bytes, void* stream) {
    CQ_REQUIRE(a != nullptr, "cq_linear_backward_input: null args");
    const cq_linear_packed_backward_args b = with_fp16_factors(a);
    return backward(&b, CQ_QFMT_UNIFORM, ws, ws_bytes, stream, "cq_linear_backward_input");
}

extern "C" int cq_linear_packed_backward_input(const cq_linear_packed_backward_args* a, void* ws, size_t ws_bytes,
                                               void* stream) {
    return backward(a, CQ_QFMT_UNIFORM, ws, ws_bytes, stream, "cq_linear_packed_backward_input");
}

extern "C" size_t cq_linear_codebook_backward_workspace(const cq_linear_codebook_backward_args* a) {
    return a == nullptr ? 0 : workspace_bytes(a->p.tokens, a->p.r);
}

extern "C" int cq_linear_codebook_backward_input(const cq_linear_codebook_backward_args* a, void* ws, size_t ws_bytes,
                                                 void* stream) {
    CQ_REQUIRE(a != nullptr, "cq_linear_codebook_backward_input: null args");
    return backward(&a->p, a->q_format, ws, ws_bytes, stream, "cq_linear_codebook_backward_input");
}
