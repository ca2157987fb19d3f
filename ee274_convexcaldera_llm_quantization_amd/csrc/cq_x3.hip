// Split-fp16 ("f16x3") products with the symmetric Gram G for the rank-r solver's
// Chebyshev filter (the dominant cost of the SVD replacing alg.py:217).
//
// Every fp32 operand x is carried as two fp16 halves, x*s = hi + lo with hi = f16(x*s) and
// lo = f16(x*s - hi) (s a power of two), so x*s is represented to 2^-22 relative.  A product
// sum_k a_k b_k is then hi_a hi_b + hi_a lo_b + lo_a hi_b (the dropped lo_a lo_b term is
// 2^-22 relative), each term one v_mfma_f32_16x16x32_f16 with fp32 accumulation: three fp16
// MFMAs give fp32-grade products (measured error at or below the fp32 MFMA GEMM's,
// DESIGN.md) on the fp16 matrix cores.
//
// Layout: the filter iterates on X^T (p x k, row-major) so both operands are K-contiguous:
//   C[j][i] = sum_k Xt[j][k] G[i][k]   ( = (G X)^T since G = G^T )
// gemm_x3v_kernel: tile 192 (rows of Xt) x 384 (rows of G) x 32, 768 threads = 12 waves of
// 96 x 64 (6 x 4 blocks of 16 x 16), operands global -> LDS by LDS-DMA into a ring of 2 to 4
// stages by product mode (144 KB; XRing in cq_x3_tile.h, which holds the LDS image, the loader
// and the K loop), XOR-swizzled 16-B chunks so fragment reads are conflict-free; the
// transposed MFMA operand order gives each lane 4 consecutive output columns for a vectorised
// epilogue (Chebyshev recurrence, split halves of the next iterate, or the Gram's mirrored
// K-blocked halves).
//
// The tiled fused Q update and residual_split, which share the tile, are in cq_qtile.hip; the
// split, transpose and scale helpers that make the operand halves in cq_split.hip.
#include "cq_x3_tile.h"

namespace cq {

// Split scale 2^(14 - e) of a symmetric Gram from the bound on max|C| in [2^(e-1), 2^e)
__device__ __forceinline__ float sym_split_scale(double bound) {
    int e = 0;
    if (bound > 0.0 && isfinite(bound)) frexp(bound, &e);
    return ldexpf(1.f, 14 - e);
}

// Gram tile order.  Only the tiles on or above the diagonal are launched: 384 x 384 blocks
// (I, J >= I) of tiles tm = 2I, 2I + 1 (192 rows) by tn = J.  The blocks are enumerated per
// matrix in 4 x 4 super-blocks (row-major over super-blocks, then over their blocks), and
// the launch index is dealt to the XCDs (workgroup i runs on XCD i % 8) in runs of
// GRAM_RUN consecutive tiles of that order: the 32 tiles an XCD holds at a time share 8 row
// and 4 column panels of Y instead of ~30 of each, so their K slices are re-read from the
// XCD's L2 rather than from the memory-side cache, and all XCDs stay on the same one or two
// matrices (whose operands fit that 256 MB cache).  The order changes nothing in a tile's
// arithmetic.
constexpr int GRAM_SB = 4, GRAM_RUN = 32;

__device__ __forceinline__ int64_t gram_block_tiles(int64_t I, int64_t tiles_m) {
    return 2 * I + 1 < tiles_m ? 2 : 1;
}

__device__ void gram_tile(const X3K& a, int64_t orig, int64_t& b, int64_t& tm, int64_t& tn) {
    const int64_t live = a.tiles_live, total = live * a.batch;
    constexpr int64_t S = 8 * GRAM_RUN;
    int64_t lin = orig;
    if (orig < total / S * S) {
        const int64_t k = orig / 8, x = orig % 8;
        lin = (k / GRAM_RUN) * S + x * GRAM_RUN + k % GRAM_RUN;
    }
    b = lin / live;
    int64_t j = lin % live;
    const int64_t nb = a.tiles_n, nsb = (nb + GRAM_SB - 1) / GRAM_SB;
    for (int64_t si = 0; si < nsb; ++si) {
        for (int64_t sj = si; sj < nsb; ++sj) {
            const int64_t i1 = min<int64_t>(GRAM_SB * si + GRAM_SB, nb), j1 = min<int64_t>(GRAM_SB * sj + GRAM_SB, nb);
            for (int64_t I = GRAM_SB * si; I < i1; ++I) {
                const int64_t per = gram_block_tiles(I, a.tiles_m);
                const int64_t jb = max<int64_t>(GRAM_SB * sj, I);
                const int64_t cnt = (j1 > jb ? j1 - jb : 0) * per;
                if (j < cnt) {
                    tn = jb + j / per;
                    tm = 2 * I + j % per;
                    return;
                }
                j -= cnt;
            }
        }
    }
    tm = tn = 0;  // unreachable for lin < total
}

// XM: 0 = three split products, 1 = one hi x hi product, 2 = exact B (two products, Bl unread)
template <int XM>
__global__ __launch_bounds__(XW_THREADS, 1) void gemm_x3v_kernel(X3K a) {
    extern __shared__ __attribute__((aligned(16))) char xv_smem_raw[];
    _Float16* smem = reinterpret_cast<_Float16*>(xv_smem_raw);
    int64_t tn, tm, b;
    if (a.sym_out) {
        gram_tile(a, blockIdx.x, b, tm, tn);
    } else {
        const int64_t total = a.tiles_n * a.tiles_m * a.batch;
        const int64_t orig = a.ksplit > 1 ? blockIdx.x / a.ksplit : blockIdx.x;   // split-K: chunk fastest
        const int64_t q = total / 8, r8 = total % 8, xcd = orig % 8;
        const int64_t lin = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + orig / 8;
        // row tiles fastest: when A has more than one 192-row tile (the filter at p > 192), the
        // tiles sharing one 384-row panel of B (G) run together on one XCD and read its K slices
        // once from HBM and again from L2
        tm = lin % a.tiles_m;
        tn = (lin / a.tiles_m) % a.tiles_n;
        b = lin / (a.tiles_n * a.tiles_m);
    }
    const int64_t m0 = tm * XW_BM, n0 = tn * XW_BN;
    if (a.tri && n0 + XW_BN <= m0) return;
    // skip form: an inactive matrix's workgroups leave before the ring prologue and write nothing
    // (C, C^T, the halves, the overflow flag and the split-K partials stay as they were)
    if (a.skip && !a.active[b]) return;

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid & 1, wn = wid >> 1;  // rows 96 wm .. +96, cols 64 wn .. +64
    const int l16 = lane & 15, lq = lane >> 4;

    f32x4v acc[6][4];
    const bool live = !a.active || a.active[b];
    const int64_t nk = a.K / XW_BK;
    int64_t kb = 0, kn = nk;
    if (a.ksplit > 1) {   // this workgroup's K chunk
        const int64_t ks = blockIdx.x % a.ksplit;
        kb = ks * nk / a.ksplit;
        kn = (ks + 1) * nk / a.ksplit - kb;
    }
    xr_mainloop<XM>(a, b, m0, n0, live ? kn : 0, smem, wid, lane, wm, wn, acc, kb);

    const float sc = a.inv_scale[b];
    if (a.ksplit > 1) {   // partial products (times the operand scale) for x3_splitk_epi_kernel
        float* part = a.part + ((blockIdx.x % a.ksplit) * a.batch + b) * a.M * a.N;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int64_t row = m0 + 96 * wm + 16 * i + l16;
            if (row >= a.M) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t col = n0 + 64 * wn + 16 * j + 4 * lq;
                if (col >= a.N) continue;
                // N % 4 == 0 (host check): 4 columns, 16-byte aligned
                *reinterpret_cast<float4*>(part + row * a.N + col) =
                    make_float4(acc[i][j][0] * sc, acc[i][j][1] * sc, acc[i][j][2] * sc, acc[i][j][3] * sc);
            }
        }
        return;
    }
    if (a.sym_out) {
        // symmetric Gram: entries on/above the diagonal are written at (row, col) and, mirrored,
        // at (col, row) of the K-blocked split (the lower triangle of a straddling tile is not
        // used, so the split is exactly symmetric); (fp32 C too if given)
        const float gs = sym_split_scale(a.out_bound[b]);
        if (tm == 0 && tn == 0 && threadIdx.x == 0) {
            a.scale_out[b] = gs;
            a.inv_out[b] = 1.f / (gs * a.out_scale);
        }
        const int64_t M = a.M;
        _Float16* Oh = a.Oh + b * a.so;
        _Float16* Ol = a.Ol + b * a.so;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int64_t row = m0 + 96 * wm + 16 * i + l16;
            if (row >= M) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t col = n0 + 64 * wn + 16 * j + 4 * lq;
                if (col + 3 < row || col >= a.N) continue;
                _Float16 h[4], l[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[i][j][r] * sc;
                    if (a.C && col + r >= row && col + r < a.N) a.C[b * a.sc + row * a.ldc + col + r] = v;
                    const float hs = v * gs;
                    h[r] = (_Float16)hs;
                    l[r] = (_Float16)(hs - (float)h[r]);
                }
                const int64_t o = (col >> 5) * (M * 32) + row * 32 + (col & 31);
                if (col >= row && col + 3 < a.N) {
                    *reinterpret_cast<uint2*>(Oh + o) = *reinterpret_cast<const uint2*>(h);
                    *reinterpret_cast<uint2*>(Ol + o) = *reinterpret_cast<const uint2*>(l);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (col + r >= row && col + r < a.N) { Oh[o + r] = h[r]; Ol[o + r] = l[r]; }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {  // mirror (col + r, row)
                    const int64_t c = col + r;
                    if (c > row && c < a.N) {
                        const int64_t om = (row >> 5) * (M * 32) + c * 32 + (row & 31);
                        Oh[om] = h[r];
                        Ol[om] = l[r];
                    }
                }
            }
        }
        return;
    }
    const float al_ = !live ? 0.f : a.alpha_v ? a.alpha_v[b] : 1.f;
    const float be_ = !live ? 0.f : a.beta_v ? a.beta_v[b] : 0.f;
    const float ga_ = !live ? 1.f : a.gamma_v ? a.gamma_v[b] : 0.f;
    bool ovf = false;
    uint32_t amx = 0u;   // |C| max bits (absmax_out)
    // lane = C row (A row), registers r = 4 consecutive C columns: 16-byte fp32 and 8-byte
    // fp16 accesses (host guarantees N % 4 == 0 and 16-byte aligned rows)
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    auto al8 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; };
    // (a null C -- only C^T is wanted -- or a null Ol -- hi halves only -- is not written)
    const bool vec = (a.N & 3) == 0 && (!a.C || ((a.ldc & 3) == 0 && (a.sc & 3) == 0 && al16(a.C))) &&
                     (!a.P || ((a.ldp & 3) == 0 && (a.sp & 3) == 0 && al16(a.P))) &&
                     (!a.D || ((a.ldd & 3) == 0 && (a.sd & 3) == 0 && al16(a.D))) &&
                     (!a.Oh || ((a.o_blocked || (a.ldo & 3) == 0) && (a.so & 3) == 0 && al8(a.Oh) && (!a.Ol || al8(a.Ol))));
    if (vec) {
        // An item q = 4 i + j is the lane's 4 columns of block (i, j).  fetch: its P and D
        // values; finish: combine and store.  P may alias C exactly (the recurrence overwrites
        // prev): an item's values are read before that item is written, and no other item's.
        // Addresses are a scalar base (the tile's corner, plus the item's offset) and one 32-bit
        // byte offset per lane and operand (the lane's row and column inside the tile; the host
        // bounds the leading dimensions), so the 24 items share their address registers.
        const bool useP = a.P && be_ != 0.f, useD = a.D && ga_ != 0.f;
        const int mr = (int)min<int64_t>(a.M - m0, XW_BM), nr = (int)min<int64_t>(a.N - n0, XW_BN);  // live rows, columns
        const uint32_t lr = 96 * wm + l16, lc = 64 * wn + 4 * lq;
        auto corner = [&](const void* p, int64_t sb_, int64_t ld, int esz) __attribute__((always_inline)) {
            return p ? reinterpret_cast<const char*>(p) + (b * sb_ + m0 * ld + n0) * esz : nullptr;
        };
        const char* Pt = corner(a.P, a.sp, a.ldp, 4);
        const char* Dt = corner(a.D, a.sd, a.ldd, 4);
        char* Ct_ = const_cast<char*>(corner(a.C, a.sc, a.ldc, 4));
        char* Tt = a.Ct ? reinterpret_cast<char*>(a.Ct + b * a.sct + n0 * a.M + m0) : nullptr;
        const float* cwt = a.colw ? a.colw + b * a.scolw + n0 : nullptr;
        const uint32_t vP = (lr * (uint32_t)a.ldp + lc) * 4u, vD = (lr * (uint32_t)a.ldd + lc) * 4u,
                       vC = (lr * (uint32_t)a.ldc + lc) * 4u, vT = (lc * (uint32_t)a.M + lr) * 4u;
        // split output: blocked, column c of the tile lies in K block n0 / 32 + c / 32 (n0 % 32 == 0)
        const int64_t oblk = a.M * 32;
        const int64_t ocorner = b * a.so + (a.o_blocked ? (n0 >> 5) * oblk + m0 * 32 : m0 * a.ldo + n0);
        const uint32_t vO = (a.o_blocked ? (uint32_t)(2 * wn) * (uint32_t)oblk + lr * 32u + 4u * lq
                                         : lr * (uint32_t)a.ldo + lc) * 2u;
        auto inside = [&](int q) __attribute__((always_inline)) {
            return (int)lr < mr - 16 * (q >> 2) && (int)lc < nr - 16 * (q & 3);
        };
        auto fetch = [&](int q, float4& pv, float4& dv) __attribute__((always_inline)) {
            if (!inside(q)) return;
            const int i = q >> 2, j = q & 3;
            if (useP) pv = *reinterpret_cast<const float4*>(Pt + (16 * i * a.ldp + 16 * j) * 4 + vP);
            if (useD) dv = *reinterpret_cast<const float4*>(Dt + (16 * i * a.ldd + 16 * j) * 4 + vD);
        };
        auto finish = [&](int q, const float4& pv, const float4& dv) __attribute__((always_inline)) {
            if (!inside(q)) return;
            const int i = q >> 2, j = q & 3;
            const f32x4v ac = acc[i][j];
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = al_ * (ac[r] * sc);
            if (cwt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] *= cwt[lc + (uint32_t)(16 * j + r)];   // (N % 4 == 0: in range)
            }
            if (useP) { v[0] += be_ * pv.x; v[1] += be_ * pv.y; v[2] += be_ * pv.z; v[3] += be_ * pv.w; }
            if (useD) { v[0] += ga_ * dv.x; v[1] += ga_ * dv.y; v[2] += ga_ * dv.z; v[3] += ga_ * dv.w; }
            if (Ct_) *reinterpret_cast<float4*>(Ct_ + (16 * i * a.ldc + 16 * j) * 4 + vC) = make_float4(v[0], v[1], v[2], v[3]);
            if (Tt) {   // C^T: lanes l16 (consecutive rows) make 64-byte runs per column
#pragma unroll
                for (int r = 0; r < 4; ++r) *reinterpret_cast<float*>(Tt + ((16 * j + r) * a.M + 16 * i) * 4 + vT) = v[r];
            }
            if (a.absmax_out)
                amx = max(amx, max(max(abs_bits(v[0]), abs_bits(v[1])), max(abs_bits(v[2]), abs_bits(v[3]))));
            if (a.Oh) {
                _Float16 h[4], l[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float hs = v[r] * a.out_scale;
                    h[r] = (_Float16)hs;
                    l[r] = (_Float16)(hs - (float)h[r]);
                    ovf |= !(fabsf(hs) < 65504.f);
                }
                const int64_t oi = ocorner + (a.o_blocked ? (j >> 1) * oblk + 16 * i * 32 + 16 * (j & 1)
                                                          : 16 * i * a.ldo + 16 * j);
                *reinterpret_cast<uint2*>(reinterpret_cast<char*>(a.Oh + oi) + vO) = *reinterpret_cast<const uint2*>(h);
                if (a.Ol) *reinterpret_cast<uint2*>(reinterpret_cast<char*>(a.Ol + oi) + vO) = *reinterpret_cast<const uint2*>(l);
            }
        };
        // item by item: measured, keeping the P and D loads of later items in flight across the
        // stores (rings of 2-4 items) is within noise of this -- the
        // epilogue already moves its own bytes at the HBM rate
#pragma unroll
        for (int q = 0; q < 24; ++q) {
            float4 pv = make_float4(0.f, 0.f, 0.f, 0.f), dv = pv;
            fetch(q, pv, dv);
            finish(q, pv, dv);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int64_t row = m0 + 96 * wm + 16 * i + l16;
            if (row >= a.M) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t col = n0 + 64 * wn + 16 * j + 4 * lq;
                if (col >= a.N) continue;
                const float* cw = a.colw ? a.colw + b * a.scolw : nullptr;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t c = col + r;
                    if (c >= a.N) continue;
                    float w = al_ * (acc[i][j][r] * sc);
                    if (cw) w *= cw[c];
                    if (a.P && be_ != 0.f) w += be_ * a.P[b * a.sp + row * a.ldp + c];
                    if (a.D && ga_ != 0.f) w += ga_ * a.D[b * a.sd + row * a.ldd + c];
                    if (a.C) a.C[b * a.sc + row * a.ldc + c] = w;
                    if (a.Ct) a.Ct[b * a.sct + c * a.M + row] = w;
                    amx = max(amx, abs_bits(w));
                    if (a.Oh) {
                        const float hs = w * a.out_scale;
                        const _Float16 h = (_Float16)hs;
                        const int64_t o = b * a.so + (a.o_blocked ? (c >> 5) * (a.M * 32) + row * 32 + (c & 31)
                                                                  : row * a.ldo + c);
                        a.Oh[o] = h;
                        if (a.Ol) a.Ol[o] = (_Float16)(hs - (float)h);
                        ovf |= !(fabsf(hs) < 65504.f);
                    }
                }
            }
        }
    }
    if (ovf) atomicOr(a.overflow + b, 1);
    if (a.absmax_out) {
        amx = wave_max_u32(amx);
        if (lane == 0 && amx) atomicMax(a.absmax_out + b, amx);
    }
}


// ------------------------------------------------------------------ 256 x 256 tile variant
// For the rank-256 products (config 5: the LPLR loop's Y Rw^T and L^T res, the normal-equation
// multiplies, all with r = 256 as M or N), where the 192 x 384 tile leaves a third of every
// tile idle (256 = 192 + 64 rows, or 256 of 384 columns).  Tile 256 x 256 x 32: 8 waves of
// 128 x 64 (8 x 4 blocks of v_mfma_f32_16x16x32_f16, 128 accumulator VGPRs, two waves per
// SIMD), the same LDS image (16-row x 64-B pieces, swizzled chunks), the same fragment reads
// and MFMA order per block as xr_mainloop<0> (al x bh, ah x bl, ah x bh per K step), so a
// block's sum is the same bits as the 192 x 384 kernel's; the same per-element bytes per flop
// (2/256 + 2/256 vs 2/192 + 2/384).  Two 64 KB stages, with a load plan of its own (16 images
// a part: shifts and masks, no row clamp).  Plain products only (C = alpha A B^T scale):
// M % 256 == 0, N % 256 == 0, no split-K / P / D / split output / colw.
constexpr int XS_BM = 256, XS_BN = 256, XS_THREADS = 512;
constexpr int XS_APART = XS_BM * XW_BK, XS_BPART = XS_BN * XW_BK;   // halves
constexpr int XS_STAGE = 2 * XS_APART + 2 * XS_BPART;
constexpr size_t XS_LDS_BYTES = (size_t)2 * XS_STAGE * sizeof(_Float16);  // 128 KB
constexpr int XS_PER_WAVE = (2 * XS_BM / 16 + 2 * XS_BN / 16) / (XS_THREADS / 64);  // 8
static_assert(XS_PER_WAVE == 8, "load split");

__device__ __forceinline__ void xs_plan(const X3K& a, int64_t m0, int64_t n0, int wid, int lane,
                                        uint32_t (&off)[XS_PER_WAVE]) {
#pragma unroll
    for (int u = 0; u < XS_PER_WAVE; ++u) {
        const int I = wid * XS_PER_WAVE + u;  // 0..63: Ah 0-15, Al 16-31, Bh 32-47, Bl 48-63
        const bool isA = I < 32;
        const int sub = I & 15;
        const int row = 16 * sub + (lane >> 2);
        const int c = (lane & 3) ^ xg_swz(row);
        const int64_t gr = (isA ? m0 : n0) + row;
        off[u] = (uint32_t)(isA ? (a.a_blocked ? gr * 32 + c * 8 : gr * a.lda + c * 8)
                                : (a.b_blocked ? gr * 32 + c * 8 : gr * a.ldb + c * 8));
    }
}

__device__ __forceinline__ void xs_issue(const X3K& a, int64_t b, int64_t k0, _Float16* stage, int wid,
                                         const uint32_t (&off)[XS_PER_WAVE]) {
#pragma unroll
    for (int u = 0; u < XS_PER_WAVE; ++u) {
        const int I = wid * XS_PER_WAVE + u;
        const bool isA = I < 32;
        const int part = (I >> 4) & 1;
        const int sub = I & 15;
        const _Float16* base = isA ? (part ? a.Al : a.Ah) + b * a.sa + (a.a_blocked ? (k0 >> 5) * (a.lda * 32) : k0)
                                   : (part ? a.Bl : a.Bh) + b * a.sb + (a.b_blocked ? (k0 >> 5) * (a.ldb * 32) : k0);
        _Float16* dst = stage + (isA ? part * XS_APART : 2 * XS_APART + part * XS_BPART) + (16 * sub) * XW_BK;
        xw_load(base + off[u], dst);
    }
}

__global__ __launch_bounds__(XS_THREADS, 1) void gemm_x3s_kernel(X3K a) {
    extern __shared__ __attribute__((aligned(16))) char xs_smem_raw[];
    _Float16* smem = reinterpret_cast<_Float16*>(xs_smem_raw);
    const int64_t total = a.tiles_n * a.tiles_m * a.batch;
    const int64_t orig = blockIdx.x;
    const int64_t q = total / 8, r8 = total % 8, xcd = orig % 8;
    const int64_t lin = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + orig / 8;
    const int64_t tm = lin % a.tiles_m, tn = (lin / a.tiles_m) % a.tiles_n, b = lin / (a.tiles_n * a.tiles_m);
    const int64_t m0 = tm * XS_BM, n0 = tn * XS_BN;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wid & 1, wn = wid >> 1;  // rows 128 wm .. +128, cols 64 wn .. +64
    const int l16 = lane & 15, lq = lane >> 4;
    f32x4v acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f};
    uint32_t off[XS_PER_WAVE];
    xs_plan(a, m0, n0, wid, lane, off);
    const int64_t nt = a.K / XW_BK;
    xs_issue(a, b, 0, smem, wid, off);
    for (int64_t t = 0; t < nt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // stage t landed everywhere; stage t-1 fully read
        if (t + 1 < nt) xs_issue(a, b, (t + 1) * XW_BK, smem + ((t + 1) & 1) * XS_STAGE, wid, off);
        const _Float16* sA = smem + (t & 1) * XS_STAGE;
        const _Float16* sB = sA + 2 * XS_APART;
        f16x8 bh[4], bl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = 64 * wn + 16 * j + l16;
            bh[j] = xg_frag(sB, row, lq);
            bl[j] = xg_frag(sB + XS_BPART, row, lq);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = 128 * wm + 16 * i + l16;
            const f16x8 ah = xg_frag(sA, row, lq);
            const f16x8 al = xg_frag(sA + XS_APART, row, lq);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[j], al, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl[j], ah, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[j], ah, acc[i][j], 0, 0, 0);
            }
        }
    }
    // C = alpha (acc scale), the same two roundings as gemm_x3v_kernel's epilogue
    const float sc = a.inv_scale[b], al = a.alpha_v ? a.alpha_v[b] : 1.f;
    uint32_t mx = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t row = m0 + 128 * wm + 16 * i + l16;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t col = n0 + 64 * wn + 16 * j + 4 * lq;
            const float4 v = make_float4(al * (acc[i][j][0] * sc), al * (acc[i][j][1] * sc), al * (acc[i][j][2] * sc),
                                         al * (acc[i][j][3] * sc));
            *reinterpret_cast<float4*>(a.C + b * a.sc + row * a.ldc + col) = v;
            mx = max(mx, max(max(abs_bits(v.x), abs_bits(v.y)), max(abs_bits(v.z), abs_bits(v.w))));
        }
    }
    if (a.absmax_out) {
        mx = wave_max_u32(mx);
        if (lane == 0 && mx) atomicMax(a.absmax_out + b, mx);
    }
}

// Split-K epilogue: C = alpha (sum of the ksplit partials, in chunk order) + beta P + gamma D,
// and the split halves of C, as gemm_x3v_kernel's epilogue does (inactive matrices: C = D).
// One thread per 4 consecutive columns (N % 4 == 0).
__global__ __launch_bounds__(256) void x3_splitk_epi_kernel(X3K a) {
    const int64_t nq = a.N / 4;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t b = blockIdx.y;
    if (a.skip && !a.active[b]) return;  // skip form: nothing written (b is uniform over the workgroup)
    const bool in = t < a.M * nq;
    uint32_t amx = 0u;
    if (in) {
    const int64_t row = t / nq, col = 4 * (t % nq);
    const bool live = !a.active || a.active[b];
    const float al_ = !live ? 0.f : a.alpha_v ? a.alpha_v[b] : 1.f;
    const float be_ = !live ? 0.f : a.beta_v ? a.beta_v[b] : 0.f;
    const float ga_ = !live ? 1.f : a.gamma_v ? a.gamma_v[b] : 0.f;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < a.ksplit; ++ks) {
        const float4 pv = *reinterpret_cast<const float4*>(a.part + ((ks * a.batch + b) * a.M + row) * a.N + col);
        s[0] += pv.x; s[1] += pv.y; s[2] += pv.z; s[3] += pv.w;
    }
    bool ovf = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float w = al_ * s[r];
        if (a.colw) w *= a.colw[b * a.scolw + col + r];
        if (a.P && be_ != 0.f) w += be_ * a.P[b * a.sp + row * a.ldp + col + r];
        if (a.D && ga_ != 0.f) w += ga_ * a.D[b * a.sd + row * a.ldd + col + r];
        if (a.C) a.C[b * a.sc + row * a.ldc + col + r] = w;
        if (a.Ct) a.Ct[b * a.sct + (col + r) * a.M + row] = w;
        amx = max(amx, abs_bits(w));
        if (a.Oh) {
            const float hs = w * a.out_scale;
            const _Float16 h = (_Float16)hs;
            const int64_t c = col + r;
            const int64_t o = b * a.so + (a.o_blocked ? (c >> 5) * (a.M * 32) + row * 32 + (c & 31) : row * a.ldo + c);
            a.Oh[o] = h;
            if (a.Ol) a.Ol[o] = (_Float16)(hs - (float)h);
            ovf |= !(fabsf(hs) < 65504.f);
        }
    }
    if (ovf) atomicOr(a.overflow + b, 1);
    }
    if (a.absmax_out) {   // (every lane reaches the wave reduction)
        amx = wave_max_u32(amx);
        if ((threadIdx.x & 63) == 0 && amx) atomicMax(a.absmax_out + b, amx);
    }
}

}  // namespace cq

using namespace cq;

static int gemm_x3_launch(const cq_x3_args* g, bool skip_form, void* stream);

extern "C" {

int cq_gemm_x3(const cq_x3_args* g, void* stream) { return gemm_x3_launch(g, false, stream); }

// cq_gemm_x3 with the skip form asked for whether or not D is given: matrices with
// active[b] == 0 are left out altogether (a recurrence step of a filter whose frozen matrices'
// iterates nobody reads), where cq_gemm_x3 would pass D through to C and the halves.
int cq_gemm_x3_skip(const cq_x3_args* g, void* stream) { return gemm_x3_launch(g, true, stream); }

}  // extern "C"

static int gemm_x3_launch(const cq_x3_args* g, bool skip_form, void* stream) {
    CQ_REQUIRE(g, "cq_gemm_x3: null args");
    CQ_REQUIRE(g->Ah && g->Al && g->Bh && (g->Bl || g->single || g->b_exact) && (g->C || g->sym_out || g->Ct) && g->inv_scale,
               "cq_gemm_x3: null operand");
    CQ_REQUIRE(!g->sym_out || (g->tri && g->out_h && g->out_l && g->out_bound && g->scale_out && g->inv_out &&
                               g->out_scale > 0.f && g->N % 32 == 0),
               "cq_gemm_x3: sym_out needs tri, out_h/out_l, out_bound, scale_out, inv_out, N % 32 == 0");
    CQ_REQUIRE(g->M > 0 && g->N > 0 && g->K > 0 && g->batch > 0, "cq_gemm_x3: bad shape");
    CQ_REQUIRE(g->K % XW_BK == 0, "cq_gemm_x3: K must be a multiple of 32");
    CQ_REQUIRE(g->lda % 8 == 0 && g->ldb % 8 == 0 && g->stride_a % 8 == 0 && g->stride_b % 8 == 0,
               "cq_gemm_x3: operand rows must be 16-byte aligned");
    CQ_REQUIRE((g->a_blocked ? g->lda >= g->M : g->lda >= g->K) && (g->b_blocked ? g->ldb >= g->N : g->ldb >= g->K) &&
                   (!g->C || g->ldc >= g->N),
               "cq_gemm_x3: leading dimension too small");
    CQ_REQUIRE(g->out_h || !g->out_l, "cq_gemm_x3: out_l needs out_h (out_h alone: hi halves only)");
    // (the vector epilogue addresses a tile with 32-bit byte offsets per lane: 192 rows of ld floats)
    CQ_REQUIRE(g->M <= (1 << 21) && g->ldc <= (1 << 22) && g->ldp <= (1 << 22) && g->ldd <= (1 << 22) && g->ldo <= (1 << 22),
               "cq_gemm_x3: M above 2^21 or a leading dimension above 2^22");
    CQ_REQUIRE(!g->out_h || g->sym_out || (g->overflow && g->out_scale > 0.f),
               "cq_gemm_x3: split output needs overflow flags");
    CQ_REQUIRE(!g->beta_v || g->P, "cq_gemm_x3: beta_v needs P");
    CQ_REQUIRE(!g->gamma_v || g->D, "cq_gemm_x3: gamma_v needs D");
    X3K a;
    a.M = g->M; a.N = g->N; a.K = g->K; a.batch = g->batch;
    a.Ah = reinterpret_cast<const _Float16*>(g->Ah); a.Al = reinterpret_cast<const _Float16*>(g->Al);
    a.lda = g->lda; a.sa = g->stride_a;
    a.Bh = reinterpret_cast<const _Float16*>(g->Bh); a.Bl = reinterpret_cast<const _Float16*>(g->Bl);
    a.ldb = g->ldb; a.sb = g->stride_b;
    a.inv_scale = g->inv_scale;
    a.C = g->C; a.ldc = g->ldc; a.sc = g->stride_c;
    a.P = g->P; a.ldp = g->ldp; a.sp = g->stride_p;
    a.D = g->D; a.ldd = g->ldd; a.sd = g->stride_d;
    a.alpha_v = g->alpha_v; a.beta_v = g->beta_v; a.gamma_v = g->gamma_v;
    a.Oh = reinterpret_cast<_Float16*>(g->out_h); a.Ol = reinterpret_cast<_Float16*>(g->out_l);
    a.ldo = g->ldo; a.so = g->stride_o; a.out_scale = g->out_scale;
    a.overflow = g->overflow;
    CQ_REQUIRE(!g->tri || (g->M == g->N && !g->P && !g->D && (!g->out_h || g->sym_out)),
               "cq_gemm_x3: tri needs a square plain product");
    a.single = g->single;
    a.colw = g->colw;
    a.scolw = g->stride_colw;
    a.absmax_out = g->absmax_out;
    a.Ct = g->Ct;
    a.sct = g->stride_ct;
    CQ_REQUIRE(!g->Ct || (!g->sym_out && !g->tri), "cq_gemm_x3: Ct needs a non-symmetric product");
    CQ_REQUIRE(!g->absmax_out || (!g->sym_out && !g->tri), "cq_gemm_x3: absmax_out needs a plain product");
    CQ_REQUIRE(!g->colw || (!g->sym_out && !g->tri), "cq_gemm_x3: colw needs a plain product");
    // single + sym_out: the Gram of an exactly-fp16 operand (lo = 0; A = W W^T of the sparse-code
    // Gram, sgram.py): the split products add exact zeros, so one product gives the same bits
    a.sym_out = g->sym_out;
    a.out_bound = g->out_bound;
    a.scale_out = g->scale_out;
    a.inv_out = g->inv_out;
    a.tri = g->tri;
    a.b_blocked = g->b_blocked;
    a.active = g->active;
    a.a_blocked = g->a_blocked;
    a.o_blocked = g->o_blocked;
    CQ_REQUIRE(!g->o_blocked || g->N % 32 == 0, "cq_gemm_x3: blocked split output needs N % 32 == 0");
    CQ_REQUIRE(!g->a_blocked || g->lda >= g->M, "cq_gemm_x3: blocked A needs lda = rows >= M");
    // active without D (no pass-through value), or cq_gemm_x3_skip: the skip form
    a.skip = (g->active && (skip_form || !g->D)) ? 1 : 0;
    CQ_REQUIRE(!a.skip || (!g->tri && !g->sym_out), "cq_gemm_x3: the skip form needs a plain product");
    CQ_REQUIRE(!g->b_blocked || g->ldb >= g->N, "cq_gemm_x3: blocked B needs ldb = rows >= N");
    a.tiles_n = ceil_div(g->N, XW_BN);
    a.tiles_m = ceil_div(g->M, XW_BM);
    int64_t total = a.tiles_n * a.tiles_m * a.batch;
    a.tiles_live = 0;
    if (a.sym_out) {  // tiles with tn >= tm / 2 (XW_BN = 2 XW_BM): the rest lie below the diagonal
        static_assert(XW_BN == 2 * XW_BM, "Gram tile enumeration");
        for (int64_t tm = 0; tm < a.tiles_m; ++tm) a.tiles_live += std::max<int64_t>(0, a.tiles_n - (tm >> 1));
        total = a.tiles_live * a.batch;
    }
    a.ksplit = g->ksplit > 1 ? g->ksplit : 1;
    a.part = g->split_ws;
    if (a.ksplit > 1) {
        CQ_REQUIRE(!a.tri && !a.sym_out && a.part && (a.C || a.Ct) && g->N % 4 == 0 && a.ksplit <= g->K / XW_BK,
                   "cq_gemm_x3: split-K needs a plain product with C or Ct, N % 4 == 0, split_ws, ksplit <= K / 32");
        total *= a.ksplit;
    }
    CQ_REQUIRE(total < (1ll << 31), "cq_gemm_x3: grid too large");
    // the 256 x 256 tile where the 192 x 384 one would leave over 15 % of its MFMA work idle
    // (rank-256 products), for plain split products
    const bool sq = !a.single && !g->b_exact && !a.tri && !a.sym_out && a.ksplit == 1 && !a.P && !a.D && !a.Oh && !a.Ct &&
                    !a.colw && !a.active && g->M % XS_BM == 0 && g->N % XS_BN == 0 && g->ldc % 4 == 0 &&
                    g->stride_c % 4 == 0 && (reinterpret_cast<uintptr_t>(g->C) & 15) == 0 &&
                    (double)(a.tiles_m * XW_BM) * (double)(a.tiles_n * XW_BN) > 1.15 * (double)g->M * (double)g->N;
    if (sq) {
        a.tiles_m = g->M / XS_BM;
        a.tiles_n = g->N / XS_BN;
        const int64_t tot = a.tiles_m * a.tiles_n * a.batch;
        CQ_REQUIRE(tot < (1ll << 31), "cq_gemm_x3: grid too large");
        gemm_x3s_kernel<<<(unsigned)tot, XS_THREADS, XS_LDS_BYTES, as_stream(stream)>>>(a);
        return check_launch("cq_gemm_x3");
    }
    if (a.single) gemm_x3v_kernel<1><<<(unsigned)total, XW_THREADS, XW_LDS_BYTES, as_stream(stream)>>>(a);
    else if (g->b_exact) gemm_x3v_kernel<2><<<(unsigned)total, XW_THREADS, XW_LDS_BYTES, as_stream(stream)>>>(a);
    else gemm_x3v_kernel<0><<<(unsigned)total, XW_THREADS, XW_LDS_BYTES, as_stream(stream)>>>(a);
    if (a.ksplit > 1)
        x3_splitk_epi_kernel<<<dim3((unsigned)ceil_div(g->M * (g->N / 4), 256), (unsigned)g->batch), 256, 0,
                               as_stream(stream)>>>(a);
    return check_launch("cq_gemm_x3");
}
