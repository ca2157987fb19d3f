// The split-fp16 operand tile shared by the products (cq_x3.hip) and the tiled fused Q update
// (cq_qtile.hip): the swizzled LDS image, the LDS-DMA loader and the ring K loop of the
// 192 x 384 tile.
#pragma once

#include "cq_x3.h"

namespace cq {

// ------------------------------------------------------------------ LDS images
// LDS images are linear per wave-instruction (16 rows x 64 B) with the 16-B chunk index
// XOR-swizzled on the global source address by xg_swz(row), a permutation of the row quad
// q = (row >> 2) & 3.  gfx950 serves a ds_read_b128 in four 16-lane groups, {0-3, 12-15,
// 20-27}, {4-11, 16-19, 28-31} and the same +32 (MI355X_MICROARCH.md, LDS banking): for the
// 16x16x32 fragment reads (lane = row l16 + 16 x chunk lq) a group holds rows of all four quads
// at two chunks, so q -> {0, 2, 3, 1} (not q itself, which left every group 2-way conflicted:
// 4 conflict cycles per read in the PMC counters) puts its 16 lanes on 16 different 16-byte
// bank slots; the 32x32x16 reads (32 rows x one chunk) stay conflict-free.
constexpr int XG_BK = 32;

__device__ __forceinline__ int xg_swz(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }

__device__ __forceinline__ f16x8g xg_frag(const _Float16* img, int row, int chunk) {
    const int pc = chunk ^ xg_swz(row);
    return *reinterpret_cast<const f16x8g*>(img + row * XG_BK + pc * 8);
}

// ------------------------------------------------------------------ 192 x 384 tile
// Tile 192 (A rows) x 384 (B rows) x 32, 768 threads = 12 waves of 96 x 64.  Per K step the CU
// loads 72 KB for 2x the MFMA work of a 192 x 192 tile (48 KB): the X^T slice is re-read by
// half as many tiles, which is what bounds the filter product (per-CU load path,
// ~10 B/clk/CU).  The K ring takes 144 KB of LDS in every mode.
constexpr int XW_BM = 192, XW_BN = 384, XW_BK = 32;
constexpr int XW_THREADS = 768;
constexpr size_t XW_LDS_BYTES = (size_t)2 * (2 * XW_BM + 2 * XW_BN) * XW_BK * sizeof(_Float16);  // 144 KB

// One 16-B-per-lane LDS-DMA load (default cache policy: non-temporal loads of the once-read
// B panels measured 0.5-3 % slower, profiles/r04aq_nt_ab)
__device__ __forceinline__ void xw_load(const _Float16* src, _Float16* dst) {
    __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// The 192 x 384 tile's K ring by product mode XM (gemm_x3v_kernel): 0 = three split products,
// 1 = one hi x hi product, 2 = exact B (B lo is zero and unread).  A stage holds the operand
// images A hi | A lo (if AL) | B hi | B lo (if BL), each rows x 32 halves: 72 / 36 / 48 KB, so
// 2 / 4 / 3 stages fit the 144 KB.  The fewer MFMAs a K step has, the more stages are in
// flight: a hi-only step has a third of the split product's MFMA work, too little to cover an
// HBM round trip with one stage ahead.  A stage is A_IMGS + B_IMGS wave-instructions of 16
// rows, dealt PER_WAVE (6 / 3 / 4) to a wave in image order.
template <int XM>
struct XRing {
    static constexpr bool AL = XM != 1, BL = XM == 0;
    static constexpr int NS = XM == 0 ? 2 : XM == 1 ? 4 : 3;
    static constexpr int BM = XW_BM, BN = XW_BN;
    static constexpr int APART = BM * XW_BK, BPART = BN * XW_BK;   // halves
    static constexpr int A_IMGS = (1 + AL) * BM / 16, B_IMGS = (1 + BL) * BN / 16;
    static constexpr int PER_WAVE = (A_IMGS + B_IMGS) / (XW_THREADS / 64);
    static constexpr int B_OFF = (1 + AL) * APART;
    static constexpr int STAGE = B_OFF + (1 + BL) * BPART;
    static_assert(PER_WAVE * (XW_THREADS / 64) == A_IMGS + B_IMGS, "load split");
    static_assert((size_t)NS * STAGE * sizeof(_Float16) <= XW_LDS_BYTES, "ring fits the LDS");
};

// Load plan: the wave-uniform part of each of this wave's LDS-DMA loads (which image, which
// 16-row group) is scalar; the per-lane part is a 32-bit element offset computed once per
// tile, so a K step costs one 64-bit add per load (keeps the loop free of spills).  Rows past
// the matrix edge are clamped to the last row (loaded, never stored).
template <class R>
__device__ __forceinline__ void xr_plan(const X3K& a, int64_t m0, int64_t n0, int wid, int lane,
                                        uint32_t (&off)[R::PER_WAVE]) {
#pragma unroll
    for (int u = 0; u < R::PER_WAVE; ++u) {
        const int I = wid * R::PER_WAVE + u;
        const bool isA = I < R::A_IMGS;
        const int part = isA ? (R::AL && I >= R::BM / 16) : (R::BL && I >= R::A_IMGS + R::BN / 16);
        const int sub = isA ? I - (R::BM / 16) * part : I - R::A_IMGS - (R::BN / 16) * part;
        const int row = 16 * sub + (lane >> 2);
        const int c = (lane & 3) ^ xg_swz(row);
        const int64_t lim = isA ? a.M : a.N;
        int64_t gr = (isA ? m0 : n0) + row;
        gr = gr < lim ? gr : lim - 1;
        off[u] = (uint32_t)(isA ? (a.a_blocked ? gr * 32 + c * 8 : gr * a.lda + c * 8)
                                : (a.b_blocked ? gr * 32 + c * 8 : gr * a.ldb + c * 8));
    }
}

// The loads of the K step at k0 into one stage (a mode without a lo half never names its
// pointer: Bl may be NULL for XM = 1 and 2).  part and sub by compares and subtractions, not
// I / and I % the images of a part: with the divisions the compiler branches per load inside
// the K loop (the split filter step measured 3 % slower).
template <class R>
__device__ __forceinline__ void xr_issue(const X3K& a, int64_t b, int64_t k0, _Float16* stage, int wid,
                                         const uint32_t (&off)[R::PER_WAVE]) {
#pragma unroll
    for (int u = 0; u < R::PER_WAVE; ++u) {
        const int I = wid * R::PER_WAVE + u;
        const bool isA = I < R::A_IMGS;
        const int part = isA ? (R::AL && I >= R::BM / 16) : (R::BL && I >= R::A_IMGS + R::BN / 16);
        const int sub = isA ? I - (R::BM / 16) * part : I - R::A_IMGS - (R::BN / 16) * part;
        const _Float16* base = isA ? (R::AL && part ? a.Al : a.Ah) + b * a.sa + (a.a_blocked ? (k0 >> 5) * (a.lda * 32) : k0)
                                   : (R::BL && part ? a.Bl : a.Bh) + b * a.sb + (a.b_blocked ? (k0 >> 5) * (a.ldb * 32) : k0);
        _Float16* dst = stage + (isA ? part * R::APART : R::B_OFF + part * R::BPART) + (16 * sub) * XW_BK;
        xw_load(base + off[u], dst);
    }
}

template <int N>
__device__ __forceinline__ void xr_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// Before step t's barrier: this wave's loads of the stages issued after step t's -- at most
// NS - 2 of them, stage t + NS - 1 being issued after the barrier -- may stay in flight
// (counted vmcnt: PER_WAVE LDS-DMA wave-instructions per wave and stage).  later = nt - 1 - t.
template <class R>
__device__ __forceinline__ void xr_wait(int64_t later) {
    static_assert(R::NS >= 2 && R::NS <= 4, "xr_wait's cases");
    if (R::NS > 3 && later >= 2) xr_wait_vm<2 * R::PER_WAVE>();
    else if (R::NS > 2 && later >= 1) xr_wait_vm<R::PER_WAVE>();
    else xr_wait_vm<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// The 192 x 384 tile's K loop (the filter / Gram products and the fused Q update):
// acc = A[m0.., :] B[n0.., :]^T over K steps kb .. kb + nt (kb: a split-K chunk's offset) in
// product mode XM; nt = 0 leaves acc = 0.  Each wave's 96 x 64 block is 6 x 4
// v_mfma_f32_16x16x32_f16 tiles: under the chip's power limit the 16x16x32 form runs at a
// higher clock than 32x32x16 for the same work (MI355X_MICROARCH.md: ~1.15x the FLOP/s in
// bare loops).  The prologue issues min(NS - 1, nt) stages; step t waits for stage t,
// barriers, issues stage t + NS - 1 into the slot step t - 1 used, and multiplies.  The terms
// of a block, always in this order: bh x al (modes with A lo), bl x ah (with B lo), bh x ah;
// a mode without a lo half drops a term that is exactly zero for its operands: the same bits.
// PERMB: block j's B fragment row for output register index t = 4 lq + r is LDS row
// 64 wn + 16 (t >> 2) + 4 j + (t & 3), so lane (l16, lq) ends up holding the 16 consecutive
// B rows 64 wn + 16 lq + [0, 16) in acc[i][0..3][0..3] (used by the fused Q update).
template <int XM, bool PERMB = false>
__device__ __forceinline__ void xr_mainloop(const X3K& a, int64_t b, int64_t m0, int64_t n0, int64_t nt,
                                            _Float16* smem, int wid, int lane, int wm, int wn,
                                            f32x4v (&acc)[6][4], int64_t kb = 0) {
    using R = XRing<XM>;
    const int l16 = lane & 15, lq = lane >> 4;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f};
    wid = __builtin_amdgcn_readfirstlane(wid);  // wave-uniform: load selection stays scalar
    uint32_t off[R::PER_WAVE];
    if (nt > 0) {
        xr_plan<R>(a, m0, n0, wid, lane, off);
        for (int64_t s = 0; s < R::NS - 1 && s < nt; ++s)
            xr_issue<R>(a, b, (kb + s) * XW_BK, smem + s * R::STAGE, wid, off);
    }
    int slot = 0, nslot = R::NS - 1;  // slot of step t, slot the stage of step t + NS - 1 goes to
    // A wave whose 96 x 64 output block lies wholly past the matrix edge (ragged last tiles)
    // or, for a symmetric Gram (tri), wholly below the diagonal is never stored: it runs only
    // its share of the loads and barriers, no fragment reads or MFMAs (fewer MFMA joules;
    // measured time-neutral -- the workgroup still waits for its live waves at every barrier:
    // Gram 6.16 vs 6.13 ms, filter 2.65 vs 2.65 ms at B = 128/32).  (PERMB: a fragment's 16
    // columns interleave with stride 16 across the wave's 64; the wave-level test only needs
    // the block's first row and column.)  This stays a loop of its own with an early return:
    // folded into the live loop as `if (live) { fragments + MFMAs }`, every instantiation goes
    // to 168 VGPRs and spills 192-228 B of scratch per lane in gemm_x3v_kernel<0/1/2> and
    // 204-212 B in q_update_v_kernel; per-strip or per-block skips inside the K loop make the
    // allocator spill the accumulators too.  (The four lines that open a step are written out
    // in both loops: through a shared lambda the split product's epilogue restores three
    // times as many spilled scalars.)
    const int64_t rs0 = m0 + 96 * wm, cs0 = n0 + 64 * wn;
    uint32_t live = (rs0 < a.M && cs0 < a.N && (!a.tri || cs0 + 63 >= rs0)) ? 1u : 0u;
    live = __builtin_amdgcn_readfirstlane(live);
    if (!live) {
        for (int64_t t = 0; t < nt; ++t) {
            xr_wait<R>(nt - 1 - t);
            __builtin_amdgcn_s_barrier();
            if (t + R::NS - 1 < nt) xr_issue<R>(a, b, (kb + t + R::NS - 1) * XW_BK, smem + nslot * R::STAGE, wid, off);
            nslot = nslot == R::NS - 1 ? 0 : nslot + 1;
        }
        return;
    }
    for (int64_t t = 0; t < nt; ++t) {
        xr_wait<R>(nt - 1 - t);
        __builtin_amdgcn_s_barrier();  // stage t landed everywhere; the slot of t - 1 fully read
        if (t + R::NS - 1 < nt) xr_issue<R>(a, b, (kb + t + R::NS - 1) * XW_BK, smem + nslot * R::STAGE, wid, off);
        nslot = nslot == R::NS - 1 ? 0 : nslot + 1;
        const _Float16* sA = smem + slot * R::STAGE;
        const _Float16* sB = sA + R::B_OFF;
        f16x8 bh[4], bl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = PERMB ? 64 * wn + 16 * (l16 >> 2) + 4 * j + (l16 & 3) : 64 * wn + 16 * j + l16;
            bh[j] = xg_frag(sB, row, lq);
            if constexpr (R::BL) bl[j] = xg_frag(sB + R::BPART, row, lq);
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int row = 96 * wm + 16 * i + l16;
            const f16x8 ah = xg_frag(sA, row, lq);
            f16x8 al;
            if constexpr (R::AL) al = xg_frag(sA + R::APART, row, lq);
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // transposed block: lanes run over A rows, registers over B rows
                if constexpr (R::AL) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[j], al, acc[i][j], 0, 0, 0);
                if constexpr (R::BL) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl[j], ah, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[j], ah, acc[i][j], 0, 0, 0);
            }
        }
        slot = slot == R::NS - 1 ? 0 : slot + 1;
    }
}

// The same tile and 2-stage ring with 3 x 2 blocks of v_mfma_f32_32x32x16_f16 per wave: another
// MFMA shape, so another summation order than xr_mainloop's.  Used only by the unaligned
// fallback q_update_x3_kernel.
__device__ __forceinline__ void xw_mainloop(const X3K& a, int64_t b, int64_t m0, int64_t n0, int64_t nt,
                                            _Float16* smem, int wid, int lane, int wm, int wn,
                                            f32x16v (&acc)[3][2]) {
    using R = XRing<0>;
    const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    wid = __builtin_amdgcn_readfirstlane(wid);  // wave-uniform: load selection stays scalar
    uint32_t off[R::PER_WAVE];
    if (nt > 0) {
        xr_plan<R>(a, m0, n0, wid, lane, off);
        xr_issue<R>(a, b, 0, smem, wid, off);
    }
    for (int64_t t = 0; t < nt; ++t) {
        xr_wait<R>(0);
        __builtin_amdgcn_s_barrier();  // stage t landed everywhere; stage t-1 fully read
        if (t + 1 < nt) xr_issue<R>(a, b, (t + 1) * XW_BK, smem + ((t + 1) & 1) * R::STAGE, wid, off);
        const _Float16* sA = smem + (t & 1) * R::STAGE;
        const _Float16* sB = sA + R::B_OFF;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const int ch = 2 * s2 + lh;
            f16x8 ah[3], al[3], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int row = 96 * wm + 32 * i + lr;
                ah[i] = xg_frag(sA, row, ch);
                al[i] = xg_frag(sA + R::APART, row, ch);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int row = 64 * wn + 32 * j + lr;
                bh[j] = xg_frag(sB, row, ch);
                bl[j] = xg_frag(sB + R::BPART, row, ch);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                }
        }
    }
}

}  // namespace cq
