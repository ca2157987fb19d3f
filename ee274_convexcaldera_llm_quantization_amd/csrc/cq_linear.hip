// Packed linear layer (cq_linear_forward): y = x (gs (Q + L R))^T straight from the 2/4-bit
// codes and the fp16 factors, never forming the dense weight.
//
//   y[t, i] = gs * ((s / k) * sum_j x[t, j] c[i, j] + sum_q z[t, q] L[i, q]) (+ bias[i])
//   z[t, q] = sum_j x[t, j] R[q, j]
//
// Every product is v_mfma_f32_16x16x32_f16 with the tokens as the A rows and 16 weight rows
// as the B columns: a lane's B fragment is 8 consecutive elements of one weight row, which is
// 2 (2-bit) or 4 (4-bit) bytes of its packed row or 16 bytes of an fp16 row.  Weights go from
// memory straight to VGPRs in 16-byte loads (a lane's load holds the B fragments of 8 / 4 / 1
// MFMAs) and are expanded in registers; x, the small operand every wave shares, comes through
// L2.  Codes are exact in fp16 and the MFMA accumulates in fp32, so the code sum is exact
// until it is scaled by s / k once per output.  z crosses between the two launches as split
// fp16 halves (hi = f16(z), lo = f16(z - hi)).
//
// Two shapes of the same kernel (kDecodeMax = CQ_LINEAR_DECODE_MAX_TOKENS):
//   decode  (T <= 16): one workgroup per 16 weight rows, its 8 waves split K in interleaved
//     chunks and add their partial tiles in wave order through LDS (fixed order, no atomics);
//     the next chunk's codes and x fragments are in flight while this one is expanded.  R has
//     only r / 16 row groups, so the z product also splits K over kDecodeSplitZ workgroups per
//     group; their fp32 partial z are added in workgroup order, and split into halves, by the
//     waves of the code kernel that multiply them with L.
//   prefill (T > 16):  a wave owns 64 weight rows x 64 tokens, so an expanded B fragment
//     feeds four MFMAs and an x fragment four more; weights are loaded a chunk ahead and x a
//     k step ahead; the code sum is scaled by s / k in the accumulator and the L product
//     continues on it.
//
// Factor codes (cq_linear_packed_forward): L and / or R as packed 2/4-bit codes with one scale
// each, in the layout of the layer's own codes.  z~ = zscale * sum_j x rho with rho the integer R
// codes (the K loop and `expand` of the code kernel, writing z) and zscale the product of the
// coded factors' scale / k, applied once to the complete fp32 z sum before it is split into halves
// (the z kernel's epilogue in prefill; after the ordered add of the partial z in decode); the L
// product then multiplies the halves with the integer L codes, a lane's 16-byte load holding its B
// fragments of 4 / 8 k steps.  cq_linear_forward is this path with fp16 factors and zscale = 1.
//
// Codebook Q (cq_linear_codebook_forward, CQ_QFMT_NF): the layer's own codes are NF4 / NF2 level
// indices in the same layout, the Q term (s / D) * sum_j x[t, j] I[idx[i, j]] with I = D level an
// integer (D = 1000 resp. 10000).  A level table is not affine, so the magic numbers do not apply:
// the workgroup fills a byte-indexed LDS table once (256 entries holding the 2 resp. 4 fp16 integers
// of a byte's indices; cq_nf.h) and `expand_nf` looks a fragment's bytes up (4 ds_read_b32 resp. 2
// ds_read_b64).  NF2's 8165 and 3333 are not fp16 values: the table holds the hi plane (8164 / 3332,
// signed), the lo plane (+-1, the level's sign) is made from it in registers, and both planes are
// multiplied into the same accumulator, hi first.  Everything around the expansion is unchanged.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "cq_codes.h"
#include "cq_common.h"
#include "cq_linear_host.h"
#include "cq_nf.h"

namespace cq {
namespace {

constexpr int kDecodeMax = CQ_LINEAR_DECODE_MAX_TOKENS;
constexpr int kDecodeWaves = 8;    // K split of a decode workgroup (chunks interleaved over its waves)
constexpr int kDecodeWavesZ = 2;   // the z product: waves per workgroup (64 bytes of R per lane and chunk) ...
constexpr int kDecodeSplitZ = 16;  // ... and workgroups per 16 rows of R: r / 16 workgroups alone would
                                   // stream R through r / 16 CUs; their partial z are added in order by
                                   // the code kernel
constexpr int kPrefillTiles = 4;   // 16-token tiles per wave
constexpr int kPrefillGroups = 4;  // 16-row groups per wave (codes)

struct LinP {
    const _Float16* x; int64_t ldx; int x_al;
    int64_t T, rows, n;        // rows: weight rows (m; r for the z product), n: contraction
    const uint8_t* w; int64_t wstride; int w_al;  // codes: bytes per row; fp16: elements per row
    int64_t r, r32;            // rank, rounded up to the MFMA's K (the z buffers' row length)
    const _Float16* L; int64_t ldl; int l_al;
    const _Float16* zh; const _Float16* zl;       // [token rows][r32] halves (read)
    float sk, gs;
    const float* bias;
    void* y; int y_f16; int64_t ldy;
    _Float16* oh; _Float16* ol;                   // z product: halves (written)
    const float* zp; float* ozp;                  // decode: [kDecodeSplitZ][16][r32] fp32 partial z (read / written)
    const uint8_t* lc; int64_t lcstride;          // packed L codes (m rows of r codes): bytes per row
    float zscale;                                 // on the complete z sum, before it is split (1 without factor codes)
};

// the grouped kernel's argument, see linear_kernel
struct GroupP {
    LinP m[CQ_LINEAR_GROUP_MAX];
    int32_t first[CQ_LINEAR_GROUP_MAX];
};
__device__ __forceinline__ const LinP& member(const LinP& p, int) { return p; }
__device__ __forceinline__ const LinP& member(const GroupP& g, int off) {
    return *reinterpret_cast<const LinP*>(reinterpret_cast<const char*>(g.m) + off);
}

// B fragment jj of a lane's 16 bytes of codes: 8 consecutive codes (cq_codes.h)
template <int BITS>
__device__ __forceinline__ h8 expand(const u4 q, int jj) {
    if constexpr (BITS == 2) return expand<2>(q[jj >> 1], jj & 1);
    else return expand<4>(q[jj], 0);
}

// WT: the weight rows of the K loop, 2 / 4 = packed codes, 16 = fp16.  ZP: the z product (the
// weight rows are R's, fp16 or codes; writes partial z or split halves), else the layer's codes
// (+ the L product and the output epilogue) with LB: L as fp16 rows (16) or packed 2 / 4-bit
// codes.  A wave owns RG groups of 16 weight rows x TT tiles of 16 tokens.  NW: waves per
// workgroup; KSPLIT: they split K over one 16-row group (else each owns its own rows).  QF: the
// layer's codes are offset-binary uniform codes (CQ_QFMT_UNIFORM) or NF level indices (CQ_QFMT_NF).
// The NF4 prefill tile keeps 16 table reads in flight and would take 172 VGPRs + 92 AGPRs, one
// workgroup per CU where the uniform tile has two; asked for two waves per SIMD it fits 220 VGPRs
// without scratch.  Every other instantiation states a minimum of one wave per SIMD, which
// is what its launch bounds imply already: their code is the same with and without the attribute.
//
// ARG: the kernel's argument.  LinP: one layer, the workgroup's place in the grid is its place in the
// layer.  GroupP (cq_linear_group_forward): up to CQ_LINEAR_GROUP_MAX layers that share x, T, n and
// the template parameters in one grid whose x extent is the members' own x extents laid end to end,
// so a workgroup never spans two members; first[i] is member i's first blockIdx.x (INT32_MAX past
// the last member).  A workgroup finds its member by comparing blockIdx.x with that table -- kernel
// arguments and blockIdx only: scalar loads, compares and selects -- and then runs on the member's
// parameters at its own place (bx) in the member's grid: the same work in the same order as alone.
// The body is one and the same text for both; with ARG = LinP, p is the kernel argument itself.
// The grouped prefill code kernels ask for two waves per SIMD as well: their fields are loaded from a
// computed address where they are used, and left alone the 2-bit tile came out at 146 VGPRs + 120
// AGPRs, one wave; asked, all of them fit 214 .. 222 VGPRs without scratch.
template <int WT, int QF, int LB, bool ZP, int TT, int RG, int NW, bool KSPLIT, typename ARG>
__global__ __launch_bounds__(NW * 64)
__attribute__((amdgpu_waves_per_eu(
    (QF == CQ_QFMT_NF && WT == 4 && TT > 1) || (std::is_same_v<ARG, GroupP> && !ZP && TT > 1) ? 2 : 1))) void
linear_kernel(const ARG arg) {
    unsigned bx = blockIdx.x;
    int off = 0;  // the member's byte offset in arg.m
    if constexpr (std::is_same_v<ARG, GroupP>) {
        int32_t base = 0;
#pragma unroll
        for (int i = 1; i < CQ_LINEAR_GROUP_MAX; ++i) {
            const bool past = (int32_t)blockIdx.x >= arg.first[i];
            off = past ? i * (int)sizeof(LinP) : off;  // the table ascends: the last member at or before blockIdx.x
            base = past ? arg.first[i] : base;
        }
        bx -= (unsigned)base;
    }
    const LinP& p = member(arg, off);
    constexpr bool CODES = WT != 16;
    constexpr bool NF = QF == CQ_QFMT_NF;
    static_assert(!NF || (CODES && !ZP), "only the layer's own codes are level indices");
    constexpr bool PLANES2 = NF && WT == 2;
    const uint32_t* nftab = nullptr;
    if constexpr (NF) {  // before any wave leaves
        __shared__ uint32_t tab[WT == 4 ? 256 : 512];
        fill_nf_table<WT>(tab, threadIdx.x, NW * 64);
        __syncthreads();
        nftab = tab;
    }
    static_assert(!ZP || LB == 16, "the z product has no L");
    static_assert(ZP || CODES, "the layer's own weight is always codes");
    constexpr int WV = CODES ? 1 : 4;                   // 16-byte weight loads per lane and chunk
    constexpr int CK = CODES ? 16 * 8 / WT * 4 : 128;   // k per chunk: 4 lane groups x WV loads
    constexpr int NM = CK / 32;                         // MFMA k steps per chunk
    constexpr int GK = CK / 4;                          // k per lane group
    static_assert(!KSPLIT || (TT == 1 && RG == 1), "the K split reduces one tile");
    struct WR { u4 v[WV]; };
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int64_t row0 = (KSPLIT ? (int64_t)bx : (int64_t)bx * NW + wave) * (16 * RG);
    // blockIdx.y: the token tile; under the K split (one tile) the workgroup's share of K
    const int64_t tok0 = KSPLIT ? 0 : (int64_t)blockIdx.y * (TT * 16);
    const int64_t rows_out = ZP ? p.r32 : p.rows;
    if (!KSPLIT && row0 >= rows_out) return;

    int64_t rowc[RG], wlim[RG];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) {
        const int64_t row = row0 + rg * 16 + li;
        rowc[rg] = row < p.rows ? row : p.rows - 1;
        wlim[rg] = row < p.rows ? p.n : 0;              // fp16 rows past the end read as zero
    }
    const _Float16* xrow[TT];
    int64_t xlim[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        const int64_t t = tok0 + tt * 16 + li;
        xrow[tt] = p.x + (t < p.T ? t : 0) * p.ldx;
        xlim[tt] = t < p.T ? p.n : 0;
    }

    f4 acc[RG][TT], accl[RG][TT];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg)
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) acc[rg][tt] = accl[rg][tt] = f4{0.f, 0.f, 0.f, 0.f};

    const int64_t nchunks = (p.n + CK - 1) / CK;
    const int64_t c0 = KSPLIT ? (int64_t)blockIdx.y * NW + wave : 0, cstep = KSPLIT ? (int64_t)NW * gridDim.y : 1;

    auto load_w = [&](int64_t c, int rg) -> WR {
        const int64_t kg = c * CK + g * GK;
        WR w;
        if constexpr (CODES) {
            const uint8_t* wrow = p.w + rowc[rg] * p.wstride;
            // a piece that starts inside n lies inside the 16-byte padded row
            w.v[0] = kg < p.n ? *reinterpret_cast<const u4*>(wrow + kg * WT / 8) : u4{0u, 0u, 0u, 0u};
        } else {
            const _Float16* wrow = reinterpret_cast<const _Float16*>(p.w) + rowc[rg] * p.wstride;
#pragma unroll
            for (int jj = 0; jj < WV; ++jj) w.v[jj] = __builtin_bit_cast(u4, ld8(wrow, kg + jj * 8, wlim[rg], p.w_al));
        }
        return w;
    };
    auto frag = [&](const WR& w, int jj) -> h8 {
        if constexpr (NF) return expand_nf<WT>(nftab, WT == 4 ? w.v[0][jj & 3] : w.v[0][jj >> 1], jj & 1);
        else if constexpr (CODES) return expand<WT>(w.v[0], jj);
        else return __builtin_bit_cast(h8, w.v[jj]);
    };
    auto load_x = [&](int64_t c, int jj, int tt) -> h8 {
        return ld8(xrow[tt], c * CK + g * GK + jj * 8, xlim[tt], p.x_al);
    };

    // L codes: a lane's 16 bytes hold its B fragments of LNM k steps, so a chunk is LCK columns of
    // z and lane group g owns columns c LCK + g LGK ... of it.  A piece that starts inside r lies
    // inside the 16-byte padded row; past r nothing is read, and the z columns there (r .. r32:
    // written as zeros; beyond: not read) are zero, so whatever the codes' tail holds contributes
    // nothing.
    constexpr int LCK = LB == 16 ? 32 : 16 * 8 / LB * 4, LNM = LCK / 32, LGK = LCK / 4;
    auto load_l = [&](int64_t c, int rg) -> u4 {
        const int64_t q0 = c * LCK + g * LGK;
        return q0 < p.r ? *reinterpret_cast<const u4*>(p.lc + rowc[rg] * p.lcstride + q0 * LB / 8)
                        : u4{0u, 0u, 0u, 0u};
    };
    // decode: the codes of the wave's first L unit are fetched before the K loop (their address
    // depends on nothing computed here), so the L product does not wait on memory
    u4 lfirst = u4{0u, 0u, 0u, 0u};
    if constexpr (!ZP && LB != 16 && KSPLIT) {
        if (c0 < (p.r + LCK - 1) / LCK * LNM) lfirst = load_l(c0 / LNM, 0);
    }

    WR q[RG], qn[RG];
    if constexpr (TT == 1) {
        // decode: the next chunk's weights and all its x fragments are in flight during this one
        h8 a[NM], an[NM];
        if (c0 < nchunks) {
#pragma unroll
            for (int rg = 0; rg < RG; ++rg) q[rg] = load_w(c0, rg);
#pragma unroll
            for (int jj = 0; jj < NM; ++jj) a[jj] = load_x(c0, jj, 0);
        }
        for (int64_t c = c0; c < nchunks; c += cstep) {
            if (c + cstep < nchunks) {
#pragma unroll
                for (int rg = 0; rg < RG; ++rg) qn[rg] = load_w(c + cstep, rg);
#pragma unroll
                for (int jj = 0; jj < NM; ++jj) an[jj] = load_x(c + cstep, jj, 0);
            }
#pragma unroll
            for (int jj = 0; jj < NM; ++jj) {
#pragma unroll
                for (int rg = 0; rg < RG; ++rg) {
                    const h8 b = frag(q[rg], jj);
                    acc[rg][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[jj], b, acc[rg][0], 0, 0, 0);
                    if constexpr (PLANES2)
                        acc[rg][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[jj], nf2_lo(b), acc[rg][0], 0, 0, 0);
                }
            }
#pragma unroll
            for (int rg = 0; rg < RG; ++rg) q[rg] = qn[rg];
#pragma unroll
            for (int jj = 0; jj < NM; ++jj) a[jj] = an[jj];
        }
    } else {
        // prefill: weights one chunk ahead, x fragments one k step ahead; an expanded B fragment
        // feeds TT MFMAs and an x fragment RG of them
        h8 a[TT], an[TT];
        if (c0 < nchunks) {
#pragma unroll
            for (int rg = 0; rg < RG; ++rg) q[rg] = load_w(c0, rg);
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) a[tt] = load_x(c0, 0, tt);
        }
        for (int64_t c = c0; c < nchunks; c += cstep) {
            const bool more = c + cstep < nchunks;
            if (more) {
#pragma unroll
                for (int rg = 0; rg < RG; ++rg) qn[rg] = load_w(c + cstep, rg);
            }
#pragma unroll
            for (int jj = 0; jj < NM; ++jj) {
                if (jj + 1 < NM) {
#pragma unroll
                    for (int tt = 0; tt < TT; ++tt) an[tt] = load_x(c, jj + 1, tt);
                } else if (more) {
#pragma unroll
                    for (int tt = 0; tt < TT; ++tt) an[tt] = load_x(c + cstep, 0, tt);
                }
#pragma unroll
                for (int rg = 0; rg < RG; ++rg) {
                    const h8 b = frag(q[rg], jj);
#pragma unroll
                    for (int tt = 0; tt < TT; ++tt)
                        acc[rg][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[tt], b, acc[rg][tt], 0, 0, 0);
                    if constexpr (PLANES2) {
                        const h8 bl = nf2_lo(b);
#pragma unroll
                        for (int tt = 0; tt < TT; ++tt)
                            acc[rg][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[tt], bl, acc[rg][tt], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) a[tt] = an[tt];
            }
#pragma unroll
            for (int rg = 0; rg < RG; ++rg) q[rg] = qn[rg];
        }
    }

    // the L product: onto its own tile under the K split, else onto the scaled code sum
    auto& lacc = *(KSPLIT ? &accl : &acc);
    if constexpr (!ZP) {
        if constexpr (!KSPLIT) {  // s / k once per output
#pragma unroll
            for (int rg = 0; rg < RG; ++rg)
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) acc[rg][tt] = acc[rg][tt] * p.sk;
        }
        // the z fragment of token tile tt at columns qq .. qq + 7 as split halves; zero where an
        // L chunk of codes reaches past the z buffers' row (qq >= r32)
        auto load_z = [&](int tt, int64_t qq, h8& zh, h8& zl) {
            const int64_t zo = (tok0 + tt * 16 + li) * p.r32 + qq;
            const bool in = LB == 16 || qq < p.r32;
            if constexpr (KSPLIT) {  // the partial z of the z kernel's workgroups, added in order
                float zs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (li < p.T && in) {  // rows past T are zero
                    for (int ks = 0; ks < kDecodeSplitZ; ++ks) {
                        const f4* pp = reinterpret_cast<const f4*>(p.zp + (int64_t)ks * 16 * p.r32 + zo);
                        const f4 u = pp[0], v = pp[1];
#pragma unroll
                        for (int j = 0; j < 4; ++j) zs[j] += u[j], zs[4 + j] += v[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float zv = zs[j] * p.zscale;  // once, on the complete sum
                    zh[j] = (_Float16)zv;
                    zl[j] = (_Float16)(zv - (float)zh[j]);
                }
            } else if (in) {
                zl = *reinterpret_cast<const h8*>(p.zl + zo);
                zh = *reinterpret_cast<const h8*>(p.zh + zo);
            } else {
                zl = zh = h8{0, 0, 0, 0, 0, 0, 0, 0};
            }
        };
        if constexpr (LB == 16) {
            const int64_t lchunks = p.r32 / 32;
            for (int64_t c = c0; c < lchunks; c += cstep) {
                const int64_t qq = c * 32 + g * 8;
                h8 b[RG];
#pragma unroll
                for (int rg = 0; rg < RG; ++rg) b[rg] = ld8(p.L + rowc[rg] * p.ldl, qq, p.r, p.l_al);
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) {
                    h8 zl, zh;
                    load_z(tt, qq, zh, zl);
#pragma unroll
                    for (int rg = 0; rg < RG; ++rg) {
                        lacc[rg][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(zl, b[rg], lacc[rg][tt], 0, 0, 0);
                        lacc[rg][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(zh, b[rg], lacc[rg][tt], 0, 0, 0);
                    }
                }
            }
        } else {
            const int64_t lchunks = (p.r + LCK - 1) / LCK;
            if constexpr (KSPLIT) {
                // decode: the unit of work is one k step of one chunk, interleaved over the waves
                // (r = 256 at 4 bits is 2 chunks but 8 k steps: one per wave, as with fp16 L)
                for (int64_t u = c0; u < lchunks * LNM; u += cstep) {
                    const int64_t c = u / LNM;
                    const int jj = (int)(u % LNM);
                    if (c * LCK + jj * 8 >= p.r32) continue;  // no lane has z columns here
                    const h8 b = expand<LB>(u == c0 ? lfirst : load_l(c, 0), jj);
                    h8 zl, zh;
                    load_z(0, c * LCK + g * LGK + jj * 8, zh, zl);
                    lacc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(zl, b, lacc[0][0], 0, 0, 0);
                    lacc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(zh, b, lacc[0][0], 0, 0, 0);
                }
            } else {
                for (int64_t c = 0; c < lchunks; ++c) {
                    u4 lw[RG];
#pragma unroll
                    for (int rg = 0; rg < RG; ++rg) lw[rg] = load_l(c, rg);
#pragma unroll
                    for (int jj = 0; jj < LNM; ++jj) {
                        if (c * LCK + jj * 8 >= p.r32) break;
                        h8 b[RG];
#pragma unroll
                        for (int rg = 0; rg < RG; ++rg) b[rg] = expand<LB>(lw[rg], jj);
#pragma unroll
                        for (int tt = 0; tt < TT; ++tt) {
                            h8 zl, zh;
                            load_z(tt, c * LCK + g * LGK + jj * 8, zh, zl);
#pragma unroll
                            for (int rg = 0; rg < RG; ++rg) {
                                lacc[rg][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(zl, b[rg], lacc[rg][tt], 0, 0, 0);
                                lacc[rg][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(zh, b[rg], lacc[rg][tt], 0, 0, 0);
                            }
                        }
                    }
                }
            }
        }
    }

    if constexpr (KSPLIT) {  // partial tiles summed in wave order
        constexpr int NA = ZP ? 1 : 2;
        __shared__ f4 red[NW][NA][64];
        red[wave][0][lane] = acc[0][0];
        if constexpr (!ZP) red[wave][1][lane] = accl[0][0];
        __syncthreads();
        if (wave != 0) return;
        f4 s0 = red[0][0][lane], s1 = f4{0.f, 0.f, 0.f, 0.f};
        if constexpr (!ZP) s1 = red[0][1][lane];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            s0 += red[w][0][lane];
            if constexpr (!ZP) s1 += red[w][1][lane];
        }
        if constexpr (!ZP) accl[0][0] = s0 * p.sk + s1;
        else acc[0][0] = s0;
    }

    // D tile: column (weight row) = lane & 15, row (token) = 4 (lane >> 4) + register
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) {
        const int64_t row = row0 + rg * 16 + li;
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t t = tok0 + tt * 16 + g * 4 + e;
                if constexpr (!ZP) {
                    if (row < p.rows && t < p.T) {
                        float v = p.gs * lacc[rg][tt][e];
                        if (p.bias) v += p.bias[row];
                        if (p.y_f16) reinterpret_cast<_Float16*>(p.y)[t * p.ldy + row] = (_Float16)v;
                        else reinterpret_cast<float*>(p.y)[t * p.ldy + row] = v;
                    }
                } else if constexpr (KSPLIT) {  // this workgroup's partial z, every element written
                    // (code rows r .. r32 are clamped to row r - 1, not zero as fp16 rows are there)
                    p.ozp[((int64_t)blockIdx.y * 16 + t) * p.r32 + row] = CODES && row >= p.rows ? 0.f : acc[rg][tt][e];
                } else if (row < rows_out) {  // the whole [token rows][r32] buffers (zeros past T, r)
                    const float v = CODES && row >= p.rows ? 0.f : acc[rg][tt][e] * p.zscale;  // once, before the split
                    const _Float16 hi = (_Float16)v;
                    p.oh[t * p.r32 + row] = hi;
                    p.ol[t * p.r32 + row] = (_Float16)(v - (float)hi);
                }
            }
        }
    }
}

inline int64_t token_rows(int64_t T) {
    return T <= kDecodeMax ? 16 : ceil_div(T, kPrefillTiles * 16) * (kPrefillTiles * 16);
}

constexpr int kPrefillWaves = 4;   // waves per prefill workgroup (codes; the z product has one)

// the x extent of a layer's own grid: workgroups over its weight rows
template <bool ZP>
inline int64_t x_extent(const LinP& p) {
    const int64_t groups = ceil_div(ZP ? p.r32 : p.rows, 16);
    return p.T <= kDecodeMax ? groups : ceil_div(groups, ZP ? 1 : kPrefillWaves * kPrefillGroups);
}

// `count` layers in one grid.  ARG = LinP: the one layer ps[0] on its own grid.  ARG = GroupP: 1 ..
// CQ_LINEAR_GROUP_MAX layers (the same T and template parameters, each with a nonempty grid of its
// own), the members' x extents end to end, the y extent they share.
template <int WT, int QF, int LB, bool ZP, typename ARG>
void launch(const LinP* ps, int count, hipStream_t s) {
    ARG arg{};
    int64_t total = 0;
    if constexpr (std::is_same_v<ARG, GroupP>) {
        for (int i = 0; i < CQ_LINEAR_GROUP_MAX; ++i) {
            arg.first[i] = i < count ? (int32_t)total : INT32_MAX;
            if (i < count) {
                arg.m[i] = ps[i];
                total += x_extent<ZP>(ps[i]);
            }
        }
    } else {
        arg = ps[0];
        total = x_extent<ZP>(ps[0]);
    }
    const int64_t T = ps[0].T;
    if (T <= kDecodeMax) {
        constexpr int NW = ZP ? kDecodeWavesZ : kDecodeWaves;
        const dim3 grid((unsigned)total, ZP ? kDecodeSplitZ : 1);
        hipLaunchKernelGGL((linear_kernel<WT, QF, LB, ZP, 1, 1, NW, true, ARG>), grid, dim3(NW * 64), 0, s, arg);
    } else {
        constexpr int NW = ZP ? 1 : kPrefillWaves, RG = ZP ? 1 : kPrefillGroups;
        const dim3 grid((unsigned)total, (unsigned)ceil_div(T, kPrefillTiles * 16));
        hipLaunchKernelGGL((linear_kernel<WT, QF, LB, ZP, kPrefillTiles, RG, NW, false, ARG>), grid, dim3(NW * 64), 0, s,
                           arg);
    }
}

// the z launch over the layers zs[0 .. count) with factors, R as fp16 rows (r_bits = 16) or codes
template <typename ARG>
int launch_z(const LinP* zs, int count, int r_bits, hipStream_t s, const char* who) {
    if (r_bits == 16) launch<16, CQ_QFMT_UNIFORM, 16, true, ARG>(zs, count, s);
    else if (r_bits == 2) launch<2, CQ_QFMT_UNIFORM, 16, true, ARG>(zs, count, s);
    else launch<4, CQ_QFMT_UNIFORM, 16, true, ARG>(zs, count, s);
    char what[64];
    snprintf(what, sizeof what, "%s (z)", who);
    return check_launch(what);
}

// the runtime triple (bits, nf, l_bits) of a code + L launch as template arguments: calls
// f(WT, QF, LB) with integral constants
template <int V>
using Const = std::integral_constant<int, V>;
template <class F>
void with_formats(int bits, bool nf, int l_bits, F f) {
    auto with_lb = [&](auto wt, auto qf) {
        if (l_bits == 2) f(wt, qf, Const<2>{});
        else if (l_bits == 4) f(wt, qf, Const<4>{});
        else f(wt, qf, Const<16>{});
    };
    if (nf) {
        if (bits == 2) with_lb(Const<2>{}, Const<CQ_QFMT_NF>{});
        else with_lb(Const<4>{}, Const<CQ_QFMT_NF>{});
    } else {
        if (bits == 2) with_lb(Const<2>{}, Const<CQ_QFMT_UNIFORM>{});
        else with_lb(Const<4>{}, Const<CQ_QFMT_UNIFORM>{});
    }
}

// Gated pair (cq_linear_glu_forward): h = act(v_g) * v_u with v_g, v_u the fp32 values linear_kernel's
// epilogue forms for the layers g (gate) and u (up), which share x, T, n, rows and the template
// parameters.  A wave owns the SAME weight rows of both layers, so both pre-activations of an output
// sit in its registers and neither is written.  The row-to-wave mapping differs from linear_kernel's
// (a prefill wave owns RG = 2 row groups of each layer where linear_kernel's owns 4 of one: the same 16
// accumulator tiles); what one output goes through does not: the loaders, `expand`, the chunk and k step
// order, hi plane before lo, s / k on the accumulator before the L product resp. s0 * sk + s1 after the
// ordered LDS add, gs, then the bias are linear_kernel's, line by line, so v_g and v_u have the bits of
// the layers run alone.  An x fragment is loaded once and feeds both layers.  The two L products run
// one after the other, each over its own rank (r = 0: no iterations).  Decode: the four partial tiles
// of a wave (code and L sums of g and of u) go through 32 KB of LDS and wave 0 adds them in wave order.
struct GluP {
    LinP g, u;                 // y, y_f16, ldy: not used
    int act;                   // CQ_ACT_*
    void* h; int h_f16; int64_t ldh;
};

template <int WT, int QF, int LB, int TT, int RG, int NW, bool KSPLIT>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(TT > 1 ? 2 : 1))) void
linear_glu_kernel(const GluP arg) {
    constexpr int M = 2;
    auto mp = [&](int mi) -> const LinP& { return mi ? arg.u : arg.g; };
    const LinP& p = arg.g;  // what the two layers share: x, ldx, x_al, T, n, rows
    constexpr bool NF = QF == CQ_QFMT_NF;
    constexpr bool PLANES2 = NF && WT == 2;
    static_assert(WT == 2 || WT == 4, "the layers' own weights are codes");
    const uint32_t* nftab = nullptr;
    if constexpr (NF) {  // before any wave leaves
        __shared__ uint32_t tab[WT == 4 ? 256 : 512];
        fill_nf_table<WT>(tab, threadIdx.x, NW * 64);
        __syncthreads();
        nftab = tab;
    }
    constexpr int CK = 16 * 8 / WT * 4;   // k per chunk: 4 lane groups x one 16-byte load
    constexpr int NM = CK / 32;           // MFMA k steps per chunk
    constexpr int GK = CK / 4;            // k per lane group
    static_assert(!KSPLIT || (TT == 1 && RG == 1), "the K split reduces one tile per layer");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int64_t row0 = (KSPLIT ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * NW + wave) * (16 * RG);
    const int64_t tok0 = KSPLIT ? 0 : (int64_t)blockIdx.y * (TT * 16);
    if (!KSPLIT && row0 >= p.rows) return;

    int64_t rowc[RG];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) {
        const int64_t row = row0 + rg * 16 + li;
        rowc[rg] = row < p.rows ? row : p.rows - 1;
    }
    const _Float16* xrow[TT];
    int64_t xlim[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        const int64_t t = tok0 + tt * 16 + li;
        xrow[tt] = p.x + (t < p.T ? t : 0) * p.ldx;
        xlim[tt] = t < p.T ? p.n : 0;
    }

    f4 acc[M][RG][TT], accl[M];
#pragma unroll
    for (int mi = 0; mi < M; ++mi) {
        accl[mi] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int rg = 0; rg < RG; ++rg)
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) acc[mi][rg][tt] = f4{0.f, 0.f, 0.f, 0.f};
    }

    const int64_t nchunks = (p.n + CK - 1) / CK;
    const int64_t c0 = KSPLIT ? wave : 0, cstep = KSPLIT ? NW : 1;

    auto load_w = [&](int mi, int64_t c, int rg) -> u4 {
        const int64_t kg = c * CK + g * GK;
        const uint8_t* wrow = mp(mi).w + rowc[rg] * mp(mi).wstride;
        // a piece that starts inside n lies inside the 16-byte padded row
        return kg < p.n ? *reinterpret_cast<const u4*>(wrow + kg * WT / 8) : u4{0u, 0u, 0u, 0u};
    };
    auto frag = [&](const u4& w, int jj) -> h8 {
        if constexpr (NF) return expand_nf<WT>(nftab, WT == 4 ? w[jj & 3] : w[jj >> 1], jj & 1);
        else return expand<WT>(w, jj);
    };
    auto load_x = [&](int64_t c, int jj, int tt) -> h8 {
        return ld8(xrow[tt], c * CK + g * GK + jj * 8, xlim[tt], p.x_al);
    };

    // L codes, as in linear_kernel: nothing is read from q0 >= r on
    constexpr int LCK = LB == 16 ? 32 : 16 * 8 / LB * 4, LNM = LCK / 32, LGK = LCK / 4;
    auto load_l = [&](const LinP& pm, int64_t c, int rg) -> u4 {
        const int64_t q0 = c * LCK + g * LGK;
        return q0 < pm.r ? *reinterpret_cast<const u4*>(pm.lc + rowc[rg] * pm.lcstride + q0 * LB / 8)
                         : u4{0u, 0u, 0u, 0u};
    };
    u4 lfirst[M] = {u4{0u, 0u, 0u, 0u}, u4{0u, 0u, 0u, 0u}};
    if constexpr (LB != 16 && KSPLIT) {  // decode: both layers' first L unit before the K loop
#pragma unroll
        for (int mi = 0; mi < M; ++mi)
            if (c0 < (mp(mi).r + LCK - 1) / LCK * LNM) lfirst[mi] = load_l(mp(mi), c0 / LNM, 0);
    }

    u4 q[M][RG], qn[M][RG];
    if constexpr (TT == 1) {
        // decode: the next chunk's codes of both layers and all its x fragments are in flight during this one
        h8 a[NM], an[NM];
        if (c0 < nchunks) {
#pragma unroll
            for (int mi = 0; mi < M; ++mi) q[mi][0] = load_w(mi, c0, 0);
#pragma unroll
            for (int jj = 0; jj < NM; ++jj) a[jj] = load_x(c0, jj, 0);
        }
        for (int64_t c = c0; c < nchunks; c += cstep) {
            if (c + cstep < nchunks) {
#pragma unroll
                for (int mi = 0; mi < M; ++mi) qn[mi][0] = load_w(mi, c + cstep, 0);
#pragma unroll
                for (int jj = 0; jj < NM; ++jj) an[jj] = load_x(c + cstep, jj, 0);
            }
#pragma unroll
            for (int jj = 0; jj < NM; ++jj) {
#pragma unroll
                for (int mi = 0; mi < M; ++mi) {
                    const h8 b = frag(q[mi][0], jj);
                    acc[mi][0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[jj], b, acc[mi][0][0], 0, 0, 0);
                    if constexpr (PLANES2)
                        acc[mi][0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[jj], nf2_lo(b), acc[mi][0][0], 0, 0, 0);
                }
            }
#pragma unroll
            for (int mi = 0; mi < M; ++mi) q[mi][0] = qn[mi][0];
#pragma unroll
            for (int jj = 0; jj < NM; ++jj) a[jj] = an[jj];
        }
    } else {
        // prefill: codes one chunk ahead, x fragments one k step ahead; an x fragment feeds M RG MFMAs
        h8 a[TT], an[TT];
        if (c0 < nchunks) {
#pragma unroll
            for (int mi = 0; mi < M; ++mi)
#pragma unroll
                for (int rg = 0; rg < RG; ++rg) q[mi][rg] = load_w(mi, c0, rg);
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) a[tt] = load_x(c0, 0, tt);
        }
        for (int64_t c = c0; c < nchunks; c += cstep) {
            const bool more = c + cstep < nchunks;
            if (more) {
#pragma unroll
                for (int mi = 0; mi < M; ++mi)
#pragma unroll
                    for (int rg = 0; rg < RG; ++rg) qn[mi][rg] = load_w(mi, c + cstep, rg);
            }
#pragma unroll
            for (int jj = 0; jj < NM; ++jj) {
                if (jj + 1 < NM) {
#pragma unroll
                    for (int tt = 0; tt < TT; ++tt) an[tt] = load_x(c, jj + 1, tt);
                } else if (more) {
#pragma unroll
                    for (int tt = 0; tt < TT; ++tt) an[tt] = load_x(c + cstep, 0, tt);
                }
#pragma unroll
                for (int mi = 0; mi < M; ++mi)
#pragma unroll
                    for (int rg = 0; rg < RG; ++rg) {
                        const h8 b = frag(q[mi][rg], jj);
#pragma unroll
                        for (int tt = 0; tt < TT; ++tt)
                            acc[mi][rg][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[tt], b, acc[mi][rg][tt], 0, 0, 0);
                        if constexpr (PLANES2) {
                            const h8 bl = nf2_lo(b);
#pragma unroll
                            for (int tt = 0; tt < TT; ++tt)
                                acc[mi][rg][tt] =
                                    __builtin_amdgcn_mfma_f32_16x16x32_f16(a[tt], bl, acc[mi][rg][tt], 0, 0, 0);
                        }
                    }
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) a[tt] = an[tt];
            }
#pragma unroll
            for (int mi = 0; mi < M; ++mi)
#pragma unroll
                for (int rg = 0; rg < RG; ++rg) q[mi][rg] = qn[mi][rg];
        }
    }

    // the z fragment of layer pm, token tile tt, columns qq .. qq + 7 as split halves (linear_kernel's)
    auto load_z = [&](const LinP& pm, int tt, int64_t qq, h8& zh, h8& zl) {
        const int64_t zo = (tok0 + tt * 16 + li) * pm.r32 + qq;
        const bool in = LB == 16 || qq < pm.r32;
        if constexpr (KSPLIT) {  // the partial z of the z kernel's workgroups, added in order
            float zs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (li < pm.T && in) {  // rows past T are zero
                for (int ks = 0; ks < kDecodeSplitZ; ++ks) {
                    const f4* pp = reinterpret_cast<const f4*>(pm.zp + (int64_t)ks * 16 * pm.r32 + zo);
                    const f4 u = pp[0], v = pp[1];
#pragma unroll
                    for (int j = 0; j < 4; ++j) zs[j] += u[j], zs[4 + j] += v[j];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float zv = zs[j] * pm.zscale;  // once, on the complete sum
                zh[j] = (_Float16)zv;
                zl[j] = (_Float16)(zv - (float)zh[j]);
            }
        } else if (in) {
            zl = *reinterpret_cast<const h8*>(pm.zl + zo);
            zh = *reinterpret_cast<const h8*>(pm.zh + zo);
        } else {
            zl = zh = h8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    };

    // the L products, one layer after the other: onto its own tile under the K split, else onto the
    // scaled code sum
#pragma unroll
    for (int mi = 0; mi < M; ++mi) {
        const LinP& pm = mp(mi);
        if constexpr (!KSPLIT) {  // s / k once per output
#pragma unroll
            for (int rg = 0; rg < RG; ++rg)
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) acc[mi][rg][tt] = acc[mi][rg][tt] * pm.sk;
        }
        if constexpr (LB == 16) {
            const int64_t lchunks = pm.r32 / 32;
            for (int64_t c = c0; c < lchunks; c += cstep) {
                const int64_t qq = c * 32 + g * 8;
                h8 b[RG];
#pragma unroll
                for (int rg = 0; rg < RG; ++rg) b[rg] = ld8(pm.L + rowc[rg] * pm.ldl, qq, pm.r, pm.l_al);
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) {
                    h8 zl, zh;
                    load_z(pm, tt, qq, zh, zl);
#pragma unroll
                    for (int rg = 0; rg < RG; ++rg) {
                        f4& d = KSPLIT ? accl[mi] : acc[mi][rg][tt];
                        d = __builtin_amdgcn_mfma_f32_16x16x32_f16(zl, b[rg], d, 0, 0, 0);
                        d = __builtin_amdgcn_mfma_f32_16x16x32_f16(zh, b[rg], d, 0, 0, 0);
                    }
                }
            }
        } else {
            const int64_t lchunks = (pm.r + LCK - 1) / LCK;
            if constexpr (KSPLIT) {
                // decode: one k step of one chunk per unit, interleaved over the waves
                for (int64_t u = c0; u < lchunks * LNM; u += cstep) {
                    const int64_t c = u / LNM;
                    const int jj = (int)(u % LNM);
                    if (c * LCK + jj * 8 >= pm.r32) continue;  // no lane has z columns here
                    const h8 b = expand<LB>(u == c0 ? lfirst[mi] : load_l(pm, c, 0), jj);
                    h8 zl, zh;
                    load_z(pm, 0, c * LCK + g * LGK + jj * 8, zh, zl);
                    accl[mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(zl, b, accl[mi], 0, 0, 0);
                    accl[mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(zh, b, accl[mi], 0, 0, 0);
                }
            } else {
                for (int64_t c = 0; c < lchunks; ++c) {
                    u4 lw[RG];
#pragma unroll
                    for (int rg = 0; rg < RG; ++rg) lw[rg] = load_l(pm, c, rg);
#pragma unroll
                    for (int jj = 0; jj < LNM; ++jj) {
                        if (c * LCK + jj * 8 >= pm.r32) break;
                        h8 b[RG];
#pragma unroll
                        for (int rg = 0; rg < RG; ++rg) b[rg] = expand<LB>(lw[rg], jj);
#pragma unroll
                        for (int tt = 0; tt < TT; ++tt) {
                            h8 zl, zh;
                            load_z(pm, tt, c * LCK + g * LGK + jj * 8, zh, zl);
#pragma unroll
                            for (int rg = 0; rg < RG; ++rg) {
                                acc[mi][rg][tt] =
                                    __builtin_amdgcn_mfma_f32_16x16x32_f16(zl, b[rg], acc[mi][rg][tt], 0, 0, 0);
                                acc[mi][rg][tt] =
                                    __builtin_amdgcn_mfma_f32_16x16x32_f16(zh, b[rg], acc[mi][rg][tt], 0, 0, 0);
                            }
                        }
                    }
                }
            }
        }
    }

    if constexpr (KSPLIT) {  // the four partial tiles summed in wave order
        __shared__ f4 red[NW][2 * M][64];
#pragma unroll
        for (int mi = 0; mi < M; ++mi) {
            red[wave][2 * mi][lane] = acc[mi][0][0];
            red[wave][2 * mi + 1][lane] = accl[mi];
        }
        __syncthreads();
        if (wave != 0) return;
#pragma unroll
        for (int mi = 0; mi < M; ++mi) {
            f4 s0 = red[0][2 * mi][lane], s1 = red[0][2 * mi + 1][lane];
#pragma unroll
            for (int w = 1; w < NW; ++w) {
                s0 += red[w][2 * mi][lane];
                s1 += red[w][2 * mi + 1][lane];
            }
            acc[mi][0][0] = s0 * mp(mi).sk + s1;
        }
    }

    // D tile: column (weight row) = lane & 15, row (token) = 4 (lane >> 4) + register
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) {
        const int64_t row = row0 + rg * 16 + li;
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t t = tok0 + tt * 16 + g * 4 + e;
                if (row < p.rows && t < p.T) {
                    float vg = arg.g.gs * acc[0][rg][tt][e];
                    if (arg.g.bias) vg += arg.g.bias[row];
                    float vu = arg.u.gs * acc[1][rg][tt][e];
                    if (arg.u.bias) vu += arg.u.bias[row];
                    float a = vg;
                    if (arg.act == CQ_ACT_SILU) {  // the device library's expf, one correctly rounded division
                        const float ex = expf(-vg);
                        const float d = 1.0f + ex;
                        a = vg / d;
                    }
                    const float h32 = a * vu;  // one fp32 multiply
                    if (arg.h_f16) reinterpret_cast<_Float16*>(arg.h)[t * arg.ldh + row] = (_Float16)h32;
                    else reinterpret_cast<float*>(arg.h)[t * arg.ldh + row] = h32;
                }
            }
        }
    }
}

constexpr int kGluPrefillGroups = 2;  // 16-row groups of each layer per prefill wave

template <int WT, int QF, int LB>
void launch_glu(const GluP& a, hipStream_t s) {
    const int64_t groups = ceil_div(a.g.rows, 16);
    if (a.g.T <= kDecodeMax) {
        hipLaunchKernelGGL((linear_glu_kernel<WT, QF, LB, 1, 1, kDecodeWaves, true>), dim3((unsigned)groups),
                           dim3(kDecodeWaves * 64), 0, s, a);
    } else {
        const dim3 grid((unsigned)ceil_div(groups, kPrefillWaves * kGluPrefillGroups),
                        (unsigned)ceil_div(a.g.T, kPrefillTiles * 16));
        hipLaunchKernelGGL((linear_glu_kernel<WT, QF, LB, kPrefillTiles, kGluPrefillGroups, kPrefillWaves, false>), grid,
                           dim3(kPrefillWaves * 64), 0, s, a);
    }
}

// with_y = false: y, y_dtype and ldy are neither used nor checked (a member of cq_linear_glu_args)
int validate(const cq_linear_packed_args* a, bool with_y = true) {
    const char* who = "cq_linear";
    CQ_REQUIRE(a != nullptr, "cq_linear: null args");
    CQ_REQUIRE(a->bits == 2 || a->bits == 4, "cq_linear: bits %d not in {2, 4}", a->bits);
    if (int st = validate_factor_bits(who, a->l_bits, a->r_bits)) return st;
    const bool lcoded = a->r > 0 && coded(a->l_bits), rcoded = a->r > 0 && coded(a->r_bits);
    CQ_REQUIRE(a->tokens >= 0 && a->m > 0 && a->n > 0 && a->r >= 0, "cq_linear: bad shape tokens=%lld m=%lld n=%lld r=%lld",
               (long long)a->tokens, (long long)a->m, (long long)a->n, (long long)a->r);
    if (int st = validate_rank(who, a->r)) return st;
    CQ_REQUIRE(a->tokens <= (int64_t)65535 * 64 && a->m <= ((int64_t)1 << 31), "cq_linear: shape too large");
    CQ_REQUIRE(!with_y || a->y_dtype == CQ_F32 || a->y_dtype == CQ_F16, "cq_linear: y dtype %d not fp32 / fp16",
               a->y_dtype);
    CQ_REQUIRE(a->x && a->codes && (!with_y || a->y), "cq_linear: null x / codes / y");
    if (int st = validate_operands(a, who, lcoded, rcoded)) return st;
    if (int st = validate_fp16_pointers(who, a->x, a->L, a->R)) return st;
    CQ_REQUIRE((!with_y || !misaligned(a->y, a->y_dtype == CQ_F16 ? 1 : 3)) && !misaligned(a->bias, 3),
               "cq_linear: misaligned y / bias pointer");
    CQ_REQUIRE(a->ldx >= a->n && (!with_y || a->ldy >= a->m) &&
                   (a->r == 0 || ((lcoded || a->ldl >= a->r) && (rcoded || a->ldr >= a->n))),
               "cq_linear: leading dimension smaller than the row");
    return CQ_OK;
}

size_t workspace_bytes(int64_t tokens, int64_t r) {
    if (r <= 0 || tokens <= 0) return 0;
    if (tokens <= kDecodeMax) return (size_t)(kDecodeSplitZ * 16 * r32_of(r)) * sizeof(float);
    return (size_t)(2 * token_rows(tokens) * r32_of(r)) * sizeof(uint16_t);
}

// cq_linear_args is the leading part of cq_linear_packed_args: the same layer with fp16 factors
cq_linear_packed_args with_fp16_factors(const cq_linear_args* a) {
    cq_linear_packed_args b{};
    b.x = a->x, b.ldx = a->ldx;
    b.tokens = a->tokens, b.m = a->m, b.n = a->n, b.r = a->r;
    b.bits = a->bits;
    b.codes = a->codes, b.code_stride = a->code_stride;
    b.qscale = a->qscale, b.gscale = a->gscale;
    b.L = a->L, b.ldl = a->ldl;
    b.R = a->R, b.ldr = a->ldr;
    b.bias = a->bias;
    b.y = a->y, b.y_dtype = a->y_dtype, b.ldy = a->ldy;
    b.l_bits = b.r_bits = 16;
    return b;
}

// The kernels' parameters of one validated layer on its own workspace ws: z, the z product (used
// for r > 0 only), and p, codes + L + epilogue.  Shared by every entry, so a grouped member's
// parameters are the ones it runs with alone.
void layer_params(const cq_linear_packed_args* a, bool nf, void* ws, LinP& z, LinP& p) {
    const bool lcoded = a->r > 0 && coded(a->l_bits), rcoded = a->r > 0 && coded(a->r_bits);
    p = LinP{};
    p.x = reinterpret_cast<const _Float16*>(a->x);
    p.ldx = a->ldx;
    p.x_al = al16(a->x, a->ldx);
    p.T = a->tokens;
    p.n = a->n;
    p.r = a->r;
    p.r32 = r32_of(a->r);
    _Float16* zh = reinterpret_cast<_Float16*>(ws);
    _Float16* zl = zh ? zh + token_rows(a->tokens) * p.r32 : nullptr;
    p.zscale = factor_scale(a, lcoded, rcoded);
    z = p;  // z = x R^T as split halves
    if (a->r > 0) {
        z.rows = a->r;
        z.ozp = reinterpret_cast<float*>(ws);
        z.oh = zh;
        z.ol = zl;
        if (rcoded) {
            z.w = a->R_codes;
            z.wstride = a->r_code_stride;
        } else {
            z.w = reinterpret_cast<const uint8_t*>(a->R);
            z.wstride = a->ldr;
            z.w_al = al16(a->R, a->ldr);
        }
    }
    p.rows = a->m;
    p.w = a->codes;
    p.wstride = a->code_stride;
    if (lcoded) {
        p.lc = a->L_codes;
        p.lcstride = a->l_code_stride;
    } else {
        p.L = reinterpret_cast<const _Float16*>(a->L);
        p.ldl = a->ldl;
        p.l_al = a->r > 0 && al16(a->L, a->ldl);
    }
    p.zp = reinterpret_cast<const float*>(ws);
    p.zh = zh;
    p.zl = zl;
    p.sk = code_scale(a->qscale, a->bits, nf);
    p.gs = a->gscale;
    p.bias = a->bias;
    p.y = a->y;
    p.y_f16 = a->y_dtype == CQ_F16;
    p.ldy = a->ldy;
}

// the layers of one call, in member order: the one layer, a group's members, or a pair's gate and up
struct Members {
    const cq_linear_packed_args* m[CQ_LINEAR_GROUP_MAX];
    int count;
};
Members members_of(const cq_linear_group_args* g) {
    Members ms{};
    for (ms.count = 0; ms.count < g->count; ++ms.count) ms.m[ms.count] = &g->members[ms.count];
    return ms;
}
Members members_of(const cq_linear_glu_args* a) { return Members{{&a->gate, &a->up}, 2}; }

// the call's workspace: the members' own, at 16-byte aligned offsets (offs, may be null) in member order
size_t group_offsets(const Members& ms, size_t* offs) {
    size_t total = 0;
    for (int i = 0; i < ms.count; ++i) {
        if (offs) offs[i] = total;
        total += align_up(workspace_bytes(ms.m[i]->tokens, ms.m[i]->r), 16);
    }
    return total;
}

// The kernels' parameters of validated members on the workspace ws: ps[i] is member i's, zs[0 .. nz)
// the z products of the members with factors, whose formats l_bits / r_bits are (validate_members:
// all the same; 16 = fp16 rows).
void prepare_members(const Members& ms, bool nf, void* ws, const size_t* offs, LinP* zs, LinP* ps, int& nz, int& l_bits,
                     int& r_bits) {
    nz = 0, l_bits = r_bits = 16;
    for (int i = 0; i < ms.count; ++i) {
        const cq_linear_packed_args* a = ms.m[i];
        LinP z;
        layer_params(a, nf, static_cast<char*>(ws) + offs[i], z, ps[i]);
        if (a->r > 0) {
            zs[nz++] = z;
            l_bits = coded(a->l_bits) ? a->l_bits : 16;
            r_bits = coded(a->r_bits) ? a->r_bits : 16;
        }
    }
}

// What the members of a group or a pair must pass, decided on the host before any launch: each its
// own checks (its message with `entry` and its name in front) and q_format's, then the fields that
// all share with the first member, and the factor formats with the first member that has factors.
int validate_members(const char* entry, const char* const* names, const Members& ms, int q_format, bool with_y,
                     bool same_m) {
    int ranked = -1;  // the first member with factors
    for (int i = 0; i < ms.count; ++i) {
        const cq_linear_packed_args* a = ms.m[i];
        char who[64];
        snprintf(who, sizeof who, "%s: %s", entry, names[i]);
        if (int st = validate(a, with_y)) {
            char msg[400];
            snprintf(msg, sizeof msg, "%s", cq_last_error());
            return set_error(st, "%s: %s", who, msg);
        }
        if (int st = validate_format(who, q_format, a->qscale)) return st;
#define CQ_SAME(field, fmt, cast, ref)                                                                           \
    CQ_REQUIRE(a->field == ms.m[ref]->field, "%s: " #field " " fmt " differs from %s's " fmt, who, (cast)a->field, \
               names[ref], (cast)ms.m[ref]->field)
        CQ_SAME(x, "%p", const void*, 0);
        CQ_SAME(ldx, "%lld", long long, 0);
        CQ_SAME(tokens, "%lld", long long, 0);
        CQ_SAME(n, "%lld", long long, 0);
        if (same_m) CQ_SAME(m, "%lld", long long, 0);
        CQ_SAME(bits, "%d", int, 0);
        if (with_y) CQ_SAME(y_dtype, "%d", int, 0);
        if (a->r > 0) {
            if (ranked < 0) ranked = i;
            CQ_SAME(l_bits, "%d", int, ranked);
            CQ_SAME(r_bits, "%d", int, ranked);
        }
#undef CQ_SAME
    }
    return CQ_OK;
}

int forward(const cq_linear_packed_args* a, int q_format, void* ws, size_t ws_bytes, void* stream, const char* who) {
    if (int st = validate(a)) return st;
    if (int st = validate_format(who, q_format, a->qscale)) return st;
    if (a->tokens == 0) return CQ_OK;
    if (int st = check_workspace(workspace_bytes(a->tokens, a->r), ws, ws_bytes, who)) return st;
    hipStream_t s = as_stream(stream);
    const size_t off = 0;
    LinP z, p;
    int nz, l_bits, r_bits;
    prepare_members(Members{{a}, 1}, q_format == CQ_QFMT_NF, ws, &off, &z, &p, nz, l_bits, r_bits);
    if (nz > 0)
        if (int st = launch_z<LinP>(&z, 1, r_bits, s, who)) return st;
    with_formats(a->bits, q_format == CQ_QFMT_NF, l_bits,
                 [&](auto wt, auto qf, auto lb) { launch<wt(), qf(), lb(), false, LinP>(&p, 1, s); });
    return check_launch(who);
}

constexpr const char* kGroupWho = "cq_linear_group_forward";
constexpr const char* kGroupNames[] = {"member 0", "member 1", "member 2", "member 3",
                                       "member 4", "member 5", "member 6", "member 7"};
static_assert(sizeof kGroupNames / sizeof *kGroupNames == CQ_LINEAR_GROUP_MAX, "one name per member");

int validate_group(const cq_linear_group_args* g) {
    CQ_REQUIRE(g != nullptr, "%s: null args", kGroupWho);
    CQ_REQUIRE(g->count >= 1 && g->count <= CQ_LINEAR_GROUP_MAX, "%s: count %d not in 1 .. %d", kGroupWho, g->count,
               CQ_LINEAR_GROUP_MAX);
    CQ_REQUIRE(g->members != nullptr, "%s: null members", kGroupWho);
    CQ_REQUIRE(g->q_format == CQ_QFMT_UNIFORM || g->q_format == CQ_QFMT_NF, "%s: unknown q_format %d", kGroupWho,
               g->q_format);
    return validate_members(kGroupWho, kGroupNames, members_of(g), g->q_format, true, false);
}

int group_forward(const cq_linear_group_args* g, void* ws, size_t ws_bytes, void* stream) {
    if (int st = validate_group(g)) return st;
    if (g->members[0].tokens == 0) return CQ_OK;
    const Members ms = members_of(g);
    size_t offs[CQ_LINEAR_GROUP_MAX];
    if (int st = check_workspace(group_offsets(ms, offs), ws, ws_bytes, kGroupWho)) return st;
    const bool nf = g->q_format == CQ_QFMT_NF;
    hipStream_t s = as_stream(stream);
    LinP zs[CQ_LINEAR_GROUP_MAX], ps[CQ_LINEAR_GROUP_MAX];
    int nz, l_bits, r_bits;
    prepare_members(ms, nf, ws, offs, zs, ps, nz, l_bits, r_bits);
    if (nz > 0)  // one z launch over the members with factors
        if (int st = launch_z<GroupP>(zs, nz, r_bits, s, kGroupWho)) return st;
    with_formats(ms.m[0]->bits, nf, l_bits,
                 [&](auto wt, auto qf, auto lb) { launch<wt(), qf(), lb(), false, GroupP>(ps, ms.count, s); });
    return check_launch(kGroupWho);
}

constexpr const char* kGluWho = "cq_linear_glu_forward";
constexpr const char* kGluNames[] = {"gate", "up"};

int validate_glu(const cq_linear_glu_args* a) {
    CQ_REQUIRE(a != nullptr, "%s: null args", kGluWho);
    CQ_REQUIRE(a->q_format == CQ_QFMT_UNIFORM || a->q_format == CQ_QFMT_NF, "%s: unknown q_format %d", kGluWho,
               a->q_format);
    CQ_REQUIRE(a->act == CQ_ACT_IDENTITY || a->act == CQ_ACT_SILU, "%s: unknown act %d", kGluWho, a->act);
    CQ_REQUIRE(a->h_dtype == CQ_F32 || a->h_dtype == CQ_F16, "%s: h_dtype %d not fp32 / fp16", kGluWho, a->h_dtype);
    if (int st = validate_members(kGluWho, kGluNames, members_of(a), a->q_format, false, true)) return st;
    CQ_REQUIRE(a->h != nullptr, "%s: null h", kGluWho);
    CQ_REQUIRE(!misaligned(a->h, a->h_dtype == CQ_F16 ? 1 : 3), "%s: misaligned h pointer", kGluWho);
    CQ_REQUIRE(a->ldh >= a->gate.m, "%s: ldh %lld < m %lld", kGluWho, (long long)a->ldh, (long long)a->gate.m);
    return CQ_OK;
}

int glu_forward(const cq_linear_glu_args* a, void* ws, size_t ws_bytes, void* stream) {
    if (int st = validate_glu(a)) return st;
    if (a->gate.tokens == 0) return CQ_OK;
    const Members ms = members_of(a);
    size_t offs[2];
    if (int st = check_workspace(group_offsets(ms, offs), ws, ws_bytes, kGluWho)) return st;
    const bool nf = a->q_format == CQ_QFMT_NF;
    hipStream_t s = as_stream(stream);
    LinP zs[2], ps[2];
    int nz, l_bits, r_bits;
    prepare_members(ms, nf, ws, offs, zs, ps, nz, l_bits, r_bits);
    GluP gp{};
    gp.g = ps[0], gp.u = ps[1];
    gp.act = a->act;
    gp.h = a->h;
    gp.h_f16 = a->h_dtype == CQ_F16;
    gp.ldh = a->ldh;
    if (nz > 0)  // the grouped z launch over the members with factors, unchanged
        if (int st = launch_z<GroupP>(zs, nz, r_bits, s, kGluWho)) return st;
    with_formats(a->gate.bits, nf, l_bits, [&](auto wt, auto qf, auto lb) { launch_glu<wt(), qf(), lb()>(gp, s); });
    return check_launch(kGluWho);
}

}  // namespace
}  // namespace cq

using namespace cq;

extern "C" size_t cq_linear_workspace(const cq_linear_args* a) {
    return a == nullptr ? 0 : workspace_bytes(a->tokens, a->r);
}

extern "C" size_t cq_linear_packed_workspace(const cq_linear_packed_args* a) {
    return a == nullptr ? 0 : workspace_bytes(a->tokens, a->r);
}

extern "C" int cq_linear_forward(const cq_linear_args* a, void* ws, size_t ws_bytes, void* stream) {
    CQ_REQUIRE(a != nullptr, "cq_linear: null args");
    const cq_linear_packed_args b = with_fp16_factors(a);
    return forward(&b, CQ_QFMT_UNIFORM, ws, ws_bytes, stream, "cq_linear_forward");
}

extern "C" int cq_linear_packed_forward(const cq_linear_packed_args* a, void* ws, size_t ws_bytes, void* stream) {
    return forward(a, CQ_QFMT_UNIFORM, ws, ws_bytes, stream, "cq_linear_packed_forward");
}

extern "C" size_t cq_linear_group_workspace(const cq_linear_group_args* g) {
    if (g == nullptr || g->members == nullptr || g->count < 1 || g->count > CQ_LINEAR_GROUP_MAX) return 0;
    return group_offsets(members_of(g), nullptr);
}

extern "C" int cq_linear_group_forward(const cq_linear_group_args* g, void* ws, size_t ws_bytes, void* stream) {
    return group_forward(g, ws, ws_bytes, stream);
}

extern "C" size_t cq_linear_codebook_workspace(const cq_linear_codebook_args* a) {
    return a == nullptr ? 0 : workspace_bytes(a->p.tokens, a->p.r);
}

extern "C" int cq_linear_codebook_forward(const cq_linear_codebook_args* a, void* ws, size_t ws_bytes, void* stream) {
    CQ_REQUIRE(a != nullptr, "cq_linear_codebook_forward: null args");
    return forward(&a->p, a->q_format, ws, ws_bytes, stream, "cq_linear_codebook_forward");
}

extern "C" size_t cq_linear_glu_workspace(const cq_linear_glu_args* a) {
    return a == nullptr ? 0 : group_offsets(members_of(a), nullptr);
}

extern "C" int cq_linear_glu_forward(const cq_linear_glu_args* a, void* ws, size_t ws_bytes, void* stream) {
    return glu_forward(a, ws, ws_bytes, stream);
}
