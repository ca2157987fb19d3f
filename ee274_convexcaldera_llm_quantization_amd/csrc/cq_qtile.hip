// The Q step's kernels on the split-fp16 operand tile (cq_x3_tile.h): the tiled fused Q update
// (q_update_v_kernel on the 16x16x32 ring loop, q_update_x3_kernel for unaligned shapes), the
// streaming first-step quantiser, and the fused residual + split that feeds the LR step.
// (The row-panel Q update for r <= 256 is cq_qupdate.hip, which builds with other flags.)
#include <numeric>

#include "cq_x3_tile.h"

namespace cq {

// ------------------------------------------------------------------ fused Q update
// maybe_update_Q (alg.py:253-283) + quantize_matrix (alg.py:245-250, quantization.py:244-269)
// without materialising the residual: res = W - L R is recomputed per 192 x 384 tile from
// the split-fp16 halves of L (m x r) and R^T (n x r) (K = r; r = 0: res = W exactly) in two
// passes over W:
//   pass 0: per-matrix max |res| (uint bits, NaN sorts above inf like torch.max) -> atomicMax;
//   pass 1: scale = max(absmax, eps); code = rint((res / scale) k) (IEEE division, then the
//           multiply, round-half-even: the reference's two roundings); packed offset-binary
//           codes (c + k, MSB-first: 4 per byte at 2 bits, 2 per byte at 4 bits) or int8/int16
//           codes; sum_j w_j (deq - res)^2 per tile in fp64 (deterministic 2-stage sum).
// Both passes evaluate res with identical code, so pass 1 sees pass 0's values bit for bit.

template <int PASS, int BITS>
__global__ __launch_bounds__(XW_THREADS, 1) void q_update_x3_kernel(QUK q) {
    extern __shared__ __attribute__((aligned(16))) char qu_smem_raw[];
    _Float16* smem = reinterpret_cast<_Float16*>(qu_smem_raw);
    const X3K& a = q.x;
    const int64_t tiles = a.tiles_n * a.tiles_m;
    const int64_t total = tiles * a.batch;
    const int64_t orig = blockIdx.x;
    const int64_t qq = total / 8, r8 = total % 8, xcd = orig % 8;
    const int64_t lin = (xcd < r8 ? xcd * (qq + 1) : r8 * (qq + 1) + (xcd - r8) * qq) + orig / 8;
    const int64_t tile = lin % tiles;
    const int64_t tn = tile % a.tiles_n, tm = tile / a.tiles_n;
    const int64_t b = lin / tiles;
    const int64_t m0 = tm * XW_BM, n0 = tn * XW_BN;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid & 1, wn = wid >> 1;
    const int lr = lane & 31, lh = lane >> 5;

    // transposed product: A operand = R^T (tile rows = columns of W), B operand = L (tile
    // columns = rows of W), so each lane owns one row of W and holds 4 runs of 4 consecutive
    // columns: W loads are 8-byte vectors and 4 two-bit codes make one byte in-lane
    f32x16v acc[3][2];
    xw_mainloop(a, b, m0, n0, a.K / XW_BK, smem, wid, lane, wm, wn, acc);
    const float sc = a.K > 0 ? a.inv_scale[b] : 0.f;
    const int64_t MN = q.m * q.n;
    const _Float16* Wh = reinterpret_cast<const _Float16*>(q.W) + b * MN;
    const float* Wf = reinterpret_cast<const float*>(q.W) + b * MN;

    constexpr float kq = (float)((1 << (BITS - 1)) - 1);
    uint32_t mx = 0;
    double err = 0.0;
    float s = 0.f;
    if (PASS == 1) s = quant_scale(q.absmax[b], q.eps);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t row = n0 + 64 * wn + 32 * j + lr;  // row of W (tile column)
        if (row >= q.m) continue;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int64_t col = m0 + 96 * wm + 32 * i + 8 * g4 + 4 * lh;  // 4 consecutive columns
                if (col >= q.n) continue;  // n % 4 == 0: a run is all in or all out
                const int64_t e = row * q.n + col;
                float w4[4];
                if (q.wf16) {
                    const uint2 raw = *reinterpret_cast<const uint2*>(Wh + e);
                    const _Float16* hv = reinterpret_cast<const _Float16*>(&raw);
#pragma unroll
                    for (int u = 0; u < 4; ++u) w4[u] = (float)hv[u];
                } else {
                    const float4 f = *reinterpret_cast<const float4*>(Wf + e);
                    w4[0] = f.x; w4[1] = f.y; w4[2] = f.z; w4[3] = f.w;
                }
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    v[u] = a.K > 0 ? w4[u] - acc[i][j][4 * g4 + u] * sc : w4[u];  // res = W - L R (alg.py:262)
                if (PASS == 0) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) mx = max(mx, abs_bits(v[u]));
                } else {
                    float c[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        c[u] = quant_code(v[u], s, kq);
                        const float d = dequant(c[u], kq, s) - v[u];
                        err += (double)(d * d) * (q.ew ? (double)q.ew[b * q.sew + col + u] : 1.0);
                    }
                    if constexpr (BITS <= 4) {
                        if (q.packed) {
                            uint32_t uq[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) uq[u] = (uint32_t)((int)c[u] + (int)kq);
                            if (BITS == 2) {
                                q.packed[(b * MN + e) / 4] = (uint8_t)((uq[0] << 6) | (uq[1] << 4) | (uq[2] << 2) | uq[3]);
                            } else {
                                *reinterpret_cast<uchar2*>(q.packed + (b * MN + e) / 2) =
                                    make_uchar2((uint8_t)((uq[0] << 4) | uq[1]), (uint8_t)((uq[2] << 4) | uq[3]));
                            }
                        }
                    }
                    if (q.codes) {
                        if (BITS <= 8)
                            *reinterpret_cast<char4*>(reinterpret_cast<int8_t*>(q.codes) + b * MN + e) =
                                make_char4((signed char)(int)c[0], (signed char)(int)c[1], (signed char)(int)c[2],
                                           (signed char)(int)c[3]);
                        else
                            *reinterpret_cast<short4*>(reinterpret_cast<int16_t*>(q.codes) + b * MN + e) =
                                make_short4((short)(int)c[0], (short)(int)c[1], (short)(int)c[2], (short)(int)c[3]);
                    }
                }
            }
    }
    if (PASS == 0) {
        mx = wave_max_u32(mx);
        if (lane == 0 && mx) atomicMax(q.absmax + b, mx);
    } else if (q.part) {
        __shared__ double red[16];
        const double tsum = block_sum_f64(err, red);
        if (threadIdx.x == 0) q.part[b * tiles + tile] = tsum;
    }
}

// Fused Q update on the 16x16x32 ring (default): A = L halves (tile rows = rows of W),
// B = R^T halves with PERMB, so each lane owns 16 consecutive columns of one W row: W loads
// of 32 B (fp16) per lane, one 32-bit store of 16 two-bit codes (64 bits at 4 bits), and a
// wave-instruction covers 16 rows x 64 columns.  Same two passes and arithmetic as
// q_update_x3_kernel (res = W - L R with identical code in both passes).  n % 16 == 0.
template <int PASS, int BITS, int DT>
__global__ __launch_bounds__(XW_THREADS, 1) void q_update_v_kernel(QUK q) {
    extern __shared__ __attribute__((aligned(16))) char qv_smem_raw[];
    _Float16* smem = reinterpret_cast<_Float16*>(qv_smem_raw);
    const X3K& a = q.x;
    const int64_t tiles = a.tiles_n * a.tiles_m;
    const int64_t total = tiles * a.batch;
    const int64_t orig = blockIdx.x;
    const int64_t qq = total / 8, r8 = total % 8, xcd = orig % 8;
    const int64_t lin = (xcd < r8 ? xcd * (qq + 1) : r8 * (qq + 1) + (xcd - r8) * qq) + orig / 8;
    const int64_t tile = lin % tiles;
    const int64_t tn = tile % a.tiles_n, tm = tile / a.tiles_n;
    const int64_t b = lin / tiles;
    const int64_t m0 = tm * XW_BM, n0 = tn * XW_BN;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid & 1, wn = wid >> 1;
    const int l16 = lane & 15, lq = lane >> 4;

    f32x4v acc[6][4];
    xr_mainloop<0, true>(a, b, m0, n0, a.K / XW_BK, smem, wid, lane, wm, wn, acc);
    const float sc = a.K > 0 ? a.inv_scale[b] : 0.f;
    const int64_t MN = q.m * q.n;
    const _Float16* Wh = reinterpret_cast<const _Float16*>(q.W) + b * MN;
    const float* Wf = reinterpret_cast<const float*>(q.W) + b * MN;
    constexpr float kq = (float)((1 << (BITS - 1)) - 1);
    uint32_t mx = 0;
    double err = 0.0;
    float s = 0.f;
    if (PASS == 1) s = quant_scale(q.absmax[b], q.eps);
    const float ys = 1.f / s, yk = 1.f / kq;  // IEEE reciprocals for div_rn
    const int64_t col = n0 + 64 * wn + 16 * lq;  // this lane's 16 consecutive columns
    const bool colok = col < q.n;                 // n % 16 == 0: a run is all in or all out
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int64_t row = m0 + 96 * wm + 16 * i + l16;
        if (row >= q.m || !colok) continue;
        const int64_t e = row * q.n + col;
        // W kept packed (fp16: 8 registers) and converted 4 columns at a time
        uint4 wr[4];
        if (DT == CQ_F16) {
            wr[0] = *reinterpret_cast<const uint4*>(Wh + e);
            wr[1] = *reinterpret_cast<const uint4*>(Wh + e + 8);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) wr[u] = *reinterpret_cast<const uint4*>(Wf + e + 4 * u);
        }
        uint32_t pk[4] = {0u, 0u, 0u, 0u};  // packed / int8 code words
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float w;
                if (DT == CQ_F16) {
                    const uint32_t pr = (&wr[j >> 1].x)[(j & 1) * 2 + (r >> 1)];
                    w = (float)__builtin_bit_cast(_Float16, (uint16_t)((r & 1) ? (pr >> 16) : (pr & 0xffffu)));
                } else {
                    w = __uint_as_float((&wr[j].x)[r]);
                }
                v[r] = a.K > 0 ? w - acc[i][j][r] * sc : w;  // res = W - L R (alg.py:262)
            }
            if (PASS == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = max(mx, abs_bits(v[r]));
                continue;
            }
            int cq[4];
            float e4[4];
            float4 wv = make_float4(1.f, 1.f, 1.f, 1.f);
            if (q.ew) wv = *reinterpret_cast<const float4*>(q.ew + b * q.sew + col + 4 * j);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float c = quant_code_r(v[r], s, ys, kq);
                const float d = dequant_r(c, kq, yk, s) - v[r];
                e4[r] = (d * d) * (&wv.x)[r];
                cq[r] = (int)c;
            }
            err += (double)((e4[0] + e4[1]) + (e4[2] + e4[3]));  // fp32 within a run of 4, fp64 across
            if (BITS == 2) {  // byte j = codes 4j..4j+3, MSB-first (offset binary c + 1)
                const uint32_t by = ((uint32_t)(cq[0] + 1) << 6) | ((uint32_t)(cq[1] + 1) << 4) |
                                    ((uint32_t)(cq[2] + 1) << 2) | (uint32_t)(cq[3] + 1);
                pk[0] |= by << (8 * j);
            } else if (BITS == 4) {  // bytes 2j, 2j+1 = codes (4j, 4j+1), (4j+2, 4j+3)
                const uint32_t b0 = ((uint32_t)(cq[0] + 7) << 4) | (uint32_t)(cq[1] + 7);
                const uint32_t b1 = ((uint32_t)(cq[2] + 7) << 4) | (uint32_t)(cq[3] + 7);
                pk[j >> 1] |= (b0 | (b1 << 8)) << (16 * (j & 1));
            } else if (BITS == 8) {
                pk[j] = (uint32_t)(uint8_t)(int8_t)cq[0] | ((uint32_t)(uint8_t)(int8_t)cq[1] << 8) |
                        ((uint32_t)(uint8_t)(int8_t)cq[2] << 16) | ((uint32_t)(uint8_t)(int8_t)cq[3] << 24);
            } else if (q.codes) {
                *reinterpret_cast<short4*>(reinterpret_cast<int16_t*>(q.codes) + b * MN + e + 4 * j) =
                    make_short4((short)cq[0], (short)cq[1], (short)cq[2], (short)cq[3]);
            }
            if (BITS <= 4 && q.codes) {  // unpacked int8 codes alongside the packed bytes
                *reinterpret_cast<uint32_t*>(reinterpret_cast<int8_t*>(q.codes) + b * MN + e + 4 * j) =
                    (uint32_t)(uint8_t)(int8_t)cq[0] | ((uint32_t)(uint8_t)(int8_t)cq[1] << 8) |
                    ((uint32_t)(uint8_t)(int8_t)cq[2] << 16) | ((uint32_t)(uint8_t)(int8_t)cq[3] << 24);
            }
        }
        if (PASS == 1) {
            if (BITS == 2 && q.packed) *reinterpret_cast<uint32_t*>(q.packed + (b * MN + e) / 4) = pk[0];
            if (BITS == 4 && q.packed) *reinterpret_cast<uint2*>(q.packed + (b * MN + e) / 2) = make_uint2(pk[0], pk[1]);
            if (BITS == 8 && q.codes)
                *reinterpret_cast<uint4*>(reinterpret_cast<int8_t*>(q.codes) + b * MN + e) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        }
        asm volatile("" ::: "memory");  // keep the row blocks' W loads from being hoisted together (VGPRs)
    }
    if (PASS == 0) {
        mx = wave_max_u32(mx);
        if (lane == 0 && mx) atomicMax(q.absmax + b, mx);
    } else if (q.part) {
        __shared__ double red[16];
        const double tsum = block_sum_f64(err, red);
        if (threadIdx.x == 0) q.part[b * tiles + tile] = tsum;
    }
}

// First Q step (r = 0, max|W| known): a plain streaming quantise of W, 16 consecutive
// elements per thread per step (32-byte fp16 loads, one 32-bit store of 16 two-bit codes),
// no LDS and no MFMA, so many workgroups per CU keep HBM busy.  Same arithmetic as pass 1 of
// the fused kernels with res = W.  n % 16 == 0; per-block fp64 error partials in part.
template <int DT, int BITS, bool FAST, bool EW>
__device__ __forceinline__ void qstream_group(const QUK& q, int64_t b, int64_t MN, int64_t e, const uint4 (&wr)[4],
                                              const float4 (&ewv)[4], float s, float ys, float yk, double& err) {
    // EW: error column weights (loaded with the group's W); without them the squared errors
    // are not multiplied by 1 (the same sums).  The 2-bit fast path dequantises as c s (k = 1:
    // (c / 1) s is exactly c s) and packs each 8 codes by FMAs on integral floats (below 2^16,
    // exact), as pass 1 of the fused Q update does: ~10 VALU instructions per element instead of
    // ~20, which made this HBM stream VALU-bound (0.60 of HBM at B = 256)
    constexpr float kq = (float)((1 << (BITS - 1)) - 1);
    uint32_t pk[4] = {0u, 0u, 0u, 0u};
    constexpr bool PK2 = BITS == 2 && FAST;
    // 2-bit: element 8 h + 4 j' + r has weight 2^(8 j' + 6 - 2 r) in the h-th 16 bits
    constexpr float wt[4] = {64.f, 16.f, 4.f, 1.f};
    float a2[2] = {0.f, 0.f};
    if (PK2) a2[0] = a2[1] = (64.f + 16.f + 4.f + 1.f) * 257.f;   // the +1 offsets of 8 codes
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int cq[4];
        float cf[4];
        float e4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v;
            if (DT == CQ_F16) {
                const uint32_t pr = (&wr[j >> 1].x)[(j & 1) * 2 + (r >> 1)];
                v = (float)__builtin_bit_cast(_Float16, (uint16_t)((r & 1) ? (pr >> 16) : (pr & 0xffffu)));
            } else {
                v = __uint_as_float((&wr[j].x)[r]);
            }
            float c, dq;
            if (FAST && BITS == 2) {
                c = rintf(div_fast(v, s, ys));
                dq = c * s;
            } else if (FAST) {
                c = rintf(div_fast(v, s, ys) * kq);
                dq = div_fast(c, kq, yk) * s;
            } else {
                c = quant_code(v, s, kq);
                dq = dequant(c, kq, s);
            }
            const float d = dq - v;
            e4[r] = EW ? (d * d) * (&ewv[j].x)[r] : d * d;
            cf[r] = c;
            if (!PK2) cq[r] = (int)c;
        }
        err += (double)((e4[0] + e4[1]) + (e4[2] + e4[3]));  // fp32 within a run of 4, fp64 across
        if (PK2) {
            const float wj = (j & 1) ? 256.f : 1.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) a2[j >> 1] = __builtin_fmaf(cf[r], wt[r] * wj, a2[j >> 1]);
        } else if (BITS == 2) {
            pk[0] |= (((uint32_t)(cq[0] + 1) << 6) | ((uint32_t)(cq[1] + 1) << 4) | ((uint32_t)(cq[2] + 1) << 2) |
                      (uint32_t)(cq[3] + 1)) << (8 * j);
        } else if (BITS == 4) {
            const uint32_t b0 = ((uint32_t)(cq[0] + 7) << 4) | (uint32_t)(cq[1] + 7);
            const uint32_t b1 = ((uint32_t)(cq[2] + 7) << 4) | (uint32_t)(cq[3] + 7);
            pk[j >> 1] |= (b0 | (b1 << 8)) << (16 * (j & 1));
        } else if (BITS == 8) {
            pk[j] = (uint32_t)(uint8_t)(int8_t)cq[0] | ((uint32_t)(uint8_t)(int8_t)cq[1] << 8) |
                    ((uint32_t)(uint8_t)(int8_t)cq[2] << 16) | ((uint32_t)(uint8_t)(int8_t)cq[3] << 24);
        } else if (q.codes) {
            *reinterpret_cast<short4*>(reinterpret_cast<int16_t*>(q.codes) + b * MN + e + 4 * j) =
                make_short4((short)cq[0], (short)cq[1], (short)cq[2], (short)cq[3]);
        }
        if (BITS <= 4 && q.codes) {
            if (PK2) {
#pragma unroll
                for (int r = 0; r < 4; ++r) cq[r] = (int)cf[r];
            }
            *reinterpret_cast<uint32_t*>(reinterpret_cast<int8_t*>(q.codes) + b * MN + e + 4 * j) =
                (uint32_t)(uint8_t)(int8_t)cq[0] | ((uint32_t)(uint8_t)(int8_t)cq[1] << 8) |
                ((uint32_t)(uint8_t)(int8_t)cq[2] << 16) | ((uint32_t)(uint8_t)(int8_t)cq[3] << 24);
        }
    }
    if (PK2) pk[0] = (uint32_t)a2[0] | ((uint32_t)a2[1] << 16);
    if (BITS == 2 && q.packed) *reinterpret_cast<uint32_t*>(q.packed + (b * MN + e) / 4) = pk[0];
    if (BITS == 4 && q.packed) *reinterpret_cast<uint2*>(q.packed + (b * MN + e) / 2) = make_uint2(pk[0], pk[1]);
    if (BITS == 8 && q.codes)
        *reinterpret_cast<uint4*>(reinterpret_cast<int8_t*>(q.codes) + b * MN + e) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
}

template <int DT>
__device__ __forceinline__ void qstream_load(const QUK& q, int64_t b, int64_t MN, int64_t e, uint4 (&wr)[4]) {
    if (DT == CQ_F16) {
        const _Float16* Wh = reinterpret_cast<const _Float16*>(q.W) + b * MN + e;
        wr[0] = *reinterpret_cast<const uint4*>(Wh);
        wr[1] = *reinterpret_cast<const uint4*>(Wh + 8);
    } else {
        const float* Wf = reinterpret_cast<const float*>(q.W) + b * MN + e;
#pragma unroll
        for (int u = 0; u < 4; ++u) wr[u] = *reinterpret_cast<const uint4*>(Wf + 4 * u);
    }
}

template <int DT>
__device__ __forceinline__ void qstream_load(const QUK& q, int64_t b, int64_t MN, int64_t e, uint4 (&wr)[4],
                                             float4 (&ewv)[4], bool load_ew = true) {
    // the group's error column weights ride with its W (a load issued at use would expose an
    // L2 round trip per group: config 3's diagonal-H first Q step ran at 0.42 of HBM);
    // load_ew false: the caller holds them (a thread whose columns do not change)
    if (!load_ew) return qstream_load<DT>(q, b, MN, e, wr);
    if (q.ew) {
        const float* ew = q.ew + b * q.sew + e % q.n;
#pragma unroll
        for (int j = 0; j < 4; ++j) ewv[j] = *reinterpret_cast<const float4*>(ew + 4 * j);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) ewv[j] = make_float4(1.f, 1.f, 1.f, 1.f);
    }
    if (DT == CQ_F16) {
        const _Float16* Wh = reinterpret_cast<const _Float16*>(q.W) + b * MN + e;
        wr[0] = *reinterpret_cast<const uint4*>(Wh);
        wr[1] = *reinterpret_cast<const uint4*>(Wh + 8);
    } else {
        const float* Wf = reinterpret_cast<const float*>(q.W) + b * MN + e;
#pragma unroll
        for (int u = 0; u < 4; ++u) wr[u] = *reinterpret_cast<const uint4*>(Wf + 4 * u);
    }
}

// First Q step (r = 0, max|W| known): a plain streaming quantise of W, 16 consecutive
// elements per thread per group, the next group's load in flight (32-byte fp16 loads, one
// 32-bit store of 16 two-bit codes), no LDS and no MFMA, so many workgroups per CU keep HBM
// busy.  Same arithmetic as pass 1 of the fused kernels with res = W.  n % 16 == 0;
// per-block fp64 error partials in part.
template <int DT, int BITS, bool EW>
__global__ __launch_bounds__(256) void quant_w_stream_kernel(QUK q) {
    constexpr float kq = (float)((1 << (BITS - 1)) - 1);
    const int64_t b = blockIdx.y;
    const int64_t MN = q.m * q.n;
    const int64_t ng = MN / 16;
    const float s = quant_scale(q.absmax[b], q.eps);
    const float ys = 1.f / s, yk = 1.f / kq;  // IEEE reciprocals for div_rn
    double err = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    // a grid stride that is a multiple of the row length (the launcher picks one when there are
    // error weights) keeps each thread on the same 16 columns: their weights are loaded once
    const bool ewfix = EW && ((stride * 16) % q.n) == 0;
    if (div_fast_ok(s)) {  // uniform: the common case, branch-free correctly rounded division
        uint4 nx[4];  // the next group's W (and weights), loaded while this one is quantised
        float4 nw[4];
        if (g < ng) qstream_load<DT>(q, b, MN, g * 16, nx, nw, EW);
        if (!EW) {
#pragma unroll
            for (int u = 0; u < 4; ++u) nw[u] = make_float4(1.f, 1.f, 1.f, 1.f);   // unused
        }
        if (ewfix || !EW) {
            // columns fixed per thread (or no weights): W two groups ahead (~100 KB of loads in
            // flight per CU at 6 waves per SIMD)
            uint4 nx2[4];
            if (g + stride < ng) qstream_load<DT>(q, b, MN, (g + stride) * 16, nx2);
            for (; g < ng; g += stride) {
                uint4 cur[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { cur[u] = nx[u]; nx[u] = nx2[u]; }
                if (g + 2 * stride < ng) qstream_load<DT>(q, b, MN, (g + 2 * stride) * 16, nx2);
                qstream_group<DT, BITS, true, EW>(q, b, MN, g * 16, cur, nw, s, ys, yk, err);
            }
        }
        for (; g < ng; g += stride) {
            uint4 cur[4];
            float4 cw[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { cur[u] = nx[u]; cw[u] = nw[u]; }
            if (g + stride < ng) qstream_load<DT>(q, b, MN, (g + stride) * 16, nx, nw);
            qstream_group<DT, BITS, true, EW>(q, b, MN, g * 16, cur, cw, s, ys, yk, err);
        }
    } else {  // non-finite / subnormal scale: IEEE divisions
        for (; g < ng; g += stride) {
            uint4 w0[4];
            float4 ew0[4];
            qstream_load<DT>(q, b, MN, g * 16, w0, ew0, EW);
            if (!EW) {
#pragma unroll
                for (int u = 0; u < 4; ++u) ew0[u] = make_float4(1.f, 1.f, 1.f, 1.f);
            }
            qstream_group<DT, BITS, false, EW>(q, b, MN, g * 16, w0, ew0, s, ys, yk, err);
        }
    }
    if (q.part) {
        __shared__ double red[16];
        const double tsum = block_sum_f64(err, red);
        if (threadIdx.x == 0) q.part[b * gridDim.x + blockIdx.x] = tsum;
    }
}

__global__ void q_update_finalize_kernel(const uint32_t* absmax, const double* part, int64_t tiles, int64_t batch,
                                         float eps, float* scale, double* err_out) {
    const int64_t b = blockIdx.x;
    if (b >= batch) return;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < tiles; t += 64) s += part[b * tiles + t];
    s = wave_sum(s);  // one wave: fixed order -> deterministic
    if (threadIdx.x == 0) {
        if (scale) scale[b] = quant_scale(absmax[b], eps);
        if (err_out) err_out[b] = s;
    }
}


// ------------------------------------------------------------------ fused residual + split
// One pass over W and the packed Q codes for the LR step (alg.py:124 res = W - Q, :211
// Y = res * sqrt(h)): writes any of res (fp32), Y (fp32), the K-blocked split halves of Y
// over its columns (A/B operand of Y Y^T) and over its rows (operand of U^T Y / Y^T Y), and
// ||Y||^2 (fp64, deterministic per-tile partials).  The split scale is a per-matrix power of
// two from the bound |Y| <= (max|W| + Q_scale) * max(ycol), so no absmax pass is needed.
// Tile 32 rows x 64 columns per step, 256 threads (8 consecutive columns each).
template <int DT, int BITS>
__global__ __launch_bounds__(256) void residual_split_kernel(
    const void* __restrict__ Ws, const uint8_t* __restrict__ qc, const float* __restrict__ qscale,
    const float* __restrict__ ycol, const float* __restrict__ wmax, float ycmax, int64_t m, int64_t n,
    float* __restrict__ res, float* __restrict__ Y, _Float16* __restrict__ hi, _Float16* __restrict__ lo,
    _Float16* __restrict__ thi, _Float16* __restrict__ tlo, float* __restrict__ scale_out,
    double* __restrict__ part, const float* __restrict__ ycol_hi, float ychmax, float* __restrict__ scale_hi_out,
    int64_t ycs, const float* __restrict__ ycmax_v, const float* __restrict__ ychmax_v) {
    __shared__ float tile[64][33];
    __shared__ double red[4];
    constexpr float k = BITS == 32 ? 1.f : (float)((1 << (BITS - 1)) - 1);
    const int64_t b = blockIdx.z;
    const int64_t MN = m * n;
    const float qs = qc ? qscale[b] : 0.f;
    // per-matrix column weights (distinct diagonal Hessians): this matrix's row of ycol / ycol_hi
    // and its own bounds
    if (ycol) ycol += b * ycs;
    if (ycol_hi) ycol_hi += b * ycs;
    if (ycmax_v) ycmax = ycmax_v[b];
    if (ychmax_v) ychmax = ychmax_v[b];
    int e2 = 0;
    {
        const float bnd = (wmax[b] + qs) * ycmax;
        if (bnd > 0.f && isfinite(bnd)) frexpf(bnd, &e2);
    }
    // fp16 W alone (no codes, no column weights): a scale >= 1 keeps W * sc exact in fp16
    // (lo = 0), so the lo halves may be skipped and their products dropped (gemm_x3 b_exact)
    const bool exact = DT == CQ_F16 && !qc && !ycol;
    const float sc = exact ? fmaxf(ldexpf(1.f, 14 - e2), 1.f) : ldexpf(1.f, 14 - e2);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && scale_out) scale_out[b] = sc;
    // ycol_hi: the column-blocked halves (hi/lo) are of res * ycol_hi instead, at their own scale
    float sch = sc;
    if (ycol_hi) {
        int e3 = 0;
        const float bnd = (wmax[b] + qs) * ychmax;
        if (bnd > 0.f && isfinite(bnd)) frexpf(bnd, &e3);
        sch = ldexpf(1.f, 14 - e3);
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) scale_hi_out[b] = sch;
    }
    const int t = threadIdx.x;
    const int r = t >> 3, c8 = (t & 7) * 8;          // row in tile, first of 8 columns
    const int64_t j0 = (int64_t)blockIdx.x * 64;
    double acc = 0.0;
    const int rows_per = (int)gridDim.y;
    for (int64_t i0 = (int64_t)blockIdx.y * 32; i0 < m; i0 += (int64_t)rows_per * 32) {
        const int64_t i = i0 + r, j = j0 + c8;
        const int64_t e = b * MN + i * n + j;
        float w[8];
        if (DT == CQ_F16) {
            const uint4 raw = *reinterpret_cast<const uint4*>(reinterpret_cast<const _Float16*>(Ws) + e);
            const _Float16* hv = reinterpret_cast<const _Float16*>(&raw);
#pragma unroll
            for (int u = 0; u < 8; ++u) w[u] = (float)hv[u];
        } else {
            const float4 f0 = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(Ws) + e);
            const float4 f1 = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(Ws) + e + 4);
            w[0] = f0.x; w[1] = f0.y; w[2] = f0.z; w[3] = f0.w; w[4] = f1.x; w[5] = f1.y; w[6] = f1.z; w[7] = f1.w;
        }
        float q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = 0.f;
        if (qc) {
            const int64_t eq = e;  // element index (codes follow the row-major element order)
            if (BITS == 2) {
                const uint16_t two = *reinterpret_cast<const uint16_t*>(qc + eq / 4);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t byte = (u < 4) ? (two & 0xffu) : (two >> 8);
                    const int sh = 6 - 2 * (u & 3);
                    q[u] = dequant((float)((int)((byte >> sh) & 3u) - 1), k, qs);
                }
            } else if (BITS == 4) {
                const uint32_t four = *reinterpret_cast<const uint32_t*>(qc + eq / 2);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t byte = (four >> (8 * (u >> 1))) & 0xffu;
                    const uint32_t v = (u & 1) ? (byte & 15u) : (byte >> 4);
                    q[u] = dequant((float)((int)v - 7), k, qs);
                }
            } else if (BITS == 8) {
                const int8_t* cp = reinterpret_cast<const int8_t*>(qc) + eq;
#pragma unroll
                for (int u = 0; u < 8; ++u) q[u] = dequant((float)cp[u], k, qs);
            } else if (BITS == 32) {  // dense fp32 Q (codebook methods); qscale = bound on |Q|
                const float4 f0 = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(qc) + eq);
                const float4 f1 = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(qc) + eq + 4);
                q[0] = f0.x; q[1] = f0.y; q[2] = f0.z; q[3] = f0.w; q[4] = f1.x; q[5] = f1.y; q[6] = f1.z; q[7] = f1.w;
            } else {
                const int16_t* cp = reinterpret_cast<const int16_t*>(qc) + eq;
#pragma unroll
                for (int u = 0; u < 8; ++u) q[u] = dequant((float)cp[u], k, qs);
            }
        }
        float rv[8], yv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            rv[u] = w[u] - q[u];
            yv[u] = ycol ? rv[u] * ycol[j + u] : rv[u];
            acc += (double)yv[u] * (double)yv[u];
        }
        if (res) {
            *reinterpret_cast<float4*>(res + e) = make_float4(rv[0], rv[1], rv[2], rv[3]);
            *reinterpret_cast<float4*>(res + e + 4) = make_float4(rv[4], rv[5], rv[6], rv[7]);
        }
        if (Y) {
            *reinterpret_cast<float4*>(Y + e) = make_float4(yv[0], yv[1], yv[2], yv[3]);
            *reinterpret_cast<float4*>(Y + e + 4) = make_float4(yv[4], yv[5], yv[6], yv[7]);
        }
        if (hi) {  // blocked over columns: (j / 32) * m * 32 + i * 32 + j % 32
            _Float16 h8[8], l8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float xs = ycol_hi ? rv[u] * ycol_hi[j + u] * sch : yv[u] * sc;
                h8[u] = (_Float16)xs;
                l8[u] = (_Float16)(xs - (float)h8[u]);
            }
            const int64_t o = b * MN + (j >> 5) * m * 32 + i * 32 + (j & 31);
            *reinterpret_cast<uint4*>(hi + o) = *reinterpret_cast<const uint4*>(h8);
            if (lo) *reinterpret_cast<uint4*>(lo + o) = *reinterpret_cast<const uint4*>(l8);
        }
        if (thi) {  // blocked over rows (Y^T as a row-major n x m operand): (i / 32) * n * 32 + j * 32 + i % 32
#pragma unroll
            for (int u = 0; u < 8; ++u) tile[c8 + u][r] = yv[u] * sc;
            __syncthreads();
            const int jc = t >> 2, r8 = (t & 3) * 8;   // column of the tile, 8 consecutive rows
            _Float16 h8[8], l8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float xs = tile[jc][r8 + u];
                h8[u] = (_Float16)xs;
                l8[u] = (_Float16)(xs - (float)h8[u]);
            }
            const int64_t o = b * MN + (i0 >> 5) * n * 32 + (j0 + jc) * 32 + r8;
            *reinterpret_cast<uint4*>(thi + o) = *reinterpret_cast<const uint4*>(h8);
            if (tlo) *reinterpret_cast<uint4*>(tlo + o) = *reinterpret_cast<const uint4*>(l8);
            __syncthreads();
        }
    }
    if (part) {
        acc = wave_sum(acc);
        if ((t & 63) == 0) red[t >> 6] = acc;
        __syncthreads();
        if (t == 0) part[(b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
    }
}

__global__ void sum_tile_parts_kernel(const double* __restrict__ part, int64_t nparts, double* __restrict__ out) {
    const int64_t b = blockIdx.x;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < nparts; t += 64) s += part[b * nparts + t];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[b] = s;
}

}  // namespace cq

using namespace cq;

extern "C" {

static int64_t qu_tiles(int64_t m, int64_t n) {
    return std::max(ceil_div(n, XW_BM) * ceil_div(m, XW_BN), ceil_div(m, XW_BM) * ceil_div(n, XW_BN));
}

// the single-recompute 2-bit path's buffers (qp_launch_cand) for one of its geometries (rows
// per wave, waves): overflow flags | list-B counts | pass-2 partials | corrections | list-A
// counts | list-B group ids | list-B residuals | list-A entries
static size_t qu_cand_geom(int64_t m, int64_t n, int64_t batch, int rpw, int nw, int64_t* regions_out,
                           int64_t* cap_out, int64_t* capa_out = nullptr) {
    const int64_t regions = ceil_div(m, (int64_t)rpw * nw) * nw, groups = (int64_t)rpw * n / 8;
    const bool big = m * n >= QP_BIG_NUMEL;
    const int64_t cap = ceil_div(groups * (big ? QP_CAPB_PERMILLE_BIG : QP_CAPB_PERMILLE_SMALL), (int64_t)1000);
    const int64_t capa = ceil_div(groups * (big ? QP_CAPA_PERMILLE_BIG : QP_CAPA_PERMILLE_SMALL), (int64_t)1000);
    if (regions_out) *regions_out = regions;
    if (cap_out) *cap_out = cap;
    if (capa_out) *capa_out = capa;
    return align_up((size_t)batch * 4, 256) + align_up((size_t)batch * regions * 4, 256) +
           align_up((size_t)batch * regions * 8, 256) * 2 + align_up((size_t)batch * regions * 4, 256) +
           align_up((size_t)batch * regions * cap * 4, 256) + align_up((size_t)batch * regions * cap * 32, 256) +
           (size_t)batch * regions * capa * 8;
}
static size_t qu_cand_bytes(int64_t m, int64_t n, int64_t batch) {
    return std::max(qu_cand_geom(m, n, batch, qp_cand_rows(128), qp_cand_waves(128), nullptr, nullptr),
                    qu_cand_geom(m, n, batch, qp_cand_rows(256), qp_cand_waves(256), nullptr, nullptr));
}

size_t cq_q_update_workspace(int64_t m, int64_t n, int64_t batch, int with_hint) {
    // tile counts of both Q-update kernels (q_update_v_kernel tiles W as m x n, the 32x32
    // kernel as n x m)
    const int64_t tiles = qu_tiles(m, n);
    // absmax bits | error partials | list path (only when a scale hint will be passed)
    return (size_t)align_up((size_t)batch * sizeof(uint32_t), 256) +
           align_up((size_t)batch * tiles * sizeof(double), 256) +
           (with_hint ? qu_cand_bytes(m, n, batch) : 0);
}

int cq_q_update_list_geometry(int64_t m, int64_t n, int64_t r, int64_t* rows_out, int64_t* cap_out,
                              int64_t* capb_out) {
    CQ_REQUIRE(rows_out && cap_out, "cq_q_update_list_geometry: null argument");
    if (!(r > 0 && r % XW_BK == 0 && qp_cand_ok(m, n, (int)r)))
        return set_error(CQ_EINVAL, "cq_q_update_list_geometry: (m, n, r) do not take the list path");
    const int rpw = qp_cand_rows((int)r);
    int64_t capb = 0;
    qu_cand_geom(m, n, 1, rpw, qp_cand_waves((int)r), nullptr, &capb, cap_out);
    if (capb_out) *capb_out = capb;
    *rows_out = rpw;
    return CQ_OK;
}

int cq_q_update_x3(int dtype, const void* W, int64_t m, int64_t n, int64_t r, int64_t batch, const uint16_t* Lh,
                   const uint16_t* Ll, const uint16_t* Rth, const uint16_t* Rtl, const float* inv_scale, int bits,
                   float eps, void* codes, uint8_t* packed, float* scale_out, const float* err_w,
                   int64_t err_w_stride, double* err_out, const float* absmax_in, const float* scale_hint,
                   int* fallback_out, void* ws, size_t ws_bytes, void* stream) {
    CQ_REQUIRE(W && m > 0 && n > 0 && batch > 0 && r >= 0, "cq_q_update_x3: bad shape");
    CQ_REQUIRE(dtype == CQ_F16 || dtype == CQ_F32, "cq_q_update_x3: dtype must be f16/f32");
    if (bits != 2 && bits != 4 && bits != 8 && bits != 16) return set_error(CQ_EINVAL, "Bit-width not supported!");
    CQ_REQUIRE(r == 0 || (Lh && Ll && Rth && Rtl && inv_scale), "cq_q_update_x3: null factor halves");
    CQ_REQUIRE(r % XW_BK == 0, "cq_q_update_x3: rank must be a multiple of 32");
    CQ_REQUIRE(n % 4 == 0, "cq_q_update_x3: n must be a multiple of 4");
    CQ_REQUIRE(!packed || bits <= 4, "cq_q_update_x3: packing needs bits <= 4");
    CQ_REQUIRE(codes || packed, "cq_q_update_x3: no code output");
    if (!ws || ws_bytes < cq_q_update_workspace(m, n, batch, scale_hint != nullptr))
        return set_error(CQ_EWORKSPACE, "cq_q_update_x3: workspace too small");
    QUK q;
    X3K& a = q.x;
    memset(&q, 0, sizeof(q));  // a_blocked = b_blocked = 0, no active mask, no list path
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vk = n % 16 == 0 && al16(W) && (!codes || al16(codes)) && (!packed || al16(packed)) &&
                    (!err_w || (al16(err_w) && err_w_stride % 4 == 0));
    if (vk) {
        // A operand L (m x r): tile rows run over W's rows; B operand R^T (n x r): tile
        // columns over W's columns (see q_update_v_kernel)
        a.M = m; a.N = n;
        a.Ah = reinterpret_cast<const _Float16*>(Lh); a.Al = reinterpret_cast<const _Float16*>(Ll);
        a.lda = r; a.sa = m * r;
        a.Bh = reinterpret_cast<const _Float16*>(Rth); a.Bl = reinterpret_cast<const _Float16*>(Rtl);
        a.ldb = r; a.sb = n * r;
        a.tiles_n = ceil_div(n, XW_BN);
        a.tiles_m = ceil_div(m, XW_BM);
    } else {
        // A operand R^T (n x r): tile rows run over W's columns; B operand L (m x r): tile
        // columns run over W's rows (see q_update_x3_kernel)
        a.M = n; a.N = m;
        a.Ah = reinterpret_cast<const _Float16*>(Rth); a.Al = reinterpret_cast<const _Float16*>(Rtl);
        a.lda = r; a.sa = n * r;
        a.Bh = reinterpret_cast<const _Float16*>(Lh); a.Bl = reinterpret_cast<const _Float16*>(Ll);
        a.ldb = r; a.sb = m * r;
        a.tiles_n = ceil_div(m, XW_BN);
        a.tiles_m = ceil_div(n, XW_BM);
    }
    a.K = r; a.batch = batch;
    a.inv_scale = inv_scale;
    const int64_t tiles = a.tiles_n * a.tiles_m;
    CQ_REQUIRE(tiles * batch < (1ll << 31), "cq_q_update_x3: grid too large");
    q.W = W; q.wf16 = dtype == CQ_F16; q.m = m; q.n = n;
    q.absmax = reinterpret_cast<uint32_t*>(ws);
    q.part = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + align_up((size_t)batch * sizeof(uint32_t), 256));
    q.eps = eps; q.codes = codes; q.packed = packed; q.scale = scale_out; q.ew = err_w; q.sew = err_w ? err_w_stride : 0;
    hipStream_t s = as_stream(stream);
    const bool known = absmax_in && r == 0;  // max|W| bits given: skip the absmax pass
    if (known) {
        if (hipMemcpyAsync(q.absmax, absmax_in, batch * sizeof(uint32_t), hipMemcpyDeviceToDevice, s) != hipSuccess)
            return set_error(CQ_EHIP, "cq_q_update_x3: copy failed");
    } else if (hipMemsetAsync(q.absmax, 0, batch * sizeof(uint32_t), s) != hipSuccess) {
        return set_error(CQ_EHIP, "cq_q_update_x3: memset failed");
    }
    const unsigned grid = (unsigned)(tiles * batch);
    // row-panel kernel (q_update_p_kernel): K <= 256, m % 16 == 0, n % 32 == 0, 16-B aligned
    const bool pk = r > 0 && r <= QP_KMAX && m % 16 == 0 && n % QP_BN == 0 && vk && al16(Lh) && al16(Ll) &&
                    al16(Rth) && al16(Rtl);
    // single recompute (2-bit packed codes, fp16 W, previous scale given):
    // pass 2 + candidate lists + code kernel, pass 1 only where a list cannot be complete
    if (pk && !known && scale_hint && bits == 2 && packed && !codes && dtype == CQ_F16 &&
        qp_cand_ok(m, n, (int)r)) {
        int64_t regions = 0, cap = 0, capa = 0;
        qu_cand_geom(m, n, batch, qp_cand_rows((int)r), qp_cand_waves((int)r), &regions, &cap, &capa);
        char* c = reinterpret_cast<char*>(q.part) + align_up((size_t)batch * tiles * sizeof(double), 256);
        q.ovf = reinterpret_cast<uint32_t*>(c); c += align_up((size_t)batch * 4, 256);
        q.cnt = reinterpret_cast<uint32_t*>(c); c += align_up((size_t)batch * regions * 4, 256);
        q.part0 = reinterpret_cast<double*>(c); c += align_up((size_t)batch * regions * 8, 256);
        q.partF = reinterpret_cast<double*>(c); c += align_up((size_t)batch * regions * 8, 256);
        q.cntA = reinterpret_cast<uint32_t*>(c); c += align_up((size_t)batch * regions * 4, 256);
        q.gid = reinterpret_cast<uint32_t*>(c); c += align_up((size_t)batch * regions * cap * 4, 256);
        q.gval = reinterpret_cast<float4*>(c); c += align_up((size_t)batch * regions * cap * 32, 256);
        q.la = reinterpret_cast<uint2*>(c);
        q.cap = cap;
        q.capA = capa;
        q.hint = scale_hint;
        q.fb_out = fallback_out;
        q.x.batch = batch;
        if (hipMemsetAsync(q.ovf, 0, batch * sizeof(uint32_t), s) != hipSuccess)
            return set_error(CQ_EHIP, "cq_q_update_x3: memset failed");
        if (qp_launch_cand(q, Lh, Ll, Rth, Rtl, (int)r, batch, eps, scale_out, err_out, s) < 0)
            return set_error(CQ_EINVAL, "cq_q_update_x3: grid too large");
        return check_launch("cq_q_update_x3");
    }
    if (fallback_out && hipMemsetAsync(fallback_out, 0, batch * sizeof(int), s) != hipSuccess)
        return set_error(CQ_EHIP, "cq_q_update_x3: memset failed");
    if (pk && !known) {
        q.x.batch = batch;
        const int64_t p1 = qp_launch(q, dtype, bits, Lh, Ll, Rth, Rtl, (int)r, batch, s);
        if (p1 < 0) return set_error(CQ_EINVAL, "cq_q_update_x3: grid too large");
        q_update_finalize_kernel<<<(unsigned)batch, 64, 0, s>>>(q.absmax, q.part, p1, batch, eps, scale_out, err_out);
        return check_launch("cq_q_update_x3");
    }
    if (known && vk) {  // r = 0 with max|W| known: one streaming pass over W
        int64_t gx = std::max<int64_t>(1, std::min<int64_t>(tiles, ceil_div(m * n / 16, 256)));
        if (err_w) {  // a stride of whole rows: each thread keeps its 16 columns (and their weights);
                      // rounded down, as the workspace holds `tiles` error partials per matrix
            const int64_t g16 = n / 16, unit = g16 / std::gcd<int64_t>(g16, 256);
            if (gx >= unit) gx = gx / unit * unit;
        }
        CQ_REQUIRE(batch < 65536, "cq_q_update_x3: batch too large");
        const dim3 sg((unsigned)gx, (unsigned)batch);
#define CQ_QS(DT, B) do { if (q.ew) quant_w_stream_kernel<DT, B, true><<<sg, 256, 0, s>>>(q); \
                             else quant_w_stream_kernel<DT, B, false><<<sg, 256, 0, s>>>(q); } while (0)
        if (dtype == CQ_F16) {
            switch (bits) { case 2: CQ_QS(CQ_F16, 2); break; case 4: CQ_QS(CQ_F16, 4); break;
                            case 8: CQ_QS(CQ_F16, 8); break; default: CQ_QS(CQ_F16, 16); }
        } else {
            switch (bits) { case 2: CQ_QS(CQ_F32, 2); break; case 4: CQ_QS(CQ_F32, 4); break;
                            case 8: CQ_QS(CQ_F32, 8); break; default: CQ_QS(CQ_F32, 16); }
        }
#undef CQ_QS
        q_update_finalize_kernel<<<(unsigned)batch, 64, 0, s>>>(q.absmax, q.part, gx, batch, eps, scale_out, err_out);
        return check_launch("cq_q_update_x3");
    }
#define CQ_QU(B) do { if (vk && dtype == CQ_F16) { \
                          if (!known) q_update_v_kernel<0, B, CQ_F16><<<grid, XW_THREADS, XW_LDS_BYTES, s>>>(q); \
                          q_update_v_kernel<1, B, CQ_F16><<<grid, XW_THREADS, XW_LDS_BYTES, s>>>(q); } \
                      else if (vk) { if (!known) q_update_v_kernel<0, B, CQ_F32><<<grid, XW_THREADS, XW_LDS_BYTES, s>>>(q); \
                                     q_update_v_kernel<1, B, CQ_F32><<<grid, XW_THREADS, XW_LDS_BYTES, s>>>(q); } \
                      else { if (!known) q_update_x3_kernel<0, B><<<grid, XW_THREADS, XW_LDS_BYTES, s>>>(q); \
                             q_update_x3_kernel<1, B><<<grid, XW_THREADS, XW_LDS_BYTES, s>>>(q); } } while (0)
    switch (bits) {
        case 2: CQ_QU(2); break;
        case 4: CQ_QU(4); break;
        case 8: CQ_QU(8); break;
        default: CQ_QU(16); break;
    }
#undef CQ_QU
    q_update_finalize_kernel<<<(unsigned)batch, 64, 0, s>>>(q.absmax, q.part, tiles, batch, eps, scale_out, err_out);
    return check_launch("cq_q_update_x3");
}

size_t cq_residual_split_workspace(int64_t m, int64_t n, int64_t batch) {
    const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(m / 32, 16));
    return (size_t)batch * gy * ceil_div(n, 64) * sizeof(double);
}

int cq_residual_split(int dtype, const void* Ws, const uint8_t* packed, const float* qscale, int bits,
                      const float* ycol, float ycol_max, const float* wmax, int64_t batch, int64_t m, int64_t n,
                      float* res_out, float* Y_out, uint16_t* hi, uint16_t* lo, uint16_t* thi, uint16_t* tlo,
                      float* scale_out, double* sq_out, const float* ycol_hi, float ycol_hi_max, float* scale_hi_out,
                      int64_t ycol_stride, const float* ycol_max_v, const float* ycol_hi_max_v,
                      void* ws, size_t ws_bytes, void* stream) {
    CQ_REQUIRE(Ws && wmax && batch > 0 && batch < 65536 && m > 0 && n > 0, "cq_residual_split: bad args");
    CQ_REQUIRE(m % 32 == 0 && n % 64 == 0, "cq_residual_split: m % 32 and n % 64 must be 0");
    CQ_REQUIRE(!packed || qscale, "cq_residual_split: scale required with codes");
    CQ_REQUIRE(!packed || bits == 2 || bits == 4 || bits == 8 || bits == 16 || bits == 32, "Bit-width not supported!");
    const bool exact = dtype == CQ_F16 && !packed && !ycol;  // lo = 0: the lo halves are optional
    CQ_REQUIRE((!lo || hi) && (!tlo || thi) && (exact || (!hi == !lo && !thi == !tlo)),
               "cq_residual_split: halves go in pairs (lo optional only for fp16 W without codes or ycol)");
    CQ_REQUIRE((!hi && !thi) || scale_out, "cq_residual_split: halves need scale_out");
    CQ_REQUIRE(!ycol_hi || (hi && lo && scale_hi_out), "cq_residual_split: ycol_hi needs hi, lo and scale_hi_out");
    CQ_REQUIRE(!sq_out || (ws && ws_bytes >= cq_residual_split_workspace(m, n, batch)), "cq_residual_split: workspace too small");
    const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(m / 32, 16));
    dim3 grid((unsigned)(n / 64), (unsigned)gy, (unsigned)batch);
    hipStream_t s = as_stream(stream);
    double* part = sq_out ? reinterpret_cast<double*>(ws) : nullptr;
    auto h = [](uint16_t* p) { return reinterpret_cast<_Float16*>(p); };
#define CQ_RS(DT, B) residual_split_kernel<DT, B><<<grid, 256, 0, s>>>(Ws, packed, qscale, ycol, wmax, ycol_max, m, n, \
        res_out, Y_out, h(hi), h(lo), h(thi), h(tlo), scale_out, part, ycol_hi, ycol_hi_max, scale_hi_out, \
        ycol_stride, ycol_max_v, ycol_hi_max_v)
    const int bsel = packed ? bits : 2;
    if (dtype == CQ_F16) {
        switch (bsel) { case 2: CQ_RS(CQ_F16, 2); break; case 4: CQ_RS(CQ_F16, 4); break;
                        case 8: CQ_RS(CQ_F16, 8); break; case 32: CQ_RS(CQ_F16, 32); break; default: CQ_RS(CQ_F16, 16); }
    } else {
        switch (bsel) { case 2: CQ_RS(CQ_F32, 2); break; case 4: CQ_RS(CQ_F32, 4); break;
                        case 8: CQ_RS(CQ_F32, 8); break; case 32: CQ_RS(CQ_F32, 32); break; default: CQ_RS(CQ_F32, 16); }
    }
#undef CQ_RS
    if (sq_out) sum_tile_parts_kernel<<<(unsigned)batch, 64, 0, s>>>(part, gy * (n / 64), sq_out);
    return check_launch("cq_residual_split");
}

}  // extern "C"
