// cq_hadamard_rows: the normalised Sylvester-Hadamard transform of every row of an activation
// matrix (fast Walsh-Hadamard transform, FWHT), the transform a layer decomposed in the
// Hadamard basis (model.apply_caldera_quantization(packed_hadamard=True)) needs around its
// packed forward:
//
//   y[t, i] = c * sum_{j < n_in} (-1)^popcount(i & j) x[t, j] (+ bias[i]),  c = 1 / sqrt(P)
//
// Structure.  A row of P = 2^p values is P / 4 chunks of four consecutive elements; chunk
// index bits are, from the bottom, [lane bits][wave bits][register bits]:
//
//   chunk = lane | wave << 6 | q << 8 | g << 10   (one row per workgroup, P >= 4096)
//   chunk = lane | q << lg_tl                     (a team of 2^lg_tl <= 64 lanes per row, P <= 2048)
//
// so every global access is one aligned 16-byte (fp32) or 8-byte (fp16 / bf16) chunk per lane,
// consecutive lanes on consecutive chunks, and each element is read once and written once.
// The p butterfly stages (a, b) -> (a + b, a - b), all fp32, run where their index bit lives:
//   - the two bits inside a chunk and the register bits q: in registers, no data movement;
//   - the lane bits: __shfl_xor with the partner lane, the upper lane keeps partner - own;
//   - the two wave bits: one LDS exchange that swaps them with the two register bits (the
//     wave bits become register bits, finished in registers).  The exchange moves whole
//     chunks: lane l writes and reads 16 bytes at (slot * 64 + l) * 16, consecutive lanes on
//     consecutive 16-byte slots, which neither ds_write_b128 nor ds_read_b128 conflicts on,
//     so the transpose needs no padding or swizzle;
//   - rows above 4096: the row is taken as sub-rows of 4096, each finished as above by its own
//     4 waves into the row's LDS buffer, and the bits above are finished from there
//     (hadamard_block_kernel).
// Rows of up to 2048 values stay inside one wave (no LDS, no barrier); shorter ones are packed
// 256 / (P / 4) to a workgroup, so P = 64 runs 16 rows per 256 threads.  A row's stage order is
// a function of P alone: its bits do not depend on the other rows, the row count, its index or
// the strides (the scalar path of an unaligned or cut chunk loads the same values).
// No atomics, no inline assembly, no workspace.
//
// cq_hadamard_group_rows runs up to eight such transforms of the same rows and P in one launch of the
// same kernels (the member is blockIdx.y), and cq_hadamard_glu_rows two of them -- the rows of gate and
// of up -- with h = a(v_g) * v_u as the epilogue of kernels of its own built from the same stages.
//
// The cq_hadamard_signed_* entries run the randomised transform diag(s_out) H diag(s_in): the same kernel
// bodies instantiated on parameter types that carry the two int8 sign vectors (HadSP and the structs built
// from it).  Only the chunk load and the scale step differ, by overload on the parameter type, so the
// unsigned instantiations are the text they were and the stage order is still a function of P alone.
#include <cmath>
#include <type_traits>

#include "cq_common.h"

namespace cq {
namespace {

struct HadP {
    const char* x;
    char* y;
    const float* bias;
    int64_t ldx, ldy, rows;  // strides in elements
    int n_in, n_out;
    int lg_tl;               // log2 of the lanes per row (one-wave kernels)
    int x_dt, y_dt;
    int x_vec, y_vec, b_vec; // whole chunks may take one aligned vector access
    float c;
};

// cq_hadamard_signed_rows: an element of x is negated iff its byte of sign_in is negative, a finished sum
// iff its byte of sign_out is (either may be null: no flips).  si_vec / so_vec: the vector is 4-byte
// aligned, so the four bytes of a whole chunk may be one load.
struct HadSP : HadP {
    const int8_t* sign_in;
    const int8_t* sign_out;
    int si_vec, so_vec;
};

// cq_hadamard_group_rows' kernel argument: the members with something to write, by value.  They share
// rows and P (the template instantiation and the grid's x extent); blockIdx.y is the member.
struct HadGroupP {
    HadP m[CQ_HADAMARD_GROUP_MAX];
};
struct HadSGroupP {
    HadSP m[CQ_HADAMARD_GROUP_MAX];
};
__device__ __forceinline__ const HadP& member(const HadP& p) { return p; }
__device__ __forceinline__ const HadP& member(const HadGroupP& g) {
    return *reinterpret_cast<const HadP*>(reinterpret_cast<const char*>(g.m) + blockIdx.y * sizeof(HadP));
}
__device__ __forceinline__ const HadSP& member(const HadSP& p) { return p; }
__device__ __forceinline__ const HadSP& member(const HadSGroupP& g) {
    return *reinterpret_cast<const HadSP*>(reinterpret_cast<const char*>(g.m) + blockIdx.y * sizeof(HadSP));
}

// cq_hadamard_glu_rows' kernel argument: g and u are the two transforms as cq_hadamard_rows would run
// them (x = the row of gate resp. up, bias, n_in, c); g's y fields and n_out describe h, u's y is unused.
struct HadGluP {
    HadP g, u;
    int act;
};
// cq_hadamard_signed_glu_rows': g.sign_out and u.sign_out are sign_g and sign_u, the sign_in are null
struct HadSGluP {
    HadSP g, u;
    int act;
};

__device__ __forceinline__ float bf16_to_f32(uint32_t h) { return __uint_as_float(h << 16); }

// round to nearest even; NaN stays a quiet NaN
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ float load1(const char* row, int dt, int i) {
    if (dt == CQ_F32) return reinterpret_cast<const float*>(row)[i];
    if (dt == CQ_F16) return (float)reinterpret_cast<const _Float16*>(row)[i];
    return bf16_to_f32(reinterpret_cast<const uint16_t*>(row)[i]);
}

// elements [i0, i0 + 4) of a row widened to fp32; columns >= n_in are zero and are not read
__device__ __forceinline__ void load4(const HadP& p, const char* row, int i0, float* v) {
    if (p.x_vec && i0 + 4 <= p.n_in) {
        if (p.x_dt == CQ_F32) {
            const float4 f = *reinterpret_cast<const float4*>(row + (size_t)i0 * 4);
            v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        } else {
            const uint2 u = *reinterpret_cast<const uint2*>(row + (size_t)i0 * 2);
            if (p.x_dt == CQ_F16) {
                const _Float16* h = reinterpret_cast<const _Float16*>(&u);
                v[0] = (float)h[0], v[1] = (float)h[1], v[2] = (float)h[2], v[3] = (float)h[3];
            } else {
                v[0] = bf16_to_f32(u.x & 0xffffu), v[1] = bf16_to_f32(u.x >> 16);
                v[2] = bf16_to_f32(u.y & 0xffffu), v[3] = bf16_to_f32(u.y >> 16);
            }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (i0 + k < p.n_in) ? load1(row, p.x_dt, i0 + k) : 0.0f;
}

// The four sign bytes of the columns [i0, i0 + 4) as one word, byte k in bits 8k .. 8k + 7; zero (no flip) for
// a null vector and for columns >= n, whose bytes are not read.  A whole chunk of an aligned vector is one
// 4-byte load, anything else the scalar path (the same word).
__device__ __forceinline__ uint32_t sign_word(const int8_t* sign, int vec, int n, int i0) {
    if (sign == nullptr) return 0u;
    if (vec && i0 + 4 <= n) return *reinterpret_cast<const uint32_t*>(sign + i0);
    uint32_t s = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i0 + k < n) s |= (uint32_t)(uint8_t)sign[i0 + k] << (8 * k);
    return s;
}

// v[k] negated where byte k of the sign word is negative: the byte's top bit goes into the float's sign bit,
// which is exact for every value
__device__ __forceinline__ void flip4(uint32_t s, float* v) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = __uint_as_float(__float_as_uint(v[k]) ^ ((s << (24 - 8 * k)) & 0x80000000u));
}

// the signed transform's load: sign_in is applied to x as it is widened.  The sign word is asked for first,
// so that its load is in flight beside x's and not behind it
__device__ __forceinline__ void load4(const HadSP& p, const char* row, int i0, float* v) {
    const uint32_t s = sign_word(p.sign_in, p.si_vec, p.n_in, i0);
    load4(static_cast<const HadP&>(p), row, i0, v);
    flip4(s, v);
}

// o = c * v (+ bias) for the columns [i0, i0 + 4), i0 < n_out: the fp32 values before the output rounding
__device__ __forceinline__ void scaled4(const HadP& p, int i0, const float* v, float* o) {
    const bool full = i0 + 4 <= p.n_out;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = v[k] * p.c;
    if (p.bias != nullptr) {
        if (full && p.b_vec) {
            const float4 b = *reinterpret_cast<const float4*>(p.bias + i0);
            o[0] += b.x, o[1] += b.y, o[2] += b.z, o[3] += b.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + k < p.n_out) o[k] += p.bias[i0 + k];
        }
    }
}

// o rounded once to y's type into the columns [i0, i0 + 4), i0 < n_out; columns >= n_out are not written
__device__ __forceinline__ void write4(const HadP& p, char* row, int i0, const float* o) {
    const bool full = i0 + 4 <= p.n_out;
    if (p.y_dt == CQ_F32) {
        float* y = reinterpret_cast<float*>(row) + i0;
        if (full && p.y_vec) {
            *reinterpret_cast<float4*>(y) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + k < p.n_out) y[k] = o[k];
        }
        return;
    }
    uint16_t h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (p.y_dt == CQ_F16) {
            const _Float16 f = (_Float16)o[k];
            h[k] = *reinterpret_cast<const uint16_t*>(&f);
        } else {
            h[k] = f32_to_bf16(o[k]);
        }
    }
    uint16_t* y = reinterpret_cast<uint16_t*>(row) + i0;
    if (full && p.y_vec) {
        *reinterpret_cast<uint2*>(y) = make_uint2(h[0] | (uint32_t)h[1] << 16, h[2] | (uint32_t)h[3] << 16);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < p.n_out) y[k] = h[k];
    }
}

// c * v (+ bias) rounded once to y's type; columns >= n_out are not written.  scaled4 then write4 in one
// text: calling the two changed the existing kernels' registers (179 -> 193 VGPRs at P = 2048), DESIGN 9.9
__device__ __forceinline__ void store4(const HadP& p, char* row, int i0, const float* v) {
    if (i0 >= p.n_out) return;
    const bool full = i0 + 4 <= p.n_out;
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = v[k] * p.c;
    if (p.bias != nullptr) {
        if (full && p.b_vec) {
            const float4 b = *reinterpret_cast<const float4*>(p.bias + i0);
            o[0] += b.x, o[1] += b.y, o[2] += b.z, o[3] += b.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + k < p.n_out) o[k] += p.bias[i0 + k];
        }
    }
    if (p.y_dt == CQ_F32) {
        float* y = reinterpret_cast<float*>(row) + i0;
        if (full && p.y_vec) {
            *reinterpret_cast<float4*>(y) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + k < p.n_out) y[k] = o[k];
        }
        return;
    }
    uint16_t h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (p.y_dt == CQ_F16) {
            const _Float16 f = (_Float16)o[k];
            h[k] = *reinterpret_cast<const uint16_t*>(&f);
        } else {
            h[k] = f32_to_bf16(o[k]);
        }
    }
    uint16_t* y = reinterpret_cast<uint16_t*>(row) + i0;
    if (full && p.y_vec) {
        *reinterpret_cast<uint2*>(y) = make_uint2(h[0] | (uint32_t)h[1] << 16, h[2] | (uint32_t)h[3] << 16);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < p.n_out) y[k] = h[k];
    }
}

// The signed transform's scale step: o = s_out * (c * v) (+ bias).  The flip is applied to v: c * (-v) and
// -(c * v) are the same bits (IEEE multiplication is sign-symmetric), and the unsigned text then serves.
__device__ __forceinline__ void scaled4(const HadSP& p, int i0, const float* v, float* o) {
    float w[4] = {v[0], v[1], v[2], v[3]};
    flip4(sign_word(p.sign_out, p.so_vec, p.n_out, i0), w);
    scaled4(static_cast<const HadP&>(p), i0, w, o);
}

__device__ __forceinline__ void store4(const HadSP& p, char* row, int i0, const float* v) {
    if (i0 >= p.n_out) return;
    float w[4] = {v[0], v[1], v[2], v[3]};
    flip4(sign_word(p.sign_out, p.so_vec, p.n_out, i0), w);
    store4(static_cast<const HadP&>(p), row, i0, w);
}

// h = a(v_g) * v_u of the columns [i0, i0 + 4): v_g and v_u are store4's fp32 values of the two
// transforms (scaled4 on each), a is the identity or e = expf(-v), d = 1 + e, v / d (the file is built
// without contraction and with the correctly rounded division); one multiply, one rounding to h's type
template <typename GLU>
__device__ __forceinline__ void glu_store4(const GLU& a, char* hrow, int i0, const float* vg, const float* vu) {
    if (i0 >= a.g.n_out) return;
    float og[4], ou[4], h[4];
    scaled4(a.g, i0, vg, og);
    scaled4(a.u, i0, vu, ou);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float act = og[k];
        if (a.act == CQ_ACT_SILU) {
            const float e = expf(-og[k]);
            const float d = 1.0f + e;
            act = og[k] / d;
        }
        h[k] = act * ou[k];
    }
    write4(a.g, hrow, i0, h);
}

// butterflies over bit `bit` of the register (chunk) index, on all four elements of a chunk
template <int CH>
__device__ __forceinline__ void reg_stage(float (&v)[CH * 4], int bit) {
#pragma unroll
    for (int q = 0; q < CH; ++q) {
        if (q & (1 << bit)) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = v[q * 4 + k], b = v[(q | (1 << bit)) * 4 + k];
            v[q * 4 + k] = a + b;
            v[(q | (1 << bit)) * 4 + k] = a - b;
        }
    }
}

// butterflies over the two index bits inside every chunk
template <int CH>
__device__ __forceinline__ void chunk_stage(float (&v)[CH * 4]) {
#pragma unroll
    for (int q = 0; q < CH; ++q) {
        const float a = v[q * 4] + v[q * 4 + 1], b = v[q * 4] - v[q * 4 + 1];
        const float c = v[q * 4 + 2] + v[q * 4 + 3], d = v[q * 4 + 2] - v[q * 4 + 3];
        v[q * 4] = a + c, v[q * 4 + 1] = b + d, v[q * 4 + 2] = a - c, v[q * 4 + 3] = b - d;
    }
}

// butterflies over the low `lg` lane bits: the partner's value by __shfl_xor, the upper lane of
// a pair keeps partner - own
template <int CH>
__device__ __forceinline__ void lane_stages(float (&v)[CH * 4], int lane, int lg) {
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        if (b < lg) {
            const bool upper = (lane >> b) & 1;
#pragma unroll
            for (int e = 0; e < CH * 4; ++e) {
                const float o = __shfl_xor(v[e], 1 << b, 64);
                v[e] = upper ? o - v[e] : v[e] + o;
            }
        }
    }
}

constexpr int ilog2(int x) { return x <= 1 ? 0 : 1 + ilog2(x / 2); }

// Rows of up to 2048 values: CH chunks of four elements per lane, a team of 2^lg_tl lanes per
// row, 256 >> lg_tl rows per workgroup (CH > 1 only with a whole wave per row).  No LDS.
//
// ARG (both kernels): HadP, the kernel argument is the transform's parameters themselves
// (cq_hadamard_rows); HadGroupP (cq_hadamard_group_rows), the grid's y extent is the member count and a
// workgroup runs on member blockIdx.y's parameters, at its own place blockIdx.x in that member's grid:
// the same body, hence the same work in the same order as alone.
template <int CH, typename ARG>
__global__ __launch_bounds__(256) void hadamard_wave_kernel(const ARG arg) {
    const auto& p = member(arg);  // HadP, or HadSP in the signed entries' instantiations
    constexpr int kQBits = ilog2(CH);
    const int tid = threadIdx.x, lane = tid & 63;
    const int lg = CH == 1 ? p.lg_tl : 6;   // lane bits of a row's chunk index
    const int cbase = tid & ((1 << lg) - 1);
    const int64_t rows_per_wg = 256 >> lg;
    const size_t xes = p.x_dt == CQ_F32 ? 4 : 2, yes = p.y_dt == CQ_F32 ? 4 : 2;

    for (int64_t row = (int64_t)blockIdx.x * rows_per_wg + (tid >> lg); row < p.rows;
         row += (int64_t)gridDim.x * rows_per_wg) {
        const char* xrow = p.x + (size_t)row * (size_t)p.ldx * xes;
        char* yrow = p.y + (size_t)row * (size_t)p.ldy * yes;
        float v[CH * 4];
#pragma unroll
        for (int q = 0; q < CH; ++q) load4(p, xrow, (cbase | (q << lg)) * 4, &v[q * 4]);
        chunk_stage<CH>(v);
        lane_stages<CH>(v, lane, lg);
#pragma unroll
        for (int b = 0; b < kQBits; ++b) reg_stage<CH>(v, b);
#pragma unroll
        for (int q = 0; q < CH; ++q) store4(p, yrow, (cbase | (q << lg)) * 4, &v[q * 4]);
    }
}

// Rows of P = 4096 G values, G in {1, 2, 4, 8}: one row per workgroup, as G sub-rows of 4096
// (1024 chunks; chunk = lane | wave << 6 | q << 8, q < 4), each taken by a team of 4 waves; the
// workgroup holds G teams (two at G = 8, which then takes four passes), so the sub-rows run side by side.
//   A. A sub-row's 12 stages: chunk, lane and register bits as above, then the two wave bits
//      through an exchange inside the sub-row's own 16 KB of the row buffer: chunk q goes to
//      slot lane + 64 (wave + 4 q), one barrier, and wave w reads the slots lane + 64 (u + 4 w),
//      u < 4 -- the wave bits have become register bits.  A lane alone reads the slots it then
//      writes the finished chunks back to (slot = chunk index), so no second barrier is needed.
//   B. The log2 G bits above: each lane of the workgroup reads chunk c of every sub-row,
//      finishes in registers and writes y.
// Every LDS access is 16 bytes per lane with consecutive lanes on consecutive slots.  The row
// buffer is static LDS, 16 KB G (128 KB of the CU's 160 KB for P = 32768).
// (P = 32768 at four teams would cap a lane at 128 registers, which the last stage's 32 values and their
// stores do not fit without scratch: two teams.  The signed single transform at P = 16384 is in the same
// place with its sign words, 44 bytes of scratch at four teams: two teams there as well)
template <typename ARG>
constexpr int block_teams(int G) { return G == 8 || (G == 4 && std::is_same_v<ARG, HadSP>) ? 2 : G; }

template <int G, typename ARG>
__global__ __launch_bounds__(256 * block_teams<ARG>(G)) void hadamard_block_kernel(const ARG arg) {
    const auto& p = member(arg);  // HadP, or HadSP in the signed entries' instantiations
    constexpr int kTeams = block_teams<ARG>(G), kThreads = 256 * kTeams;
    __shared__ float4 rowbuf[G * 1024];
    const int tid = threadIdx.x & 255, lane = tid & 63, w = tid >> 6, team = threadIdx.x >> 8;
    const size_t xes = p.x_dt == CQ_F32 ? 4 : 2, yes = p.y_dt == CQ_F32 ? 4 : 2;

    for (int64_t row = blockIdx.x; row < p.rows; row += gridDim.x) {
        const char* xrow = p.x + (size_t)row * (size_t)p.ldx * xes;
        char* yrow = p.y + (size_t)row * (size_t)p.ldy * yes;
#pragma unroll 1
        for (int g = team; g < G; g += kTeams) {  // G / kTeams passes for every team: the barrier is uniform
            float4* buf = rowbuf + g * 1024;
            float v[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) load4(p, xrow, (g * 1024 + (tid | (q << 8))) * 4, &v[q * 4]);
            chunk_stage<4>(v);
            lane_stages<4>(v, lane, 6);
            reg_stage<4>(v, 0);
            reg_stage<4>(v, 1);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                buf[lane + 64 * (w + 4 * q)] = make_float4(v[q * 4], v[q * 4 + 1], v[q * 4 + 2], v[q * 4 + 3]);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 f = buf[lane + 64 * (u + 4 * w)];
                v[u * 4] = f.x, v[u * 4 + 1] = f.y, v[u * 4 + 2] = f.z, v[u * 4 + 3] = f.w;
            }
            reg_stage<4>(v, 0);
            reg_stage<4>(v, 1);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = lane + 64 * (u + 4 * w);
                if constexpr (G == 1) store4(p, yrow, c * 4, &v[u * 4]);
                else buf[c] = make_float4(v[u * 4], v[u * 4 + 1], v[u * 4 + 2], v[u * 4 + 3]);
            }
        }
        if constexpr (G > 1) {
            __syncthreads();
#pragma unroll 1
            for (int c = threadIdx.x; c < 1024; c += kThreads) {
                float v[G * 4];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float4 f = rowbuf[g * 1024 + c];
                    v[g * 4] = f.x, v[g * 4 + 1] = f.y, v[g * 4 + 2] = f.z, v[g * 4 + 3] = f.w;
                }
#pragma unroll
                for (int b = 0; b < ilog2(G); ++b) reg_stage<G>(v, b);
#pragma unroll
                for (int g = 0; g < G; ++g) store4(p, yrow, (g * 1024 + c) * 4, &v[g * 4]);
            }
        }
        __syncthreads();  // the next row's exchange writes the buffer again
    }
}

// cq_hadamard_glu_rows, rows of up to 2048 values: hadamard_wave_kernel's stages run twice, on the row
// of gate and on the row of up, into two register sets; the epilogue takes both.
// GLU: HadGluP, or HadSGluP (cq_hadamard_signed_glu_rows)
template <int CH, typename GLU>
__global__ __launch_bounds__(256) void hadamard_wave_glu_kernel(const GLU a) {
    constexpr int kQBits = ilog2(CH);
    const int tid = threadIdx.x, lane = tid & 63;
    const int lg = CH == 1 ? a.g.lg_tl : 6;
    const int cbase = tid & ((1 << lg) - 1);
    const int64_t rows_per_wg = 256 >> lg;
    const size_t ges = a.g.x_dt == CQ_F32 ? 4 : 2, ues = a.u.x_dt == CQ_F32 ? 4 : 2, hes = a.g.y_dt == CQ_F32 ? 4 : 2;

    for (int64_t row = (int64_t)blockIdx.x * rows_per_wg + (tid >> lg); row < a.g.rows;
         row += (int64_t)gridDim.x * rows_per_wg) {
        const char* grow = a.g.x + (size_t)row * (size_t)a.g.ldx * ges;
        const char* urow = a.u.x + (size_t)row * (size_t)a.u.ldx * ues;
        char* hrow = a.g.y + (size_t)row * (size_t)a.g.ldy * hes;
        float vg[CH * 4], vu[CH * 4];
#pragma unroll
        for (int q = 0; q < CH; ++q) load4(a.g, grow, (cbase | (q << lg)) * 4, &vg[q * 4]);
        chunk_stage<CH>(vg);
        lane_stages<CH>(vg, lane, lg);
#pragma unroll
        for (int b = 0; b < kQBits; ++b) reg_stage<CH>(vg, b);
#pragma unroll
        for (int q = 0; q < CH; ++q) load4(a.u, urow, (cbase | (q << lg)) * 4, &vu[q * 4]);
        chunk_stage<CH>(vu);
        lane_stages<CH>(vu, lane, lg);
#pragma unroll
        for (int b = 0; b < kQBits; ++b) reg_stage<CH>(vu, b);
#pragma unroll
        for (int q = 0; q < CH; ++q) glu_store4(a, hrow, (cbase | (q << lg)) * 4, &vg[q * 4], &vu[q * 4]);
    }
}

// cq_hadamard_glu_rows, rows of P = 4096 G values, G in {1, 2, 4}: hadamard_block_kernel's stage A on
// the row of gate and then on the row of up, each into its own row buffer (2 x 16 KB G of static LDS,
// 128 KB at P = 16384; P = 32768 would need 256 KB and is refused on the host), then stage B on both:
// a lane reads chunk c of every sub-row of both buffers, finishes the log2 G bits of each in registers
// and writes h.  G = 1 goes through the buffers too (stage B is then the epilogue alone).
// (P = 16384 at four teams caps a lane at 128 registers, which stage B's 2 x 16 values, the two epilogues
// and the stores do not fit without scratch: two teams, as hadamard_block_kernel has at P = 32768)
constexpr int glu_teams(int G) { return G == 4 ? 2 : G; }

template <int G, typename GLU>
__global__ __launch_bounds__(256 * glu_teams(G)) void hadamard_block_glu_kernel(const GLU a) {
    static_assert(G == 1 || G == 2 || G == 4, "two row buffers of 16 KB G must fit the CU's LDS");
    constexpr int kTeams = glu_teams(G), kThreads = 256 * kTeams;
    __shared__ float4 rowbuf[2 * G * 1024];
    const int tid = threadIdx.x & 255, lane = tid & 63, w = tid >> 6, team = threadIdx.x >> 8;
    const size_t hes = a.g.y_dt == CQ_F32 ? 4 : 2;

    for (int64_t row = blockIdx.x; row < a.g.rows; row += gridDim.x) {
        char* hrow = a.g.y + (size_t)row * (size_t)a.g.ldy * hes;
#pragma unroll 1
        for (int sg = team; sg < 2 * G; sg += kTeams) {  // gate's sub-rows, then up's: 2 G / kTeams passes for
            const int s = sg >= G, g = sg - s * G;       // every team, so the barrier is uniform
            const auto& p = s ? a.u : a.g;
            const char* xrow = p.x + (size_t)row * (size_t)p.ldx * (p.x_dt == CQ_F32 ? 4 : 2);
            float4* buf = rowbuf + sg * 1024;
            float v[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) load4(p, xrow, (g * 1024 + (tid | (q << 8))) * 4, &v[q * 4]);
            chunk_stage<4>(v);
            lane_stages<4>(v, lane, 6);
            reg_stage<4>(v, 0);
            reg_stage<4>(v, 1);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                buf[lane + 64 * (w + 4 * q)] = make_float4(v[q * 4], v[q * 4 + 1], v[q * 4 + 2], v[q * 4 + 3]);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 f = buf[lane + 64 * (u + 4 * w)];
                v[u * 4] = f.x, v[u * 4 + 1] = f.y, v[u * 4 + 2] = f.z, v[u * 4 + 3] = f.w;
            }
            reg_stage<4>(v, 0);
            reg_stage<4>(v, 1);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                buf[lane + 64 * (u + 4 * w)] = make_float4(v[u * 4], v[u * 4 + 1], v[u * 4 + 2], v[u * 4 + 3]);
        }
        __syncthreads();
#pragma unroll 1
        for (int c = threadIdx.x; c < 1024; c += kThreads) {
            float vg[G * 4], vu[G * 4];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float4 f = rowbuf[g * 1024 + c];
                vg[g * 4] = f.x, vg[g * 4 + 1] = f.y, vg[g * 4 + 2] = f.z, vg[g * 4 + 3] = f.w;
                const float4 e = rowbuf[(G + g) * 1024 + c];
                vu[g * 4] = e.x, vu[g * 4 + 1] = e.y, vu[g * 4 + 2] = e.z, vu[g * 4 + 3] = e.w;
            }
#pragma unroll
            for (int b = 0; b < ilog2(G); ++b) {
                reg_stage<G>(vg, b);
                reg_stage<G>(vu, b);
            }
#pragma unroll
            for (int g = 0; g < G; ++g) glu_store4(a, hrow, (g * 1024 + c) * 4, &vg[g * 4], &vu[g * 4]);
        }
        __syncthreads();  // the next row's exchange writes the buffers again
    }
}

constexpr int64_t kMaxGridRows = (int64_t)1 << 20;  // more rows take the grid-stride loop

// ny: the grid's y extent (1 for HadP, the member count for HadGroupP)
template <int CH, typename ARG>
void launch_wave(const ARG& arg, int64_t rows, int lg_tl, unsigned ny, hipStream_t s) {
    const int64_t wgs = ceil_div(rows, (int64_t)(256 >> lg_tl));
    hipLaunchKernelGGL((hadamard_wave_kernel<CH, ARG>), dim3((unsigned)(wgs < kMaxGridRows ? wgs : kMaxGridRows), ny),
                       dim3(256), 0, s, arg);
}

template <int G, typename ARG>
void launch_block(const ARG& arg, int64_t rows, unsigned ny, hipStream_t s) {
    hipLaunchKernelGGL((hadamard_block_kernel<G, ARG>), dim3((unsigned)(rows < kMaxGridRows ? rows : kMaxGridRows), ny),
                       dim3(256 * block_teams<ARG>(G)), 0, s, arg);
}

// lg: log2 of the row's chunks of four (0 for P <= 4)
int log2_chunks(int64_t P) {
    // P < 4 runs as one chunk: the pad columns are zero, and adding zero changes no sum
    const int64_t chunks = P < 4 ? 1 : P / 4;
    int lg = 0;
    while (((int64_t)1 << lg) < chunks) ++lg;
    return lg;
}

template <typename ARG>
void launch_rows(const ARG& arg, int64_t rows, int lg, unsigned ny, hipStream_t s) {
    const int lg_tl = lg < 6 ? lg : 6;
    switch (lg) {
        case 7: launch_wave<2>(arg, rows, lg_tl, ny, s); break;   // P = 512
        case 8: launch_wave<4>(arg, rows, lg_tl, ny, s); break;   // 1024
        case 9: launch_wave<8>(arg, rows, lg_tl, ny, s); break;   // 2048
        case 10: launch_block<1>(arg, rows, ny, s); break;        // 4096
        case 11: launch_block<2>(arg, rows, ny, s); break;        // 8192
        case 12: launch_block<4>(arg, rows, ny, s); break;        // 16384
        case 13: launch_block<8>(arg, rows, ny, s); break;        // 32768
        default: launch_wave<1>(arg, rows, lg_tl, ny, s); break;  // P <= 256: 2^lg lanes per row
    }
}

template <int CH, typename GLU>
void launch_wave_glu(const GLU& a, hipStream_t s) {
    const int64_t wgs = ceil_div(a.g.rows, (int64_t)(256 >> a.g.lg_tl));
    hipLaunchKernelGGL((hadamard_wave_glu_kernel<CH, GLU>), dim3((unsigned)(wgs < kMaxGridRows ? wgs : kMaxGridRows)),
                       dim3(256), 0, s, a);
}

template <int G, typename GLU>
void launch_block_glu(const GLU& a, hipStream_t s) {
    hipLaunchKernelGGL((hadamard_block_glu_kernel<G, GLU>),
                       dim3((unsigned)(a.g.rows < kMaxGridRows ? a.g.rows : kMaxGridRows)), dim3(256 * glu_teams(G)), 0, s,
                       a);
}

bool dtype_ok(int dt) { return dt == CQ_F32 || dt == CQ_F16 || dt == CQ_BF16; }
size_t esize(int dt) { return dt == CQ_F32 ? 4 : 2; }
const char* dtype_name(int dt) { return dt == CQ_F32 ? "fp32" : dt == CQ_F16 ? "fp16" : "bf16"; }

// one aligned vector access per chunk of four: base and row pitch on the chunk's size
bool vec_ok(const void* ptr, int64_t ld, size_t es) {
    return (reinterpret_cast<uintptr_t>(ptr) % (4 * es)) == 0 && ((size_t)ld * es) % (4 * es) == 0;
}

// what a transform's fields are called in the caller's struct (the messages name them)
struct Names {
    const char *x, *y, *ldx, *ldy, *bias;
};
constexpr Names kRowsNames{"x", "y", "ldx", "ldy", "bias"};

// cq_hadamard_rows' checks of one transform; `who` names the entry (and the member) in the message, `nm`
// the fields, max_P the entry's largest transform
int validate(const cq_hadamard_args* a, const char* who, const Names& nm = kRowsNames, int max_P = CQ_HADAMARD_MAX_N) {
    CQ_REQUIRE(a->P >= 1 && a->P <= max_P && (a->P & (a->P - 1)) == 0,
               "%s: P = %lld is not a power of two in [1, %d]", who, (long long)a->P, max_P);
    CQ_REQUIRE(a->n_in >= 1 && a->n_in <= a->P, "%s: n_in = %lld is not in [1, P = %lld]", who, (long long)a->n_in,
               (long long)a->P);
    CQ_REQUIRE(a->n_out >= 0 && a->n_out <= a->P, "%s: n_out = %lld is not in [0, P = %lld]", who,
               (long long)a->n_out, (long long)a->P);
    CQ_REQUIRE(a->rows >= 0, "%s: rows = %lld is negative", who, (long long)a->rows);
    CQ_REQUIRE(dtype_ok(a->x_dtype), "%s: unknown %s dtype %d (fp32 | fp16 | bf16)", who, nm.x, a->x_dtype);
    CQ_REQUIRE(dtype_ok(a->y_dtype), "%s: unknown %s dtype %d (fp32 | fp16 | bf16)", who, nm.y, a->y_dtype);
    CQ_REQUIRE(reinterpret_cast<uintptr_t>(a->x) % esize(a->x_dtype) == 0, "%s: %s is not aligned to its %s element",
               who, nm.x, dtype_name(a->x_dtype));
    CQ_REQUIRE(reinterpret_cast<uintptr_t>(a->y) % esize(a->y_dtype) == 0, "%s: %s is not aligned to its %s element",
               who, nm.y, dtype_name(a->y_dtype));
    CQ_REQUIRE(reinterpret_cast<uintptr_t>(a->bias) % sizeof(float) == 0,
               "%s: %s is not aligned to its fp32 element", who, nm.bias);
    CQ_REQUIRE(a->ldx >= a->n_in && a->ldy >= a->n_out,
               "%s: leading dimension smaller than the row (%s %lld < n_in %lld or %s %lld < n_out %lld)", who, nm.ldx,
               (long long)a->ldx, (long long)a->n_in, nm.ldy, (long long)a->ldy, (long long)a->n_out);
    return CQ_OK;
}

// the kernels' parameters of one validated transform with rows > 0 and n_out > 0
HadP params(const cq_hadamard_args* a) {
    HadP p{};
    p.x = reinterpret_cast<const char*>(a->x);
    p.y = reinterpret_cast<char*>(a->y);
    p.bias = a->bias;
    p.ldx = a->ldx, p.ldy = a->ldy, p.rows = a->rows;
    p.n_in = (int)a->n_in, p.n_out = (int)a->n_out;
    p.x_dt = a->x_dtype, p.y_dt = a->y_dtype;
    p.x_vec = vec_ok(a->x, a->ldx, esize(a->x_dtype));
    p.y_vec = vec_ok(a->y, a->ldy, esize(a->y_dtype));
    p.b_vec = reinterpret_cast<uintptr_t>(a->bias) % 16 == 0;
    p.c = (float)(1.0 / std::sqrt((double)a->P));
    const int lg = log2_chunks(a->P);
    p.lg_tl = lg < 6 ? lg : 6;
    return p;
}

// the signed kernels' parameters: `params` and the two sign vectors (either may be null)
HadSP signed_params(const cq_hadamard_args* a, const int8_t* sign_in, const int8_t* sign_out) {
    HadSP p{};
    static_cast<HadP&>(p) = params(a);
    p.sign_in = sign_in, p.sign_out = sign_out;
    p.si_vec = reinterpret_cast<uintptr_t>(sign_in) % 4 == 0;
    p.so_vec = reinterpret_cast<uintptr_t>(sign_out) % 4 == 0;
    return p;
}

// a group member's transform and its kernel parameters, for both group entries
const cq_hadamard_args& args_of(const cq_hadamard_args& m) { return m; }
const cq_hadamard_args& args_of(const cq_hadamard_signed_args& m) { return m.a; }
HadP params_of(const cq_hadamard_args& m) { return params(&m); }
HadSP params_of(const cq_hadamard_signed_args& m) { return signed_params(&m.a, m.sign_in, m.sign_out); }

// cq_hadamard_group_rows (GP = HadGroupP, M = cq_hadamard_args) and cq_hadamard_signed_group_rows
template <typename GP, typename M>
int group_rows(const char* kWho, int count, const M* members, void* stream) {
    CQ_REQUIRE(count >= 1 && count <= CQ_HADAMARD_GROUP_MAX, "%s: count = %d is not in [1, %d]", kWho, count,
               CQ_HADAMARD_GROUP_MAX);
    CQ_REQUIRE(members != nullptr, "%s: null members", kWho);
    const cq_hadamard_args* m0 = &args_of(members[0]);
    char who[64];
    for (int i = 0; i < count; ++i) {
        const cq_hadamard_args* m = &args_of(members[i]);
        snprintf(who, sizeof who, "%s: member %d", kWho, i);
        if (const int st = validate(m, who)) return st;
        CQ_REQUIRE(m->rows == m0->rows, "%s: rows = %lld differs from member 0's %lld", who, (long long)m->rows,
                   (long long)m0->rows);
        CQ_REQUIRE(m->P == m0->P, "%s: P = %lld differs from member 0's %lld", who, (long long)m->P, (long long)m0->P);
    }
    if (m0->rows == 0) return CQ_OK;
    GP arg{};
    unsigned ny = 0;
    for (int i = 0; i < count; ++i) {
        const cq_hadamard_args* m = &args_of(members[i]);
        if (m->n_out == 0) continue;  // nothing to write: the member takes no part in the grid
        CQ_REQUIRE(m->x != nullptr && m->y != nullptr, "%s: member %d: null x or y", kWho, i);
        arg.m[ny++] = params_of(members[i]);
    }
    if (ny == 0) return CQ_OK;
    launch_rows(arg, m0->rows, log2_chunks(m0->P), ny, as_stream(stream));
    return check_launch(kWho);
}

// cq_hadamard_glu_rows (GLU = HadGluP; the signs are unused) and cq_hadamard_signed_glu_rows (HadSGluP)
template <typename GLU>
int glu_rows(const char* kWho, const cq_hadamard_glu_args* a, const int8_t* sign_g, const int8_t* sign_u,
             void* stream) {
    CQ_REQUIRE(a->act == CQ_ACT_IDENTITY || a->act == CQ_ACT_SILU, "%s: unknown act %d", kWho, a->act);
    // the two transforms as cq_hadamard_rows' arguments, h standing for y in both: the single entry's checks
    // on each, with the fields under this struct's names
    const cq_hadamard_args ga{a->g, a->g_dtype, a->ldg, a->h, a->h_dtype, a->ldh, a->rows, a->n_in, a->n_out, a->P,
                              a->bias_g};
    const cq_hadamard_args ua{a->u, a->u_dtype, a->ldu, a->h, a->h_dtype, a->ldh, a->rows, a->n_in, a->n_out, a->P,
                              a->bias_u};
    if (const int st = validate(&ga, kWho, Names{"g", "h", "ldg", "ldh", "bias_g"}, CQ_HADAMARD_GLU_MAX_N)) return st;
    if (const int st = validate(&ua, kWho, Names{"u", "h", "ldu", "ldh", "bias_u"}, CQ_HADAMARD_GLU_MAX_N)) return st;
    if (a->rows == 0 || a->n_out == 0) return CQ_OK;
    CQ_REQUIRE(a->g != nullptr && a->u != nullptr && a->h != nullptr, "%s: null g, u or h", kWho);
    GLU p{};
    if constexpr (std::is_same_v<GLU, HadSGluP>) {
        p.g = signed_params(&ga, nullptr, sign_g), p.u = signed_params(&ua, nullptr, sign_u);
    } else {
        p.g = params(&ga), p.u = params(&ua);
    }
    p.act = a->act;
    hipStream_t s = as_stream(stream);
    switch (log2_chunks(a->P)) {
        case 7: launch_wave_glu<2>(p, s); break;     // P = 512
        case 8: launch_wave_glu<4>(p, s); break;     // 1024
        case 9: launch_wave_glu<8>(p, s); break;     // 2048
        case 10: launch_block_glu<1>(p, s); break;   // 4096
        case 11: launch_block_glu<2>(p, s); break;   // 8192
        case 12: launch_block_glu<4>(p, s); break;   // 16384
        default: launch_wave_glu<1>(p, s); break;    // P <= 256
    }
    return check_launch(kWho);
}

}  // namespace
}  // namespace cq

using namespace cq;

extern "C" int cq_hadamard_rows(const cq_hadamard_args* a, void* stream) {
    CQ_REQUIRE(a != nullptr, "cq_hadamard_rows: null args");
    if (const int st = validate(a, "cq_hadamard_rows")) return st;
    if (a->rows == 0 || a->n_out == 0) return CQ_OK;
    CQ_REQUIRE(a->x != nullptr && a->y != nullptr, "cq_hadamard_rows: null x or y");
    launch_rows(params(a), a->rows, log2_chunks(a->P), 1, as_stream(stream));
    return check_launch("cq_hadamard_rows");
}

extern "C" int cq_hadamard_signed_rows(const cq_hadamard_signed_args* s, void* stream) {
    static const char* kWho = "cq_hadamard_signed_rows";
    CQ_REQUIRE(s != nullptr, "%s: null args", kWho);
    const cq_hadamard_args* a = &s->a;
    if (const int st = validate(a, kWho)) return st;
    if (a->rows == 0 || a->n_out == 0) return CQ_OK;
    CQ_REQUIRE(a->x != nullptr && a->y != nullptr, "%s: null x or y", kWho);
    launch_rows(signed_params(a, s->sign_in, s->sign_out), a->rows, log2_chunks(a->P), 1, as_stream(stream));
    return check_launch(kWho);
}

extern "C" int cq_hadamard_group_rows(const cq_hadamard_group_args* g, void* stream) {
    static const char* kWho = "cq_hadamard_group_rows";
    CQ_REQUIRE(g != nullptr, "%s: null args", kWho);
    return group_rows<HadGroupP>(kWho, (int)g->count, g->members, stream);
}

extern "C" int cq_hadamard_signed_group_rows(const cq_hadamard_signed_group_args* g, void* stream) {
    static const char* kWho = "cq_hadamard_signed_group_rows";
    CQ_REQUIRE(g != nullptr, "%s: null args", kWho);
    return group_rows<HadSGroupP>(kWho, (int)g->count, g->members, stream);
}

extern "C" int cq_hadamard_glu_rows(const cq_hadamard_glu_args* a, void* stream) {
    static const char* kWho = "cq_hadamard_glu_rows";
    CQ_REQUIRE(a != nullptr, "%s: null args", kWho);
    return glu_rows<HadGluP>(kWho, a, nullptr, nullptr, stream);
}

extern "C" int cq_hadamard_signed_glu_rows(const cq_hadamard_signed_glu_args* s, void* stream) {
    static const char* kWho = "cq_hadamard_signed_glu_rows";
    CQ_REQUIRE(s != nullptr, "%s: null args", kWho);
    return glu_rows<HadSGluP>(kWho, &s->a, s->sign_g, s->sign_u, stream);
}
