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
#include <cmath>

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

// c * v (+ bias) rounded once to y's type; columns >= n_out are not written
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
template <int CH>
__global__ __launch_bounds__(256) void hadamard_wave_kernel(const HadP p) {
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
// stores do not fit without scratch: two teams)
constexpr int block_teams(int G) { return G == 8 ? 2 : G; }

template <int G>
__global__ __launch_bounds__(256 * block_teams(G)) void hadamard_block_kernel(const HadP p) {
    constexpr int kTeams = block_teams(G), kThreads = 256 * kTeams;
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

constexpr int64_t kMaxGridRows = (int64_t)1 << 20;  // more rows take the grid-stride loop

template <int CH>
void launch_wave(const HadP& p, hipStream_t s) {
    const int64_t wgs = ceil_div(p.rows, (int64_t)(256 >> p.lg_tl));
    hipLaunchKernelGGL((hadamard_wave_kernel<CH>), dim3((unsigned)(wgs < kMaxGridRows ? wgs : kMaxGridRows)),
                       dim3(256), 0, s, p);
}

template <int G>
void launch_block(const HadP& p, hipStream_t s) {
    hipLaunchKernelGGL((hadamard_block_kernel<G>), dim3((unsigned)(p.rows < kMaxGridRows ? p.rows : kMaxGridRows)),
                       dim3(256 * block_teams(G)), 0, s, p);
}

bool dtype_ok(int dt) { return dt == CQ_F32 || dt == CQ_F16 || dt == CQ_BF16; }
size_t esize(int dt) { return dt == CQ_F32 ? 4 : 2; }
const char* dtype_name(int dt) { return dt == CQ_F32 ? "fp32" : dt == CQ_F16 ? "fp16" : "bf16"; }

// one aligned vector access per chunk of four: base and row pitch on the chunk's size
bool vec_ok(const void* ptr, int64_t ld, size_t es) {
    return (reinterpret_cast<uintptr_t>(ptr) % (4 * es)) == 0 && ((size_t)ld * es) % (4 * es) == 0;
}

}  // namespace
}  // namespace cq

using namespace cq;

extern "C" int cq_hadamard_rows(const cq_hadamard_args* a, void* stream) {
    CQ_REQUIRE(a != nullptr, "cq_hadamard_rows: null args");
    CQ_REQUIRE(a->P >= 1 && a->P <= CQ_HADAMARD_MAX_N && (a->P & (a->P - 1)) == 0,
               "cq_hadamard_rows: P = %lld is not a power of two in [1, %d]", (long long)a->P, CQ_HADAMARD_MAX_N);
    CQ_REQUIRE(a->n_in >= 1 && a->n_in <= a->P, "cq_hadamard_rows: n_in = %lld is not in [1, P = %lld]",
               (long long)a->n_in, (long long)a->P);
    CQ_REQUIRE(a->n_out >= 0 && a->n_out <= a->P, "cq_hadamard_rows: n_out = %lld is not in [0, P = %lld]",
               (long long)a->n_out, (long long)a->P);
    CQ_REQUIRE(a->rows >= 0, "cq_hadamard_rows: rows = %lld is negative", (long long)a->rows);
    CQ_REQUIRE(dtype_ok(a->x_dtype), "cq_hadamard_rows: unknown x dtype %d (fp32 | fp16 | bf16)", a->x_dtype);
    CQ_REQUIRE(dtype_ok(a->y_dtype), "cq_hadamard_rows: unknown y dtype %d (fp32 | fp16 | bf16)", a->y_dtype);
    CQ_REQUIRE(reinterpret_cast<uintptr_t>(a->x) % esize(a->x_dtype) == 0,
               "cq_hadamard_rows: x is not aligned to its %s element", dtype_name(a->x_dtype));
    CQ_REQUIRE(reinterpret_cast<uintptr_t>(a->y) % esize(a->y_dtype) == 0,
               "cq_hadamard_rows: y is not aligned to its %s element", dtype_name(a->y_dtype));
    CQ_REQUIRE(reinterpret_cast<uintptr_t>(a->bias) % sizeof(float) == 0,
               "cq_hadamard_rows: bias is not aligned to its fp32 element");
    CQ_REQUIRE(a->ldx >= a->n_in && a->ldy >= a->n_out,
               "cq_hadamard_rows: leading dimension smaller than the row (ldx %lld < n_in %lld or ldy %lld < n_out "
               "%lld)", (long long)a->ldx, (long long)a->n_in, (long long)a->ldy, (long long)a->n_out);
    if (a->rows == 0 || a->n_out == 0) return CQ_OK;
    CQ_REQUIRE(a->x != nullptr && a->y != nullptr, "cq_hadamard_rows: null x or y");

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
    // P < 4 runs as one chunk: the pad columns are zero, and adding zero changes no sum
    const int64_t chunks = a->P < 4 ? 1 : a->P / 4;
    int lg = 0;
    while (((int64_t)1 << lg) < chunks) ++lg;
    p.lg_tl = lg < 6 ? lg : 6;
    hipStream_t s = as_stream(stream);
    switch (lg) {
        case 7: launch_wave<2>(p, s); break;         // P = 512
        case 8: launch_wave<4>(p, s); break;         // 1024
        case 9: launch_wave<8>(p, s); break;         // 2048
        case 10: launch_block<1>(p, s); break;       // 4096
        case 11: launch_block<2>(p, s); break;       // 8192
        case 12: launch_block<4>(p, s); break;       // 16384
        case 13: launch_block<8>(p, s); break;       // 32768
        default: launch_wave<1>(p, s); break;        // P <= 256: 2^lg lanes per row
    }
    return check_launch("cq_hadamard_rows");
}
