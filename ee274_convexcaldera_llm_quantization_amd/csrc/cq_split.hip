// Helpers around the split-fp16 products (cq_x3.hip): per-matrix max |x| and power-of-two
// split scales, the fp16 hi/lo split of fp32 operands (plain, K-blocked, of a symmetric
// matrix's upper triangle) and the batched transpose with split.
#include "cq_x3.h"

namespace cq {

template <int DT>
__global__ void absmax_dt_kernel(const void* __restrict__ X, int64_t n_per, uint32_t* __restrict__ out) {
    const int64_t b = blockIdx.y;
    uint32_t mx = 0;
    // 16-byte vector loads (8 halves / 4 floats per load) where the rows allow it
    constexpr int V = DT == CQ_F16 ? 8 : 4;
    const bool vec = n_per % V == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
    if (vec) {
        const uint4* Xv = reinterpret_cast<const uint4*>(X) + b * (n_per / V);
        for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n_per / V; q += (int64_t)gridDim.x * blockDim.x) {
            const uint4 r = Xv[q];
            if (DT == CQ_F16) {
                const _Float16* h = reinterpret_cast<const _Float16*>(&r);
#pragma unroll
                for (int u = 0; u < 8; ++u) mx = max(mx, abs_bits((float)h[u]));
            } else {
                mx = max(mx, max(max(abs_bits(__uint_as_float(r.x)), abs_bits(__uint_as_float(r.y))),
                                 max(abs_bits(__uint_as_float(r.z)), abs_bits(__uint_as_float(r.w)))));
            }
        }
        mx = wave_max_u32(mx);
        if ((threadIdx.x & 63) == 0 && mx) atomicMax(out + b, mx);
        return;
    }
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n_per; q += (int64_t)gridDim.x * blockDim.x) {
        const float v = DT == CQ_F16 ? (float)reinterpret_cast<const _Float16*>(X)[b * n_per + q]
                                     : reinterpret_cast<const float*>(X)[b * n_per + q];
        mx = max(mx, abs_bits(v));
    }
    mx = wave_max_u32(mx);
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(out + b, mx);
}

// ------------------------------------------------------------------ split / transpose helpers

// Per-batch power-of-two scale s = 2^(14 - ceil(log2 max_i G_ii)) for a PSD G (|G_ij| <=
// max diag), so the scaled hi halves stay <= 2^14 (fp16 max 65504) with headroom; the
// kernel stores 1 / (s * x_scale) for the GEMM epilogue and s for the split.
__global__ void sym_scale_kernel(const float* __restrict__ G, int64_t n, int64_t ldg, int64_t sg,
                                 float x_scale, float* __restrict__ s_out, float* __restrict__ inv_out) {
    const int64_t b = blockIdx.x;
    float m = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) m = fmaxf(m, fabsf(G[b * sg + i * ldg + i]));
    m = wave_max(m);
    __shared__ float red[16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) red[wid] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float mm = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) mm = fmaxf(mm, red[w]);
        int e = 0;
        if (mm > 0.f && isfinite(mm)) {
            frexpf(mm, &e);  // mm in [2^(e-1), 2^e)
        }
        const float s = ldexpf(1.f, 14 - e);
        s_out[b] = s;
        inv_out[b] = 1.f / (s * x_scale);
    }
}

__global__ void split_kernel(const float* __restrict__ X, int64_t n_per, const float* __restrict__ s_v,
                             float s_fixed, _Float16* __restrict__ hi, _Float16* __restrict__ lo, int64_t batch) {
    const int64_t tot4 = batch * n_per / 4;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < tot4; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = q * 4;
        const int64_t o = e;
        const float s = s_v ? s_v[e / n_per] : s_fixed;
        const float4 v = *reinterpret_cast<const float4*>(X + e);
        const float xs[4] = {v.x * s, v.y * s, v.z * s, v.w * s};
        _Float16 h[4], l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            h[u] = (_Float16)xs[u];
            l[u] = (_Float16)(xs[u] - (float)h[u]);
        }
        *reinterpret_cast<uint2*>(hi + o) = *reinterpret_cast<const uint2*>(h);
        *reinterpret_cast<uint2*>(lo + o) = *reinterpret_cast<const uint2*>(l);
    }
}

// Split of a symmetric matrix of which only the upper triangle (j >= i) is valid: 64 x 64
// tiles, lower tiles read from the transposed upper tile through LDS.
__device__ __forceinline__ int64_t blk_off(int64_t i, int64_t j, int64_t n, int blocked) {
    return blocked ? ((j >> 5) * n * 32 + i * 32 + (j & 31)) : (i * n + j);
}

__global__ __launch_bounds__(256) void sym_split_upper_kernel(const float* __restrict__ G, int64_t n,
                                                              const float* __restrict__ s_v,
                                                              _Float16* __restrict__ hi, _Float16* __restrict__ lo,
                                                              int blocked) {
    __shared__ float tile[64][65];
    const int64_t b = blockIdx.z;
    const int64_t ti = blockIdx.y, tj = blockIdx.x;
    const float* Gb = G + b * n * n;
    const float s = s_v[b];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const bool lower = ti > tj;
    const int64_t si = lower ? tj : ti, sj = lower ? ti : tj;  // source tile (upper)
    for (int r = ty; r < 64; r += 4) {
        const int64_t i = si * 64 + r, j = sj * 64 + tx;
        // inside a diagonal tile, take (min, max) so only upper entries are read
        float v = 0.f;
        if (i < n && j < n) v = (j >= i) ? Gb[i * n + j] : Gb[j * n + i];
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int64_t i = ti * 64 + r, j = tj * 64 + tx;
        if (i < n && j < n) {
            const float v = (lower ? tile[tx][r] : tile[r][tx]) * s;
            const _Float16 h = (_Float16)v;
            const int64_t o = b * n * n + blk_off(i, j, n, blocked);
            hi[o] = h;
            lo[o] = (_Float16)(v - (float)h);
        }
    }
}

// Per-batch max |x| as uint bits (atomicMax into a zeroed buffer), then
// s[b] = 2^(log2_target - e) with max in [2^(e-1), 2^e): the scaled values stay below 2^log2_target.
__global__ void absmax_bits_kernel(const float* __restrict__ X, int64_t n_per, uint32_t* __restrict__ out) {
    const int64_t b = blockIdx.y;
    const float* Xb = X + b * n_per;
    uint32_t m = 0;
    const int64_t n4 = n_per / 4;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n4; q += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = *reinterpret_cast<const float4*>(Xb + 4 * q);
        m = max(m, max(max(abs_bits(v.x), abs_bits(v.y)), max(abs_bits(v.z), abs_bits(v.w))));
    }
    for (int64_t q = 4 * n4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n_per;
         q += (int64_t)gridDim.x * blockDim.x)
        m = max(m, abs_bits(Xb[q]));
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out + b, m);
}

__global__ void pow2_scale_kernel(float* __restrict__ s, int64_t batch, int log2_target) {
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const float mm = __uint_as_float(reinterpret_cast<const uint32_t*>(s)[b]);
    int e = 0;
    if (mm > 0.f && isfinite(mm)) frexpf(mm, &e);
    s[b] = ldexpf(1.f, log2_target - e);
}

// K-blocked split (ncols % 32 == 0): element (row, col) of a rows x ncols matrix goes to
// (col / 32) * rows * 32 + row * 32 + col % 32 — the K-blocked operand layout of cq_gemm_x3.
// grid (rows / 4, batch): one row per wave, no integer division.
__global__ __launch_bounds__(256) void split_blocked_kernel(const float* __restrict__ X, int64_t rows, int64_t ncols,
                                                            const float* __restrict__ s_v, float s_fixed,
                                                            _Float16* __restrict__ hi, _Float16* __restrict__ lo) {
    const int64_t b = blockIdx.y;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float s = s_v ? s_v[b] : s_fixed;
    const float* xr = X + b * rows * ncols + row * ncols;
    _Float16* hb = hi + b * rows * ncols + row * 32;
    _Float16* lb = lo + b * rows * ncols + row * 32;
    for (int64_t c = 4 * (threadIdx.x & 63); c < ncols; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + c);
        const float xs[4] = {v.x * s, v.y * s, v.z * s, v.w * s};
        _Float16 h[4], l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            h[u] = (_Float16)xs[u];
            l[u] = (_Float16)(xs[u] - (float)h[u]);
        }
        const int64_t o = (c >> 5) * rows * 32 + (c & 31);
        *reinterpret_cast<uint2*>(hb + o) = *reinterpret_cast<const uint2*>(h);
        *reinterpret_cast<uint2*>(lb + o) = *reinterpret_cast<const uint2*>(l);
    }
}

// Batched transpose Y = X^T (X rows x cols, row-major) through a 64 x 65 LDS tile, with an
// optional fp16 split of Y (scale s).  VEC (rows % 8 == 0, cols % 4 == 0, 16-byte aligned
// buffers; the solver's k x p blocks): 16-byte loads of X, and each thread writes 8
// consecutive Y columns of one Y row -- two 16-byte fp32 stores and one 16-byte store per
// half -- instead of one 4-byte and two 2-byte stores per element (the tile's column reads
// (8 g + q) x 65 + i, lane = (i, g), hit 64 different banks).  The same values either way.
template <bool VEC>
__global__ __launch_bounds__(256) void transpose_split_kernel(const float* __restrict__ X, int64_t rows, int64_t cols,
                                                              float* __restrict__ Y, _Float16* __restrict__ hi,
                                                              _Float16* __restrict__ lo, float s_fixed,
                                                              const float* __restrict__ s_v, int blocked,
                                                              const int* __restrict__ active) {
    __shared__ float tile[64][65];
    const int64_t b = blockIdx.z;
    if (active && !active[b]) return;  // masked-out matrix: Y and the halves untouched
    const int64_t r0 = (int64_t)blockIdx.y * 64, c0 = (int64_t)blockIdx.x * 64;
    const float* Xb = X + b * rows * cols;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t ob = b * rows * cols;
    const float s = s_v ? s_v[b] : s_fixed;
    if constexpr (VEC) {
        // load: 64 rows x 16 float4, 4 per thread (thread t: rows t / 16 + 16 u, float4 t % 16)
        const int q4 = threadIdx.x & 15, rq = threadIdx.x >> 4;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = rq + 16 * u;
            const int64_t r = r0 + i, c = c0 + 4 * q4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows && c < cols) v = *reinterpret_cast<const float4*>(Xb + r * cols + c);
            tile[i][4 * q4] = v.x; tile[i][4 * q4 + 1] = v.y; tile[i][4 * q4 + 2] = v.z; tile[i][4 * q4 + 3] = v.w;
        }
        __syncthreads();
        // store: Y row orow = c0 + i (64 of them), columns r0 + 8 g .. + 7 (g = 0..7): 512 tasks,
        // 2 per thread; a wave covers 8 Y rows x 64 columns
        const int g = threadIdx.x & 7, il = threadIdx.x >> 3;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = il + 32 * u;
            const int64_t orow = c0 + i, ocol = r0 + 8 * g;
            if (orow >= cols || ocol >= rows) continue;
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = tile[8 * g + q][i];
            if (Y) {
                float* yp = Y + ob + orow * rows + ocol;
                *reinterpret_cast<float4*>(yp) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4*>(yp + 4) = make_float4(v[4], v[5], v[6], v[7]);
            }
            if (hi) {
                _Float16 h[8], l[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float xs = v[q] * s;
                    h[q] = (_Float16)xs;
                    l[q] = (_Float16)(xs - (float)h[q]);
                }
                const int64_t o = blocked ? ob + (ocol >> 5) * cols * 32 + orow * 32 + (ocol & 31) : ob + orow * rows + ocol;
                *reinterpret_cast<uint4*>(hi + o) = *reinterpret_cast<const uint4*>(h);
                if (lo) *reinterpret_cast<uint4*>(lo + o) = *reinterpret_cast<const uint4*>(l);
            }
        }
        return;
    }
    for (int i = ty; i < 64; i += 4) {
        const int64_t r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? Xb[r * cols + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int64_t orow = c0 + i, ocol = r0 + tx;  // Y is cols x rows
        if (orow < cols && ocol < rows) {
            const float v = tile[tx][i];
            if (Y) Y[ob + orow * rows + ocol] = v;
            if (hi) {
                const float xs = v * s;
                const _Float16 h = (_Float16)xs;
                // Y is cols x rows: K-blocked halves put (orow, ocol) at (ocol/32)*cols*32 + orow*32 + ocol%32
                const int64_t o = blocked ? ob + (ocol >> 5) * cols * 32 + orow * 32 + (ocol & 31) : ob + orow * rows + ocol;
                hi[o] = h;
                if (lo) lo[o] = (_Float16)(xs - (float)h);
            }
        }
    }
}


}  // namespace cq

using namespace cq;

extern "C" {

int cq_sym_split_f16(const float* G, int64_t n, int64_t batch, int upper_only, int blocked, float x_scale,
                     uint16_t* Gh, uint16_t* Gl, float* scale_out, float* inv_scale_out, void* stream) {
    CQ_REQUIRE(G && Gh && Gl && scale_out && inv_scale_out, "cq_sym_split_f16: null pointer");
    CQ_REQUIRE(n > 0 && batch > 0 && (n * n) % 4 == 0, "cq_sym_split_f16: bad shape");
    CQ_REQUIRE(x_scale > 0.f, "cq_sym_split_f16: x_scale must be > 0");
    hipStream_t s = as_stream(stream);
    sym_scale_kernel<<<(unsigned)batch, 256, 0, s>>>(G, n, n, n * n, x_scale, scale_out, inv_scale_out);
    CQ_REQUIRE(!blocked || n % 32 == 0, "cq_sym_split_f16: blocked layout needs n % 32 == 0");
    if (upper_only || blocked) {
        CQ_REQUIRE(batch < 65536, "cq_sym_split_f16: batch too large");
        const unsigned t64 = (unsigned)ceil_div(n, 64);
        sym_split_upper_kernel<<<dim3(t64, t64, (unsigned)batch), 256, 0, s>>>(
            G, n, scale_out, reinterpret_cast<_Float16*>(Gh), reinterpret_cast<_Float16*>(Gl), blocked);
        return check_launch("cq_sym_split_f16");
    }
    const int64_t tot4 = batch * n * n / 4;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(tot4, 256), 8192);
    split_kernel<<<grid, 256, 0, s>>>(G, n * n, scale_out, 1.f, reinterpret_cast<_Float16*>(Gh),
                                      reinterpret_cast<_Float16*>(Gl), batch);
    return check_launch("cq_sym_split_f16");
}

int cq_pow2_scale(const float* X, int64_t n_per, int64_t batch, int log2_target, float* scale_out, void* stream) {
    CQ_REQUIRE(X && scale_out, "cq_pow2_scale: null pointer");
    CQ_REQUIRE(n_per > 0 && batch > 0 && batch < 65536 && n_per % 4 == 0, "cq_pow2_scale: bad shape");
    CQ_REQUIRE(log2_target > -100 && log2_target < 100, "cq_pow2_scale: bad target");
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(scale_out, 0, batch * sizeof(float), s) != hipSuccess)
        return set_error(CQ_EHIP, "cq_pow2_scale: memset failed");
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n_per / 4, 256), std::max<int64_t>(1, 2048 / batch)));
    absmax_bits_kernel<<<dim3(gx, (unsigned)batch), 256, 0, s>>>(X, n_per, reinterpret_cast<uint32_t*>(scale_out));
    pow2_scale_kernel<<<(unsigned)ceil_div(batch, 256), 256, 0, s>>>(scale_out, batch, log2_target);
    return check_launch("cq_pow2_scale");
}

int cq_pow2_from_absmax(float* scale_inout, int64_t batch, int log2_target, void* stream) {
    CQ_REQUIRE(scale_inout && batch > 0, "cq_pow2_from_absmax: bad args");
    CQ_REQUIRE(log2_target > -100 && log2_target < 100, "cq_pow2_from_absmax: bad target");
    pow2_scale_kernel<<<(unsigned)ceil_div(batch, 256), 256, 0, as_stream(stream)>>>(scale_inout, batch, log2_target);
    return check_launch("cq_pow2_from_absmax");
}

int cq_split_f16(const float* X, int64_t n_per, int64_t batch, const float* scale_v, float scale, uint16_t* hi,
                 uint16_t* lo, int64_t blocked_ncols, void* stream) {
    CQ_REQUIRE(X && hi && lo, "cq_split_f16: null pointer");
    CQ_REQUIRE(n_per > 0 && batch > 0 && n_per % 4 == 0, "cq_split_f16: n_per must be a positive multiple of 4");
    CQ_REQUIRE(blocked_ncols == 0 || (blocked_ncols % 32 == 0 && n_per % blocked_ncols == 0),
               "cq_split_f16: blocked layout needs ncols % 32 == 0 dividing n_per");
    const int64_t tot4 = batch * n_per / 4;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(tot4, 256), 8192);
    if (blocked_ncols) {
        const int64_t rows = n_per / blocked_ncols;
        CQ_REQUIRE(batch < 65536, "cq_split_f16: batch too large");
        split_blocked_kernel<<<dim3((unsigned)ceil_div(rows, 4), (unsigned)batch), 256, 0, as_stream(stream)>>>(
            X, rows, blocked_ncols, scale_v, scale, reinterpret_cast<_Float16*>(hi), reinterpret_cast<_Float16*>(lo));
        return check_launch("cq_split_f16");
    }
    split_kernel<<<grid, 256, 0, as_stream(stream)>>>(X, n_per, scale_v, scale, reinterpret_cast<_Float16*>(hi),
                                                      reinterpret_cast<_Float16*>(lo), batch);
    return check_launch("cq_split_f16");
}

int cq_transpose_split(const float* X, int64_t rows, int64_t cols, int64_t batch, float* Y, uint16_t* hi,
                       uint16_t* lo, float scale, const float* scale_v, int blocked, void* stream) {
    return cq_transpose_split_masked(X, rows, cols, batch, Y, hi, lo, scale, scale_v, blocked, nullptr, stream);
}

int cq_transpose_split_masked(const float* X, int64_t rows, int64_t cols, int64_t batch, float* Y, uint16_t* hi,
                              uint16_t* lo, float scale, const float* scale_v, int blocked, const int* active,
                              void* stream) {
    CQ_REQUIRE(!blocked || rows % 32 == 0, "cq_transpose_split: blocked halves need rows % 32 == 0");
    CQ_REQUIRE(X && (Y || hi), "cq_transpose_split: null pointer");
    CQ_REQUIRE(hi || !lo, "cq_transpose_split: lo needs hi (hi alone: the operand of a single product)");
    CQ_REQUIRE(rows > 0 && cols > 0 && batch > 0 && batch < 65536, "cq_transpose_split: bad shape");
    dim3 grid((unsigned)ceil_div(cols, 64), (unsigned)ceil_div(rows, 64), (unsigned)batch);
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec = rows % 8 == 0 && cols % 4 == 0 && al16(X) && (!Y || al16(Y)) && (!hi || al16(hi)) && (!lo || al16(lo));
    if (vec)
        transpose_split_kernel<true><<<grid, 256, 0, as_stream(stream)>>>(
            X, rows, cols, Y, reinterpret_cast<_Float16*>(hi), reinterpret_cast<_Float16*>(lo), scale, scale_v, blocked, active);
    else
        transpose_split_kernel<false><<<grid, 256, 0, as_stream(stream)>>>(
            X, rows, cols, Y, reinterpret_cast<_Float16*>(hi), reinterpret_cast<_Float16*>(lo), scale, scale_v, blocked, active);
    return check_launch("cq_transpose_split");
}

int cq_absmax(int dtype, const void* X, int64_t n_per, int64_t batch, float* out, void* stream) {
    CQ_REQUIRE(X && out && n_per > 0 && batch > 0 && batch < 65536, "cq_absmax: bad args");
    CQ_REQUIRE(dtype == CQ_F16 || dtype == CQ_F32, "cq_absmax: dtype must be f16/f32");
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(out, 0, batch * sizeof(float), s) != hipSuccess) return set_error(CQ_EHIP, "cq_absmax: memset");
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n_per, 256), std::max<int64_t>(1, 4096 / batch)));
    if (dtype == CQ_F16) absmax_dt_kernel<CQ_F16><<<dim3(gx, (unsigned)batch), 256, 0, s>>>(X, n_per, reinterpret_cast<uint32_t*>(out));
    else absmax_dt_kernel<CQ_F32><<<dim3(gx, (unsigned)batch), 256, 0, s>>>(X, n_per, reinterpret_cast<uint32_t*>(out));
    return check_launch("cq_absmax");  // max |x| bits are the float's bits: out reads as float
}

}  // extern "C"
