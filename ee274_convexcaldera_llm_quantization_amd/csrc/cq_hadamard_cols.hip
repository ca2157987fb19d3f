// cq_hadamard_cols: the normalised Sylvester-Hadamard transform down the columns of a row-major fp32
// matrix (fast Walsh-Hadamard transform, FWHT), the other direction of cq_hadamard_rows.  Together they
// form H1 pad(W) H2 of a weight decomposed in the Hadamard basis (model.hadamard_transform(kernels=True))
// without a Hadamard matrix and without a padded copy of W:
//
//   y[i, j] = s_out[i] * c * sum_{k < n_in} (-1)^popcount(i & k) s_in[k] x[k, j],   i < n_out, c = 1 / sqrt(P)
//
// Structure.  A column butterfly pairs the same column of two rows, so a thread that holds several rows
// of its own four consecutive columns (one 16-byte chunk per row) runs those stages in registers with no
// data movement: the opposite of the row kernel, whose lane bits need shuffles.
//
//   - Tile.  A workgroup of 128 threads owns 2^LG <= 256 rows of 32 columns: a row segment is one whole
//     128-byte line, eight lanes of one chunk each.  tid = cc | slot << 3: cc is the chunk of the line,
//     slot < 16 the thread's place among the rows.  A thread holds 16 rows (64 fp32 registers).
//   - Phase 1.  The thread holds the rows r = slot << 4 | q, q < 16: the low four row bits are register
//     bits and are finished in registers.
//   - Exchange.  Register plane q goes to LDS at slot q * 136 + tid (16 bytes per lane, consecutive lanes
//     on consecutive slots), one barrier, and the thread reads back the rows r = s | e_l << B | e_h << 4
//     (B = LG - 4 high bits, s its low B slot bits, e < 16 its register index, e_h the top B bits of e):
//     the high row bits have become register bits and are finished in registers.  The plane pitch of
//     136 slots (128 + one line) puts the planes that the eight lanes of consecutive s read 128 bytes
//     apart modulo 1024, so a wave's 64 reads fall on 64 different 16-byte positions of any 1 KB window
//     of banks, as its 64 writes do: no swizzle.  16 x 136 x 16 bytes = 34 KB of LDS per workgroup.
//   - Tiles of fewer than 256 rows (a small P, or the second pass) use the slot bits that the rows leave
//     free for further column tiles: a workgroup is then 16 >> B tiles wide (512 columns for LG <= 4,
//     which needs no LDS at all).
//   - One pass, P <= 256: x -> y.  Rows >= n_in are zero and are not read, s_in is applied as a row is
//     loaded; c, s_out and the cut to n_out are applied as a row is stored.
//   - Two passes, P = 256 * 2^LG2 <= 32768: pass 1 finishes the low eight bits on blocks of 256
//     consecutive rows, x -> workspace (P x cols fp32); pass 2 finishes the high LG2 bits on rows 256
//     apart, workspace -> y.  A block of 256 rows that lies wholly at or past n_in is zero: pass 1 does
//     not run it and pass 2 does not read it.
//   - A group of column tiles that is cut by `cols`, or every group when a matrix is not 16-byte aligned
//     (base or leading dimension), runs in a second instantiation whose scalar path loads the same values.
//     Columns never mix, so a column's stage order, and with it its bits, is a function of P alone: not
//     of its index, of cols or of the alignment.
//   - Grid: x is the groups of column tiles, y the row blocks (pass 1) or the 256 row offsets (pass 2):
//     16384 x 4096 is 128 x 64 workgroups, then 16 x 256.
// All arithmetic is fp32.  No atomics, no inline assembly, no host synchronisation.
#include <cmath>

#include "cq_common.h"

namespace cq {
namespace {

constexpr int kThreads = 128;
constexpr int kLgTile = 8;              // a pass finishes up to 8 row bits: tiles of up to 256 rows
constexpr int kTileRows = 1 << kLgTile;
constexpr int kPlane = kThreads + 8;    // LDS slots (16 bytes) between two register planes
constexpr int64_t kMaxCols = (int64_t)1 << 35;  // 2^30 column tiles of 32: the grid's x extent

struct ColsP {
    const float* x;
    float* y;
    int64_t ldx, ldy, cols;
    int64_t base_mul, row_stride;  // tile row r of row block b is the matrix row b * base_mul + r * row_stride
    int n_in, n_out;               // rows >= n_in are zero and not read, rows >= n_out are not written
    const int8_t* sign_in;
    const int8_t* sign_out;
    int64_t g0;                    // the launch's first group of column tiles (blockIdx.x counts from it)
    float c;
};

// v negated iff the sign byte is negative: the byte's top bit goes into the float's sign bit (exact)
__device__ __forceinline__ uint32_t flip_bit(const int8_t* sign, int64_t row) {
    return sign == nullptr ? 0u : (uint32_t)(int32_t)sign[row] & 0x80000000u;
}
__device__ __forceinline__ float flipped(float v, uint32_t bit) { return __uint_as_float(__float_as_uint(v) ^ bit); }

// v[q] = s_in[row] * x[row, j0 .. j0 + 4) for the rows row_of(q), q < N; a row >= n_in and columns >= cols are
// zero and are not read.  WHOLE: every chunk of the launch is one aligned 16-byte load.  The loads then stand
// in a row without a branch between them, so that all of a thread's rows are in flight together: a row
// >= n_in loads row n_in - 1 in its place and drops the value.
template <bool WHOLE, int N, typename RowOf>
__device__ __forceinline__ void load_rows(const ColsP& p, RowOf row_of, int64_t j0, float (&v)[N][4]) {
    if constexpr (WHOLE) {
        uint32_t bit[N];
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const int64_t row = row_of(q), src = row < p.n_in ? row : p.n_in - 1;
            const float4 f = *reinterpret_cast<const float4*>(p.x + src * p.ldx + j0);
            v[q][0] = f.x, v[q][1] = f.y, v[q][2] = f.z, v[q][3] = f.w;
            bit[q] = flip_bit(p.sign_in, src);
        }
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const bool zero = row_of(q) >= p.n_in;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[q][k] = zero ? 0.0f : flipped(v[q][k], bit[q]);
        }
    } else {
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const int64_t row = row_of(q);
            v[q][0] = v[q][1] = v[q][2] = v[q][3] = 0.0f;
            if (row >= p.n_in) continue;
            const float* src = p.x + row * p.ldx + j0;
            const uint32_t bit = flip_bit(p.sign_in, row);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < p.cols) v[q][k] = flipped(src[k], bit);
        }
    }
}

// y[row, j0 .. j0 + 4) = s_out[row] * (c * v[q]) for the rows row_of(q); a row >= n_out and columns >= cols
// are not written.  WHOLE: as in load_rows.
template <bool WHOLE, int N, typename RowOf>
__device__ __forceinline__ void store_rows(const ColsP& p, RowOf row_of, int64_t j0, const float (&v)[N][4]) {
    if constexpr (WHOLE) {
        uint32_t bit[N];
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const int64_t row = row_of(q);
            bit[q] = flip_bit(p.sign_out, row < p.n_out ? row : p.n_out - 1);
        }
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const int64_t row = row_of(q);
            if (row < p.n_out)
                *reinterpret_cast<float4*>(p.y + row * p.ldy + j0) =
                    make_float4(flipped(v[q][0] * p.c, bit[q]), flipped(v[q][1] * p.c, bit[q]),
                                flipped(v[q][2] * p.c, bit[q]), flipped(v[q][3] * p.c, bit[q]));
        }
    } else {
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const int64_t row = row_of(q);
            if (row >= p.n_out) continue;
            float* dst = p.y + row * p.ldy + j0;
            const uint32_t bit = flip_bit(p.sign_out, row);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < p.cols) dst[k] = flipped(v[q][k] * p.c, bit);
        }
    }
}

// butterflies (a, b) -> (a + b, a - b) over bit `bit` of the register (row) index, on the four columns
template <int N>
__device__ __forceinline__ void reg_stage(float (&v)[N][4], int bit) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
        if (q & (1 << bit)) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = v[q][k], b = v[q | (1 << bit)][k];
            v[q][k] = a + b;
            v[q | (1 << bit)][k] = a - b;
        }
    }
}

// One pass over tiles of 2^LG rows: LG row bits finished between one load and one store of every element.
// WHOLE: x and y are 16-byte aligned and no chunk of the launch's groups is cut by cols; the
// other instantiation runs the cut last group, or every group of an unaligned matrix.
template <int LG, bool WHOLE>
__global__ __launch_bounds__(kThreads) void hadamard_cols_kernel(const ColsP p) {
    constexpr int A = LG < 4 ? LG : 4;  // row bits that are register bits in phase 1
    constexpr int B = LG - A;           // row bits that are slot bits in phase 1, register bits in phase 2
    constexpr int N = 1 << A;           // rows a thread holds
    constexpr int kTiles = 16 >> B;     // column tiles of 32 a workgroup is wide
    __shared__ float4 planes[B > 0 ? 16 * kPlane : 1];

    const int tid = threadIdx.x, cc = tid & 7, slot = tid >> 3;
    const int s = slot & ((1 << B) - 1), tile = slot >> B;
    const int64_t row0 = (int64_t)blockIdx.y * p.base_mul;
    const int64_t j0 = (((p.g0 + blockIdx.x) * kTiles + tile) * 8 + cc) * 4;
    float v[N][4];
    // phase 1: the rows r = s << A | q
    const auto row1 = [&](int q) { return row0 + (int64_t)(s << A | q) * p.row_stride; };
    load_rows<WHOLE, N>(p, row1, j0, v);
#pragma unroll
    for (int b = 0; b < A; ++b) reg_stage<N>(v, b);
    if constexpr (B == 0) {
        store_rows<WHOLE, N>(p, row1, j0, v);
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) planes[q * kPlane + tid] = make_float4(v[q][0], v[q][1], v[q][2], v[q][3]);
        __syncthreads();
        // phase 2: the rows r = s | e_l << B | e_h << 4, e_h the top B bits of e; row r was register
        // r & 15 of the thread with slot bits r >> 4
        const auto r2 = [&](int e) { return s | (e & ((1 << (4 - B)) - 1)) << B | (e >> (4 - B)) << 4; };
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = r2(e);
            const float4 f = planes[(r & 15) * kPlane + (cc | (tile << B | r >> 4) << 3)];
            v[e][0] = f.x, v[e][1] = f.y, v[e][2] = f.z, v[e][3] = f.w;
        }
#pragma unroll
        for (int b = 4 - B; b < 4; ++b) reg_stage<16>(v, b);
        store_rows<WHOLE, N>(p, [&](int e) { return row0 + (int64_t)r2(e) * p.row_stride; }, j0, v);
    }
}

template <int LG, bool WHOLE>
void launch_groups(ColsP p, int64_t g0, int64_t g1, int64_t row_blocks, hipStream_t s) {
    if (g0 == g1) return;
    p.g0 = g0;
    hipLaunchKernelGGL((hadamard_cols_kernel<LG, WHOLE>), dim3((unsigned)(g1 - g0), (unsigned)row_blocks),
                       dim3(kThreads), 0, s, p);
}

// the whole groups of an aligned matrix in one launch, whatever is left in another
template <int LG>
void launch_pass(const ColsP& p, bool aligned, int64_t row_blocks, hipStream_t s) {
    constexpr int kTiles = 16 >> (LG < 4 ? 0 : LG - 4);
    const int64_t whole = aligned ? p.cols / (32 * kTiles) : 0;
    launch_groups<LG, true>(p, 0, whole, row_blocks, s);
    launch_groups<LG, false>(p, whole, ceil_div(p.cols, (int64_t)32 * kTiles), row_blocks, s);
}

// one pass over tiles of 2^lg rows, row_blocks <= 256 of them down the matrix
void launch(int lg, const ColsP& p, bool aligned, int64_t row_blocks, hipStream_t s) {
    switch (lg) {
        case 0: launch_pass<0>(p, aligned, row_blocks, s); break;
        case 1: launch_pass<1>(p, aligned, row_blocks, s); break;
        case 2: launch_pass<2>(p, aligned, row_blocks, s); break;
        case 3: launch_pass<3>(p, aligned, row_blocks, s); break;
        case 4: launch_pass<4>(p, aligned, row_blocks, s); break;
        case 5: launch_pass<5>(p, aligned, row_blocks, s); break;
        case 6: launch_pass<6>(p, aligned, row_blocks, s); break;
        case 7: launch_pass<7>(p, aligned, row_blocks, s); break;
        default: launch_pass<8>(p, aligned, row_blocks, s); break;
    }
}

int ilog2(int64_t x) {
    int lg = 0;
    while (((int64_t)1 << lg) < x) ++lg;
    return lg;
}

bool vec_ok(const void* ptr, int64_t ld) { return reinterpret_cast<uintptr_t>(ptr) % 16 == 0 && ld % 4 == 0; }

bool valid_P(int32_t P) { return P >= 1 && P <= CQ_HADAMARD_MAX_N && (P & (P - 1)) == 0; }

}  // namespace
}  // namespace cq

using namespace cq;

extern "C" size_t cq_hadamard_cols_workspace(const cq_hadamard_cols_args* a) {
    if (a == nullptr || !valid_P(a->P) || a->P <= kTileRows || a->cols <= 0) return 0;
    return (size_t)a->P * (size_t)a->cols * sizeof(float);
}

extern "C" int cq_hadamard_cols(const cq_hadamard_cols_args* a, void* ws, size_t ws_bytes, void* stream) {
    static const char* kWho = "cq_hadamard_cols";
    CQ_REQUIRE(a != nullptr, "%s: null args", kWho);
    CQ_REQUIRE(valid_P(a->P), "%s: P = %d is not a power of two in [1, %d]", kWho, (int)a->P, CQ_HADAMARD_MAX_N);
    CQ_REQUIRE(a->n_in >= 1 && a->n_in <= a->P, "%s: n_in = %d is not in [1, P = %d]", kWho, (int)a->n_in, (int)a->P);
    CQ_REQUIRE(a->n_out >= 1 && a->n_out <= a->P, "%s: n_out = %d is not in [1, P = %d]", kWho, (int)a->n_out,
               (int)a->P);
    CQ_REQUIRE(a->cols >= 0 && a->cols <= kMaxCols, "%s: cols = %lld is not in [0, 2^35]", kWho, (long long)a->cols);
    CQ_REQUIRE(a->ldx >= a->cols && a->ldy >= a->cols,
               "%s: leading dimension smaller than the row (ldx %lld or ldy %lld < cols %lld)", kWho, (long long)a->ldx,
               (long long)a->ldy, (long long)a->cols);
    CQ_REQUIRE(reinterpret_cast<uintptr_t>(a->x) % sizeof(float) == 0, "%s: x is not aligned to its fp32 element", kWho);
    CQ_REQUIRE(reinterpret_cast<uintptr_t>(a->y) % sizeof(float) == 0, "%s: y is not aligned to its fp32 element", kWho);
    if (a->cols == 0) return CQ_OK;
    CQ_REQUIRE(a->x != nullptr && a->y != nullptr, "%s: null x or y", kWho);
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(a->x), y0 = reinterpret_cast<uintptr_t>(a->y);
    const uintptr_t x1 = x0 + (size_t)((int64_t)(a->n_in - 1) * a->ldx + a->cols) * sizeof(float);
    const uintptr_t y1 = y0 + (size_t)((int64_t)(a->n_out - 1) * a->ldy + a->cols) * sizeof(float);
    CQ_REQUIRE(x1 <= y0 || y1 <= x0, "%s: x and y overlap", kWho);
    const size_t need = cq_hadamard_cols_workspace(a);
    if (need > 0 && (ws == nullptr || ws_bytes < need))
        return set_error(CQ_EWORKSPACE, "%s: workspace of %zu bytes is smaller than the %zu needed", kWho, ws_bytes, need);
    CQ_REQUIRE(need == 0 || reinterpret_cast<uintptr_t>(ws) % sizeof(float) == 0,
               "%s: the workspace is not aligned to its fp32 element", kWho);
    const uintptr_t w0 = reinterpret_cast<uintptr_t>(ws), w1 = w0 + need;  // the bytes the two passes use
    CQ_REQUIRE(need == 0 || ((x1 <= w0 || w1 <= x0) && (y1 <= w0 || w1 <= y0)), "%s: the workspace overlaps x or y", kWho);

    hipStream_t s = as_stream(stream);
    const int lg = ilog2(a->P);
    ColsP p{};
    p.x = a->x, p.y = a->y, p.ldx = a->ldx, p.ldy = a->ldy, p.cols = a->cols;
    p.n_in = a->n_in, p.n_out = a->n_out;
    p.sign_in = a->sign_in, p.sign_out = a->sign_out;
    p.c = (float)(1.0 / std::sqrt((double)a->P));
    if (lg <= kLgTile) {
        p.base_mul = 0, p.row_stride = 1;
        launch(lg, p, vec_ok(a->x, a->ldx) && vec_ok(a->y, a->ldy), 1, s);
        return check_launch(kWho);
    }
    // pass 1: the low eight bits of every block of 256 rows that holds a row of x, unscaled, into the workspace
    const int64_t blocks = ceil_div((int64_t)a->n_in, (int64_t)kTileRows);
    ColsP p1 = p;
    p1.y = static_cast<float*>(ws), p1.ldy = a->cols;
    p1.n_out = (int)(blocks * kTileRows);
    p1.sign_out = nullptr, p1.c = 1.0f;
    p1.base_mul = kTileRows, p1.row_stride = 1;
    launch(kLgTile, p1, vec_ok(a->x, a->ldx) && vec_ok(ws, a->cols), blocks, s);
    if (const int st = check_launch(kWho)) return st;
    // pass 2: the bits above on rows 256 apart; the blocks pass 1 left out are zero and are not read
    ColsP p2 = p;
    p2.x = p1.y, p2.ldx = p1.ldy;
    p2.n_in = p1.n_out;
    p2.sign_in = nullptr;
    p2.base_mul = 1, p2.row_stride = kTileRows;
    launch(lg - kLgTile, p2, vec_ok(ws, a->cols) && vec_ok(a->y, a->ldy), kTileRows, s);
    return check_launch(kWho);
}
