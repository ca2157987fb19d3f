// Host helpers shared by the packed linear layer's entries (cq_linear.hip, cq_linear_bwd.hip,
// cq_linear_dequant.hip): the small predicates and the validation rules that are the same rule
// for every argument struct.  `who` is the entry's name, the prefix of its messages.  The templates
// take any of the argument structs: the fields they read have the same names in all of them.
#pragma once

#include <cmath>

#include "cq_common.h"
#include "cq_nf.h"

namespace cq {
namespace {

inline bool coded(int bits) { return bits == 2 || bits == 4; }
inline float kmax(int bits) { return (float)((1 << (bits - 1)) - 1); }
inline int64_t r32_of(int64_t r) { return ceil_div(r, 32) * 32; }
inline bool al16(const void* ptr, int64_t ld_elems) {
    return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0 && ld_elems % 8 == 0;
}
inline bool misaligned(const void* ptr, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(ptr) & mask) != 0; }

// one fp32 division: s / k, or s / D with the level table's denominator
inline float code_scale(float qscale, int bits, bool nf) {
    return qscale / (nf ? (bits == 4 ? kNF4D : kNF2D) : kmax(bits));
}

// the coded factors' scale / k (one fp32 division each), multiplied in fp32; 1 without factor codes
template <class A>
float factor_scale(const A* a, bool lcoded, bool rcoded) {
    float f = 1.0f;
    if (lcoded) f = a->lscale / kmax(a->l_bits);
    if (rcoded) f = lcoded ? f * (a->rscale / kmax(a->r_bits)) : a->rscale / kmax(a->r_bits);
    return f;
}

// short_status: what a workspace that is too small is reported as
inline int check_workspace(size_t need, const void* ws, size_t ws_bytes, const char* who,
                           int short_status = CQ_EWORKSPACE) {
    if (need) {
        CQ_REQUIRE(ws != nullptr && !misaligned(ws, 15), "%s: workspace must be 16-byte aligned", who);
        if (ws_bytes < need) return set_error(short_status, "%s: workspace %zu < %zu", who, ws_bytes, need);
    }
    return CQ_OK;
}

inline int validate_format(const char* who, int q_format, float qscale) {
    CQ_REQUIRE(q_format == CQ_QFMT_UNIFORM || q_format == CQ_QFMT_NF, "%s: unknown q_format %d", who, q_format);
    CQ_REQUIRE(q_format != CQ_QFMT_NF || (std::isfinite(qscale) && qscale >= 0.f),
               "%s: NF scale %g is not finite and >= 0", who, (double)qscale);
    return CQ_OK;
}

inline int validate_factor_bits(const char* who, int l_bits, int r_bits) {
    CQ_REQUIRE((coded(l_bits) || l_bits == 16) && (coded(r_bits) || r_bits == 16),
               "%s: factor bits L %d / R %d not in {2, 4, 16}", who, l_bits, r_bits);
    return CQ_OK;
}

inline int validate_rank(const char* who, int64_t r) {
    CQ_REQUIRE(r <= CQ_LINEAR_MAX_RANK, "%s: rank %lld > %d", who, (long long)r, CQ_LINEAR_MAX_RANK);
    return CQ_OK;
}

// rows of `cols` codes in the inference layout; label: "" for the layer's own codes, "L " / "R "
inline int validate_code_rows(const char* who, const char* label, int bits, const uint8_t* codes, int64_t stride,
                              int64_t cols) {
    CQ_REQUIRE(!misaligned(codes, 15) && stride % 16 == 0,
               "%s: %scodes and their row stride must be 16-byte aligned (inference layout)", who, label);
    CQ_REQUIRE(stride >= (cols * bits + 7) / 8, "%s: %scode row stride %lld < %lld bytes", who, label, (long long)stride,
               (long long)((cols * bits + 7) / 8));
    return CQ_OK;
}

// one factor's codes (name: "L" / "R"): code rows as above with one finite scale >= 0
inline int validate_factor(const char* who, const char* name, int bits, const uint8_t* codes, int64_t stride,
                           int64_t cols, float scale) {
    CQ_REQUIRE(codes != nullptr, "%s: null %s codes with %s bits = %d", who, name, name, bits);
    const char label[3] = {name[0], ' ', '\0'};
    if (int st = validate_code_rows(who, label, bits, codes, stride, cols)) return st;
    CQ_REQUIRE(std::isfinite(scale) && scale >= 0.f, "%s: %s scale %g is not finite and >= 0", who, name, (double)scale);
    return CQ_OK;
}

// the factors as they are given (fp16 pointer or codes) and the layer's own code rows, in this order
template <class A>
int validate_operands(const A* a, const char* who, bool lcoded, bool rcoded) {
    CQ_REQUIRE(a->r == 0 || ((lcoded || a->L) && (rcoded || a->R)), "%s: null L / R with r = %lld", who, (long long)a->r);
    if (lcoded)
        if (int st = validate_factor(who, "L", a->l_bits, a->L_codes, a->l_code_stride, a->r, a->lscale)) return st;
    if (rcoded)
        if (int st = validate_factor(who, "R", a->r_bits, a->R_codes, a->r_code_stride, a->n, a->rscale)) return st;
    return validate_code_rows(who, "", a->bits, a->codes, a->code_stride, a->n);
}

// fp16 operands; a pointer that the entry does not look at is passed as null
inline int validate_fp16_pointers(const char* who, const void* x, const void* L, const void* R) {
    CQ_REQUIRE(!misaligned(x, 1) && !misaligned(L, 1) && !misaligned(R, 1), "%s: misaligned fp16 pointer", who);
    return CQ_OK;
}

}  // namespace
}  // namespace cq
