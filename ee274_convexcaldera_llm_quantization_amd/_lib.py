"""ctypes binding of libcaldera_hip.so (include/caldera_hip.h) + thin torch-tensor wrappers.

PyTorch is plumbing here: it owns device memory (caching allocator workspaces), the HIP
stream (`torch.cuda.current_stream().cuda_stream`) and RNG.  Every arithmetic step of the
hot path goes through one of the C-ABI entry points below; there is no torch or CPU
fallback — a missing library or a non-HIP tensor raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import threading

import torch

from . import scratch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcaldera_hip.so")

CQ_F32, CQ_F16, CQ_BF16, CQ_F64 = 0, 1, 2, 3
EPI_LINEAR, EPI_RESID, EPI_WERR = 0, 1, 2
CQ_EINVAL, CQ_EHIP, CQ_EWORKSPACE = -1, -2, -3

c_i64, c_int, c_float, c_double, c_size, c_vp = (ctypes.c_int64, ctypes.c_int, ctypes.c_float,
                                                 ctypes.c_double, ctypes.c_size_t, ctypes.c_void_p)


class GemmArgs(ctypes.Structure):
    _fields_ = [
        ("M", c_i64), ("N", c_i64), ("K", c_i64), ("batch", c_i64),
        ("trans_a", c_int), ("trans_b", c_int),
        ("A", c_vp), ("lda", c_i64), ("stride_a", c_i64),
        ("B", c_vp), ("ldb", c_i64), ("stride_b", c_i64),
        ("C", c_vp), ("ldc", c_i64), ("stride_c", c_i64),
        ("D", c_vp), ("ldd", c_i64), ("stride_d", c_i64), ("d_f16", c_int),
        ("alpha", c_float), ("beta", c_float), ("gamma", c_float),
        ("alpha_v", c_vp), ("beta_v", c_vp), ("gamma_v", c_vp),
        ("epi", c_int),
        ("absmax_bits", c_vp),
        ("w", c_vp), ("stride_w", c_i64),
        ("err_out", c_vp),
        ("syrk", c_int),
        ("b_triu", c_int),
    ]


class X3Args(ctypes.Structure):
    _fields_ = [
        ("M", c_i64), ("N", c_i64), ("K", c_i64), ("batch", c_i64),
        ("Ah", c_vp), ("Al", c_vp), ("lda", c_i64), ("stride_a", c_i64),
        ("Bh", c_vp), ("Bl", c_vp), ("ldb", c_i64), ("stride_b", c_i64),
        ("inv_scale", c_vp),
        ("C", c_vp), ("ldc", c_i64), ("stride_c", c_i64),
        ("P", c_vp), ("ldp", c_i64), ("stride_p", c_i64),
        ("D", c_vp), ("ldd", c_i64), ("stride_d", c_i64),
        ("alpha_v", c_vp), ("beta_v", c_vp), ("gamma_v", c_vp),
        ("out_h", c_vp), ("out_l", c_vp), ("ldo", c_i64), ("stride_o", c_i64),
        ("out_scale", c_float),
        ("overflow", c_vp),
        ("tri", c_int),
        ("b_blocked", c_int),
        ("active", c_vp),
        ("a_blocked", c_int),
        ("o_blocked", c_int),
        ("sym_out", c_int),
        ("out_bound", c_vp),
        ("scale_out", c_vp),
        ("inv_out", c_vp),
        ("single", c_int),
        ("ksplit", c_int),
        ("split_ws", c_vp),
        ("b_exact", c_int),
        ("colw", c_vp),
        ("absmax_out", c_vp),
        ("Ct", c_vp),
        ("stride_ct", c_i64),
        ("stride_colw", c_i64),
    ]


class LinearArgs(ctypes.Structure):
    _fields_ = [
        ("x", c_vp), ("ldx", c_i64),
        ("tokens", c_i64), ("m", c_i64), ("n", c_i64), ("r", c_i64),
        ("bits", c_int),
        ("codes", c_vp), ("code_stride", c_i64),
        ("qscale", c_float), ("gscale", c_float),
        ("L", c_vp), ("ldl", c_i64),
        ("R", c_vp), ("ldr", c_i64),
        ("bias", c_vp),
        ("y", c_vp), ("y_dtype", c_int), ("ldy", c_i64),
    ]


class LinearPackedArgs(ctypes.Structure):
    _fields_ = LinearArgs._fields_ + [
        ("l_bits", c_int), ("r_bits", c_int),
        ("L_codes", c_vp), ("l_code_stride", c_i64),
        ("R_codes", c_vp), ("r_code_stride", c_i64),
        ("lscale", c_float), ("rscale", c_float),
    ]


class LinearBackwardArgs(ctypes.Structure):
    _fields_ = [
        ("dy", c_vp), ("lddy", c_i64),
        ("tokens", c_i64), ("m", c_i64), ("n", c_i64), ("r", c_i64),
        ("bits", c_int),
        ("codes", c_vp), ("code_stride", c_i64),
        ("qscale", c_float), ("gscale", c_float),
        ("L", c_vp), ("ldl", c_i64),
        ("R", c_vp), ("ldr", c_i64),
        ("dx", c_vp), ("dx_dtype", c_int), ("lddx", c_i64),
        ("u_out", c_vp), ("ldu", c_i64),
    ]


class LinearPackedBackwardArgs(ctypes.Structure):
    _fields_ = LinearBackwardArgs._fields_ + [
        ("l_bits", c_int), ("r_bits", c_int),
        ("L_codes", c_vp), ("l_code_stride", c_i64),
        ("R_codes", c_vp), ("r_code_stride", c_i64),
        ("lscale", c_float), ("rscale", c_float),
    ]


class LinearCodebookArgs(ctypes.Structure):
    """cq_linear_codebook_args: the packed struct, then q_format."""
    _fields_ = [("p", LinearPackedArgs), ("q_format", c_int)]


class LinearCodebookBackwardArgs(ctypes.Structure):
    _fields_ = [("p", LinearPackedBackwardArgs), ("q_format", c_int)]


class LinearGroupArgs(ctypes.Structure):
    """cq_linear_group_args: `members` points at a host array of `count` cq_linear_packed_args."""
    _fields_ = [("count", ctypes.c_int32), ("q_format", ctypes.c_int32), ("members", ctypes.POINTER(LinearPackedArgs))]


class LinearGluArgs(ctypes.Structure):
    """cq_linear_glu_args: the two members by value (their y fields unused), then the pair's own fields."""
    _fields_ = [("gate", LinearPackedArgs), ("up", LinearPackedArgs), ("q_format", c_int), ("act", c_int),
                ("h", c_vp), ("h_dtype", c_int), ("ldh", c_i64)]


class LinearDequantArgs(ctypes.Structure):
    _fields_ = [
        ("m", c_i64), ("n", c_i64), ("r", c_i64),
        ("bits", c_int), ("q_format", c_int),
        ("codes", c_vp), ("code_stride", c_i64),
        ("qscale", c_float), ("gscale", c_float),
        ("L", c_vp), ("ldl", c_i64),
        ("R", c_vp), ("ldr", c_i64),
        ("l_bits", c_int), ("r_bits", c_int),
        ("L_codes", c_vp), ("l_code_stride", c_i64),
        ("R_codes", c_vp), ("r_code_stride", c_i64),
        ("lscale", c_float), ("rscale", c_float),
        ("w", c_vp), ("w_dtype", c_int), ("ldw", c_i64),
    ]


class HadamardArgs(ctypes.Structure):
    _fields_ = [
        ("x", c_vp), ("x_dtype", c_int), ("ldx", c_i64),
        ("y", c_vp), ("y_dtype", c_int), ("ldy", c_i64),
        ("rows", c_i64), ("n_in", c_i64), ("n_out", c_i64), ("P", c_i64),
        ("bias", c_vp),
    ]


class HadamardGroupArgs(ctypes.Structure):
    """cq_hadamard_group_args: `members` points at a host array of `count` cq_hadamard_args."""
    _fields_ = [("count", ctypes.c_int32), ("members", ctypes.POINTER(HadamardArgs))]


class HadamardGluArgs(ctypes.Structure):
    _fields_ = [
        ("g", c_vp), ("g_dtype", c_int), ("ldg", c_i64),
        ("u", c_vp), ("u_dtype", c_int), ("ldu", c_i64),
        ("h", c_vp), ("h_dtype", c_int), ("ldh", c_i64),
        ("rows", c_i64), ("n_in", c_i64), ("n_out", c_i64), ("P", c_i64),
        ("bias_g", c_vp), ("bias_u", c_vp),
        ("act", c_int),
    ]


class HadamardSignedArgs(ctypes.Structure):
    """cq_hadamard_signed_args: cq_hadamard_args and the two int8 sign vectors (device pointers or NULL)."""
    _fields_ = [("a", HadamardArgs), ("sign_in", c_vp), ("sign_out", c_vp)]


class HadamardSignedGroupArgs(ctypes.Structure):
    """cq_hadamard_signed_group_args: `members` points at a host array of `count` cq_hadamard_signed_args."""
    _fields_ = [("count", ctypes.c_int32), ("members", ctypes.POINTER(HadamardSignedArgs))]


class HadamardSignedGluArgs(ctypes.Structure):
    """cq_hadamard_signed_glu_args: cq_hadamard_glu_args and the output signs of the gate and up transforms."""
    _fields_ = [("a", HadamardGluArgs), ("sign_g", c_vp), ("sign_u", c_vp)]


_SIGS = {
    "cq_abi_version": (c_int, []),
    "cq_last_error": (ctypes.c_char_p, []),
    "cq_rms_scale_workspace": (c_size, [c_i64, c_i64]),
    "cq_rms_scale": (c_int, [c_int, c_vp, c_i64, c_i64, c_int, c_vp, c_vp, c_vp, c_size, c_vp]),
    "cq_quantize_workspace": (c_size, [c_i64, c_i64, c_i64]),
    "cq_quantize_uniform": (c_int, [c_vp, c_i64, c_i64, c_i64, c_int, c_float, c_vp, c_vp, c_vp,
                                    c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_size, c_vp]),
    "cq_quantize_uniform_known_max": (c_int, [c_vp, c_i64, c_i64, c_int, c_float, c_vp, c_vp, c_vp,
                                              c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_size, c_vp]),
    "cq_unpack_codes": (c_int, [c_vp, c_i64, c_i64, c_int, c_vp, c_vp]),
    "cq_quantize_nf_workspace": (c_size, [c_i64, c_i64, c_i64]),
    "cq_quantize_nf": (c_int, [c_vp, c_i64, c_i64, c_i64, c_int, c_float, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64,
                               c_vp, c_vp, c_size, c_vp]),
    "cq_dequant_nf": (c_int, [c_vp, c_vp, c_i64, c_i64, c_int, c_vp, c_vp]),
    "cq_quantize_nf_std_workspace": (c_size, [c_i64, c_i64, c_i64]),
    "cq_quantize_nf_std": (c_int, [c_vp, c_i64, c_i64, c_i64, c_int, c_float, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64,
                                   c_i64, c_vp, c_vp, c_size, c_vp]),
    "cq_dequant_nf_std": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_vp, c_vp]),
    "cq_bbint_workspace": (c_size, [c_i64, c_i64, c_i64]),
    "cq_bbint_stats": (c_int, [c_vp, c_i64, c_i64, c_i64, c_int, c_float, c_vp, c_vp, c_vp, c_vp, c_size, c_vp]),
    "cq_bbint_emit": (c_int, [c_vp, c_i64, c_i64, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64,
                              c_i64, c_vp, c_vp, c_size, c_vp]),
    "cq_dequant_bbint": (c_int, [c_vp, c_int, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "cq_dequant_uniform": (c_int, [c_vp, c_int, c_vp, c_i64, c_i64, c_int, c_vp, c_vp]),
    "cq_build_residual": (c_int, [c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp,
                                  c_vp, c_vp]),
    "cq_gemm_workspace": (c_size, [ctypes.POINTER(GemmArgs)]),
    "cq_gemm_f32": (c_int, [ctypes.POINTER(GemmArgs), c_vp, c_size, c_vp]),
    "cq_gram_f64_workspace": (c_size, [c_i64, c_i64, c_i64, c_i64]),
    "cq_gram_f64": (c_int, [c_i64, c_i64, c_i64, c_i64, c_vp, c_int, c_i64, c_i64, c_vp, c_int, c_i64,
                            c_i64, c_vp, c_vp, c_size, c_vp]),
    "cq_spd_whiten": (c_int, [c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "cq_spd_whiten_rcond": (c_int, [c_vp, c_i64, c_i64, c_double, c_vp, c_vp, c_vp, c_vp]),
    "cq_jacobi_workspace": (c_size, [c_i64, c_i64]),
    "cq_jacobi_eigh": (c_int, [c_vp, c_i64, c_i64, c_int, c_double, c_vp, c_vp, c_vp, c_vp, c_vp,
                               c_size, c_vp]),
    "cq_jacobi_staged_workspace": (c_size, [c_i64, c_i64]),
    "cq_jacobi_eigh_staged": (c_int, [c_vp, c_i64, c_i64, c_int, c_int, c_double, c_int, c_vp, c_vp, c_vp, c_vp,
                                      c_vp, c_vp, c_size, c_vp]),
    "cq_extreme_eigs": (c_int, [c_vp, c_i64, c_i64, c_int, c_vp, c_vp]),
    "cq_ritz_workspace": (c_size, [c_i64, c_i64, c_i64]),
    "cq_ritz_residual": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_size,
                                 c_vp]),
    "cq_weighted_sqsum": (c_int, [c_int, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_vp, c_size, c_vp]),
    "cq_scale_rc": (c_int, [c_vp, c_i64, c_i64, c_int, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp,
                            c_i64, c_vp, c_i64, c_vp]),
    "cq_sym_split_f16": (c_int, [c_vp, c_i64, c_i64, c_int, c_int, c_float, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "cq_transpose_split": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_float, c_vp, c_int, c_vp]),
    "cq_gemm_triu_split": (c_int, [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_float, c_vp]),
    "cq_pow2_scale": (c_int, [c_vp, c_i64, c_i64, c_int, c_vp, c_vp]),
    "cq_split_f16": (c_int, [c_vp, c_i64, c_i64, c_vp, c_float, c_vp, c_vp, c_i64, c_vp]),
    "cq_gemm_x3": (c_int, [ctypes.POINTER(X3Args), c_vp]),
    "cq_q_update_workspace": (c_size, [c_i64, c_i64, c_i64, c_int]),
    "cq_q_update_list_geometry": (c_int, [c_i64, c_i64, c_i64, c_vp, c_vp, c_vp]),
    "cq_absmax": (c_int, [c_int, c_vp, c_i64, c_i64, c_vp, c_vp]),
    "cq_residual_split_workspace": (c_size, [c_i64, c_i64, c_i64]),
    "cq_residual_split": (c_int, [c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_float, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp,
                                  c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_float, c_vp, c_i64, c_vp, c_vp, c_vp,
                                  c_size, c_vp]),
    "cq_sgram_count": (c_int, [c_vp, c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp,
                               c_vp, c_i64, c_vp, c_vp, c_vp]),
    "cq_sgram_fill": (c_int, [c_vp, c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp]),
    "cq_sgram_rows": (c_int, [c_i64]),
    "cq_pow2_from_absmax": (c_int, [c_vp, c_i64, c_int, c_vp]),
    "cq_sgram_split": (c_i64, [c_i64, c_i64]),
    "cq_sgram_spmm": (c_int, [c_int, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64,
                              c_i64, c_vp, c_vp]),
    "cq_sgram_combine": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_float, c_vp, c_vp, c_vp, c_vp, c_vp,
                                 c_vp]),
    "cq_codes_transpose": (c_int, [c_vp, c_int, c_i64, c_i64, c_i64, c_vp, c_vp]),
    "cq_codes_matmul": (c_int, [c_vp, c_int, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_i64,
                                c_vp, c_i64, c_i64, c_int, c_vp]),
    "cq_codes_ysq_corr": (c_int, [c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp]),
    "cq_transpose_f16": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp]),
    "cq_q_update_x3": (c_int, [c_int, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
                               c_float, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_size, c_vp]),
    "cq_ritz_product_error": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_size, c_vp]),
    "cq_batched_dot": (c_int, [c_int, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_size, c_vp]),
    "cq_act_sqsum_workspace": (c_size, [c_i64, c_i64]),
    "cq_act_sqsum_cols": (c_int, [c_int, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_double, c_vp, c_size, c_vp]),
    "cq_act_sqsum_rows": (c_int, [c_int, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_double, c_vp]),
    "cq_linear_workspace": (c_size, [ctypes.POINTER(LinearArgs)]),
    "cq_linear_forward": (c_int, [ctypes.POINTER(LinearArgs), c_vp, c_size, c_vp]),
    "cq_linear_packed_workspace": (c_size, [ctypes.POINTER(LinearPackedArgs)]),
    "cq_linear_packed_forward": (c_int, [ctypes.POINTER(LinearPackedArgs), c_vp, c_size, c_vp]),
    "cq_linear_backward_workspace": (c_size, [ctypes.POINTER(LinearBackwardArgs)]),
    "cq_linear_backward_input": (c_int, [ctypes.POINTER(LinearBackwardArgs), c_vp, c_size, c_vp]),
    "cq_linear_packed_backward_workspace": (c_size, [ctypes.POINTER(LinearPackedBackwardArgs)]),
    "cq_linear_packed_backward_input": (c_int, [ctypes.POINTER(LinearPackedBackwardArgs), c_vp, c_size, c_vp]),
    "cq_linear_codebook_workspace": (c_size, [ctypes.POINTER(LinearCodebookArgs)]),
    "cq_linear_codebook_forward": (c_int, [ctypes.POINTER(LinearCodebookArgs), c_vp, c_size, c_vp]),
    "cq_linear_codebook_backward_workspace": (c_size, [ctypes.POINTER(LinearCodebookBackwardArgs)]),
    "cq_linear_codebook_backward_input": (c_int, [ctypes.POINTER(LinearCodebookBackwardArgs), c_vp, c_size, c_vp]),
    "cq_linear_group_workspace": (c_size, [ctypes.POINTER(LinearGroupArgs)]),
    "cq_linear_group_forward": (c_int, [ctypes.POINTER(LinearGroupArgs), c_vp, c_size, c_vp]),
    "cq_linear_glu_workspace": (c_size, [ctypes.POINTER(LinearGluArgs)]),
    "cq_linear_glu_forward": (c_int, [ctypes.POINTER(LinearGluArgs), c_vp, c_size, c_vp]),
    "cq_linear_dequant": (c_int, [ctypes.POINTER(LinearDequantArgs), c_vp]),
    "cq_hadamard_rows": (c_int, [ctypes.POINTER(HadamardArgs), c_vp]),
    "cq_hadamard_group_rows": (c_int, [ctypes.POINTER(HadamardGroupArgs), c_vp]),
    "cq_hadamard_glu_rows": (c_int, [ctypes.POINTER(HadamardGluArgs), c_vp]),
    "cq_hadamard_signed_rows": (c_int, [ctypes.POINTER(HadamardSignedArgs), c_vp]),
    "cq_hadamard_signed_group_rows": (c_int, [ctypes.POINTER(HadamardSignedGroupArgs), c_vp]),
    "cq_hadamard_signed_glu_rows": (c_int, [ctypes.POINTER(HadamardSignedGluArgs), c_vp]),
    # masked entries: the unmasked signature with `active` ([batch] int32 or NULL) added
    "cq_gemm_x3_skip": (c_int, [ctypes.POINTER(X3Args), c_vp]),
    "cq_gram_f64_masked": (c_int, [c_i64, c_i64, c_i64, c_i64, c_vp, c_int, c_i64, c_i64, c_vp, c_int, c_i64,
                                   c_i64, c_vp, c_vp, c_vp, c_size, c_vp]),
    "cq_spd_whiten_masked": (c_int, [c_vp, c_i64, c_i64, c_double, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "cq_jacobi_eigh_masked": (c_int, [c_vp, c_i64, c_i64, c_int, c_double, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                      c_size, c_vp]),
    "cq_jacobi_eigh_staged_masked": (c_int, [c_vp, c_i64, c_i64, c_int, c_int, c_double, c_int, c_vp, c_vp, c_vp,
                                             c_vp, c_vp, c_vp, c_vp, c_size, c_vp]),
    "cq_extreme_eigs_masked": (c_int, [c_vp, c_i64, c_i64, c_int, c_vp, c_vp, c_vp]),
    "cq_ritz_residual_masked": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_size,
                                        c_vp]),
    "cq_ritz_product_error_masked": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp,
                                             c_size, c_vp]),
    "cq_gemm_f32_masked": (c_int, [ctypes.POINTER(GemmArgs), c_vp, c_vp, c_size, c_vp]),
    "cq_gemm_triu_split_masked": (c_int, [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_float, c_vp, c_vp]),
    "cq_transpose_split_masked": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_float, c_vp, c_int, c_vp,
                                          c_vp]),
}
EXPORTS = tuple(_SIGS)
ABI_VERSION = 5  # include/caldera_hip.h CQ_ABI_VERSION

_lib = None


def load(path: str = LIB_PATH):
    """Load libcaldera_hip.so and declare every export (no device calls)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; "
                           f"g.build()'` (hipcc --offload-arch=gfx950)")
    if path == LIB_PATH and not os.environ.get("CQ_ALLOW_STALE_LIB"):
        from . import build as _build
        if _build.needs_build():  # never run kernels older than the sources in the tree
            raise RuntimeError(f"{path} is stale (built from other sources than csrc/ now holds, or "
                               f"unstamped): rebuild with `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(path)
    # any build (also another one for an A/B timing, tools/probes/build_rev.sh) must speak this
    # ABI: the declarations below are this ABI's signatures, and calling an export of another
    # layout through them is undefined behaviour on the GPU rather than a clean error
    abi = getattr(lib, "cq_abi_version", None)
    if abi is None:
        raise RuntimeError(f"{path} does not export cq_abi_version")
    abi.restype, abi.argtypes = c_int, []
    if abi() != ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version {abi()} != {ABI_VERSION} (include/caldera_hip.h); rebuild it "
                           f"from these sources")
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise RuntimeError(f"{path} does not export {name}")
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


class CalderaHipError(RuntimeError):
    pass


_SYNC_CHECK = bool(os.environ.get("CQ_SYNC_CHECK"))


def _check(st: int, what: str):
    if _SYNC_CHECK and st == 0:  # debugging: attribute an asynchronous fault to its launch
        import sys
        import traceback
        fr = traceback.extract_stack(limit=4)
        print(f"[cq] {what} <- {' <- '.join(f'{f.name}:{f.lineno}' for f in reversed(fr[:-1]))}",
              file=sys.stderr, flush=True)
        torch.cuda.synchronize()
    if st != 0:
        msg = load().cq_last_error().decode(errors="replace")
        if st == CQ_EINVAL:
            if "Bit-width not supported" in msg:
                raise AssertionError("Bit-width not supported!")
            raise ValueError(f"{what}: {msg}")
        raise CalderaHipError(f"{what}: status {st}: {msg}")


def _p(t: torch.Tensor | None):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _act(active: torch.Tensor | None, B: int):
    """Pointer of a per-matrix mask (B,) int32 on the device (1 = live, 0 = left out), or NULL."""
    if active is None:
        return None
    assert active.is_cuda and active.dtype == torch.int32 and active.is_contiguous() and active.numel() == B, \
        "active must be a contiguous int32 device tensor of one entry per matrix"
    return ctypes.c_void_p(active.data_ptr())


def _stream(dev: torch.device):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _require_hip(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("caldera-mi355x kernels need HIP device tensors (no CPU fallback)")


def _wst(w: torch.Tensor | None, B: int) -> int:
    """Batch stride of a column / error weight vector (ABI 5): (n,) is shared by the batch
    (stride 0); (B, n) holds one vector per matrix (distinct diagonal Hessians, stride n)."""
    if w is None or w.dim() == 1:
        return 0
    assert w.dim() == 2 and w.shape[0] == B and w.is_contiguous(), (tuple(w.shape), B)
    return w.shape[1] if B > 1 else 0


def workspace(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


# ---------------------------------------------------------------------------- wrappers
def rms_scale(W: torch.Tensor, do_scale: bool):
    """W (B, m, n) fp16/fp32 -> (gs (B,) fp32, Ws same dtype).  alg.py:38-42."""
    _require_hip(W)
    W = W.contiguous()
    dt = {torch.float16: CQ_F16, torch.float32: CQ_F32}[W.dtype]
    B = W.shape[0]
    numel = W[0].numel()
    gs = torch.empty(B, dtype=torch.float32, device=W.device)
    Ws = torch.empty_like(W)
    lib = load()
    ws = workspace(lib.cq_rms_scale_workspace(B, numel), W.device)
    _check(lib.cq_rms_scale(dt, _p(W), B, numel, int(bool(do_scale)), _p(gs), _p(Ws), _p(ws), ws.numel(),
                            _stream(W.device)), "cq_rms_scale")
    return gs, Ws


def weighted_sqsum(x: torch.Tensor, w: torch.Tensor | None, ncols: int) -> torch.Tensor:
    _require_hip(x, w)
    dt = {torch.float16: CQ_F16, torch.float32: CQ_F32}[x.dtype]
    B = x.shape[0]
    numel = x[0].numel()
    out = torch.empty(B, dtype=torch.float64, device=x.device)
    lib = load()
    ws = workspace(lib.cq_rms_scale_workspace(B, numel), x.device)
    _check(lib.cq_weighted_sqsum(dt, _p(x), B, numel, _p(w), ncols, _wst(w, B), _p(out), _p(ws), ws.numel(),
                                 _stream(x.device)), "cq_weighted_sqsum")
    return out


def batched_dot(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """out[b] = <x[b], y[b]> in fp64 (x, y (B, ...) fp32 or fp64, same shape, contiguous)."""
    _require_hip(x, y)
    assert x.shape == y.shape and x.dtype == y.dtype and x.is_contiguous() and y.is_contiguous()
    dt = {torch.float32: CQ_F32, torch.float64: CQ_F64}[x.dtype]
    B = x.shape[0]
    numel = x[0].numel()
    out = torch.empty(B, dtype=torch.float64, device=x.device)
    lib = load()
    ws = workspace(lib.cq_rms_scale_workspace(B, numel), x.device)
    _check(lib.cq_batched_dot(dt, _p(x), _p(y), B, numel, _p(out), _p(ws), ws.numel(), _stream(x.device)),
           "cq_batched_dot")
    return out


def code_dtype(bits: int):
    return torch.int8 if bits <= 8 else torch.int16


def quantize_uniform(x: torch.Tensor, block_size: int, bits: int, eps: float = 1e-8, *,
                     codes=True, packed=False, deq=True, err_w=None, err_ncols=1, want_err=False):
    """x (B, numel) fp32 contiguous.  quantization.py:244-269 / :290-307 (uniform)."""
    _require_hip(x, err_w)
    assert x.dtype == torch.float32 and x.is_contiguous()
    B, numel = x.shape
    dev = x.device
    out = {}
    out["codes"] = torch.empty((B, numel), dtype=code_dtype(bits), device=dev) if codes else None
    out["packed"] = (torch.empty((B, numel * bits // 8), dtype=torch.uint8, device=dev)
                     if packed and bits <= 4 else None)
    out["deq"] = torch.empty((B, numel), dtype=torch.float32, device=dev) if deq else None
    out["scale"] = torch.empty((B, numel // block_size), dtype=torch.float32, device=dev)
    out["err"] = torch.empty(B, dtype=torch.float64, device=dev) if (want_err or err_w is not None) else None
    lib = load()
    ws = workspace(lib.cq_quantize_workspace(B, numel, block_size), dev)
    _check(lib.cq_quantize_uniform(_p(x), B, numel, block_size, bits, eps, _p(out["codes"]),
                                   _p(out["packed"]), _p(out["deq"]), _p(out["scale"]), _p(err_w),
                                   err_ncols, _wst(err_w, B), _p(out["err"]), _p(ws), ws.numel(), _stream(dev)),
           "cq_quantize_uniform")
    return out


def quantize_known_max(x, absmax_bits, bits, eps=1e-8, *, codes=None, packed=None, deq=None,
                       scale=None, err_w=None, err_ncols=1, err_out=None):
    _require_hip(x)
    B = x.shape[0]
    numel = x[0].numel()
    lib = load()
    ws = workspace(lib.cq_quantize_workspace(B, numel, numel), x.device)
    _check(lib.cq_quantize_uniform_known_max(_p(x), B, numel, bits, eps, _p(absmax_bits), _p(codes),
                                             _p(packed), _p(deq), _p(scale), _p(err_w), err_ncols, _wst(err_w, B),
                                             _p(err_out), _p(ws), ws.numel(), _stream(x.device)),
           "cq_quantize_uniform_known_max")


def dequantize_uniform(codes: torch.Tensor, scale: torch.Tensor, bits: int, packed: bool = False,
                       numel: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """(float(c)/k) * scale per block; codes (..., ) int8/int16 or packed uint8; scale (nblocks,)."""
    _require_hip(codes, scale, out)
    total = numel if numel is not None else codes.numel()
    nb = scale.numel()
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=codes.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == total
    _check(load().cq_dequant_uniform(_p(codes), int(packed), _p(scale), total, total // nb, bits, _p(out),
                                     _stream(codes.device)), "cq_dequant_uniform")
    return out


def unpack_codes(packed: torch.Tensor, numel: int, bits: int, out: torch.Tensor | None = None) -> torch.Tensor:
    _require_hip(packed, out)
    B = packed.shape[0]
    codes = torch.empty((B, numel), dtype=torch.int8, device=packed.device) if out is None else out
    assert codes.shape == (B, numel) and codes.dtype == torch.int8 and codes.is_contiguous()
    _check(load().cq_unpack_codes(_p(packed), B, numel, bits, _p(codes), _stream(packed.device)),
           "cq_unpack_codes")
    return codes


def quantize_nf(x: torch.Tensor, block_size: int, bits: int, eps: float = 1e-8, *, idx=True, deq=True,
                err_w=None, err_ncols=1, err_out=None):
    """NF4 / NF2 (quantization.py:39-91, :270-279).  x (B, numel) fp32 contiguous ->
    dict(idx (B, numel) uint8, deq (B, numel) fp32, scale (B, numel // block_size) fp32)."""
    _require_hip(x, err_w, err_out)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    B, numel = x.shape
    dev = x.device
    out = {"idx": torch.empty((B, numel), dtype=torch.uint8, device=dev) if idx else None,
           "deq": torch.empty((B, numel), dtype=torch.float32, device=dev) if deq else None,
           "scale": torch.empty((B, numel // block_size), dtype=torch.float32, device=dev)}
    lib = load()
    ws = workspace(lib.cq_quantize_nf_workspace(B, numel, block_size), dev)
    _check(lib.cq_quantize_nf(_p(x), B, numel, block_size, bits, eps, _p(out["idx"]), _p(out["deq"]),
                              _p(out["scale"]), _p(err_w), err_ncols, _wst(err_w, B), _p(err_out), _p(ws), ws.numel(),
                              _stream(dev)), "cq_quantize_nf")
    return out


def dequantize_nf(idx: torch.Tensor, scale: torch.Tensor, bits: int) -> torch.Tensor:
    """level[idx] * scale[blk] (quantization.py:87-91); idx uint8, scale (nblocks,) fp32."""
    _require_hip(idx, scale)
    total = idx.numel()
    out = torch.empty(total, dtype=torch.float32, device=idx.device)
    _check(load().cq_dequant_nf(_p(idx), _p(scale), total, total // scale.numel(), bits, _p(out),
                                _stream(idx.device)), "cq_dequant_nf")
    return out


def quantize_nf_std(x: torch.Tensor, block_size: int, bits: int, eps: float = 1e-8, *, idx=True, deq=True,
                    err_w=None, err_ncols=None, err_out=None):
    """Standardised NF4 / NF2 (quantization_stable_nf4.py:187-200).  x (B, numel) fp32 contiguous ->
    dict(idx (B, numel) uint8, deq (B, numel) fp32, mean / std (B, numel // block_size) fp32).
    block_size = 1 (no unbiased std) raises ValueError."""
    _require_hip(x, err_w, err_out)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    B, numel = x.shape
    dev = x.device
    block_size = int(block_size)
    nblk = numel // block_size if block_size > 0 else 0
    out = {"idx": torch.empty((B, numel), dtype=torch.uint8, device=dev) if idx else None,
           "deq": torch.empty((B, numel), dtype=torch.float32, device=dev) if deq else None,
           "mean": torch.empty((B, nblk), dtype=torch.float32, device=dev),
           "std": torch.empty((B, nblk), dtype=torch.float32, device=dev)}
    lib = load()
    ws = workspace(lib.cq_quantize_nf_std_workspace(B, numel, block_size), dev)
    _check(lib.cq_quantize_nf_std(_p(x), B, numel, block_size, bits, eps, _p(out["idx"]), _p(out["deq"]),
                                  _p(out["mean"]), _p(out["std"]), _p(err_w), err_ncols or 0, _wst(err_w, B),
                                  _p(err_out), _p(ws), ws.numel(), _stream(dev)), "cq_quantize_nf_std")
    return out


def dequantize_nf_std(idx: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, bits: int) -> torch.Tensor:
    """level[idx] * std[blk] + mean[blk] (quantization_stable_nf4.py:221-224); idx uint8, mean / std
    (nblocks,) fp32."""
    _require_hip(idx, mean, std)
    assert mean.numel() == std.numel()
    total = idx.numel()
    out = torch.empty(total, dtype=torch.float32, device=idx.device)
    _check(load().cq_dequant_nf_std(_p(idx), _p(mean), _p(std), total, total // mean.numel(), bits, _p(out),
                                    _stream(idx.device)), "cq_dequant_nf_std")
    return out


def quantize_bbint(x: torch.Tensor, block_size: int, bits: int, eps: float = 1e-8, *, packed=True, deq=True,
                   outliers=True, err_w=None, err_ncols=1, err_out=None):
    """bbint4 / bbint2 (quantization.py:107-243).  x (B, numel) fp32 contiguous -> dict(packed
    (B, numel*bits/8) uint8, deq (B, numel), bmin / bscale (B, nblk), n_out [B] (host ints),
    vals (sum n_out,) fp32, idx (sum n_out, 2) int64 — matrix b's rows follow matrix b-1's).
    One host synchronisation (the outlier count sizes the list)."""
    _require_hip(x, err_w, err_out)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    B, numel = x.shape
    dev = x.device
    nblk = numel // block_size
    lib = load()
    nws = lib.cq_bbint_workspace(B, numel, block_size)
    if nws == 0:
        raise ValueError(f"bbint: numel {numel} is not divisible by block size {block_size}")
    ws = workspace(nws, dev)
    bmin = torch.empty((B, nblk), dtype=torch.float32, device=dev)
    bscale = torch.empty((B, nblk), dtype=torch.float32, device=dev)
    n_out = torch.empty(B, dtype=torch.int64, device=dev)
    st = _stream(dev)
    _check(lib.cq_bbint_stats(_p(x), B, numel, block_size, bits, eps, _p(bmin), _p(bscale), _p(n_out), _p(ws),
                              ws.numel(), st), "cq_bbint_stats")
    counts = [int(v) for v in n_out.tolist()] if outliers else [0] * B
    tot = sum(counts)
    vals = torch.empty(tot, dtype=torch.float32, device=dev) if outliers else None
    oidx = torch.empty((tot, 2), dtype=torch.int64, device=dev) if outliers else None
    pk = torch.empty((B, numel * bits // 8), dtype=torch.uint8, device=dev) if packed else None
    dq = torch.empty((B, numel), dtype=torch.float32, device=dev) if deq else None
    _check(lib.cq_bbint_emit(_p(x), B, numel, block_size, bits, _p(bmin), _p(bscale), _p(pk), _p(dq),
                             _p(vals) if tot else None, _p(oidx) if tot else None, _p(err_w), err_ncols,
                             _wst(err_w, B), _p(err_out), _p(ws), ws.numel(), st), "cq_bbint_emit")
    return {"packed": pk, "deq": dq, "bmin": bmin, "bscale": bscale, "n_out": counts, "vals": vals, "idx": oidx}


def dequantize_bbint(packed: torch.Tensor, bits: int, bmin: torch.Tensor, bscale: torch.Tensor,
                     vals: torch.Tensor | None, idx: torch.Tensor | None, block_size: int) -> torch.Tensor:
    """u * scale + min per block, outliers scattered back (quantization.py:157-172, :224-243)."""
    _require_hip(packed, bmin, bscale, vals, idx)
    total = packed.numel() * 8 // bits
    out = torch.empty(total, dtype=torch.float32, device=packed.device)
    k = 0 if vals is None else vals.numel()
    _check(load().cq_dequant_bbint(_p(packed), bits, _p(bmin), _p(bscale), total, block_size,
                                   _p(vals) if k else None, _p(idx.contiguous()) if k else None, k, _p(out),
                                   _stream(packed.device)), "cq_dequant_bbint")
    return out


def build_residual(Ws, qcodes, qscale, bits, ycol, Y=None, res=None):
    """Y = (Ws - deq(Q)) * ycol[col];  res = Ws - deq(Q).  alg.py:124 + :211 (diagonal H)."""
    _require_hip(Ws, qcodes, qscale, ycol, Y, res)
    dt = {torch.float16: CQ_F16, torch.float32: CQ_F32}[Ws.dtype]
    B, m, n = Ws.shape
    _check(load().cq_build_residual(dt, _p(Ws), _p(qcodes), _p(qscale), bits, _p(ycol), _wst(ycol, B), B, m, n,
                                    _p(Y), _p(res), _stream(Ws.device)), "cq_build_residual")


def _mat(t: torch.Tensor):
    """(tensor (B, r, c) or (r, c) with unit column stride) -> (ptr, ld, batch_stride)."""
    if t.dim() == 2:
        assert t.stride(1) == 1
        return t, t.stride(0), 0
    assert t.dim() == 3 and t.stride(2) == 1, "matrices must have unit column stride"
    return t, t.stride(1), (t.stride(0) if t.shape[0] > 1 else 0)


def gemm(A, B, *, ta=False, tb=False, C=None, alpha=1.0, beta=0.0, D=None, gamma=0.0,
         epi=EPI_LINEAR, absmax=None, w=None, err_out=None, alpha_v=None, beta_v=None,
         gamma_v=None, batch=None, syrk=False, b_triu=False, active=None):
    """Batched C = alpha op(A) op(B) + beta C + gamma D (or RESID / WERR epilogues).
    b_triu: B (not transposed) is upper triangular -- its zero K slices are skipped.
    active (batch,) int32 (LINEAR epilogue, no syrk): matrices with active[b] == 0 are left out
    (C[b] not written); None = all."""
    _require_hip(A, B, C, D, w)
    A_, lda, sa = _mat(A)
    B_, ldb, sb = _mat(B)
    M = A.shape[-1] if ta else A.shape[-2]
    K = A.shape[-2] if ta else A.shape[-1]
    N = B.shape[-2] if tb else B.shape[-1]
    Kb = B.shape[-1] if tb else B.shape[-2]
    assert K == Kb, f"gemm: inner dims {K} vs {Kb}"
    if batch is None:
        batch = max(t.shape[0] if t is not None and t.dim() == 3 else 1 for t in (A, B, C, D))
    g = GemmArgs()
    g.M, g.N, g.K, g.batch = M, N, K, batch
    g.trans_a, g.trans_b = int(ta), int(tb)
    g.A, g.lda, g.stride_a = A_.data_ptr(), lda, sa
    g.B, g.ldb, g.stride_b = B_.data_ptr(), ldb, sb
    if C is not None:
        C_, ldc, sc = _mat(C)
        assert C.shape[-2] == M and C.shape[-1] == N
        g.C, g.ldc, g.stride_c = C_.data_ptr(), ldc, sc
    if D is not None:
        D_, ldd, sd = _mat(D)
        assert D.shape[-2] == M and D.shape[-1] == N, f"D shape {tuple(D.shape)} vs {(M, N)}"
        g.D, g.ldd, g.stride_d, g.d_f16 = D_.data_ptr(), ldd, sd, int(D.dtype == torch.float16)
        if D.dtype not in (torch.float16, torch.float32):
            raise TypeError("D must be fp16/fp32")
    g.alpha, g.beta, g.gamma = alpha, beta, gamma
    g.alpha_v = alpha_v.data_ptr() if alpha_v is not None else None
    g.beta_v = beta_v.data_ptr() if beta_v is not None else None
    g.gamma_v = gamma_v.data_ptr() if gamma_v is not None else None
    g.epi = epi
    g.absmax_bits = absmax.data_ptr() if absmax is not None else None
    if w is not None:
        g.w = w.data_ptr()
        g.stride_w = w.shape[-1] if (w.dim() == 2 and w.shape[0] > 1) else 0
    g.err_out = err_out.data_ptr() if err_out is not None else None
    g.syrk = int(bool(syrk))
    g.b_triu = int(bool(b_triu))
    lib = load()
    dev = A.device
    nws = lib.cq_gemm_workspace(ctypes.byref(g))
    ws = workspace(nws, dev) if nws else None
    if active is not None:
        _check(lib.cq_gemm_f32_masked(ctypes.byref(g), _act(active, batch), _p(ws), 0 if ws is None else ws.numel(),
                                      _stream(dev)), "cq_gemm_f32_masked")
        return C
    _check(lib.cq_gemm_f32(ctypes.byref(g), _p(ws), 0 if ws is None else ws.numel(), _stream(dev)),
           "cq_gemm_f32")
    return C


def gram_f64(A, B, *, ta=False, tb=False, out=None, active=None):
    """C = op(A)^T op(B) style Gram: A is K x M (or M x K if ta), B is K x N (or N x K if tb).
    active (batch,) int32: matrices with active[b] == 0 are left out (out[b] not written)."""
    _require_hip(A, B)
    A_, lda, sa = _mat(A)
    B_, ldb, sb = _mat(B)
    K = A.shape[-1] if ta else A.shape[-2]
    M = A.shape[-2] if ta else A.shape[-1]
    N = B.shape[-2] if tb else B.shape[-1]
    batch = max(t.shape[0] if t.dim() == 3 else 1 for t in (A, B))
    if out is None:
        out = torch.empty((batch, M, N), dtype=torch.float64, device=A.device)
    lib = load()
    ws = workspace(lib.cq_gram_f64_workspace(M, N, K, batch), A.device)
    if active is not None:
        _check(lib.cq_gram_f64_masked(M, N, K, batch, _p(A_), int(ta), lda, sa, _p(B_), int(tb), ldb, sb, _p(out),
                                      _act(active, batch), _p(ws), ws.numel(), _stream(A.device)), "cq_gram_f64_masked")
        return out
    _check(lib.cq_gram_f64(M, N, K, batch, _p(A_), int(ta), lda, sa, _p(B_), int(tb), ldb, sb, _p(out),
                           _p(ws), ws.numel(), _stream(A.device)), "cq_gram_f64")
    return out


def spd_whiten(S: torch.Tensor, rcond2: float = 1e-30, active=None):
    """S (B, p, p) fp64 SPD (overwritten) -> (Wt32, Wt64, info) with Wt^T S Wt = I on the
    independent columns; pivots <= rcond2 * max diag are dropped (info = their count).
    Wt64 is S itself: the kernel leaves the fp64 Wt there (its Wt64 argument is scratch)."""
    _require_hip(S)
    B, p, _ = S.shape
    Wt32 = torch.empty((B, p, p), dtype=torch.float32, device=S.device)
    scr = torch.empty((B, p, p), dtype=torch.float64, device=S.device)
    info = torch.empty(B, dtype=torch.int32, device=S.device)
    if active is not None:  # masked-out matrices: S, Wt32 and info are left as they are
        _check(load().cq_spd_whiten_masked(_p(S), p, B, float(rcond2), _p(Wt32), _p(scr), _p(info), _act(active, B),
                                           _stream(S.device)), "cq_spd_whiten_masked")
        return Wt32, S, info
    _check(load().cq_spd_whiten_rcond(_p(S), p, B, float(rcond2), _p(Wt32), _p(scr), _p(info),
                                      _stream(S.device)), "cq_spd_whiten_rcond")
    return Wt32, S, info


def jacobi_eigh(A: torch.Tensor, max_sweeps: int = 30, tol: float = 1e-13, want64=False, want_vectors=True,
                active=None):
    """A (B, p, p) fp64 symmetric (overwritten) -> (evals desc (B,p) fp64, V32, V64, sweeps);
    want_vectors=False: eigenvalues only (V32 = V64 = None; the p <= 192 register kernel then
    skips its eigenvector rotations)."""
    _require_hip(A)
    B, p, _ = A.shape
    ev = torch.empty((B, p), dtype=torch.float64, device=A.device)
    V32 = torch.empty((B, p, p), dtype=torch.float32, device=A.device) if want_vectors else None
    want64 = want64 and want_vectors
    V64 = torch.empty((B, p, p), dtype=torch.float64, device=A.device) if want64 else None
    sw = torch.empty(B, dtype=torch.int32, device=A.device)
    lib = load()
    ws = workspace(lib.cq_jacobi_workspace(p, B), A.device)
    if active is not None:  # masked-out matrices: no values, no vectors, sweeps 0
        _check(lib.cq_jacobi_eigh_masked(_p(A), p, B, max_sweeps, tol, _p(ev), _p(V32), _p(V64), _p(sw),
                                         _act(active, B), _p(ws), ws.numel(), _stream(A.device)),
               "cq_jacobi_eigh_masked")
        return ev, V32, V64, sw
    _check(lib.cq_jacobi_eigh(_p(A), p, B, max_sweeps, tol, _p(ev), _p(V32), _p(V64), _p(sw), _p(ws),
                              ws.numel(), _stream(A.device)), "cq_jacobi_eigh")
    return ev, V32, V64, sw


def extreme_eigs(T: torch.Tensor, steps: int = 40, active=None) -> torch.Tensor:
    """T (B, p, p) fp64 symmetric, p <= 512 (not overwritten) -> (B, 2) fp64 [largest,
    smallest eigenvalue] by Lanczos + bisection (cq_extreme_eigs): the filter bounds of the
    solver's cheap outer iterations without a values-only eigensolve."""
    _require_hip(T)
    B, p, _ = T.shape
    ends = torch.empty((B, 2), dtype=torch.float64, device=T.device)
    if active is not None:
        _check(load().cq_extreme_eigs_masked(_p(T), p, B, int(steps), _p(ends), _act(active, B), _stream(T.device)),
               "cq_extreme_eigs_masked")
        return ends
    _check(load().cq_extreme_eigs(_p(T), p, B, int(steps), _p(ends), _stream(T.device)), "cq_extreme_eigs")
    return ends


class BlockJacobi:
    """cq_jacobi_eigh_staged (block Jacobi): begin + a first batch of sweeps, then further sweeps
    only while the device count of unconverged matrices (read back by the caller) is nonzero."""
    BEGIN, SWEEPS, END = 1, 2, 4

    def __init__(self, A: torch.Tensor, tol: float, want_vectors: bool = True, active=None):
        _require_hip(A)
        self.A, self.tol, self.want = A, tol, bool(want_vectors)
        self.B, self.p, _ = A.shape
        # masked-out matrices are done from the begin stage on (never pending) and finish() leaves
        # their values and vectors alone; the mask must hold its value until finish()
        self.active = active
        self.ws = workspace(load().cq_jacobi_staged_workspace(self.p, self.B), A.device)
        self.pending = torch.zeros(1, dtype=torch.int32, device=A.device)
        self.swept = 0

    def _call(self, phase, nsweeps=0, ev=None, V32=None, sw=None):
        if self.active is not None:
            _check(load().cq_jacobi_eigh_staged_masked(_p(self.A), self.p, self.B, phase, nsweeps, self.tol,
                                                       int(self.want), _p(ev), _p(V32), None, _p(sw), _p(self.pending),
                                                       _act(self.active, self.B), _p(self.ws), self.ws.numel(),
                                                       _stream(self.A.device)), "cq_jacobi_eigh_staged_masked")
            return
        _check(load().cq_jacobi_eigh_staged(_p(self.A), self.p, self.B, phase, nsweeps, self.tol, int(self.want),
                                            _p(ev), _p(V32), None, _p(sw), _p(self.pending), _p(self.ws),
                                            self.ws.numel(), _stream(self.A.device)), "cq_jacobi_eigh_staged")

    def launch(self, n: int, begin: bool = False):
        """n more sweeps (stream-ordered, no host sync)."""
        self._call((self.BEGIN if begin else 0) | self.SWEEPS, n)
        self.swept += n

    def pending_count(self) -> int:
        """Matrices still unconverged after the sweeps launched so far (host read-back)."""
        return int(self.pending.item())

    def sweeps(self, n: int, begin: bool = False) -> int:
        """n more sweeps; returns the number of matrices still unconverged (host read-back)."""
        self.launch(n, begin)
        return self.pending_count()

    def finish(self):
        dev = self.A.device
        ev = torch.empty((self.B, self.p), dtype=torch.float64, device=dev)
        V32 = torch.empty((self.B, self.p, self.p), dtype=torch.float32, device=dev) if self.want else None
        sw = torch.empty(self.B, dtype=torch.int32, device=dev)
        self._call(self.END, 0, ev, V32, sw)
        return ev, V32, None, sw


def ritz_residual(X, Z, theta, r, active=None):
    _require_hip(X, Z, theta)
    B, k, p = X.shape
    out = torch.empty(B, dtype=torch.float32, device=X.device)
    lib = load()
    ws = workspace(lib.cq_ritz_workspace(k, r, B), X.device)
    if active is not None:
        _check(lib.cq_ritz_residual_masked(_p(X), _p(Z), _p(theta), k, p, r, B, _p(out), _act(active, B), _p(ws),
                                           ws.numel(), _stream(X.device)), "cq_ritz_residual_masked")
        return out
    _check(lib.cq_ritz_residual(_p(X), _p(Z), _p(theta), k, p, r, B, _p(out), _p(ws), ws.numel(),
                                _stream(X.device)), "cq_ritz_residual")
    return out


def ritz_product_error(X, Z, theta, r, ysq, active=None):
    """Per-matrix estimate of the relative error of the rank-r projection (cq_ritz_product_error)."""
    _require_hip(X, Z, theta, ysq)
    B, k, p = X.shape
    out = torch.empty(B, dtype=torch.float32, device=X.device)
    lib = load()
    ws = workspace(lib.cq_ritz_workspace(k, r, B), X.device)
    if active is not None:
        _check(lib.cq_ritz_product_error_masked(_p(X), _p(Z), _p(theta), k, p, r, B, _p(ysq), _p(out), _act(active, B),
                                                _p(ws), ws.numel(), _stream(X.device)), "cq_ritz_product_error_masked")
        return out
    _check(lib.cq_ritz_product_error(_p(X), _p(Z), _p(theta), k, p, r, B, _p(ysq), _p(out), _p(ws), ws.numel(),
                                     _stream(X.device)), "cq_ritz_product_error")
    return out


def scale_rc(X, *, trans=False, rowscale=None, colscale=None, out=None):
    """out[b] = op(X[b]) * rowscale[b][:,None] * colscale[b][None,:] (scales (B,len) or (len,))."""
    _require_hip(X, rowscale, colscale)
    X_, ldx, sx = _mat(X)
    B = X.shape[0] if X.dim() == 3 else 1
    rows, cols = (X.shape[-1], X.shape[-2]) if trans else (X.shape[-2], X.shape[-1])
    if out is None:
        out = torch.empty((B, rows, cols), dtype=torch.float32, device=X.device)
    Y_, ldy, sy = _mat(out)
    rss = rowscale.shape[-1] if rowscale is not None and rowscale.dim() == 2 and rowscale.shape[0] > 1 else 0
    css = colscale.shape[-1] if colscale is not None and colscale.dim() == 2 and colscale.shape[0] > 1 else 0
    if X.dim() == 3 and X.shape[0] > 1:
        sx = X.stride(0)
    if out.dim() == 3 and out.shape[0] > 1:
        sy = out.stride(0)
    _check(load().cq_scale_rc(_p(X_), ldx, sx, int(trans), _p(Y_), ldy, sy, rows, cols, B, _p(rowscale),
                              rss, _p(colscale), css, _stream(X.device)), "cq_scale_rc")
    return out


# ---------------------------------------------------------------------------- split-fp16 products
def sym_split_f16(G: torch.Tensor, x_scale: float, *, hi=None, lo=None, scale=None, inv_scale=None,
                  upper_only=False, blocked=False):
    """G (B, n, n) fp32 PSD -> (hi, lo fp16, scale (B,), inv_scale (B,) = 1/(scale*x_scale)).
    upper_only: only G's upper triangle is valid (x3 tri Gram); the split is mirrored."""
    _require_hip(G)
    assert G.dtype == torch.float32 and G.is_contiguous() and G.dim() == 3 and G.shape[1] == G.shape[2]
    B, n, _ = G.shape
    dev = G.device
    hi = torch.empty((B, n, n), dtype=torch.float16, device=dev) if hi is None else hi
    lo = torch.empty((B, n, n), dtype=torch.float16, device=dev) if lo is None else lo
    scale = torch.empty(B, dtype=torch.float32, device=dev) if scale is None else scale
    inv_scale = torch.empty(B, dtype=torch.float32, device=dev) if inv_scale is None else inv_scale
    _check(load().cq_sym_split_f16(_p(G), n, B, int(bool(upper_only)), int(bool(blocked)), float(x_scale), _p(hi),
                                   _p(lo), _p(scale),
                                   _p(inv_scale),
                                   _stream(dev)), "cq_sym_split_f16")
    return hi, lo, scale, inv_scale


def transpose_split(X: torch.Tensor, *, out=None, hi=None, lo=None, scale: float | torch.Tensor = 1.0,
                    blocked: bool = False, active=None):
    """X (B, r, c) fp32 contiguous -> X^T (B, c, r) fp32 (out) and/or its fp16 split (hi, lo)
    scaled by `scale` (a float, or a (B,) fp32 tensor of per-matrix scales); hi without lo: the
    hi half alone (the operand of a single product)."""
    _require_hip(X)
    assert X.dtype == torch.float32 and X.is_contiguous() and X.dim() == 3
    B, r, c = X.shape
    sv = scale if torch.is_tensor(scale) else None
    sf = 1.0 if sv is not None else float(scale)
    if active is not None:  # masked-out matrices: out and the halves left as they are
        _check(load().cq_transpose_split_masked(_p(X), r, c, B, _p(out), _p(hi), _p(lo), sf, _p(sv), int(bool(blocked)),
                                                _act(active, B), _stream(X.device)), "cq_transpose_split_masked")
        return out, hi, lo
    _check(load().cq_transpose_split(_p(X), r, c, B, _p(out), _p(hi), _p(lo), sf, _p(sv), int(bool(blocked)),
                                     _stream(X.device)),
           "cq_transpose_split")
    return out, hi, lo


TRIU_SPLIT_MAX_P = 192


def triu_split_ok(M: int, p: int) -> bool:
    """Shapes cq_gemm_triu_split takes (p % 32 == 0, p <= 192, M % 32 == 0)."""
    return p % 32 == 0 and 0 < p <= TRIU_SPLIT_MAX_P and M % 32 == 0


def gemm_triu_split(X: torch.Tensor, Wt: torch.Tensor, C: torch.Tensor, hi: torch.Tensor, lo: torch.Tensor,
                    scale: float, active=None):
    """C = X Wt (Wt upper triangular) and hi/lo = the K-blocked split of C^T at `scale`: the
    same bits as gemm(X, Wt, b_triu=True) followed by transpose_split(C, blocked=True)."""
    _require_hip(X)
    B, M, p = X.shape
    assert X.dtype == Wt.dtype == C.dtype == torch.float32 and hi.dtype == lo.dtype == torch.float16
    assert X.is_contiguous() and Wt.is_contiguous() and C.is_contiguous() and hi.is_contiguous() and lo.is_contiguous()
    assert Wt.shape == (B, p, p) and C.shape == X.shape and hi.shape == (B, p, M) and lo.shape == hi.shape
    if active is not None:
        _check(load().cq_gemm_triu_split_masked(_p(X), _p(Wt), M, p, B, _p(C), _p(hi), _p(lo), float(scale),
                                                _act(active, B), _stream(X.device)), "cq_gemm_triu_split_masked")
        return
    _check(load().cq_gemm_triu_split(_p(X), _p(Wt), M, p, B, _p(C), _p(hi), _p(lo), float(scale),
                                     _stream(X.device)), "cq_gemm_triu_split")
    return C


def pow2_scale(X: torch.Tensor, log2_target: int = 14, out=None):
    """(B,) fp32 power-of-two scales s[b] with max|X[b]| * s[b] < 2^log2_target."""
    _require_hip(X)
    assert X.dtype == torch.float32 and X.is_contiguous()
    B = X.shape[0]
    out = torch.empty(B, dtype=torch.float32, device=X.device) if out is None else out
    _check(load().cq_pow2_scale(_p(X), X.numel() // B, B, int(log2_target), _p(out), _stream(X.device)),
           "cq_pow2_scale")
    return out


def pow2_from_absmax(bits: torch.Tensor, log2_target: int = 14) -> torch.Tensor:
    """In place: (B,) bits of max|X[b]| (as written by gemm_x3 absmax_out, or a positive fp32
    bound such as a quantiser's scale) -> the fp32 power-of-two split scales pow2_scale would
    give for X (cq_pow2_from_absmax).  Returns the tensor viewed as fp32."""
    _require_hip(bits)
    assert bits.element_size() == 4 and bits.is_contiguous()
    out = bits.view(torch.float32)
    _check(load().cq_pow2_from_absmax(_p(out), bits.numel(), int(log2_target), _stream(bits.device)),
           "cq_pow2_from_absmax")
    return out


def split_f16(X: torch.Tensor, scale, *, hi=None, lo=None, blocked: bool = False):
    """fp16 halves of X * scale (scale: float or (B,) tensor), same shape as X; blocked: the
    K-blocked operand layout over X's last dimension (storage size unchanged)."""
    _require_hip(X)
    assert X.dtype == torch.float32 and X.is_contiguous()
    B = X.shape[0]
    hi = torch.empty(X.shape, dtype=torch.float16, device=X.device) if hi is None else hi
    lo = torch.empty(X.shape, dtype=torch.float16, device=X.device) if lo is None else lo
    sv = scale if torch.is_tensor(scale) else None
    sf = 1.0 if sv is not None else float(scale)
    _check(load().cq_split_f16(_p(X), X.numel() // B, B, _p(sv), sf, _p(hi), _p(lo),
                               X.shape[-1] if blocked else 0, _stream(X.device)),
           "cq_split_f16")
    return hi, lo


# automatic split-K of small-batch split-fp16 products (gemm_x3); False: every product in one
# pass, so results do not depend on the batch a matrix is decomposed in (slower at small B).
# The process default; split_k_policy() overrides it for the calling thread only.
AUTO_SPLIT_K = True
_POLICY = threading.local()


@contextlib.contextmanager
def split_k_policy(enabled: bool):
    """Within the block, this thread's gemm_x3 calls use automatic split-K iff `enabled`
    (overlap.run_interleaved turns it off while batches share the chip); other threads keep
    their own policy."""
    prev = getattr(_POLICY, "auto", None)
    _POLICY.auto = bool(enabled)
    try:
        yield
    finally:
        _POLICY.auto = prev


def auto_split_k() -> bool:
    v = getattr(_POLICY, "auto", None)
    return AUTO_SPLIT_K if v is None else v


def gemm_x3(Ah, Al, Bh, Bl, inv_scale, C, *, P=None, D=None, alpha_v=None, beta_v=None, gamma_v=None,
            out_h=None, out_l=None, out_scale=1.0, overflow=None, tri=False, b_blocked=False, active=None,
            a_blocked=False, o_blocked=False, sym_bound=None, scale_out=None, inv_out=None, lda=None, M=None,
            single=False, ksplit=None, b_exact=False, colw=None, absmax_out=None, Ct=None, skip=False):
    """C (B, M, N) = alpha * A B^T * inv_scale + beta P + gamma D with A = Ah + Al (B, M, K) and
    B = Bh + Bl (B, N, K) fp16 halves (b_blocked: in the K-blocked layout of sym_split_f16,
    same storage size); optional fp16 split of C into out_h/out_l.
    sym_bound (B,) fp64: symmetric Gram mode (tri): the K-blocked split of C is written from
    its upper triangle with scale s[b] from the bound (scale_out, inv_out = 1/(s out_scale));
    C may then be None.  lda / M (a_blocked only): A holds lda >= M rows of which the first M
    are used (C has M rows).  b_exact: B is exactly fp16 (Bl = 0, e.g. W's halves written
    under a split scale >= 1); Bl is not read and may be None.  colw (N,) fp32: the product
    term of column j scaled by colw[j] (before beta P + gamma D; (B, N): per matrix).  absmax_out (B,) int32/uint32/fp32
    (plain products): zeroed here, receives the bits of max|C[b]| (pow2_from_absmax turns them
    into the next split's scale without a pass over C).  Ct (B, N, M) fp32: C^T as well (not
    with tri / sym_out); C may then be None (only C^T is written).  out_l may be None with
    out_h given (hi halves only, for a single product that follows; not with sym_bound).
    active (B,) int32: a matrix with active[b] == 0 skips the product and gets C = D and its split
    (D required) -- or, in the skip form (D None, or skip=True), is left out: nothing of it is
    written (C, Ct, halves, overflow flag)."""
    assert Bl is not None or b_exact or single
    _require_hip(Ah, Al, Bh, Bl, C)
    Bt, MA, Kd = Ah.shape
    M = MA if M is None else M
    N = Bh.shape[1]
    assert lda is None or (a_blocked and lda == MA and M <= MA)
    assert Bh.shape[2] == Kd and (C is None or C.shape == (Bt, M, N))
    for t in (Ah, Al, Bh, Bl, C, P, D, out_h, out_l):
        assert t is None or t.is_contiguous()
    for t in (out_h, out_l):  # the split output is M x N per matrix (sym_out: M = N)
        assert t is None or t.numel() >= Bt * M * N, "gemm_x3: split output buffer too small"
    g = X3Args()
    g.M, g.N, g.K, g.batch = M, N, Kd, Bt
    g.Ah, g.Al, g.lda, g.stride_a = Ah.data_ptr(), Al.data_ptr(), (MA if a_blocked else Kd), MA * Kd
    g.Bh, g.Bl, g.ldb, g.stride_b = Bh.data_ptr(), (Bl.data_ptr() if Bl is not None else None), (
        N if b_blocked else Kd), N * Kd
    g.inv_scale = inv_scale.data_ptr()
    g.C, g.ldc, g.stride_c = (C.data_ptr() if C is not None else None), N, M * N
    if P is not None:
        g.P, g.ldp, g.stride_p = P.data_ptr(), N, M * N
    if D is not None:
        g.D, g.ldd, g.stride_d = D.data_ptr(), N, M * N
    g.alpha_v = alpha_v.data_ptr() if alpha_v is not None else None
    g.beta_v = beta_v.data_ptr() if beta_v is not None else None
    g.gamma_v = gamma_v.data_ptr() if gamma_v is not None else None
    if out_h is not None and sym_bound is None:
        g.out_h, g.out_l, g.ldo, g.stride_o = out_h.data_ptr(), (out_l.data_ptr() if out_l is not None else None), N, M * N
        g.out_scale = out_scale
        g.overflow = overflow.data_ptr()
    g.tri = int(bool(tri))
    g.b_blocked = int(b_blocked)  # 1: K-blocked by 32, 2: by 16 (4-stage kernel only)
    g.active = active.data_ptr() if active is not None else None
    g.a_blocked = int(a_blocked)
    g.o_blocked = int(bool(o_blocked))
    g.single = int(bool(single))
    g.b_exact = int(bool(b_exact))
    if colw is not None:
        assert colw.dtype == torch.float32 and colw.is_contiguous() and colw.shape[-1] == N
        g.colw, g.stride_colw = colw.data_ptr(), _wst(colw, Bt)
    if absmax_out is not None:
        assert absmax_out.numel() == Bt and absmax_out.element_size() == 4 and absmax_out.is_contiguous()
        absmax_out.zero_()
        g.absmax_out = absmax_out.data_ptr()
    if Ct is not None:
        _require_hip(Ct)
        assert not tri and Ct.dtype == torch.float32 and Ct.is_contiguous() and Ct.shape == (Bt, N, M)
        g.Ct, g.stride_ct = Ct.data_ptr(), N * M
    # split-K where the batch has fewer output tiles than the chip has CUs (one caldera() call:
    # the filter's 192 x 4096 product is 11 tiles): chunks of >= 8 K steps, ~512 workgroups.
    # The chunked sum has another fp32 summation order than the one-pass product, so a matrix
    # decomposed alone (or in a small batch) and the same matrix inside a large batch agree to
    # the products' rounding, not bit for bit; AUTO_SPLIT_K = False pins one pass everywhere
    tiles = -(-N // 384) * -(-M // 192) * Bt
    splittable = not tri and sym_bound is None and (C is not None or Ct is not None) and N % 4 == 0
    if ksplit is None and not auto_split_k():
        ksplit = 1
    if ksplit is None:  # automatic
        ks = min(Kd // 32 // 8, -(-512 // tiles)) if splittable and tiles < 256 and Kd >= 512 else 1
    else:
        ks = int(ksplit)
        assert ks == 1 or (splittable and ks <= Kd // 32), "gemm_x3: split-K not possible here"
    if ks > 1:
        g.ksplit = ks
        g.split_ws = scratch.get_flat("gemm_x3.split", ks * Bt * M * N, torch.float32, Ah.device).data_ptr()
    if sym_bound is not None:
        g.sym_out = 1
        g.out_bound, g.scale_out, g.inv_out = sym_bound.data_ptr(), scale_out.data_ptr(), inv_out.data_ptr()
        g.out_h, g.out_l, g.ldo, g.stride_o = out_h.data_ptr(), out_l.data_ptr(), N, M * N
        g.out_scale = out_scale
    if skip and active is not None:
        _check(load().cq_gemm_x3_skip(ctypes.byref(g), _stream(Ah.device)), "cq_gemm_x3_skip")
        return C
    _check(load().cq_gemm_x3(ctypes.byref(g), _stream(Ah.device)), "cq_gemm_x3")
    return C


def q_update_x3(W: torch.Tensor, L: torch.Tensor | None, R: torch.Tensor | None, bits: int, *, eps: float = 1e-8,
                codes=None, packed=None, scale=None, err_w=None, err_out=None, events=None, absmax_in=None,
                scale_hint=None, fallback_out=None):
    """Fused Q update: quantise res = W - L R (W alone if L is None) per matrix, never
    materialising res.  W (B, m, n) fp16/fp32, L (B, m, r), R (B, r, n) fp32 with r % 32 == 0.
    Fills packed (B, m*n*bits/8) uint8 and/or codes, scale (B,), err_out (B,) fp64.
    scale_hint (B,) fp32 (may be `scale` itself): the previous Q update's scales -- 2-bit
    packed codes are then produced with one recompute of L R (candidate lists, see
    include/caldera_hip.h); fallback_out (B,) int32 reports matrices that needed the second."""
    _require_hip(W, L, R, codes, packed, scale, err_w, err_out, scale_hint, fallback_out)
    assert W.is_contiguous()
    B, m, n = W.shape
    dt = {torch.float16: CQ_F16, torch.float32: CQ_F32}[W.dtype]
    dev = W.device
    r = 0 if L is None else L.shape[-1]
    halves = [None] * 4
    inv = None
    if r:
        sL = pow2_scale(L.contiguous(), 14)
        sR = pow2_scale(R.contiguous(), 14)
        Lh, Ll = split_f16(L.contiguous(), sL)
        Rth = torch.empty((B, n, r), dtype=torch.float16, device=dev)
        Rtl = torch.empty_like(Rth)
        transpose_split(R.contiguous(), hi=Rth, lo=Rtl, scale=sR)
        inv = 1.0 / (sL * sR)
        halves = [Lh, Ll, Rth, Rtl]
    lib = load()
    # the hint only matters to the 2-bit packed path on fp16 W (the C side ignores it
    # otherwise): only then is the list workspace (~0.22 B per element from 2^22 elements on:
    # single candidates 8 B each for 15.5 % of the 8-element groups, whole groups 36 B each for
    # 1.5 %; smaller matrices 50 % and 25 %) sized and cached (scratch.py)
    hint = (scale_hint is not None and r > 0 and bits == 2 and packed is not None and codes is None
            and W.dtype == torch.float16)
    if not hint:
        scale_hint = None
    ws = scratch.get("q_update.ws_list" if hint else "q_update.ws",
                     (max(int(lib.cq_q_update_workspace(m, n, B, int(hint))), 16),), torch.uint8, dev)
    if events is not None:  # HIP events around the quantise kernels only (bench roofline)
        events[0].record()
    _check(lib.cq_q_update_x3(dt, _p(W), m, n, r, B, *[_p(t) for t in halves], _p(inv), bits, float(eps), _p(codes),
                              _p(packed), _p(scale), _p(err_w), _wst(err_w, B), _p(err_out),
                              _p(absmax_in if r == 0 else None),
                              _p(scale_hint if r else None), _p(fallback_out), _p(ws), ws.numel(), _stream(dev)),
           "cq_q_update_x3")
    if events is not None:
        events[1].record()


def q_update_list_geometry(m: int, n: int, r: int, both: bool = False):
    """(rows of W per list region, capacity of its single-candidate list[, capacity of its
    list of groups with two or more candidates]) of the 2-bit single-recompute Q update
    (cq_q_update_list_geometry), or None where it does not apply."""
    rows, cap, capb = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    if load().cq_q_update_list_geometry(m, n, r, ctypes.byref(rows), ctypes.byref(cap), ctypes.byref(capb)) != 0:
        return None
    return (int(rows.value), int(cap.value), int(capb.value)) if both else (int(rows.value), int(cap.value))


def absmax(X: torch.Tensor) -> torch.Tensor:
    """(B,) fp32 max |X[b]| of a (B, ...) fp16/fp32 tensor."""
    _require_hip(X)
    X = X.contiguous()
    B = X.shape[0]
    dt = {torch.float16: CQ_F16, torch.float32: CQ_F32}[X.dtype]
    out = torch.empty(B, dtype=torch.float32, device=X.device)
    _check(load().cq_absmax(dt, _p(X), X.numel() // B, B, _p(out), _stream(X.device)), "cq_absmax")
    return out


def sgram_split(k: int, L: int) -> int:
    """The l-split point of the sparse-code Gram's ELL for a k x L code matrix (L: no split)."""
    return int(load().cq_sgram_split(k, L))


def sgram_count(packed, k, L, row_nnz, perm, slice_off, total, W=None, qscale=None, wcol=None, corr_ws=None,
                corr_out=None, Lh=None, row_nnz1=None, slice_w1=None):
    """Sliced-ELL layout of the nonzero 2-bit codes per row (cq_sgram_count): packed (B, k*L/4).
    With W (B, k, L) fp16: corr_out (B,) fp64 = ||(W - s c) diag(ycol)||^2 - ||W diag(ycol)||^2
    (wcol = ycol^2), corr_ws (B * k,) fp64 scratch.  Lh < L (sgram_split): the l-split layout,
    row_nnz1 (B * k,) int32 scratch, slice_w1 (B * ceil(k / 64),) int32 out."""
    _require_hip(packed, row_nnz, perm, slice_off, total, W, qscale, wcol, corr_ws, corr_out, row_nnz1, slice_w1)
    B = total.numel()
    Lh = L if Lh is None else Lh
    ns = -(-k // 64)
    assert row_nnz.numel() >= B * k and perm.numel() >= B * k and slice_off.numel() >= B * (ns + 1)
    assert Lh >= L or (row_nnz1.numel() >= B * k and slice_w1.numel() >= B * ns and slice_w1.dtype == torch.int32)
    if W is not None:
        assert W.dtype == torch.float16 and W.is_contiguous() and W.shape == (B, k, L)
        assert corr_ws.numel() >= B * k and corr_ws.dtype == torch.float64 and corr_out.numel() == B
    _check(load().cq_sgram_count(_p(packed), 2, B, k, L, _p(row_nnz), _p(perm), _p(slice_off), _p(total), Lh,
                                 _p(row_nnz1), _p(slice_w1), _p(W), _p(qscale), _p(wcol), _wst(wcol, B), _p(corr_ws),
                                 _p(corr_out),
                                 _stream(packed.device)), "cq_sgram_count")


def sgram_fill(packed, k, L, row_nnz, perm, slice_off, ell, stride, Lh=None, slice_w1=None):
    _require_hip(packed, row_nnz, perm, slice_off, ell, slice_w1)
    B = slice_off.numel() // (-(-k // 64) + 1)
    assert ell.numel() >= B * stride
    Lh = L if Lh is None else Lh
    _check(load().cq_sgram_fill(_p(packed), 2, B, k, L, _p(row_nnz), _p(perm), _p(slice_off), _p(slice_w1), Lh,
                                stride, _p(ell), _stream(packed.device)), "cq_sgram_fill")


def codes_transpose(packed, rows, cols, out=None):
    """2-bit packed codes (B, rows*cols/4) -> the packed codes of the transposes (B, cols*rows/4)."""
    _require_hip(packed, out)
    B = packed.shape[0]
    assert packed.dtype == torch.uint8 and packed.is_contiguous() and packed.numel() == B * rows * cols // 4
    if out is None:
        out = torch.empty_like(packed)
    assert out.shape == packed.shape and out.is_contiguous() and out.data_ptr() != packed.data_ptr()
    _check(load().cq_codes_transpose(_p(packed), 2, B, rows, cols, _p(out), _stream(packed.device)),
           "cq_codes_transpose")
    return out


CODES_MATMUL_MAX_R = 256  # cq_codes_matmul's r limit (cq_sgram.hip: RV <= 4 columns per lane)


def codes_matmul(packed, rows, cols, X, r, out, *, colw=None, roww=None, trans=False):
    """out[b] = diag(roww) c[b] diag(colw) X[b][:, :r] (rows x r; trans: its transpose, r x rows) for
    2-bit packed codes c (B, rows, cols) and X (B, cols, ldx) fp32 (cq_codes_matmul)."""
    _require_hip(packed, X, colw, roww, out)
    B = packed.shape[0]
    assert roww is None or (roww.shape[-1] == rows and roww.dtype == torch.float32 and roww.is_contiguous())
    assert packed.numel() == B * rows * cols // 4 and X.shape[:2] == (B, cols) and X.stride(2) == 1
    assert X.dtype == torch.float32 and out.dtype == torch.float32 and out.is_contiguous()
    assert out.shape == ((B, r, rows) if trans else (B, rows, r))
    assert colw is None or (colw.shape[-1] == cols and colw.dtype == torch.float32 and colw.is_contiguous())
    _check(load().cq_codes_matmul(_p(packed), 2, B, rows, cols, _p(X), X.stride(1), X.stride(0), _p(colw), _wst(colw, B),
                                  _p(roww), _wst(roww, B), r, _p(out),
                                  out.shape[2], out.stride(0), int(bool(trans)), _stream(packed.device)),
           "cq_codes_matmul")
    return out


def codes_ysq_corr(packed, W, qscale, colw=None, out=None):
    """(B,) fp64: ||(W - s c) diag(ycol)||^2 - ||W diag(ycol)||^2 (colw = ycol^2) over the nonzero
    2-bit codes c of W (B, m, n) fp16 (cq_codes_ysq_corr)."""
    _require_hip(packed, W, qscale, colw, out)
    B, m, n = W.shape
    assert W.dtype == torch.float16 and W.is_contiguous() and packed.numel() == B * m * n // 4
    if out is None:
        out = torch.empty(B, dtype=torch.float64, device=W.device)
    _check(load().cq_codes_ysq_corr(_p(packed), 2, _p(W), CQ_F16, _p(qscale), _p(colw), _wst(colw, B), B, m, n, _p(out),
                                    _stream(W.device)), "cq_codes_ysq_corr")
    return out


def transpose_f16(X, out=None):
    """(B, rows, cols) fp16 -> (B, cols, rows) (cq_transpose_f16)."""
    _require_hip(X, out)
    B, rows, cols = X.shape
    assert X.dtype == torch.float16 and X.is_contiguous()
    if out is None:
        out = torch.empty((B, cols, rows), dtype=torch.float16, device=X.device)
    assert out.shape == (B, cols, rows) and out.is_contiguous()
    _check(load().cq_transpose_f16(_p(X), B, rows, cols, _p(out), _stream(X.device)), "cq_transpose_f16")
    return out


def sgram_rows(L: int) -> int:
    return int(load().cq_sgram_rows(L))


def sgram_spmm(W, packed, qscale, wcol, ell, perm, slice_off, stride, P, Lh=None, slice_w1=None):
    """P (B, k, k) = (W - (s/2) c) diag(wcol) c^T over the ELL codes (cq_sgram_spmm); wcol = the Gram's
    column weights w = ycol^2 (None: 1).  Lh / slice_w1: the l-split layout of sgram_count."""
    _require_hip(W, packed, qscale, wcol, ell, perm, slice_off, P, slice_w1)
    B, k, L = W.shape
    assert W.dtype == torch.float16 and W.is_contiguous() and P.shape == (B, k, k) and P.is_contiguous()
    assert wcol is None or (wcol.shape[-1] == L and wcol.dtype == torch.float32)
    Lh = L if Lh is None else Lh
    _check(load().cq_sgram_spmm(CQ_F16, _p(W), _p(packed), _p(qscale), _p(wcol), _wst(wcol, B), B, k, L, _p(ell), _p(perm),
                                _p(slice_off), _p(slice_w1), Lh, stride, _p(P), _stream(W.device)), "cq_sgram_spmm")


def sgram_combine(A, P, qscale, bound, out_scale, Gh, Gl, scale_out, inv_out, G32=None):
    """G = A - s (P + P^T) -> K-blocked split halves (cq_sgram_combine)."""
    _require_hip(A, P, qscale, bound, Gh, Gl, scale_out, inv_out, G32)
    B, k, _ = P.shape
    assert A.shape == P.shape and Gh.numel() >= B * k * k and Gl.numel() >= B * k * k
    assert G32 is None or G32.shape == (B, k, k)
    _check(load().cq_sgram_combine(_p(A), _p(P), _p(qscale), B, k, _p(bound), float(out_scale), _p(Gh), _p(Gl),
                                   _p(scale_out), _p(inv_out), _p(G32), _stream(P.device)), "cq_sgram_combine")


def residual_split(Ws, packed, qscale, bits, wmax, *, ycol=None, ycol_max=1.0, res=None, Y=None, hi=None, lo=None,
                   thi=None, tlo=None, scale=None, sq=None, ycol_hi=None, ycol_hi_max=1.0, scale_hi=None):
    """Fused LR-step residual (see include/caldera_hip.h cq_residual_split).  Ws (B, m, n).
    ycol_hi: hi/lo are the halves of res * ycol_hi (their scale in scale_hi) instead.
    Per-matrix weights: ycol / ycol_hi (B, n) with ycol_max / ycol_hi_max (B,) fp32 tensors."""
    _require_hip(Ws, packed, qscale, wmax, ycol, res, Y, hi, lo, thi, tlo, scale, sq, ycol_hi, scale_hi)
    B, m, n = Ws.shape
    dt = {torch.float16: CQ_F16, torch.float32: CQ_F32}[Ws.dtype]
    yst = max(_wst(ycol, B), _wst(ycol_hi, B))
    assert ycol is None or ycol_hi is None or ycol.shape == ycol_hi.shape
    ymv = ycol_max if torch.is_tensor(ycol_max) else None
    yhmv = ycol_hi_max if torch.is_tensor(ycol_hi_max) else None
    for t in (ymv, yhmv):
        assert t is None or (t.dtype == torch.float32 and t.numel() == B and t.is_contiguous() and t.is_cuda)
    lib = load()
    ws = workspace(lib.cq_residual_split_workspace(m, n, B), Ws.device) if sq is not None else None
    _check(lib.cq_residual_split(dt, _p(Ws), _p(packed), _p(qscale), int(bits), _p(ycol),
                                 1.0 if ymv is not None else float(ycol_max), _p(wmax),
                                 B, m, n, _p(res), _p(Y), _p(hi), _p(lo), _p(thi), _p(tlo), _p(scale), _p(sq),
                                 _p(ycol_hi), 1.0 if yhmv is not None else float(ycol_hi_max), _p(scale_hi), yst,
                                 _p(ymv), _p(yhmv), _p(ws),
                                 0 if ws is None else ws.numel(), _stream(Ws.device)), "cq_residual_split")


# ---------------------------------------------------------------------------- calibration
_ACT_DT = {torch.float32: CQ_F32, torch.float16: CQ_F16, torch.bfloat16: CQ_BF16}


def _act_2d(x: torch.Tensor):
    """(rows, cols) view with unit column stride, or a contiguous copy."""
    if x.dtype not in _ACT_DT:
        raise TypeError(f"activations must be fp32/fp16/bf16, got {x.dtype}")
    if x.dim() != 2:
        raise ValueError("activations must be 2-D (rows, cols)")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x, (x.stride(0) if x.shape[0] > 1 else x.shape[1])


def act_sqsum_cols(x: torch.Tensor, out: torch.Tensor, *, accumulate: bool = True, post: float = 1.0):
    """out (cols,) fp64 <- ((accumulate ? out : 0) + sum_i x[i, :]^2) * post  (diag of X^T X)."""
    _require_hip(x, out)
    x, ld = _act_2d(x)
    rows, cols = x.shape
    assert out.dtype == torch.float64 and out.numel() == cols and out.is_contiguous()
    lib = load()
    nws = lib.cq_act_sqsum_workspace(rows, cols)
    ws = workspace(nws, x.device) if nws else None
    _check(lib.cq_act_sqsum_cols(_ACT_DT[x.dtype], _p(x) if rows else None, rows, cols, max(ld, cols), _p(out),
                                 int(bool(accumulate)), float(post), _p(ws), 0 if ws is None else ws.numel(),
                                 _stream(x.device)), "cq_act_sqsum_cols")
    return out


def act_sqsum_rows(x: torch.Tensor, out: torch.Tensor, *, accumulate: bool = True, post: float = 1.0):
    """out (rows,) fp64 <- ((accumulate ? out : 0) + sum_j x[:, j]^2) * post  (diag of X X^T)."""
    _require_hip(x, out)
    x, ld = _act_2d(x)
    rows, length = x.shape
    assert out.dtype == torch.float64 and out.numel() == rows and out.is_contiguous()
    _check(load().cq_act_sqsum_rows(_ACT_DT[x.dtype], _p(x) if length else None, rows, length, max(ld, length),
                                    _p(out), int(bool(accumulate)), float(post), _stream(x.device)),
           "cq_act_sqsum_rows")
    return out


# ---------------------------------------------------------------------------- packed linear layer
LINEAR_DECODE_MAX_TOKENS = 16  # include/caldera_hip.h CQ_LINEAR_DECODE_MAX_TOKENS
LINEAR_MAX_RANK = 1024         # CQ_LINEAR_MAX_RANK


def linear_args(x, codes, qscale, gscale, L, R, bias, y, *, m, n, bits) -> LinearArgs:
    """cq_linear_args for x (T, n) fp16, inference-layout codes (m, row bytes) uint8, L (m, r) /
    R (r, n) fp16 (None or r = 0: codes only), bias (m,) fp32 or None and y (T, m) fp32 / fp16;
    x, L, R and y may be views with a row stride (unit column stride)."""
    return _fill_linear_args(LinearArgs(), x, codes, qscale, gscale, L, R, bias, y, m=m, n=n, bits=bits,
                             r=0 if L is None else L.shape[1])


def _linear_need(cond, what):
    if not cond:
        raise ValueError(f"cq_linear: {what}")


def _resolve_rank(L, R, L_codes, R_codes, r) -> int:
    """The rank: r as given, else an fp16 factor's; with r > 0 each factor comes in exactly one form."""
    need = _linear_need
    if r is None:
        need(L is not None or R is not None or (L_codes is None and R_codes is None),
             "r is needed when both factors are coded")
        r = L.shape[1] if L is not None else R.shape[0] if R is not None else 0
    r = int(r)
    if r:
        need((L is None) != (L_codes is None), "give exactly one of L and L_codes")
        need((R is None) != (R_codes is None), "give exactly one of R and R_codes")
    return r


def _fp16_factors(L, R, r, L_coded, R_coded):
    """(name, tensor) of the factors that are looked at as fp16: none for r = 0, not a coded one."""
    return ((("L", L),) if r and not L_coded else ()) + ((("R", R),) if r and not R_coded else ())


def _check_fp16_factors(fp16, m, r, n):
    need = _linear_need
    if fp16:
        need(all(t.dtype == torch.float16 for _, t in fp16),
             "L and R must be fp16, got " + ", ".join(str(t.dtype) for _, t in fp16))
        need(all(tuple(t.shape) == ((m, r) if name == "L" else (r, n)) for name, t in fp16),
             " / ".join(f"{name} {tuple(t.shape)}" for name, t in fp16) + f" do not fit {(m, r)} / {(r, n)}")


def _fill_factor_codes(a, L_codes, R_codes, m, r):
    """l_bits / r_bits and, for a factor given as (codes, scale, bits), its code fields."""
    a.l_bits = a.r_bits = 16
    for what, spec, rows in (("L", L_codes, m), ("R", R_codes, r)):
        if spec is None or not r:
            continue
        t, scale, fbits = spec
        _linear_need(t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.uint8 and t.shape[0] == rows,
                     f"{what}_codes must be a uint8 matrix with {rows} rows and unit column stride")
        setattr(a, what.lower() + "_bits", int(fbits))
        setattr(a, what + "_codes", t.data_ptr())
        setattr(a, what.lower() + "_code_stride", t.stride(0))
        setattr(a, what.lower() + "scale", float(scale))


def _factor_code_tensors(L_codes, R_codes):
    return (None if L_codes is None else L_codes[0], None if R_codes is None else R_codes[0])


def _member_tensors(mem):
    """The tensors of a member dict (`linear_group_args`), as `_require_hip` takes them."""
    return (mem["codes"], mem.get("L"), mem.get("R"), mem.get("bias"),
            *_factor_code_tensors(mem.get("L_codes"), mem.get("R_codes")))


def _run(entry, workspace_entry, a, out, device, ws):
    """The wrappers' common tail: the workspace (sized by `workspace_entry` when None), the call, `out`."""
    lib = load()
    if ws is None:
        ws = workspace(getattr(lib, workspace_entry)(ctypes.byref(a)), device)
    _check(getattr(lib, entry)(ctypes.byref(a), _p(ws), ws.numel(), _stream(device)), entry)
    return out


def _fill_linear_args(a, x, codes, qscale, gscale, L, R, bias, y, *, m, n, bits, r, L_coded=False, R_coded=False):
    """The fields cq_linear_args and cq_linear_packed_args share; a coded factor's fp16 operand
    is not looked at."""
    need = _linear_need
    fp16 = _fp16_factors(L, R, r, L_coded, R_coded)
    for name, t in (("x", x), ("codes", codes), ("y", y)) + fp16:
        need(t.dim() == 2 and t.stride(1) == 1, f"{name} must be a matrix with unit column stride")
    need(x.dtype == torch.float16, f"x must be fp16, got {x.dtype}")
    need(codes.dtype == torch.uint8 and codes.shape[0] == m, "codes must be uint8 with one row per output")
    need(x.shape[1] == n and tuple(y.shape) == (x.shape[0], m), f"x {tuple(x.shape)} / y {tuple(y.shape)} do not fit "
         f"(tokens, {n}) / (tokens, {m})")
    need(y.dtype in (torch.float32, torch.float16), f"y must be fp32 or fp16, got {y.dtype}")
    _check_fp16_factors(fp16, m, r, n)
    if bias is not None:
        need(bias.dtype == torch.float32 and tuple(bias.shape) == (m,) and bias.is_contiguous(),
             f"bias must be a contiguous fp32 ({m},) vector, got {bias.dtype} {tuple(bias.shape)}")
    a.x, a.ldx = x.data_ptr(), x.stride(0)
    a.tokens, a.m, a.n, a.r = x.shape[0], m, n, r
    a.bits = bits
    a.codes, a.code_stride = codes.data_ptr(), codes.stride(0)
    a.qscale, a.gscale = float(qscale), float(gscale)
    for name, t in fp16:
        setattr(a, name, t.data_ptr())
        setattr(a, "ld" + name.lower(), t.stride(0))
    if bias is not None:
        a.bias = bias.data_ptr()
    a.y, a.ldy = y.data_ptr(), y.stride(0)
    a.y_dtype = {torch.float32: CQ_F32, torch.float16: CQ_F16}[y.dtype]
    return a


def linear_packed_args(x, codes, qscale, gscale, L, R, bias, y, *, m, n, bits, r=None, L_codes=None,
                       R_codes=None, into=None) -> LinearPackedArgs:
    """cq_linear_packed_args: `linear_args` with either factor given by its codes instead of fp16.
    L_codes / R_codes: (uint8 inference-layout codes with one row per m resp. r, scale, bits in
    {2, 4}); the fp16 L / R of a coded factor is None.  r: the rank, needed when both factors are
    coded (else taken from the fp16 one).  into: the struct to fill (a codebook struct's `p`)."""
    r = _resolve_rank(L, R, L_codes, R_codes, r)
    a = _fill_linear_args(LinearPackedArgs() if into is None else into, x, codes, qscale, gscale, L, R, bias, y, m=m,
                          n=n, bits=bits, r=r, L_coded=L_codes is not None, R_coded=R_codes is not None)
    _fill_factor_codes(a, L_codes, R_codes, m, r)
    return a


def linear_packed_forward(x, codes, qscale, gscale, L, R, bias, y, *, m, n, bits, r=None, L_codes=None,
                          R_codes=None, ws=None):
    """y = x (gs (Q + L R))^T (+ bias) with either factor applied from its packed 2/4-bit codes
    (cq_linear_packed_forward); operands as `linear_packed_args`, ws as `linear_forward`.  No
    host synchronisation."""
    _require_hip(x, codes, L, R, bias, y, *_factor_code_tensors(L_codes, R_codes))
    a = linear_packed_args(x, codes, qscale, gscale, L, R, bias, y, m=m, n=n, bits=bits, r=r, L_codes=L_codes,
                           R_codes=R_codes)
    return _run("cq_linear_packed_forward", "cq_linear_packed_workspace", a, y, x.device, ws)


QFMT_UNIFORM = 0  # include/caldera_hip.h CQ_QFMT_UNIFORM: offset-binary uniform codes
QFMT_NF = 1       # CQ_QFMT_NF: NF4 / NF2 level indices
# the integer levels I = D level of the codebook contract (include/caldera_hip.h), by bits
NF_LEVELS = {4: (-1334, -1000, -784, -617, -476, -347, -226, -112, 0, 112, 226, 347, 476, 617, 784, 1000),
             2: (-8165, -3333, 3333, 8165)}
NF_DENOM = {4: 1000.0, 2: 10000.0}


def _check_q_format(q_format, qscale):
    _linear_need(q_format in (QFMT_UNIFORM, QFMT_NF), f"unknown q_format {q_format!r}")
    if q_format == QFMT_NF:
        s = float(qscale)
        _linear_need(s >= 0.0 and s != float("inf"), f"NF scale {s} is not finite and >= 0")


def linear_codebook_args(x, codes, qscale, gscale, L, R, bias, y, *, m, n, bits, q_format, r=None, L_codes=None,
                         R_codes=None) -> LinearCodebookArgs:
    """cq_linear_codebook_args: `linear_packed_args` (the same host-side checks) plus q_format
    (QFMT_UNIFORM: offset-binary codes; QFMT_NF: `codes` holds NF4 / NF2 level indices, qscale the
    matrix scale)."""
    _check_q_format(q_format, qscale)
    a = LinearCodebookArgs()
    linear_packed_args(x, codes, qscale, gscale, L, R, bias, y, m=m, n=n, bits=bits, r=r, L_codes=L_codes,
                       R_codes=R_codes, into=a.p)
    a.q_format = int(q_format)
    return a


def linear_codebook_forward(x, codes, qscale, gscale, L, R, bias, y, *, m, n, bits, q_format, r=None, L_codes=None,
                            R_codes=None, ws=None):
    """y = x (gs (Q + L R))^T (+ bias) with Q in q_format (cq_linear_codebook_forward); operands as
    `linear_codebook_args`, ws as `linear_forward`.  No host synchronisation."""
    _require_hip(x, codes, L, R, bias, y, *_factor_code_tensors(L_codes, R_codes))
    a = linear_codebook_args(x, codes, qscale, gscale, L, R, bias, y, m=m, n=n, bits=bits, q_format=q_format, r=r,
                             L_codes=L_codes, R_codes=R_codes)
    return _run("cq_linear_codebook_forward", "cq_linear_codebook_workspace", a, y, x.device, ws)


LINEAR_GROUP_MAX = 8  # include/caldera_hip.h CQ_LINEAR_GROUP_MAX


def _fill_member(into, x, mem, y, q_format, where, gate_m=None):
    """A member dict (`linear_group_args`) into the struct `into`, with q_format's checks and
    `linear_packed_args`'; its ValueError names `where`.  gate_m: the m a gated pair's member must have."""
    try:
        _check_q_format(q_format, mem["qscale"])
        if gate_m is not None:
            _linear_need(mem["m"] == gate_m, f"m {mem['m']} differs from gate's {gate_m}")
        return linear_packed_args(x, mem["codes"], mem["qscale"], mem["gscale"], mem.get("L"), mem.get("R"),
                                  mem.get("bias"), y, m=mem["m"], n=mem["n"], bits=mem["bits"], r=mem.get("r"),
                                  L_codes=mem.get("L_codes"), R_codes=mem.get("R_codes"), into=into)
    except ValueError as e:
        raise ValueError(f"cq_linear: {where}: {str(e).removeprefix('cq_linear: ')}") from None


def _need_same(a, ref, fields, where, ref_name):
    for field in fields:
        _linear_need(getattr(a, field) == getattr(ref, field),
                     f"{where}: {field} {getattr(a, field)} differs from {ref_name}'s {getattr(ref, field)}")


def linear_group_args(x, members, ys, q_format) -> LinearGroupArgs:
    """cq_linear_group_args of layers that share the activation x (T, n) fp16.  members: one dict per
    layer with `linear_packed_args`' operands after x and before y as keys (codes, qscale, gscale, L,
    R, bias, m, n, bits and optionally r, L_codes, R_codes); ys: the layers' outputs (T, m_i), all fp32
    or all fp16.  Each member passes `linear_packed_args`' host-side checks and `q_format`'s; the
    members must share n, bits and the output dtype, and those with r > 0 the factor formats.  The
    struct keeps the member array alive."""
    need = _linear_need
    members, ys = list(members), list(ys)
    need(1 <= len(members) <= LINEAR_GROUP_MAX, f"group: count {len(members)} not in 1 .. {LINEAR_GROUP_MAX}")
    need(len(ys) == len(members), f"group: {len(ys)} outputs for {len(members)} members")
    need(q_format in (QFMT_UNIFORM, QFMT_NF), f"group: unknown q_format {q_format!r}")
    arr = (LinearPackedArgs * len(members))()
    ranked = None
    for i, (mem, y) in enumerate(zip(members, ys)):
        where = f"group member {i}"
        a = _fill_member(arr[i], x, mem, y, q_format, where)
        _need_same(a, arr[0], ("n", "bits", "y_dtype"), where, "member 0")
        if a.r > 0:
            if ranked is None:
                ranked = i
            _need_same(a, arr[ranked], ("l_bits", "r_bits"), where, f"member {ranked}")
    g = LinearGroupArgs()
    g.count, g.q_format = len(members), int(q_format)
    g.members = ctypes.cast(arr, ctypes.POINTER(LinearPackedArgs))
    g._members = arr
    return g


def linear_group_forward(x, members, ys, q_format, ws=None):
    """The layers `members` (see `linear_group_args`) on the one activation x in one z launch and one
    code + L launch (cq_linear_group_forward): ys[i] receives, bit for bit, what member i's own entry
    writes.  ws as `linear_forward`.  No host synchronisation."""
    members = list(members)
    for mem in members:
        _require_hip(x, *_member_tensors(mem))
    _require_hip(*ys)
    g = linear_group_args(x, members, ys, q_format)
    return _run("cq_linear_group_forward", "cq_linear_group_workspace", g, ys, x.device, ws)


ACT_IDENTITY = 0  # include/caldera_hip.h CQ_ACT_IDENTITY: h = g * u
ACT_SILU = 1      # CQ_ACT_SILU: h = g / (1 + exp(-g)) * u


def linear_glu_args(x, gate, up, h, q_format, act) -> LinearGluArgs:
    """cq_linear_glu_args of a gated pair on the activation x (T, n) fp16.  gate, up: member dicts as
    `linear_group_args` takes them; h: the output (T, m) fp32 / fp16, may be a view with a row stride.
    Each member passes `linear_packed_args`' host-side checks and `q_format`'s; the two must share m, n
    and bits, and when both have r > 0 the factor formats.  The members' y fields stay zero."""
    need = _linear_need
    need(q_format in (QFMT_UNIFORM, QFMT_NF), f"glu: unknown q_format {q_format!r}")
    need(act in (ACT_IDENTITY, ACT_SILU), f"glu: unknown act {act!r}")
    need(torch.is_tensor(h) and h.dim() == 2 and h.stride(1) == 1, "glu: h must be a matrix with unit column stride")
    need(h.dtype in (torch.float32, torch.float16), f"glu: h must be fp32 or fp16, got {h.dtype}")
    need(tuple(h.shape) == (x.shape[0], gate["m"]), f"glu: h {tuple(h.shape)} does not fit (tokens, m) = "
         f"{(x.shape[0], gate['m'])}")
    need(h.shape[0] <= 1 or h.stride(0) >= h.shape[1], f"glu: ldh {h.stride(0)} < m {h.shape[1]}")
    a = LinearGluArgs()
    for name, mem in (("gate", gate), ("up", up)):
        # h stands in for y while the member's other operands are checked
        p = _fill_member(getattr(a, name), x, mem, h, q_format, f"glu {name}", gate_m=gate["m"])
        p.y, p.y_dtype, p.ldy = None, 0, 0
        _need_same(p, a.gate, ("n", "bits"), f"glu {name}", "gate")
    if a.gate.r > 0 and a.up.r > 0:
        _need_same(a.up, a.gate, ("l_bits", "r_bits"), "glu up", "gate")
    a.q_format, a.act = int(q_format), int(act)
    a.h, a.ldh = h.data_ptr(), h.stride(0) if h.shape[0] > 1 else max(h.stride(0), h.shape[1])
    a.h_dtype = {torch.float32: CQ_F32, torch.float16: CQ_F16}[h.dtype]
    return a


def linear_glu_forward(x, gate, up, h, q_format, act=ACT_SILU, ws=None):
    """h = a(gate(x)) * up(x) of a gated pair in one z launch and one code + L launch
    (cq_linear_glu_forward): the pre-activations have the bits of the members' own fp32 outputs and are
    never written.  Operands as `linear_glu_args`, ws as `linear_forward`.  No host synchronisation."""
    for mem in (gate, up):
        _require_hip(x, *_member_tensors(mem))
    _require_hip(h)
    a = linear_glu_args(x, gate, up, h, q_format, act)
    return _run("cq_linear_glu_forward", "cq_linear_glu_workspace", a, h, x.device, ws)


def linear_forward(x, codes, qscale, gscale, L, R, bias, y, *, m, n, bits, ws=None):
    """y = x (gs (Q + L R))^T (+ bias) from the packed codes (cq_linear_forward); ws: a uint8
    workspace of at least cq_linear_workspace bytes (allocated here when None).  No host
    synchronisation."""
    _require_hip(x, codes, L, R, bias, y)
    a = linear_args(x, codes, qscale, gscale, L, R, bias, y, m=m, n=n, bits=bits)
    return _run("cq_linear_forward", "cq_linear_workspace", a, y, x.device, ws)


def linear_backward_args(dy, codes, qscale, gscale, L, R, dx, *, m, n, bits, u_out=None) -> LinearBackwardArgs:
    """cq_linear_backward_args for dy (T, m) fp16, inference-layout codes (m, row bytes) uint8,
    L (m, r) / R (r, n) fp16 (None or r = 0: codes only), dx (T, n) fp32 / fp16 and u_out (T, r)
    fp32 or None; dy, L, R, dx and u_out may be views with a row stride (unit column stride)."""
    r = 0 if L is None else int(L.shape[1])
    _linear_need(not r or R is not None, "L without R")
    return _fill_linear_backward_args(LinearBackwardArgs(), dy, codes, qscale, gscale, L, R, dx, m=m, n=n, bits=bits,
                                      r=r, u_out=u_out)


def _fill_linear_backward_args(a, dy, codes, qscale, gscale, L, R, dx, *, m, n, bits, r, u_out, L_coded=False,
                               R_coded=False):
    """The fields cq_linear_backward_args and cq_linear_packed_backward_args share; a coded
    factor's fp16 operand is not looked at."""
    need = _linear_need
    fp16 = _fp16_factors(L, R, r, L_coded, R_coded)
    mats = (("dy", dy), ("codes", codes), ("dx", dx)) + fp16 + ((("u_out", u_out),) if r and u_out is not None else ())
    for name, t in mats:
        need(t.dim() == 2 and t.stride(1) == 1, f"{name} must be a matrix with unit column stride")
    need(dy.dtype == torch.float16, f"dy must be fp16, got {dy.dtype}")
    need(codes.dtype == torch.uint8 and codes.shape[0] == m, "codes must be uint8 with one row per output")
    need(dy.shape[1] == m and tuple(dx.shape) == (dy.shape[0], n), f"dy {tuple(dy.shape)} / dx {tuple(dx.shape)} do not "
         f"fit (tokens, {m}) / (tokens, {n})")
    need(dx.dtype in (torch.float32, torch.float16), f"dx must be fp32 or fp16, got {dx.dtype}")
    _check_fp16_factors(fp16, m, r, n)
    a.dy, a.lddy = dy.data_ptr(), dy.stride(0)
    a.tokens, a.m, a.n, a.r = dy.shape[0], m, n, r
    a.bits = bits
    a.codes, a.code_stride = codes.data_ptr(), codes.stride(0)
    a.qscale, a.gscale = float(qscale), float(gscale)
    for name, t in fp16:
        setattr(a, name, t.data_ptr())
        setattr(a, "ld" + name.lower(), t.stride(0))
    a.dx, a.lddx = dx.data_ptr(), dx.stride(0)
    a.dx_dtype = {torch.float32: CQ_F32, torch.float16: CQ_F16}[dx.dtype]
    if r and u_out is not None:
        need(u_out.dtype == torch.float32 and tuple(u_out.shape) == (dy.shape[0], r),
             f"u_out must be fp32 (tokens, {r}), got {u_out.dtype} {tuple(u_out.shape)}")
        a.u_out, a.ldu = u_out.data_ptr(), u_out.stride(0)
    return a


def linear_backward_input(dy, codes, qscale, gscale, L, R, dx, *, m, n, bits, u_out=None, ws=None):
    """dx = dy (gs (Q + L R)) from the packed codes (cq_linear_backward_input); u_out (T, r) fp32
    receives u = dy L (without gs).  ws: a uint8 workspace of at least
    cq_linear_backward_workspace bytes (allocated here when None).  No host synchronisation."""
    _require_hip(dy, codes, L, R, dx, u_out)
    a = linear_backward_args(dy, codes, qscale, gscale, L, R, dx, m=m, n=n, bits=bits, u_out=u_out)
    return _run("cq_linear_backward_input", "cq_linear_backward_workspace", a, dx, dy.device, ws)


def linear_packed_backward_args(dy, codes, qscale, gscale, L, R, dx, *, m, n, bits, r=None, L_codes=None,
                                R_codes=None, u_out=None, into=None) -> LinearPackedBackwardArgs:
    """cq_linear_packed_backward_args: `linear_backward_args` with either factor given by its codes
    instead of fp16.  L_codes / R_codes: (uint8 inference-layout codes with one row per m resp. r,
    scale, bits in {2, 4}); the fp16 L / R of a coded factor is None.  r: the rank, needed when both
    factors are coded (else taken from the fp16 one).  into: the struct to fill (a codebook struct's `p`)."""
    r = _resolve_rank(L, R, L_codes, R_codes, r)
    a = _fill_linear_backward_args(LinearPackedBackwardArgs() if into is None else into, dy, codes, qscale, gscale, L,
                                   R, dx, m=m, n=n, bits=bits, r=r, u_out=u_out, L_coded=L_codes is not None,
                                   R_coded=R_codes is not None)
    _fill_factor_codes(a, L_codes, R_codes, m, r)
    return a


def linear_packed_backward_input(dy, codes, qscale, gscale, L, R, dx, *, m, n, bits, r=None, L_codes=None,
                                 R_codes=None, u_out=None, ws=None):
    """dx = dy (gs (Q + L R)) with either factor applied from its packed 2/4-bit codes
    (cq_linear_packed_backward_input); operands as `linear_packed_backward_args`.  u_out (T, r) fp32
    receives u~ = uscale dy lam, which carries a coded R's scale.  ws as `linear_backward_input`.  No
    host synchronisation."""
    _require_hip(dy, codes, L, R, dx, u_out, *_factor_code_tensors(L_codes, R_codes))
    a = linear_packed_backward_args(dy, codes, qscale, gscale, L, R, dx, m=m, n=n, bits=bits, r=r, L_codes=L_codes,
                                    R_codes=R_codes, u_out=u_out)
    return _run("cq_linear_packed_backward_input", "cq_linear_packed_backward_workspace", a, dx, dy.device, ws)


def linear_codebook_backward_args(dy, codes, qscale, gscale, L, R, dx, *, m, n, bits, q_format, r=None, L_codes=None,
                                  R_codes=None, u_out=None) -> LinearCodebookBackwardArgs:
    """cq_linear_codebook_backward_args: `linear_packed_backward_args` (the same host-side checks)
    plus q_format, as `linear_codebook_args`."""
    _check_q_format(q_format, qscale)
    a = LinearCodebookBackwardArgs()
    linear_packed_backward_args(dy, codes, qscale, gscale, L, R, dx, m=m, n=n, bits=bits, r=r, L_codes=L_codes,
                                R_codes=R_codes, u_out=u_out, into=a.p)
    a.q_format = int(q_format)
    return a


def linear_codebook_backward_input(dy, codes, qscale, gscale, L, R, dx, *, m, n, bits, q_format, r=None,
                                   L_codes=None, R_codes=None, u_out=None, ws=None):
    """dx = dy (gs (Q + L R)) with Q in q_format (cq_linear_codebook_backward_input); operands as
    `linear_codebook_backward_args`, u_out and ws as `linear_packed_backward_input`.  No host
    synchronisation."""
    _require_hip(dy, codes, L, R, dx, u_out, *_factor_code_tensors(L_codes, R_codes))
    a = linear_codebook_backward_args(dy, codes, qscale, gscale, L, R, dx, m=m, n=n, bits=bits, q_format=q_format,
                                      r=r, L_codes=L_codes, R_codes=R_codes, u_out=u_out)
    return _run("cq_linear_codebook_backward_input", "cq_linear_codebook_backward_workspace", a, dx, dy.device, ws)


def linear_dequant_args(codes, qscale, gscale, L, R, w, *, m, n, bits, q_format, r=None, L_codes=None,
                        R_codes=None) -> LinearDequantArgs:
    """cq_linear_dequant_args for inference-layout codes (m, row bytes) uint8, L (m, r) / R (r, n) fp16
    or L_codes / R_codes = (uint8 inference-layout codes, scale, bits in {2, 4}) as `linear_packed_args`
    takes them (the fp16 operand of a coded factor is None; r is needed when both are coded), and
    w (m, n) fp32 / fp16 / bf16; L, R and w may be views with a row stride (unit column stride).  The
    packed and codebook builders' host-side checks."""
    need = _linear_need
    _check_q_format(q_format, qscale)
    r = _resolve_rank(L, R, L_codes, R_codes, r)
    fp16 = _fp16_factors(L, R, r, L_codes is not None, R_codes is not None)
    for name, t in (("codes", codes), ("w", w)) + fp16:
        need(t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1), f"{name} must be a matrix with unit column stride")
    need(codes.dtype == torch.uint8 and codes.shape[0] == m, "codes must be uint8 with one row per output")
    need(tuple(w.shape) == (m, n), f"w {tuple(w.shape)} does not fit {(m, n)}")
    need(w.dtype in _ACT_DT, f"w must be fp32, fp16 or bf16, got {w.dtype}")
    _check_fp16_factors(fp16, m, r, n)
    a = LinearDequantArgs()
    a.m, a.n, a.r = m, n, r
    a.bits, a.q_format = bits, int(q_format)
    a.codes, a.code_stride = codes.data_ptr(), codes.stride(0)
    a.qscale, a.gscale = float(qscale), float(gscale)
    for name, t in fp16:
        setattr(a, name, t.data_ptr())
        setattr(a, "ld" + name.lower(), t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))
    _fill_factor_codes(a, L_codes, R_codes, m, r)
    a.w, a.w_dtype = w.data_ptr(), _ACT_DT[w.dtype]
    a.ldw = w.stride(0) if m > 1 else max(w.stride(0), n)
    return a


def linear_dequant(codes, qscale, gscale, L, R, w, *, m, n, bits, q_format, r=None, L_codes=None, R_codes=None):
    """w = gs (Q + L R), the dense weight of a packed layer (cq_linear_dequant); operands as
    `linear_dequant_args`.  No workspace, no host synchronisation."""
    _require_hip(codes, L, R, w, *_factor_code_tensors(L_codes, R_codes))
    a = linear_dequant_args(codes, qscale, gscale, L, R, w, m=m, n=n, bits=bits, q_format=q_format, r=r,
                            L_codes=L_codes, R_codes=R_codes)
    _check(load().cq_linear_dequant(ctypes.byref(a), _stream(w.device)), "cq_linear_dequant")
    return w


# ---------------------------------------------------------------------------- Hadamard transform
HADAMARD_MAX_N = 32768      # include/caldera_hip.h CQ_HADAMARD_MAX_N
HADAMARD_GROUP_MAX = 8      # CQ_HADAMARD_GROUP_MAX
HADAMARD_GLU_MAX_N = 16384  # CQ_HADAMARD_GLU_MAX_N

# The six builders below (rows, group, glu; unsigned and signed) are made of the four pieces that follow, and
# every piece raises in the name `who` of the entry it is building for: a signed entry, or a group's
# "<entry>: member i", passes its own name down instead of rewriting the callee's message.


def _hadamard_operand(a, who, name, t, cols, first):
    """One activation operand of a transform, `t` called `name`: a (rows, cols) fp16 / bf16 / fp32 matrix with
    unit column stride and the row count of the call's first operand, `first` = (its name, the tensor).
    Fills a.<name>, a.<name>_dtype and a.ld<name>; a single row may have any stride, so its leading dimension
    is raised to cols (the C entries refuse a smaller one)."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{who}: {name} must be a matrix with unit column stride")
    dtype = _ACT_DT.get(t.dtype)
    if dtype is None:
        raise ValueError(f"{who}: {name} must be fp16, bf16 or fp32, got {t.dtype}")
    rows, width = t.shape
    if width != cols:
        raise ValueError(f"{who}: {name} {tuple(t.shape)} does not have {cols} columns")
    if rows != first[1].shape[0]:
        raise ValueError(f"{who}: {first[0]} {tuple(first[1].shape)} and {name} {tuple(t.shape)} differ in rows")
    setattr(a, name, t.data_ptr())
    setattr(a, name + "_dtype", dtype)
    setattr(a, "ld" + name, t.stride(0) if rows > 1 else max(t.stride(0), cols))


def _hadamard_extents(a, who, rows, n_in, n_out, P, max_P):
    """a.rows, a.n_in, a.n_out, a.P of a transform of length P, a power of two up to max_P."""
    P = int(P)
    if not 1 <= P <= max_P or P & (P - 1):
        raise ValueError(f"{who}: P = {P} is not a power of two in [1, {max_P}]")
    if not (1 <= n_in <= P and 0 <= n_out <= P):
        raise ValueError(f"{who}: n_in = {n_in} / n_out = {n_out} do not fit P = {P}")
    a.rows, a.n_in, a.n_out, a.P = rows, n_in, n_out, P


def _hadamard_bias(a, who, name, bias, n_out):
    """a.<name> of a contiguous fp32 (n_out,) bias; None leaves the struct's NULL."""
    if bias is not None:
        if bias.dtype != torch.float32 or tuple(bias.shape) != (n_out,) or not bias.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous fp32 ({n_out},) vector, got {bias.dtype} "
                             f"{tuple(bias.shape)}")
        setattr(a, name, bias.data_ptr())


def _hadamard_sign(s, who, name, sign, length, device):
    """s.<name> of the int8 sign vector `sign` (at least `length` entries, contiguous, on `device`); None
    leaves the struct's NULL."""
    if sign is None:
        return
    if not isinstance(sign, torch.Tensor) or sign.dtype != torch.int8:
        raise ValueError(f"{who}: {name} must be an int8 tensor, got {getattr(sign, 'dtype', type(sign).__name__)}")
    if sign.dim() != 1 or not sign.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous vector, got shape {tuple(sign.shape)}")
    if sign.numel() < length:
        raise ValueError(f"{who}: {name} has {sign.numel()} entries, fewer than the {length} the transform reads")
    if sign.device != device:
        raise ValueError(f"{who}: {name} is on {sign.device}, the transform's operands on {device}")
    setattr(s, name, sign.data_ptr())


def _hadamard_group(who, members, member_args, Member, Group):
    """The group struct `Group` over an array of 1 .. HADAMARD_GROUP_MAX `Member` structs.  member_args(mem, into,
    who) fills one member from its dict, in the name "<who>: member i", and returns its cq_hadamard_args; the
    members must share the row count and P.  The struct keeps the member array alive."""
    members = list(members)
    if not 1 <= len(members) <= HADAMARD_GROUP_MAX:
        raise ValueError(f"{who}: count {len(members)} not in 1 .. {HADAMARD_GROUP_MAX}")
    arr = (Member * len(members))()
    first = None
    for i, mem in enumerate(members):
        a = member_args(mem, arr[i], f"{who}: member {i}")
        first = a if first is None else first
        for field in ("rows", "P"):
            if getattr(a, field) != getattr(first, field):
                raise ValueError(f"{who}: member {i}: {field} {getattr(a, field)} differs from member 0's "
                                 f"{getattr(first, field)}")
    g = Group()
    g.count = len(members)
    g.members = ctypes.cast(arr, ctypes.POINTER(Member))
    g._members = arr
    return g


def _hadamard_run(name, build, tensors, built_first=False):
    """The tail of the six wrappers: no CPU tensor among `tensors`, the struct from build(), the entry `name`
    on the stream of the first tensor's device.  The unsigned wrappers look at the device before they build the
    struct; the signed ones build first (built_first), so a wrong sign vector is reported before a CPU tensor."""
    if not built_first:
        _require_hip(*tensors)
    a = build()
    if built_first:
        _require_hip(*tensors)
    _check(getattr(load(), name)(ctypes.byref(a), _stream(tensors[0].device)), name)


def hadamard_args(x, y, *, n_in, n_out, P, bias=None, into=None, who="cq_hadamard_rows") -> HadamardArgs:
    """cq_hadamard_args for x (rows, n_in) and y (rows, n_out), each fp16 / bf16 / fp32 and
    possibly a view with a row stride (unit column stride), bias (n_out,) fp32 or None.  into: the
    (zeroed) struct to fill, e.g. an element of a member array.  who: the entry the checks speak for."""
    a = HadamardArgs() if into is None else into
    _hadamard_operand(a, who, "x", x, n_in, ("x", x))
    _hadamard_operand(a, who, "y", y, n_out, ("x", x))
    _hadamard_extents(a, who, x.shape[0], n_in, n_out, P, HADAMARD_MAX_N)
    _hadamard_bias(a, who, "bias", bias, n_out)
    return a


def hadamard_rows(x, y, *, n_in, n_out, P, bias=None):
    """y[t, :n_out] = (H_P pad(x[t, :n_in]))[:n_out] / sqrt(P) (+ bias): the normalised
    Sylvester-Hadamard transform of every row (cq_hadamard_rows).  x and y must not overlap.
    No workspace, no host synchronisation."""
    _hadamard_run("cq_hadamard_rows", lambda: hadamard_args(x, y, n_in=n_in, n_out=n_out, P=P, bias=bias), (x, y, bias))
    return y


def hadamard_group_args(members) -> HadamardGroupArgs:
    """cq_hadamard_group_args of 1 .. HADAMARD_GROUP_MAX transforms.  members: one dict per transform with
    `hadamard_args`' arguments as keys (x, y, n_in, n_out, P and optionally bias).  Each member passes
    `hadamard_args`' host-side checks; the members must share the row count and P.  The struct keeps
    the member array alive."""
    def member_args(mem, into, who):
        return hadamard_args(mem["x"], mem["y"], n_in=mem["n_in"], n_out=mem["n_out"], P=mem["P"], bias=mem.get("bias"),
                             into=into, who=who)
    return _hadamard_group("cq_hadamard_group_rows", members, member_args, HadamardArgs, HadamardGroupArgs)


def hadamard_group_rows(members):
    """The transforms `members` (see `hadamard_group_args`) in one launch (cq_hadamard_group_rows): each
    member's y receives, bit for bit, what `hadamard_rows` writes on the same arguments.  No member's y
    may overlap an x or another y.  No workspace, no host synchronisation."""
    members = list(members)
    _hadamard_run("cq_hadamard_group_rows", lambda: hadamard_group_args(members),
                  [t for mem in members for t in (mem["x"], mem["y"], mem.get("bias"))])
    return [mem["y"] for mem in members]


def hadamard_glu_args(g, u, h, *, n_in, n_out, P, bias_g=None, bias_u=None, act=ACT_SILU, into=None,
                      who="cq_hadamard_glu_rows") -> HadamardGluArgs:
    """cq_hadamard_glu_args for g and u (rows, n_in) and h (rows, n_out), each fp16 / bf16 / fp32 and
    possibly a view with a row stride (unit column stride); bias_g / bias_u (n_out,) fp32 or None.  into: the
    (zeroed) struct to fill.  who: the entry the checks speak for."""
    if act not in (ACT_IDENTITY, ACT_SILU):
        raise ValueError(f"{who}: unknown act {act!r}")
    a = HadamardGluArgs() if into is None else into
    for name, t, cols in (("g", g, n_in), ("u", u, n_in), ("h", h, n_out)):
        _hadamard_operand(a, who, name, t, cols, ("g", g))
    _hadamard_extents(a, who, g.shape[0], n_in, n_out, P, HADAMARD_GLU_MAX_N)
    _hadamard_bias(a, who, "bias_g", bias_g, n_out)
    _hadamard_bias(a, who, "bias_u", bias_u, n_out)
    a.act = int(act)
    return a


def hadamard_glu_rows(g, u, h, *, n_in, n_out, P, bias_g=None, bias_u=None, act=ACT_SILU):
    """h[t, :n_out] = a(H g[t] / sqrt(P) + bias_g) * (H u[t] / sqrt(P) + bias_u) (cq_hadamard_glu_rows): the
    two pre-activations have the bits of `hadamard_rows`' fp32 outputs and are never written; a is the
    identity or silu, h is rounded once.  P <= HADAMARD_GLU_MAX_N.  h must not overlap g or u.  No
    workspace, no host synchronisation."""
    _hadamard_run("cq_hadamard_glu_rows",
                  lambda: hadamard_glu_args(g, u, h, n_in=n_in, n_out=n_out, P=P, bias_g=bias_g, bias_u=bias_u, act=act),
                  (g, u, h, bias_g, bias_u))
    return h


# ---------------------------------------------------------------------------- randomised Hadamard transform
def hadamard_signed_args(x, y, *, n_in, n_out, P, bias=None, sign_in=None, sign_out=None, into=None,
                         who="cq_hadamard_signed_rows") -> HadamardSignedArgs:
    """cq_hadamard_signed_args: `hadamard_args`' operands and checks, and sign_in (>= n_in,) / sign_out
    (>= n_out,): contiguous int8 vectors on x's device, or None.  An entry flips its element iff it is
    negative."""
    s = HadamardSignedArgs() if into is None else into
    hadamard_args(x, y, n_in=n_in, n_out=n_out, P=P, bias=bias, into=s.a, who=who)
    _hadamard_sign(s, who, "sign_in", sign_in, n_in, x.device)
    _hadamard_sign(s, who, "sign_out", sign_out, n_out, x.device)
    return s


def hadamard_signed_rows(x, y, *, n_in, n_out, P, bias=None, sign_in=None, sign_out=None):
    """y[t, :n_out] = sign_out * (H_P pad(sign_in * x[t, :n_in]))[:n_out] / sqrt(P) (+ bias): the randomised
    Hadamard transform of every row (cq_hadamard_signed_rows).  Both flips are exact; with both vectors
    None the bits are `hadamard_rows`'.  x and y must not overlap.  No workspace, no host synchronisation."""
    _hadamard_run("cq_hadamard_signed_rows",
                  lambda: hadamard_signed_args(x, y, n_in=n_in, n_out=n_out, P=P, bias=bias, sign_in=sign_in,
                                               sign_out=sign_out),
                  (x, y, bias, sign_in, sign_out), built_first=True)
    return y


def hadamard_signed_group_args(members) -> HadamardSignedGroupArgs:
    """cq_hadamard_signed_group_args of 1 .. HADAMARD_GROUP_MAX transforms.  members: one dict per transform
    with `hadamard_signed_args`' arguments as keys (x, y, n_in, n_out, P and optionally bias, sign_in,
    sign_out); `hadamard_group_args`' rules.  The struct keeps the member array alive."""
    def member_args(mem, into, who):
        return hadamard_signed_args(mem["x"], mem["y"], n_in=mem["n_in"], n_out=mem["n_out"], P=mem["P"],
                                    bias=mem.get("bias"), sign_in=mem.get("sign_in"), sign_out=mem.get("sign_out"),
                                    into=into, who=who).a
    return _hadamard_group("cq_hadamard_signed_group_rows", members, member_args, HadamardSignedArgs,
                           HadamardSignedGroupArgs)


def hadamard_signed_group_rows(members):
    """The signed transforms `members` (see `hadamard_signed_group_args`) in one launch
    (cq_hadamard_signed_group_rows): each member's y receives, bit for bit, what `hadamard_signed_rows`
    writes on the same arguments.  No member's y may overlap an x or another y."""
    members = list(members)
    _hadamard_run("cq_hadamard_signed_group_rows", lambda: hadamard_signed_group_args(members),
                  [t for mem in members for t in (mem["x"], mem["y"], mem.get("bias"), mem.get("sign_in"),
                                                  mem.get("sign_out"))], built_first=True)
    return [mem["y"] for mem in members]


def hadamard_signed_glu_args(g, u, h, *, n_in, n_out, P, bias_g=None, bias_u=None, act=ACT_SILU, sign_g=None,
                             sign_u=None) -> HadamardSignedGluArgs:
    """cq_hadamard_signed_glu_args: `hadamard_glu_args`' operands and checks, and sign_g / sign_u (>= n_out,):
    contiguous int8 vectors on g's device, or None."""
    who = "cq_hadamard_signed_glu_rows"
    s = HadamardSignedGluArgs()
    hadamard_glu_args(g, u, h, n_in=n_in, n_out=n_out, P=P, bias_g=bias_g, bias_u=bias_u, act=act, into=s.a, who=who)
    _hadamard_sign(s, who, "sign_g", sign_g, n_out, g.device)
    _hadamard_sign(s, who, "sign_u", sign_u, n_out, g.device)
    return s


def hadamard_signed_glu_rows(g, u, h, *, n_in, n_out, P, bias_g=None, bias_u=None, act=ACT_SILU, sign_g=None,
                             sign_u=None):
    """`hadamard_glu_rows` with output signs: h = a(sign_g * (H g / sqrt(P)) + bias_g) * (sign_u * (H u / sqrt(P))
    + bias_u) (cq_hadamard_signed_glu_rows); the pre-activations have the bits of `hadamard_signed_rows`' fp32
    outputs with sign_out = sign_g resp. sign_u.  With both None the bits are `hadamard_glu_rows`'."""
    _hadamard_run("cq_hadamard_signed_glu_rows",
                  lambda: hadamard_signed_glu_args(g, u, h, n_in=n_in, n_out=n_out, P=P, bias_g=bias_g, bias_u=bias_u,
                                                   act=act, sign_g=sign_g, sign_u=sign_u),
                  (g, u, h, bias_g, bias_u, sign_g, sign_u), built_first=True)
    return h
