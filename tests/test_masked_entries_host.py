"""The masked entries (include/caldera_hip.h) agree across the header, the ctypes table and the
library: each is exported, declared in _lib.py, and takes its unmasked entry's arguments plus
the one `active` pointer.  No device calls."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "caldera_hip.h")

# masked entry -> the entry it extends
MASKED = {
    "cq_gram_f64_masked": "cq_gram_f64",
    "cq_spd_whiten_masked": "cq_spd_whiten_rcond",
    "cq_jacobi_eigh_masked": "cq_jacobi_eigh",
    "cq_jacobi_eigh_staged_masked": "cq_jacobi_eigh_staged",
    "cq_extreme_eigs_masked": "cq_extreme_eigs",
    "cq_ritz_residual_masked": "cq_ritz_residual",
    "cq_ritz_product_error_masked": "cq_ritz_product_error",
    "cq_gemm_f32_masked": "cq_gemm_f32",
    "cq_gemm_triu_split_masked": "cq_gemm_triu_split",
    "cq_transpose_split_masked": "cq_transpose_split",
}


def prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\b(cq_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


def test_masked_entries_in_header_ctypes_and_library():
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    lib = K.load()
    protos = prototypes()
    for name, base in MASKED.items():
        assert name in protos and base in protos, name
        assert hasattr(lib, name), name
        assert name in K._SIGS, name
        args, bargs = protos[name], protos[base]
        # the unmasked prototype with `const int* active` inserted, nothing else moved
        extra = [a for a in args if a not in bargs]
        assert extra == ["const int* active"], (name, extra)
        assert [a for a in args if a != "const int* active"] == bargs, name
        res, cargs = K._SIGS[name]
        bres, bcargs = K._SIGS[base]
        assert res is bres and len(cargs) == len(bcargs) + 1 == len(args), name
        i = args.index("const int* active")
        assert cargs[i] is K.c_vp and list(cargs[:i]) + list(cargs[i + 1:]) == list(bcargs), name
    # the skip form of the split-fp16 product: the same argument block, another entry
    assert protos["cq_gemm_x3_skip"] == protos["cq_gemm_x3"]
    assert K._SIGS["cq_gemm_x3_skip"] == K._SIGS["cq_gemm_x3"] and hasattr(lib, "cq_gemm_x3_skip")
    assert lib.cq_abi_version() == 5   # additive: the ABI version stays


def test_solver_switch_and_counters():
    from ee274_convexcaldera_llm_quantization_amd import solver as S
    assert S.SKIP_FROZEN is True
    d = S.SolverStats().as_dict()
    assert d["frozen_iters"] == 0 and d["frozen_matrices"] == 0
