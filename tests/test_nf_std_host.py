"""Standardised NF4 / NF2 quantiser, host side: the numpy restatement of the kernel contract
(tests/nf_std_cases.py) against the reference's own outputs (tests/golden/nf_std_kat.npz), the
drop-in module's surface (src.caldera.utils.quantization_stable_nf4), the engine's method names and
the packed-form refusals, and the error returns of the new C entries.  No device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import nf_std_cases as C
import ee274_convexcaldera_llm_quantization_amd._lib as K
from ee274_convexcaldera_llm_quantization_amd import model as M
from ee274_convexcaldera_llm_quantization_amd import qlog
from ee274_convexcaldera_llm_quantization_amd.engine import CalderaEngine, EngineParams
from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
from ee274_convexcaldera_llm_quantization_amd.src.caldera.utils import quantization as QA
from ee274_convexcaldera_llm_quantization_amd.src.caldera.utils import quantization_stable_nf4 as QS
from ee274_convexcaldera_llm_quantization_amd.src.caldera.utils.dataclasses import CalderaDecomposition, CalderaParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "caldera_hip.h")
f32, f64 = np.float32, np.float64


bits_of = C.bits_of


@pytest.fixture(scope="module")
def fx():
    return C.fixture()


@pytest.fixture(scope="module")
def inputs():
    return C.kat_inputs()


# ---------------------------------------------------------------------------- restatement vs reference
def test_restatement_against_reference(fx, inputs):
    """All 24 quantiser cases of the fixture (one test: the cases share the inputs and the file)."""
    cases = C.kat_cases()
    assert len(cases) == 24
    for key, name, method, bits, bs in cases:
        x = inputs[name]
        same = C.compare_with_fixture(C.quantize(x, bits, bs), fx, key, x, bits, bs)
        if bs == 64:
            assert same, key       # every block-64 mean has the reference's bits


def test_fixture_covers_every_kat_input_and_the_end_to_end_runs(fx, inputs):
    assert set(inputs) == {"ties", "zeros", "rand", "wide", "outl", "odd"}
    assert len(C.kat_cases()) == 24
    whole_same = sum(np.array_equal(bits_of(C.quantize(inputs[n], b, bs)["mean"]), bits_of(fx[k + "_mean"]))
                     for k, n, _, b, bs in C.kat_cases() if bs != 64)
    assert whole_same >= 7      # most whole-matrix means have the reference's bits too
    assert fx["W"].dtype == np.float16 and fx["W"].shape == (128, 256)
    for tag in "abc":
        assert fx[tag + "_QLR"].dtype == f32 and fx[tag + "_QLR"].shape == (128, 256)
        assert fx[tag + "_errors_Q"].shape == fx[tag + "_errors_LR"].shape == (2,)


def test_restatement_numbers():
    """The contract's own arithmetic on hand-made blocks."""
    x = np.array([[1.0, 2.0, 3.0, 6.0]], f32)
    q = C.quantize(x, 2, 4)
    assert q["mean"][0, 0] == f32(3.0) and q["std"][0, 0] == f32(np.sqrt(14.0 / 3.0))
    assert q["idx"].tolist() == [[0, 1, 1, 3]]                     # z = 0 is not above the threshold 0
    const = C.quantize(np.full((1, 8), 0.25, f32), 4, 8)          # std floored at eps; z = 0 -> level 0.0
    assert const["std"][0, 0] == f32(1e-8) and (const["idx"] == 8).all() and (const["deq"] == f32(0.25)).all()
    t = C.thresholds(2)
    assert t[1] == 0 and t[0] == -t[2] and abs(t[2] - 0.5749) < 1e-6 and C.thresholds(4).size == 15
    with pytest.raises(AssertionError):
        C.quantize(np.ones((4, 1), f32), 4, 1)


# ---------------------------------------------------------------------------- the drop-in module
def test_module_surface_matches_the_reference():
    assert QS._QUANTIZER_METHODS == ["uniform", "nf4", "nf2"] and QS._BITWIDTHS == [2, 4, 8, 16]
    assert issubclass(QS.LowMemoryQuantizer, QS.AbstractQuantizer)
    with pytest.raises(NotImplementedError, match=r"^Quantization method 'bbint4' not supported yet\.$"):
        QS.LowMemoryQuantizer(4, "bbint4", 64)
    with pytest.raises(AssertionError, match="Bit-width not supported!"):
        QS.LowMemoryQuantizer(3, "uniform", 64)
    with pytest.raises(ValueError, match=r"^NF4 quantization supports only 4 bits\.$"):
        QS.LowMemoryQuantizer(2, "nf4", 64)
    with pytest.raises(ValueError, match=r"^NF2 quantization supports only 2 bits\.$"):
        QS.LowMemoryQuantizer(4, "nf2", 64)
    q = QS.LowMemoryQuantizer(4, "NF4", 64)
    assert (q.num_bits, q.method, q.block_size) == (4, "nf4", 64)
    with pytest.raises(ValueError, match=r"^Support only for 2D matrix, but your input has 3 dimensions\.$"):
        q.quantize_block(torch.zeros(2, 4, 8))
    with pytest.raises(ValueError, match=r"^Weight with shape 3 x 5 is not divisible by block size 64$"):
        q.quantize_block(torch.zeros(3, 5))
    with pytest.raises(ValueError, match="no unbiased std"):        # the stated deviation (reference: NaN)
        QS.LowMemoryQuantizer(4, "nf4", 1).quantize_block(torch.zeros(3, 5))
    f = QS.QuantizerFactory("nf2", 128)
    assert str(f) == "QuantizerFactory(method=nf2, block_size=128)"
    assert str(QS.QuantizerFactory()) == "QuantizerFactory(method=uniform, block_size=64)"
    got = f.get_quantizer(2, device="cpu")
    assert isinstance(got, QS.LowMemoryQuantizer) and (got.num_bits, got.method, got.block_size) == (2, "nf2", 128)
    assert QS.QuantizerFactory.nf_variant == QS.LowMemoryQuantizer.nf_variant == "standardized"
    assert not hasattr(QA.QuantizerFactory, "nf_variant")            # quantization.py is untouched
    import src.caldera.utils.quantization_stable_nf4 as by_reference_path
    assert by_reference_path.QuantizerFactory.nf_variant == "standardized"


# ---------------------------------------------------------------------------- the engine's names
def _params(fq, flr, **kw):
    return CalderaParams(update_order=["Q", "LR"], quant_factory_Q=fq, quant_factory_LR=flr, **kw)


def test_from_caldera_params_maps_q_and_lr_independently():
    S, A = QS.QuantizerFactory, QA.QuantizerFactory
    cases = [(S("nf4"), S("nf2"), "nf4_std", "nf2_std"), (S("NF2"), A("nf4"), "nf2_std", "nf4"),
             (S("nf4"), A("uniform"), "nf4_std", "uniform"), (A("nf4"), S("nf4"), "nf4", "nf4_std"),
             (S("uniform"), S("uniform"), "uniform", "uniform"), (A("bbint4"), S("nf2"), "bbint4", "nf2_std"),
             (A("nf2"), A("nf2"), "nf2", "nf2")]
    for fq, flr, mq, mlr in cases:
        p = EngineParams.from_caldera_params(_params(fq, flr))
        assert (p.method_Q, p.method_LR) == (mq, mlr)


def test_qlog_knows_the_new_names():
    assert qlog.code_bits("nf4_std", 4) == 4 and qlog.code_bits("nf2_std", 2) == 2
    assert qlog.code_bits("nf2_std", 4) == 2 and qlog.code_bits("uniform", 8) == 8
    qlog.check_method_bits("nf4_std", 4)
    qlog.check_method_bits("nf2_std", 2)
    with pytest.raises(ValueError, match=r"^NF4 quantization supports only 4 bits\.$"):
        qlog.check_method_bits("nf4_std", 2)
    with pytest.raises(ValueError, match=r"^NF2 quantization supports only 2 bits\.$"):
        qlog.check_method_bits("nf2_std", 4)
    with pytest.raises(AssertionError, match="Bit-width not supported!"):
        qlog.check_method_bits("nf4_std", 3)
    with pytest.raises(NotImplementedError, match="'nf8_std' not supported yet"):
        qlog.check_method_bits("nf8_std", 4)


def test_engine_accepts_the_new_names_and_still_refuses_ragged_columns():
    for mq, mlr, qb in (("nf4_std", "uniform", 4), ("nf2_std", "nf4", 2), ("uniform", "nf4_std", 2)):
        CalderaEngine(EngineParams(method_Q=mq, method_LR=mlr, Q_bits=qb))
    with pytest.raises(NotImplementedError, match="'nf4_standard' not supported yet"):
        CalderaEngine(EngineParams(method_Q="nf4_standard"))
    qp = _params(QS.QuantizerFactory("nf4"), QA.QuantizerFactory(), Q_bits=4, L_bits=16, R_bits=16, rank=4, iters=1)
    eng = CalderaEngine(EngineParams.from_caldera_params(qp))
    with pytest.raises(NotImplementedError, match="% 4 != 0 needs uniform quantisers"):
        eng.run(torch.zeros(1, 8, 198))


# ---------------------------------------------------------------------------- no packed form
def test_packed_layers_refuse_a_standardised_q():
    model = torch.nn.Sequential(torch.nn.Linear(64, 12))

    def never(*a):
        raise AssertionError("decomposed before the refusal")
    for method, bits in (("nf4", 4), ("nf2", 2)):
        qp = _params(QS.QuantizerFactory(method), QA.QuantizerFactory(), Q_bits=bits, L_bits=16, R_bits=16, rank=4)
        with pytest.raises(ValueError, match="no packed form"):
            M.apply_caldera_quantization(model, None, qp, packed=True, decompose=never)
        with pytest.raises(ValueError, match="no packed form"):
            M.apply_caldera_quantization(model, None, qp, packed=True, packed_hadamard=True, decompose=never)
    # a tuple Q_scale, the (mean, std) pair, never becomes a packed layer's one scale
    idx = torch.zeros(1, 12 * 64, dtype=torch.uint8)
    dec = CalderaDecomposition(Q=torch.zeros(12, 64), L=torch.zeros(12, 4), R=torch.zeros(4, 64), Q_idxs=idx,
                               Q_scale=(torch.zeros(1, 1), torch.ones(1, 1)), global_scale=1.0)
    with pytest.raises(ValueError, match="one scale"):
        CalderaLinear.from_decomposition(dec, 4, Q_method="nf4")
    with pytest.raises(ValueError, match="one scale"):
        CalderaLinear.from_decomposition(dec, 4)


# ---------------------------------------------------------------------------- the C entries
def test_abi_is_additive_and_still_5():
    txt = open(HEADER).read()
    assert int(re.search(r"#define CQ_ABI_VERSION (\d+)", txt).group(1)) == K.ABI_VERSION == 5
    new = {"cq_quantize_nf_std_workspace", "cq_quantize_nf_std", "cq_dequant_nf_std"}
    assert new <= set(K.EXPORTS)
    lib = K.load()
    assert lib.cq_abi_version() == 5
    for name in new:
        assert name + "(" in txt and getattr(lib, name) is not None


def test_entries_refuse_bad_arguments_before_any_device_call():
    lib = K.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = (ctypes.c_char * (1 << 20))()
    ws, nws = ctypes.cast(big, ctypes.c_void_p), 1 << 20

    def quant(numel=64, bs=16, bits=4, err_w=None, ncols=0, ws=ws, nws=nws, x=p, mean=p, std=p):
        return lib.cq_quantize_nf_std(x, 1, numel, bs, bits, 1e-8, None, None, mean, std, err_w, ncols, 0, None, ws, nws,
                                      None)
    need = lib.cq_quantize_nf_std_workspace(1, 64, 16)
    assert 0 < need <= nws
    for bits in (0, 1, 3, 8):
        assert quant(bits=bits) == K.CQ_EINVAL and b"bits" in lib.cq_last_error()
    assert quant(numel=64, bs=24) == K.CQ_EINVAL and b"block_size" in lib.cq_last_error()
    for bs in (1, 0, -4):
        assert quant(bs=bs) == K.CQ_EINVAL and b"block_size must be >= 2" in lib.cq_last_error()
    assert quant(err_w=p, ncols=0) == K.CQ_EINVAL and b"err_ncols" in lib.cq_last_error()
    for kw in (dict(x=None), dict(mean=None), dict(std=None)):
        assert quant(**kw) == K.CQ_EINVAL
    assert quant(ws=None) == K.CQ_EWORKSPACE
    assert quant(nws=need - 1) == K.CQ_EWORKSPACE and b"workspace too small" in lib.cq_last_error()
    idx = ctypes.cast((ctypes.c_uint8 * 64)(), ctypes.c_void_p)
    assert lib.cq_dequant_nf_std(idx, p, p, 64, 16, 3, p, None) == K.CQ_EINVAL
    assert lib.cq_dequant_nf_std(None, p, p, 64, 16, 4, p, None) == K.CQ_EINVAL
    assert lib.cq_dequant_nf_std(idx, p, None, 64, 16, 4, p, None) == K.CQ_EINVAL
    assert lib.cq_dequant_nf_std(idx, p, p, 64, 0, 4, p, None) == K.CQ_EINVAL
