"""CPU side of the materialise kernel and the dense-GEMM path (cq_linear_dequant,
CalderaLinear.materialize / dense_prefill_tokens, model.set_dense_prefill / unpack_packed_layers):
that the cases of linear_dequant_cases.py are exact where they claim to be and can see the planted
faults, the C ABI and its argument checks without a device, and the layer and model surface's
validation."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import linear_dequant_cases as DC
from linear_dequant_cases import f32, f64
from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import model as M
from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear, HadamardCalderaLinear, row_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "caldera_hip.h")
CSRC = os.path.join(ROOT, "ee274_convexcaldera_llm_quantization_amd", "csrc")


# ---------------------------------------------------------------------------- the cases
def test_the_issues_cases_are_all_there():
    for kind in (DC.EXACT, DC.RANDOM):
        for (m, n, r) in DC.FULL_SHAPES:
            got = {(c.fmt, c.bits, c.lb, c.rb) for c in kind if (c.m, c.n, c.r) == (m, n, r)}
            assert got == {(f, b, lb, rb) for (f, b) in DC.QFORMATS for lb in (16, 4, 2) for rb in (16, 4, 2)}
        for (m, n, r) in ((12, 198, 5), (130, 520, 72), DC.PAST_TILE):
            got = {(c.fmt, c.bits, c.lb, c.rb) for c in kind if (c.m, c.n, c.r) == (m, n, r)}
            assert got == {(f, b, lb, rb) for (f, b) in DC.QFORMATS for (lb, rb) in ((16, 16), (4, 4), (2, 16))}
        assert {(c.fmt, c.bits) for c in kind if (c.m, c.n, c.r) == (1, 8, 0)} == set(DC.QFORMATS)
    assert DC.FULL_SHAPES == ((48, 198, 40), (160, 256, 128))
    assert len({c.id for c in DC.ALL}) == len(DC.ALL)
    assert [(c.m, c.n, c.r, c.fmt, c.bits, c.lb, c.rb) for c in DC.RANDOM] == \
        [(c.m, c.n, c.r, c.fmt, c.bits, c.lb, c.rb) for c in DC.EXACT]


def test_tile_constants_are_the_kernels():
    """TILE, CHUNK_ROWS and PAST_TILE follow csrc/cq_linear_dequant.hip and cq_linear_tile.h."""
    src = open(os.path.join(CSRC, "cq_linear_dequant.hip")).read()
    tile = open(os.path.join(CSRC, "cq_linear_tile.h")).read()
    waves = int(re.search(r"constexpr int kWaves = (\d+);", src).group(1))
    rt = int(re.search(r"constexpr int kRT = (\d+);", src).group(1))
    blocks = int(re.search(r"constexpr int kBlocks = (\d+);", tile).group(1))
    rows = int(re.search(r"constexpr int kChunkRows = (\d+);", tile).group(1))
    assert DC.TILE == (waves * rt * 16, blocks * 16) and DC.CHUNK_ROWS == rows
    m, n, _ = DC.PAST_TILE
    assert m > 2 * DC.TILE[0] and n > DC.TILE[1]
    assert any(c.m > DC.TILE[0] and c.n > 2 * DC.TILE[1] and c.r > 2 * rows and c.r % rows for c in DC.ALL)
    # the level tables are cq_nf.h's: the kernel holds no copy
    assert "8165" not in src and "1334" not in src and "cq_nf.h" in tile and "expand_nf" in src


@pytest.mark.parametrize("shape", DC.FULL_SHAPES + DC.OTHER_SHAPES, ids=lambda s: "m%dn%dr%d" % s)
def test_exact_references_are_exact_in_fp32(shape):
    """qs = 0.5, fscale in {1, 2, 4}, gs = 4; the integer factor sum, fscale * sum, 0.5 V + that and
    4 times that are all fp32 values, in any operation order.  Every format of the shape."""
    cases = [c for c in DC.EXACT if (c.m, c.n, c.r) == shape]
    assert len(cases) in (4, 12, 36)
    for case in cases:
        _check_exact(case)


def _check_exact(case):
    d = DC.inputs(case)
    qs, z = DC.scales(case)
    assert qs == f32(0.5) and d["gs"] == f32(4.0)
    coded = [b for b in (case.lb, case.rb) if b != 16]
    assert z == f32(2.0 ** len(coded) if case.r else 1.0)
    for key, bits in (("l", case.lb), ("rho", case.rb)):
        v = d[key].astype(f64)
        assert np.array_equal(np.round(v), v)                              # integer-valued, fp16 no-op
        assert np.abs(v).max(initial=0) <= (2 if bits == 16 else 2 ** (bits - 1) - 1)
    units, smax = DC.exact_units(case)
    assert units < 2 ** 24 and 4 * smax < 2 ** 24
    w, _ = DC.reference(case)
    assert np.array_equal(w.astype(f32).astype(f64), w) and np.array_equal(np.round(w), w)


# one test per fault, every case it applies to inside: a test per (case, fault) pair would be ~1800 ids
@pytest.mark.parametrize("fault", DC.FAULTS)
def test_planted_fault_changes_every_exact_case(fault):
    cases = [c for c in DC.EXACT if DC.fault_applies(c, fault)]
    assert cases
    for case in cases:
        w, _ = DC.reference(case)
        bad, _ = DC.reference(case, fault)
        assert not np.array_equal(w, bad), case.id


@pytest.mark.parametrize("fault", DC.RANDOM_FAULTS)
def test_planted_fault_exceeds_ten_bars_on_random_cases(fault):
    cases = [c for c in DC.RANDOM if DC.fault_applies(c, fault)]
    assert cases
    for case in cases:
        w, bar = DC.reference(case)
        bad, _ = DC.reference(case, fault)
        ok = bar > 0
        assert (np.abs(bad - w)[ok] / bar[ok]).max() >= 10.0, case.id


def test_every_fault_meets_exact_and_random_cases():
    assert len(DC.FAULTS) == 10 and set(DC.RANDOM_FAULTS) <= set(DC.FAULTS)
    for fault in DC.FAULTS:
        for (fmt, bits) in DC.QFORMATS:
            if fault == "s_for_sk" and (fmt, bits) == (DC.UNIFORM, 2):
                continue
            assert any(DC.fault_applies(c, fault) for c in DC.EXACT if (c.fmt, c.bits) == (fmt, bits)), fault
            assert any(DC.fault_applies(c, fault) for c in DC.RANDOM if (c.fmt, c.bits) == (fmt, bits)), fault
    assert any(DC.fault_applies(c, "drop_last_chunk") and c.r == 72 for c in DC.ALL)


def test_operands_are_the_inference_layout():
    for case in DC.EXACT[:40:7]:
        codes = DC.q_operand(case)
        assert codes.dtype == np.uint8 and codes.shape == (case.m, row_bytes(case.n, case.bits))
        for which, rows, cols in (("l", case.m, case.r), ("rho", case.r, case.n)):
            op = DC.factor_operand(case, which)
            if op[0] == "codes":
                assert op[1].shape == (rows, row_bytes(cols, op[3]))


# ---------------------------------------------------------------------------- the ABI
def _struct_fields(name):
    txt = open(HEADER).read()
    body = txt[txt.index(f"typedef struct {name}"):txt.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*[;,]", body.split("{", 1)[1])


def test_dequant_abi_is_additive():
    txt = open(HEADER).read()
    assert int(re.search(r"#define CQ_ABI_VERSION (\d+)", txt).group(1)) == K.ABI_VERSION == 5
    assert "cq_linear_dequant" in K.EXPORTS
    lib = K.load()                      # raises for a missing export
    assert lib.cq_abi_version() == 5 and lib.cq_linear_dequant is not None
    fields = [f for f, _ in K.LinearDequantArgs._fields_]
    assert fields == _struct_fields("cq_linear_dequant_args")
    assert fields == ["m", "n", "r", "bits", "q_format", "codes", "code_stride", "qscale", "gscale", "L", "ldl", "R",
                      "ldr", "l_bits", "r_bits", "L_codes", "l_code_stride", "R_codes", "r_code_stride", "lscale",
                      "rscale", "w", "w_dtype", "ldw"]
    # natural alignment, as the C compiler lays it out
    off = 0
    for name, ct in K.LinearDequantArgs._fields_:
        size = ctypes.sizeof(ct)
        off = (off + size - 1) // size * size
        assert getattr(K.LinearDequantArgs, name).offset == off, name
        off += size
    assert K.LINEAR_DECODE_MAX_TOKENS == int(re.search(r"#define CQ_LINEAR_DECODE_MAX_TOKENS (\d+)", txt).group(1))


def test_entry_rejects_bad_arguments_without_a_device():
    """Validation runs before any launch: CQ_EINVAL with a message for everything the packed and
    codebook entries reject, an unknown w_dtype and ldw < n; an empty shape returns 0."""
    lib = K.load()
    buf = torch.zeros(16384, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16

    def args(**kw):
        a = K.LinearDequantArgs()
        a.m, a.n, a.r, a.bits, a.q_format = 16, 64, 0, 4, K.QFMT_UNIFORM
        a.codes, a.code_stride, a.qscale, a.gscale = base + 256, 32, 1.0, 1.0
        a.l_bits = a.r_bits = 16
        a.w, a.w_dtype, a.ldw = base + 1024, K.CQ_F32, 64
        for key, v in kw.items():
            setattr(a, key, v)
        return a

    ranked = dict(r=8, L=base + 8192, ldl=8, R=base + 9216, ldr=64)
    lcoded = dict(r=8, l_bits=4, L_codes=base + 8192, l_code_stride=16, lscale=1.0, R=base + 9216, ldr=64)
    rcoded = dict(r=8, r_bits=2, R_codes=base + 9216, r_code_stride=16, rscale=1.0, L=base + 8192, ldl=8)
    bad = ((dict(q_format=2), "q_format"), (dict(q_format=-1), "q_format"), (dict(bits=3), "bits"),
           (dict(bits=8), "bits"), (dict(r=K.LINEAR_MAX_RANK + 1), "rank"), (dict(codes=base + 260), "aligned"),
           (dict(code_stride=17), "aligned"), (dict(code_stride=16), "stride"), (dict(l_bits=3), "factor bits"),
           (dict(r_bits=8), "factor bits"), (dict(q_format=K.QFMT_NF, qscale=float("nan")), "scale"),
           (dict(q_format=K.QFMT_NF, qscale=-1.0), "scale"), (dict(w_dtype=3), "dtype"), (dict(w_dtype=-1), "dtype"),
           (dict(ldw=63), "ldw"), (dict(m=-1), "shape"), (dict(n=-2), "shape"), (dict(r=-1), "shape"),
           (dict(codes=None), "null"), (dict(w=None), "null"), (dict(w=base + 1026), "misaligned"),
           (dict(w=base + 1025, w_dtype=K.CQ_BF16), "misaligned"), (dict(r=8), "null L / R"),
           (dict(ranked, L=base + 8193), "misaligned"), (dict(ranked, ldl=7), "leading dimension"),
           (dict(ranked, ldr=63), "leading dimension"), (dict(lcoded, L_codes=None), "null L codes"),
           (dict(lcoded, L_codes=base + 8196), "aligned"), (dict(lcoded, l_code_stride=24), "aligned"),
           (dict(lcoded, r=40), "stride"), (dict(lcoded, lscale=float("inf")), "scale"),
           (dict(rcoded, rscale=-0.5), "scale"), (dict(rcoded, r_code_stride=0), "stride"))
    for kw, word in bad:
        assert lib.cq_linear_dequant(ctypes.byref(args(**kw)), None) == K.CQ_EINVAL, kw
        assert word in lib.cq_last_error().decode(), (kw, lib.cq_last_error())
    assert lib.cq_linear_dequant(None, None) == K.CQ_EINVAL
    # nothing to write: 0 without a launch (and without looking at the pointers)
    for kw in (dict(m=0), dict(n=0, ldw=0), dict(m=0, codes=None, w=None)):
        assert lib.cq_linear_dequant(ctypes.byref(args(**kw)), None) == 0, kw
    # ... but a bad format is still one
    assert lib.cq_linear_dequant(ctypes.byref(args(m=0, bits=5)), None) == K.CQ_EINVAL


def test_args_builder_checks_like_the_packed_ones():
    codes = torch.zeros(12, row_bytes(198, 4), dtype=torch.uint8)
    L, R = torch.zeros(12, 5, dtype=torch.float16), torch.zeros(5, 198, dtype=torch.float16)
    w = torch.zeros(12, 198, dtype=torch.float16)
    ok = dict(codes=codes, qscale=1.0, L=L, R=R, w=w, q_format=K.QFMT_NF, r=None, L_codes=None, R_codes=None)

    def build(**kw):
        o = dict(ok)
        o.update(kw)
        return K.linear_dequant_args(o["codes"], o["qscale"], 1.0, o["L"], o["R"], o["w"], m=12, n=198, bits=4,
                                     q_format=o["q_format"], r=o["r"], L_codes=o["L_codes"], R_codes=o["R_codes"])

    a = build()
    assert (a.q_format, a.bits, a.r, a.l_bits, a.r_bits, a.code_stride) == (K.QFMT_NF, 4, 5, 16, 16, row_bytes(198, 4))
    assert (a.m, a.n, a.ldl, a.ldr, a.ldw, a.w_dtype) == (12, 198, 5, 198, 198, K.CQ_F16)
    assert build(w=torch.zeros(12, 198, dtype=torch.bfloat16)).w_dtype == K.CQ_BF16
    view = torch.zeros(12, 203)[:, 2:200]
    a = build(w=view)
    assert (a.ldw, a.w_dtype, a.w) == (203, K.CQ_F32, view.data_ptr())
    Lc = (torch.zeros(12, 16, dtype=torch.uint8), 0.3, 4)
    Rc = (torch.zeros(5, row_bytes(198, 2), dtype=torch.uint8), 0.2, 2)
    a = build(L=None, R=None, L_codes=Lc, R_codes=Rc, r=5)
    assert (a.r, a.l_bits, a.r_bits, a.l_code_stride, a.r_code_stride) == (5, 4, 2, 16, row_bytes(198, 2))
    assert (a.lscale, a.rscale) == (f32(0.3), f32(0.2)) and a.L is None and a.R is None
    assert build(L=None, R=None).r == 0
    for kw, word in ((dict(q_format=7), "q_format"), (dict(qscale=float("inf")), "NF scale"),
                     (dict(qscale=-0.5), "NF scale"), (dict(L=L.float()), "fp16"), (dict(R=R[:4]), "do not fit"),
                     (dict(w=w.double()), "w must be"), (dict(w=w[:, :100]), "does not fit"),
                     (dict(w=torch.zeros(198, 12, dtype=torch.float16).t()), "unit column stride"),
                     (dict(codes=codes[:5]), "codes"), (dict(codes=codes.to(torch.int8)), "codes"),
                     (dict(L=None, R=None, L_codes=Lc, R_codes=Rc), "r is needed"),
                     (dict(L_codes=Lc), "exactly one of L"), (dict(R=None), "exactly one of R"),
                     (dict(R=None, R_codes=(Rc[0][:3], 0.2, 2)), "R_codes must be")):
        with pytest.raises(ValueError, match=word):
            build(**kw)
    with pytest.raises(RuntimeError, match="HIP"):
        K.linear_dequant(codes, 1.0, 1.0, L, R, w, m=12, n=198, bits=4, q_format=K.QFMT_UNIFORM)


# ---------------------------------------------------------------------------- layer and model
def _layer(m=12, n=198, r=5, bits=4, seed=0, bias=False):
    rng = np.random.default_rng(seed)
    k = 2 ** (bits - 1) - 1
    c = torch.from_numpy(rng.integers(-k, k + 1, (m, n)).astype(np.int8))
    L = torch.from_numpy((0.1 * rng.standard_normal((m, r))).astype(np.float16))
    R = torch.from_numpy((0.1 * rng.standard_normal((r, n))).astype(np.float16))
    b = torch.from_numpy(rng.standard_normal(m).astype(np.float32)) if bias else None
    return CalderaLinear.from_codes(c, L, R, b, qscale=0.05, gscale=1.7, bits=bits)


def _hadamard(seed=1):
    return HadamardCalderaLinear(_layer(16, 256, 4, seed=seed), 198, 12)


def test_dense_prefill_tokens_is_validated_and_not_state():
    lin = _layer()
    keys, extra = set(lin.state_dict()), dict(lin.get_extra_state())
    assert lin.dense_prefill_tokens is None
    for bad in (0, 1, K.LINEAR_DECODE_MAX_TOKENS, -5, 17.0, "64", True):
        with pytest.raises(ValueError, match="dense_prefill_tokens"):
            lin.dense_prefill_tokens = bad
    assert lin.dense_prefill_tokens is None
    lin.dense_prefill_tokens = K.LINEAR_DECODE_MAX_TOKENS + 1
    assert lin.dense_prefill_tokens == 17
    assert set(lin.state_dict()) == keys and lin.get_extra_state() == extra
    assert "dense_prefill_tokens" not in extra and not any("dense" in k for k in keys)
    other = _layer(seed=3)
    other.load_state_dict(lin.state_dict())
    assert other.dense_prefill_tokens is None          # it does not travel with the state
    lin.dense_prefill_tokens = None
    assert lin.dense_prefill_tokens is None
    had = _hadamard()
    hkeys, hextra = set(had.state_dict()), dict(had.get_extra_state())
    had.dense_prefill_tokens = 64
    assert had.inner.dense_prefill_tokens == had.dense_prefill_tokens == 64
    assert set(had.state_dict()) == hkeys and had.get_extra_state() == hextra
    with pytest.raises(ValueError, match="dense_prefill_tokens"):
        had.dense_prefill_tokens = 16


def test_materialize_needs_device_tensors():
    lin, had = _layer(), _hadamard()
    for layer in (lin, had):
        with pytest.raises(RuntimeError, match="HIP"):
            layer.materialize()
        with pytest.raises(RuntimeError, match="HIP"):
            layer.materialize(out=torch.zeros(12, 198, dtype=torch.float16))
    # the dense path has no CPU fallback either
    lin.dense_prefill_tokens = 17
    with pytest.raises(RuntimeError, match="HIP"):
        lin(torch.zeros(32, 198))


def test_set_dense_prefill_names_every_packed_layer():
    net = torch.nn.Sequential(_layer(), torch.nn.ReLU(), torch.nn.Linear(12, 198), _hadamard())
    assert M.set_dense_prefill(net, 128) == ["0", "3"]
    assert net[0].dense_prefill_tokens == net[3].inner.dense_prefill_tokens == 128
    with pytest.raises(ValueError, match="dense_prefill_tokens"):
        M.set_dense_prefill(net, 8)
    assert net[0].dense_prefill_tokens == 128             # nothing changed
    assert M.set_dense_prefill(net, None) == ["0", "3"]
    assert net[0].dense_prefill_tokens is None and net[3].dense_prefill_tokens is None
    assert M.set_dense_prefill(torch.nn.Linear(4, 4), 64) == []


def test_unpack_packed_layers_refuses_trainable_factors():
    net = torch.nn.Sequential(_layer(), _hadamard())
    net[1].enable_factor_training()
    with pytest.raises(ValueError, match="finish_factor_finetuning") as e:
        M.unpack_packed_layers(net)
    assert "1" in str(e.value) and isinstance(net[0], CalderaLinear)      # before anything is changed
    net[0].enable_factor_training()
    M.finish_factor_finetuning(net)
    with pytest.raises(RuntimeError, match="HIP"):                       # past the refusal: no CPU path
        M.unpack_packed_layers(net)
    with pytest.raises(ValueError, match="nothing to replace"):
        M.unpack_packed_layers(_layer())
