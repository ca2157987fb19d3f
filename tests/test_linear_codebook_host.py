"""CPU side of the NF4 / NF2 codebook Q of the packed linear layer: that the cases of
linear_codebook_cases.py are exact where they claim to be and can see the planted faults, that the
kernel's Q = I[idx] (s / D) is the NF quantiser's level32[idx] * scale up to rounding, the index
packers, the C ABI and its argument checks, and CalderaLinear / MatrixResult round trips."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import linear_codebook_cases as CC
from linear_codebook_cases import f32, f64
from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import linear as LIN
from ee274_convexcaldera_llm_quantization_amd import model as M
from ee274_convexcaldera_llm_quantization_amd.linear import (CalderaLinear, HadamardCalderaLinear, pack_index_rows,
                                                              row_bytes, unpack_index_bytes)
from ee274_convexcaldera_llm_quantization_amd.sharding import (MatrixResult, load_results, pack_results, save_results,
                                                                unpack_results)
from ee274_convexcaldera_llm_quantization_amd.src.caldera.utils.dataclasses import CalderaDecomposition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "caldera_hip.h")
NF, UNIFORM = LIN.Q_FORMAT_NF, LIN.Q_FORMAT_UNIFORM


# ---------------------------------------------------------------------------- the cases
def test_the_issues_cases_are_all_there():
    fwd = {(c.m, c.n, c.r, c.T) for c in CC.EXACT if c.dirn == "fwd" and c.lb == c.rb == 16 and not c.bias}
    assert fwd == ({(33, 64, 8, T) for T in (1, 5)} | {(48, 198, 40, T) for T in (3, 16)}
                   | {(80, 898, 200, T) for T in (16, 17, 64)} | {(48, 198, 0, T) for T in (3, 17)}
                   | {(48, 2600, 40, T) for T in (1, 16)})
    bwd = {(c.m, c.n, c.r, c.T) for c in CC.EXACT if c.dirn == "bwd" and c.lb == c.rb == 16}
    shapes = ((33, 64, 8), (80, 898, 200), (272, 512, 16), (198, 48, 0), (160, 256, 128))
    assert bwd == ({(*s, T) for s in shapes for T in (1, 17, 64)} | {(272, 512, 16, 130), (160, 256, 128, 130)})
    for kind in (CC.EXACT, CC.RANDOM):
        for bits in (4, 2):
            mine = [c for c in kind if c.bits == bits]
            assert {(c.lb, c.rb) for c in mine} == {(16, 16), (4, 4), (2, 16)}
            assert any(c.bias for c in mine)
            assert {c.dirn for c in mine if (c.lb, c.rb) != (16, 16)} == {"fwd", "bwd"}
    assert [(c.kind, c.dirn, c.bits) for c in CC.RANDOM] == [("random", c.dirn, c.bits) for c in CC.EXACT]
    assert len({c.id for c in CC.ALL}) == len(CC.ALL)


@pytest.mark.parametrize("case", CC.EXACT + CC.EXACT16, ids=lambda c: c.id)
def test_exact_references_are_exact_in_fp32(case):
    """sum |a| |I| + LR terms < 2^24 units of 0.5, z~ splits exactly into fp16 halves, and the
    result is an fp32 value; an exact16 result lies inside fp16's range."""
    d = CC.inputs(case)
    assert f32(d["s"] / f32(CC.DENOM[case.bits])) == f32(0.5) and CC.scales(case)[1] == f32(1.0)
    assert np.abs(d["a"].astype(f64)).max() <= CC.amax_exact(case)
    units, zmax = CC.exact_units(case)
    assert units < 2 ** 24, units
    assert zmax < 2 ** 22 and zmax < 65504          # an integer below 2^22 is hi + lo exactly
    y, _ = CC.reference(case)
    assert np.array_equal(y.astype(f32).astype(f64), y)
    core = (y - (0 if d["bias"] is None else d["bias"].astype(f64))) / f64(d["gs"])
    assert np.array_equal(np.round(core * 2), core * 2)          # multiples of 0.5 before gs and the bias
    if case.kind == "exact16":
        assert np.abs(y).max() < 65504
    if case.bits == 2 and case.K > 2048:   # the bounded nonzeros reach every chunk of every token
        nz = d["a"] != 0
        assert nz.sum(axis=1).max() <= CC.NF2_LONG_NONZERO + 3
        for lo in range(0, case.K, 256):
            assert nz[:, lo:lo + 256].any(axis=1).all()


def _pairs(cases, faults=CC.FAULTS):
    return [pytest.param(c, f, id=f"{c.id}-{f}") for c in cases for f in faults if CC.fault_applies(c, f)]


@pytest.mark.parametrize("case,fault", _pairs(CC.EXACT))
def test_planted_fault_changes_every_exact_case(case, fault):
    y, _ = CC.reference(case)
    bad, _ = CC.reference(case, fault)
    assert not np.array_equal(y, bad)


@pytest.mark.parametrize("case,fault", _pairs(CC.RANDOM, CC.RANDOM_FAULTS))
def test_planted_fault_exceeds_ten_bars_on_random_cases(case, fault):
    y, bar = CC.reference(case)
    bad, _ = CC.reference(case, fault)
    assert (np.abs(bad - y) / bar).max() >= 10.0


def test_every_fault_meets_exact_and_random_cases():
    for fault in CC.FAULTS:
        for bits in ((4,) if fault == "sym_table" else (2,) if fault == "drop_lo" else (4, 2)):
            assert any(CC.fault_applies(c, fault) for c in CC.EXACT if c.bits == bits), fault
            if fault in CC.RANDOM_FAULTS:
                assert any(CC.fault_applies(c, fault) for c in CC.RANDOM if c.bits == bits), fault
    assert "drop_lo" not in CC.RANDOM_FAULTS      # below every random bar: the exact cases' job


# ---------------------------------------------------------------------------- the contract's numbers
@pytest.mark.parametrize("bits", [4, 2])
def test_integer_levels_are_the_quantisers_levels_and_exact_in_fp16(bits):
    I, D = CC.LEVELS[bits], CC.DENOM[bits]
    assert tuple(I) == tuple(float(v) for v in K.NF_LEVELS[bits]) and D == K.NF_DENOM[bits]
    assert np.array_equal((I / D).astype(f32), CC.LEVEL32[bits])          # the quantiser's fp32 levels
    if bits == 4:
        assert np.array_equal(I.astype(np.float16).astype(f64), I)
        assert np.array_equal(I[9:], -I[7:0:-1]) and I[0] == -1334 and I[8] == 0   # symmetric but for index 0
    else:
        hi = I - np.sign(I)
        assert sorted(set(np.abs(hi))) == [3332.0, 8164.0]
        assert np.array_equal(hi.astype(np.float16).astype(f64), hi)
        assert not np.array_equal(I.astype(np.float16).astype(f64), I)    # 8165 itself is not an fp16 value
    src = open(os.path.join(ROOT, "ee274_convexcaldera_llm_quantization_amd", "csrc", "cq_codebook.hip")).read()
    lev = re.search(r"kNF%d\[\d+\] = \{([^}]*)\}" % bits, src).group(1)
    assert np.array_equal(np.array([float(v.strip().rstrip("f")) for v in lev.split(",")], f32), CC.LEVEL32[bits])


@pytest.mark.parametrize("bits", [4, 2])
def test_kernel_dequantisation_is_the_reference_up_to_four_roundings(bits):
    """level32[idx] * scale (fp32, the NF quantiser) against I (s / D) (fp32 division, fp32 product):
    within 4 * 2^-24 relative on every level."""
    rng = np.random.default_rng(5 + bits)
    # 200 000 scales (uniform and log-uniform), and every fp32 within 64 ulps of a power of two or of
    # D times one (where s / D and s change binade): the edges are where a rounding is largest
    pows = 2.0 ** np.arange(-20, 11)
    ulps = np.arange(-64, 65, dtype=np.int32)
    edges = [f32(b) for b in np.concatenate([pows, pows * CC.DENOM[bits]])]
    near = np.concatenate([(np.array([e], f32).view(np.int32) + ulps).view(f32) for e in edges])
    s = np.concatenate([rng.uniform(1e-4, 4.0, 100000), np.exp(rng.uniform(np.log(1e-6), np.log(1e3), 100000)),
                        near, [0.05, 1.0, 0.37]]).astype(f32)
    assert s.size >= 200000 and np.isfinite(s).all() and (s > 0).all()
    sd = (s / f32(CC.DENOM[bits])).astype(f32)
    worst = 0.0
    for i, lev in enumerate(CC.LEVEL32[bits]):
        if lev == 0:
            continue
        ref = (lev * s).astype(f32).astype(f64)
        got = (f32(CC.LEVELS[bits][i]) * sd).astype(f32).astype(f64)
        worst = max(worst, float((np.abs(got - ref) / np.abs(ref)).max()))
    assert worst <= 4 * 2.0 ** -24, worst / 2.0 ** -24


def test_kernels_share_one_level_table_and_it_is_the_contracts():
    """cq_nf.h holds the only definition of the kernels' integer levels; both kernel files include it
    and restate none of it; its integers are _lib.NF_LEVELS (hi plane + sign at NF2)."""
    csrc = os.path.join(ROOT, "ee274_convexcaldera_llm_quantization_amd", "csrc")
    hdr = open(os.path.join(csrc, "cq_nf.h")).read()

    def ints(name):
        return [int(v) for v in re.search(name + r"\[\d+\] = \{([^}]*)\}", hdr).group(1).split(",")]

    assert tuple(ints("kNF4I")) == K.NF_LEVELS[4]
    assert tuple(h + (1 if h > 0 else -1) for h in ints("kNF2Hi")) == K.NF_LEVELS[2]
    assert float(re.search(r"kNF4D = ([0-9.]+)f", hdr).group(1)) == K.NF_DENOM[4]
    assert float(re.search(r"kNF2D = ([0-9.]+)f", hdr).group(1)) == K.NF_DENOM[2]
    for name in ("cq_linear.hip", "cq_linear_bwd.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "cq_nf.h"' in src
        for definition in ("kNF4I[16] =", "kNF2Hi[4] =", "void fill_nf_table", "expand_nf(const", "nf2_lo(const"):
            assert definition not in src, (name, definition)
    from ee274_convexcaldera_llm_quantization_amd import build
    assert any(d.endswith("cq_nf.h") for d in build._deps())      # a change of the table rebuilds the library


def test_engine_refuses_ragged_columns_with_a_codebook_q():
    """n % 4 != 0 never reaches engine._finalize with an NF Q (so last_packed needs no n_padded there):
    the engine raises before any device work."""
    from ee274_convexcaldera_llm_quantization_amd.engine import CalderaEngine, EngineParams
    from ee274_convexcaldera_llm_quantization_amd.src.caldera.utils.dataclasses import CalderaParams
    from ee274_convexcaldera_llm_quantization_amd.src.caldera.utils.quantization import QuantizerFactory
    for method, bits in (("nf4", 4), ("nf2", 2)):
        qp = CalderaParams(Q_bits=bits, L_bits=16, R_bits=16, rank=4, iters=1, update_order=["Q", "LR"],
                           quant_factory_Q=QuantizerFactory(method, 64))
        eng = CalderaEngine(EngineParams.from_caldera_params(qp))
        with pytest.raises(NotImplementedError, match="% 4 != 0 needs uniform quantisers"):
            eng.run(torch.zeros(1, 8, 198))


# ---------------------------------------------------------------------------- packing
@pytest.mark.parametrize("bits,n", [(4, 198), (2, 198), (4, 64), (2, 898), (4, 1), (2, 2600)])
def test_index_packers_round_trip_and_match_numpy(bits, n):
    rng = np.random.default_rng(n + bits)
    idx = rng.integers(0, 2 ** bits, (7, n)).astype(np.uint8)
    got = pack_index_rows(torch.from_numpy(idx), bits)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (7, row_bytes(n, bits)) and got.shape[1] % 16 == 0
    assert np.array_equal(got.numpy(), CC.index_codes(idx, bits))
    un = unpack_index_bytes(got, bits)
    assert un.dtype == torch.uint8 and np.array_equal(un[:, :n].numpy(), idx)
    assert (un[:, n:] == CC.TAIL_INDEX[bits]).all()
    # MSB-first: the first index of a row sits in the top bits of its first byte
    assert int(got[0, 0]) >> (8 - bits) == int(idx[0, 0])
    assert LIN.NF_TAIL_INDEX == CC.TAIL_INDEX and K.NF_LEVELS[4][LIN.NF_TAIL_INDEX[4]] == 0


# ---------------------------------------------------------------------------- the ABI
def _struct_fields(name):
    txt = open(HEADER).read()
    body = txt[txt.index(f"typedef struct {name}"):txt.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*[;,]", body.split("{", 1)[1])


def test_codebook_abi_is_additive():
    txt = open(HEADER).read()
    assert int(re.search(r"#define CQ_ABI_VERSION (\d+)", txt).group(1)) == K.ABI_VERSION == 5
    assert int(re.search(r"#define CQ_QFMT_UNIFORM (\d+)", txt).group(1)) == K.QFMT_UNIFORM == 0
    assert int(re.search(r"#define CQ_QFMT_NF (\d+)", txt).group(1)) == K.QFMT_NF == 1
    new = {"cq_linear_codebook_workspace", "cq_linear_codebook_forward", "cq_linear_codebook_backward_workspace",
           "cq_linear_codebook_backward_input"}
    assert new <= set(K.EXPORTS)
    lib = K.load()                      # raises for a missing export
    assert lib.cq_abi_version() == 5
    for name in new:
        assert getattr(lib, name) is not None
    # the packed struct, then q_format; the packed structs themselves are unchanged
    assert _struct_fields("cq_linear_codebook_args") == ["p", "q_format"]
    assert _struct_fields("cq_linear_codebook_backward_args") == ["p", "q_format"]
    assert [f for f, _ in K.LinearCodebookArgs._fields_] == ["p", "q_format"]
    assert K.LinearCodebookArgs._fields_[0][1] is K.LinearPackedArgs
    assert K.LinearCodebookBackwardArgs._fields_[0][1] is K.LinearPackedBackwardArgs
    assert [f for f, _ in K.LinearPackedArgs._fields_] == _struct_fields("cq_linear_packed_args")
    assert K.LinearCodebookArgs.q_format.offset == ctypes.sizeof(K.LinearPackedArgs)
    assert K.LinearCodebookBackwardArgs.q_format.offset == ctypes.sizeof(K.LinearPackedBackwardArgs)


def test_codebook_entries_reject_bad_arguments_without_a_device():
    """Validation runs before any launch: CQ_EINVAL with a message, for an unknown format and for
    everything the packed entries reject."""
    lib = K.load()
    buf = torch.zeros(8192, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16

    def fwd(q_format=K.QFMT_NF, **kw):
        a = K.LinearCodebookArgs()
        p = a.p
        p.x, p.ldx, p.tokens, p.m, p.n, p.r, p.bits = base, 64, 1, 16, 64, 0, 4
        p.codes, p.code_stride, p.qscale, p.gscale = base + 256, 32, 1.0, 1.0
        p.y, p.y_dtype, p.ldy = base + 1024, K.CQ_F32, 16
        p.l_bits = p.r_bits = 16
        for key, v in kw.items():
            setattr(p, key, v)
        a.q_format = q_format
        return a

    def bwd(q_format=K.QFMT_NF, **kw):
        a = K.LinearCodebookBackwardArgs()
        p = a.p
        p.dy, p.lddy, p.tokens, p.m, p.n, p.r, p.bits = base, 16, 1, 16, 64, 0, 4
        p.codes, p.code_stride, p.qscale, p.gscale = base + 256, 32, 1.0, 1.0
        p.dx, p.dx_dtype, p.lddx = base + 1024, K.CQ_F32, 64
        p.l_bits = p.r_bits = 16
        for key, v in kw.items():
            setattr(p, key, v)
        a.q_format = q_format
        return a

    bad = ((dict(q_format=2), "q_format"), (dict(q_format=-1), "q_format"), (dict(bits=3), "bits"),
           (dict(bits=8), "bits"), (dict(r=K.LINEAR_MAX_RANK + 1), "rank"), (dict(codes=base + 260), "aligned"),
           (dict(code_stride=17), "aligned"), (dict(code_stride=16), "stride"), (dict(l_bits=3), "factor bits"),
           (dict(qscale=float("nan")), "scale"), (dict(qscale=-1.0), "scale"))
    for kw, word in bad:
        for make, entry in ((fwd, lib.cq_linear_codebook_forward), (bwd, lib.cq_linear_codebook_backward_input)):
            a = make(**kw)
            assert entry(ctypes.byref(a), None, 0, None) == K.CQ_EINVAL, kw
            assert word in lib.cq_last_error().decode(), (kw, lib.cq_last_error())
    assert lib.cq_linear_codebook_forward(ctypes.byref(fwd(x=base + 1)), None, 0, None) == K.CQ_EINVAL
    assert lib.cq_linear_codebook_backward_input(ctypes.byref(bwd(lddx=8)), None, 0, None) == K.CQ_EINVAL
    assert lib.cq_linear_codebook_forward(None, None, 0, None) == K.CQ_EINVAL
    # a negative uniform scale is the packed entries' business (they take it): only NF checks it
    # the workspace is the packed entries' function of tokens and r
    a = fwd(r=8, L=base + 2048, ldl=8, R=base + 3072, ldr=64)
    p = K.LinearPackedArgs.from_buffer_copy(a.p)
    assert lib.cq_linear_codebook_workspace(ctypes.byref(a)) == lib.cq_linear_packed_workspace(ctypes.byref(p)) \
        == 16 * 16 * 32 * 4
    a.p.tokens = 17
    assert lib.cq_linear_codebook_workspace(ctypes.byref(a)) == 2 * 64 * 32 * 2
    assert lib.cq_linear_codebook_forward(ctypes.byref(a), base, 16, None) == K.CQ_EWORKSPACE
    b = bwd(r=8, L=base + 2048, ldl=8, R=base + 3072, ldr=64, tokens=5)
    assert lib.cq_linear_codebook_backward_workspace(ctypes.byref(b)) == 2 * 5 * 32 * 2


def test_args_builders_check_like_the_packed_ones():
    x16, y32 = torch.zeros(2, 198, dtype=torch.float16), torch.zeros(2, 12)
    codes = torch.zeros(12, row_bytes(198, 4), dtype=torch.uint8)
    L, R = torch.zeros(12, 5, dtype=torch.float16), torch.zeros(5, 198, dtype=torch.float16)
    ok = dict(x=x16, codes=codes, qscale=1.0, gscale=1.0, L=L, R=R, bias=None, y=y32)

    def build(q_format=K.QFMT_NF, **kw):
        ops = dict(ok)
        ops.update(kw)
        return K.linear_codebook_args(ops["x"], ops["codes"], ops["qscale"], ops["gscale"], ops["L"], ops["R"],
                                      ops["bias"], ops["y"], m=12, n=198, bits=4, q_format=q_format)

    a = build()
    assert (a.q_format, a.p.bits, a.p.r, a.p.l_bits, a.p.code_stride) == (K.QFMT_NF, 4, 5, 16, row_bytes(198, 4))
    assert build(K.QFMT_UNIFORM).q_format == K.QFMT_UNIFORM
    for kw, word in ((dict(q_format=7), "q_format"), (dict(qscale=float("inf")), "NF scale"),
                     (dict(qscale=-0.5), "NF scale"), (dict(L=L.float()), "fp16"),
                     (dict(x=x16.float()), "x must be fp16"),
                     (dict(y=y32.double()), "y must be"), (dict(bias=torch.zeros(12, dtype=torch.float16)), "bias"),
                     (dict(codes=codes[:5]), "codes")):
        with pytest.raises(ValueError, match=word):
            build(**kw)
    dy16, dx32 = torch.zeros(2, 12, dtype=torch.float16), torch.zeros(2, 198)
    b = K.linear_codebook_backward_args(dy16, codes, 1.0, 1.0, L, R, dx32, m=12, n=198, bits=4, q_format=K.QFMT_NF)
    assert (b.q_format, b.p.r, b.p.lddx) == (K.QFMT_NF, 5, 198)
    for kw, word in ((dict(q_format=3), "q_format"), (dict(qscale=float("nan")), "NF scale")):
        args = dict(q_format=K.QFMT_NF, qscale=1.0)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            K.linear_codebook_backward_args(dy16, codes, args["qscale"], 1.0, L, R, dx32, m=12, n=198, bits=4,
                                            q_format=args["q_format"])
    with pytest.raises(ValueError, match="dy must be fp16"):
        K.linear_codebook_backward_args(dy16.float(), codes, 1.0, 1.0, L, R, dx32, m=12, n=198, bits=4,
                                        q_format=K.QFMT_NF)


# ---------------------------------------------------------------------------- CalderaLinear
def _layer(m=12, n=198, r=5, bits=4, seed=0):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, 2 ** bits, (m, n)).astype(np.uint8)
    L = rng.standard_normal((m, r)).astype(np.float32)
    R = rng.standard_normal((r, n)).astype(np.float32)
    return idx, L, R, 0.37, 1.25


def _result(idx, L, R, s, gs, bits, name="layer"):
    packed, npad = CC.storage_index_codes(idx, bits)
    extra = {"n_padded": npad} if npad != idx.shape[1] else {}
    return MatrixResult(name, idx.shape[0], idx.shape[1], L.shape[1], bits, torch.from_numpy(packed), s,
                        torch.from_numpy(L), torch.from_numpy(R), gs, {}, extra, Q_method=f"nf{bits}")


def _decomposition(idx, L, R, s, gs, bits):
    Q = torch.from_numpy(CC.LEVEL32[bits][idx.astype(np.int64)]) * np.float32(s)   # the NF dequantiser
    return CalderaDecomposition(Q=Q, L=torch.from_numpy(L), R=torch.from_numpy(R),
                                Q_idxs=torch.from_numpy(idx).reshape(1, -1), Q_scale=torch.tensor([[s]]),
                                global_scale=gs)


@pytest.mark.parametrize("bits,n", [(4, 198), (2, 198), (2, 64), (4, 898), (2, 899)])
def test_constructors_build_the_same_state_and_the_references_weight(bits, n):
    idx, L, R, s, gs = _layer(n=n, bits=bits)
    dec = _decomposition(idx, L, R, s, gs, bits)
    a = CalderaLinear.from_result(_result(idx, L, R, s, gs, bits))
    b = CalderaLinear.from_decomposition(dec, bits, Q_method=f"nf{bits}")
    c = CalderaLinear.from_codes(torch.from_numpy(idx), torch.from_numpy(L), torch.from_numpy(R), qscale=s, gscale=gs,
                                 bits=bits, q_format=NF)
    assert (a.in_features, a.out_features, a.rank, a.bits, a.q_format) == (n, 12, 5, bits, NF)
    for other in (b, c):
        assert a.get_extra_state() == pytest.approx(other.get_extra_state())
        sa, sb = a.state_dict(), other.state_dict()
        assert set(sa) == set(sb)
        for key in ("codes", "L", "R"):
            assert sa[key].dtype == sb[key].dtype and torch.equal(sa[key], sb[key]), key
    assert np.array_equal(a.codes.numpy(), CC.index_codes(idx, bits))
    assert f"q_format=nf{bits}" in repr(a) and not list(a.parameters())
    # dense_weight(): the kernel's formula, I (s / D) with the fp32 division, in fp32 ...
    sd = f32(f32(s) / f32(CC.DENOM[bits]))
    lr = a.L.float() @ a.R.float()
    want = gs * (torch.from_numpy((CC.LEVELS[bits][idx.astype(np.int64)]).astype(f32) * sd) + lr)
    assert torch.equal(a.dense_weight(), want)
    # ... which is the reference's weight gs (Q + fp16(L) fp16(R)) within 4 * 2^-24 |gs Q| (+ the
    # fp32 matmul L R, r + 1 roundings on |L| |R| alone, and one rounding each for the sum and the
    # product with gs on the result's terms)
    ref = gs * (dec.Q.double() + a.L.double() @ a.R.double())
    absLR = a.L.double().abs() @ a.R.double().abs()
    aQ = dec.Q.double().abs()
    tol = 4 * 2.0 ** -24 * gs * aQ + (a.rank + 1) * 2.0 ** -24 * gs * absLR + 2 * 2.0 ** -24 * gs * (aQ + absLR)
    assert ((a.dense_weight().double() - ref).abs() <= tol).all()
    # the bytes a forward streams: no buffer beside the uniform layer's
    assert a.packed_bytes() == 12 * row_bytes(n, bits) + 2 * (12 * 5 + 5 * n)
    # back to the storage form and in again, also through the payload
    res = a.to_result("layer")
    assert res.Q_method == f"nf{bits}" and res.Q_scale == s
    assert np.array_equal(res.codes.numpy(), CC.storage_index_codes(idx, bits)[0])
    for again in (CalderaLinear.from_result(res),
                  CalderaLinear.from_result(unpack_results(pack_results([res]))[0])):
        assert again.q_format == NF
        assert torch.equal(again.codes, a.codes) and torch.equal(again.L, a.L) and torch.equal(again.R, a.R)
        assert again.get_extra_state() == pytest.approx(a.get_extra_state())


def test_uniform_layers_are_unchanged():
    """No new buffer, the default format, and a payload without the new meta key."""
    rng = np.random.default_rng(0)
    c = torch.from_numpy(rng.integers(-1, 2, (12, 198)).astype(np.int8))
    L, R = torch.randn(12, 5), torch.randn(5, 198)
    u = CalderaLinear.from_codes(c, L, R, qscale=0.3, gscale=1.0, bits=2)
    idx = torch.from_numpy(rng.integers(0, 4, (12, 198)).astype(np.uint8))
    nf = CalderaLinear.from_codes(idx, L, R, qscale=0.3, gscale=1.0, bits=2, q_format=NF)
    assert u.q_format == UNIFORM and "q_format" not in repr(u)
    assert set(u.state_dict()) == set(nf.state_dict()) == {"codes", "L", "R", "_extra_state"}
    assert u.get_extra_state()["q_format"] == 0 and isinstance(nf.get_extra_state()["q_format"], int)
    assert u.packed_bytes() == nf.packed_bytes()
    ru, rn = u.to_result("u"), nf.to_result("n")
    assert ru.Q_method == "uniform" and rn.Q_method == "nf2"
    assert MatrixResult("x", 1, 4, 0, 2, torch.zeros(1, dtype=torch.uint8), 1.0, torch.zeros(1, 0), torch.zeros(0, 4),
                        1.0).Q_method == "uniform"
    import json
    import struct
    buf = pack_results([ru, rn]).numpy().tobytes()
    head = struct.Struct("<4sIQ")       # sharding.py's header: magic, format version, JSON length
    magic, version, mlen = head.unpack(buf[:head.size])
    assert magic == b"CQRS"
    metas = json.loads(buf[head.size:head.size + mlen].decode())
    assert version == 2
    assert "Q_method" not in metas[0] and metas[1]["Q_method"] == "nf2"
    back = unpack_results(torch.frombuffer(bytearray(buf), dtype=torch.uint8))
    assert [r.Q_method for r in back] == ["uniform", "nf2"]


def test_state_dict_and_extra_state_round_trip(tmp_path):
    idx, L, R, s, gs = _layer()
    a = CalderaLinear.from_result(_result(idx, L, R, s, gs, 4), bias=torch.arange(12, dtype=torch.float32))
    # into a uniform layer of the same geometry: the format travels in the extra state
    rng = np.random.default_rng(1)
    b = CalderaLinear.from_codes(torch.from_numpy(rng.integers(-7, 8, (12, 198)).astype(np.int8)), torch.zeros(12, 5),
                                 torch.zeros(5, 198), torch.zeros(12), qscale=9.0, gscale=9.0, bits=4)
    assert b.q_format == UNIFORM
    torch.save(a.state_dict(), tmp_path / "sd.pt")
    b.load_state_dict(torch.load(tmp_path / "sd.pt"))
    for key in ("codes", "L", "R", "bias"):
        assert torch.equal(getattr(a, key), getattr(b, key))
    assert (b.qscale, b.gscale, b.bits, b.rank, b.q_format) == (a.qscale, a.gscale, 4, 5, NF)
    assert torch.equal(a.dense_weight(), b.dense_weight())
    # a state saved before the key existed keeps the layer's own format
    old = {k: v for k, v in a.get_extra_state().items() if k != "q_format"}
    for lin, fmt in ((a, NF), (CalderaLinear.from_codes(torch.zeros(12, 198, dtype=torch.int8), None, None, qscale=1.0,
                                                         gscale=1.0, bits=4), UNIFORM)):
        lin.set_extra_state(dict(old, rank=lin.rank))
        assert lin.q_format == fmt


def test_documented_errors():
    idx, L, R, s, gs = _layer()
    dec = _decomposition(idx, L, R, s, gs, 4)
    with pytest.raises(ValueError, match="uniform"):         # the method must be named
        CalderaLinear.from_decomposition(dec, 4)
    with pytest.raises(ValueError, match="Q_bits = 4"):
        CalderaLinear.from_decomposition(dec, 2, Q_method="nf4")
    with pytest.raises(ValueError, match="Q_bits = 2"):
        CalderaLinear.from_decomposition(dec, 4, Q_method="nf2")
    for method in ("bbint4", "bbint2"):
        with pytest.raises(ValueError, match="per block.*outlier"):
            CalderaLinear.from_decomposition(dec, 4, Q_method=method)
    with pytest.raises(ValueError, match="unknown Q method"):
        CalderaLinear.from_decomposition(dec, 4, Q_method="fp4")
    int8 = copy.copy(dec)
    int8.Q_idxs = dec.Q_idxs.to(torch.int8)
    with pytest.raises(ValueError, match="uint8 level indices"):
        CalderaLinear.from_decomposition(int8, 4, Q_method="nf4")
    blk = copy.copy(dec)
    blk.Q_scale = torch.ones(4, 1)
    with pytest.raises(ValueError, match="one scale"):
        CalderaLinear.from_decomposition(blk, 4, Q_method="nf4")
    for bad in (torch.full((3, 8), 16), torch.full((3, 8), -1), torch.zeros(3, 8)):
        with pytest.raises(ValueError, match="NF indices"):
            CalderaLinear.from_codes(bad, None, None, qscale=1.0, gscale=1.0, bits=4, q_format=NF)
    with pytest.raises(ValueError, match="q_format"):
        CalderaLinear.from_codes(torch.zeros(3, 8, dtype=torch.uint8), None, None, qscale=1.0, gscale=1.0, bits=4,
                                 q_format=5)
    with pytest.raises(ValueError, match="NF scale"):
        CalderaLinear.from_codes(torch.zeros(3, 8, dtype=torch.uint8), None, None, qscale=-1.0, gscale=1.0, bits=4,
                                 q_format=NF)
    res = _result(idx, L, R, s, gs, 4)
    res.Q_method = "bbint4"
    with pytest.raises(ValueError, match="no packed form"):
        CalderaLinear.from_result(res)
    lin = CalderaLinear.from_result(_result(idx, L, R, s, gs, 4))
    with pytest.raises(RuntimeError, match="HIP"):
        lin(torch.zeros(2, 198))

    class QP:
        Q_bits, L_bits, R_bits = 4, 16, 16

        class quant_factory_Q:
            method = "bbint4"
    model = torch.nn.Sequential(torch.nn.Linear(198, 12))

    def never(*a):
        raise AssertionError("decomposed before the refusal")
    with pytest.raises(ValueError, match="no packed form"):
        M.apply_caldera_quantization(model, None, QP(), packed=True, decompose=never)
    QP.quant_factory_Q.method = "nf2"
    with pytest.raises(ValueError, match="Q_bits = 2"):
        M.apply_caldera_quantization(model, None, QP(), packed=True, decompose=never)


def test_nf_layers_train_their_factors_and_wrap_in_the_hadamard_basis():
    idx, L, R, s, gs = _layer(m=16, n=256, bits=2)
    dec = _decomposition(idx, L, R, s, gs, 2)
    had = HadamardCalderaLinear.from_decomposition(dec, 2, (13, 200), Q_method="nf2")
    assert had.inner.q_format == NF and had.padded_shape == (16, 256)
    again = HadamardCalderaLinear.from_result(unpack_results(pack_results([had.to_result("h")]))[0])
    assert again.inner.q_format == NF and torch.equal(again.inner.codes, had.inner.codes)
    assert (again.in_features, again.out_features) == (200, 13)
    model = torch.nn.Sequential(CalderaLinear.from_decomposition(dec, 2, Q_method="nf2"), had)
    params = M.prepare_factor_finetuning(model, hadamard=True)
    assert len(params) == 4 and all(p.requires_grad and p.dtype == torch.float32 for p in params)
    assert model[0].factors_trainable and had.factors_trainable
    M.finish_factor_finetuning(model)
    assert not model[0].factors_trainable and model[0].L.dtype == torch.float16


def test_results_file_round_trip_into_a_model(tmp_path):
    idx, L, R, s, gs = _layer(bits=4)
    idx2, L2, R2, _, _ = _layer(m=16, n=256, bits=2, seed=3)
    had = HadamardCalderaLinear.from_decomposition(_decomposition(idx2, L2, R2, s, gs, 2), 2, (13, 200), Q_method="nf2")
    path = str(tmp_path / "res.cqrs")
    save_results(path, [_result(idx, L, R, s, gs, 4, name="proj"), had.to_result("hproj")])
    model = torch.nn.Module()
    model.proj = torch.nn.Linear(198, 12, bias=False)
    model.hproj = torch.nn.Linear(200, 13, bias=True)
    assert M.apply_packed_results(model, load_results(path)) == ["proj", "hproj"]
    direct = CalderaLinear.from_decomposition(_decomposition(idx, L, R, s, gs, 4), 4, Q_method="nf4")
    assert model.proj.q_format == NF and torch.equal(model.proj.codes, direct.codes)
    assert torch.equal(model.proj.L, direct.L) and (model.proj.qscale, model.proj.gscale) == (s, gs)
    assert isinstance(model.hproj, HadamardCalderaLinear) and model.hproj.inner.q_format == NF
    assert torch.equal(model.hproj.inner.codes, had.inner.codes) and model.hproj.bias is not None
