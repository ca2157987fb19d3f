"""Host-side checks of the packed linear layer's backward: the cases of linear_backward_cases.py
can see the faults they are meant to catch (planted in the reference), the ctypes struct matches
the header, the C entry refuses bad arguments before any HIP call and sizes its workspace by
tokens and r alone, and the fine-tuning surface of CalderaLinear / model.py on CPU tensors.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import linear_backward_cases as BC
from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import model as M
from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear, HadamardCalderaLinear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "caldera_hip.h")


# ---------------------------------------------------------------------------- the cases
def test_case_table():
    shapes = {(c.m, c.n, c.r) for c in BC.EXACT}
    assert shapes == set(BC.SHAPES) == {(c.m, c.n, c.r) for c in BC.RANDOM}
    for cases in (BC.EXACT, BC.RANDOM):
        for shape in BC.SHAPES:
            for bits in (2, 4):
                assert {c.T for c in cases if (c.m, c.n, c.r) == shape and c.bits == bits and not c.bias} >= {1, 5, 17, 64}
        assert {c.bits for c in cases if (c.m, c.T) == (272, 130)} == {2, 4}
        assert any(c.bias for c in cases)
    assert -(-272 // BC.CHUNK_ROWS) == 9 and -(-600 // BC.CHUNK_ROWS) == 19 and -(-2600 // BC.CHUNK_ROWS) == 82
    src = open(os.path.join(ROOT, "ee274_convexcaldera_llm_quantization_amd", "csrc", "cq_linear_bwd.hip")).read()
    assert int(re.search(r"constexpr int kRows = (\d+);", src).group(1)) == BC.CHUNK_ROWS


@pytest.mark.parametrize("case", BC.EXACT + BC.EXACT16, ids=lambda c: c.id)
def test_exact_references_are_exact_in_fp32(case):
    dx, u, _, _ = BC.reference(case)
    assert np.array_equal(dx * 2, np.rint(dx * 2)) and np.array_equal(u, np.rint(u))
    d = BC.inputs(case)
    dy, c, L, R = (np.abs(d[key].astype(np.float64)) for key in ("dy", "c", "L", "R"))
    worst = 4.0 * (0.5 * (dy @ c) + (dy @ L) @ R)       # bound on every partial sum
    assert worst.max() * 2 < 2 ** 24
    # u is exact as hi + lo, and its own partial sums are exact in fp32
    uh = u.astype(np.float16).astype(np.float64)
    ul = (u - uh).astype(np.float16).astype(np.float64)
    assert np.array_equal(uh + ul, u) and (dy @ L).max(initial=0) <= 20800
    if case.kind == "exact16":
        assert np.abs(dx).max() <= 1518 and np.array_equal(dx, np.rint(dx / 2) * 2)
        assert np.array_equal(dx, dx.astype(np.float16).astype(np.float64))


def _pairs(cases):
    return [pytest.param(c, f, id=f"{c.id}-{f}") for c in cases for f in BC.FAULTS if BC.fault_applies(c, f)]


@pytest.mark.parametrize("case,fault", _pairs(BC.EXACT))
def test_planted_fault_changes_every_exact_case(case, fault):
    dx, u, _, _ = BC.reference(case)
    dxf, uf, _, _ = BC.reference(case, fault)
    assert (dx != dxf).any()
    if fault in ("drop_last_rows", "drop_L_last") and case.r:
        assert (u != uf).any()


@pytest.mark.parametrize("case,fault", _pairs(BC.RANDOM))
def test_planted_fault_exceeds_ten_bars_on_random_cases(case, fault):
    dx, _, bar, _ = BC.reference(case)
    dxf, _, _, _ = BC.reference(case, fault)
    worst = (np.abs(dxf - dx) / bar).max()
    print(f"{case.id} {fault}: {worst:.1f} bars")
    assert worst >= 10


def test_every_fault_meets_exact_and_random_cases_and_global_faults_the_long_one():
    for cases in (BC.EXACT, BC.RANDOM):
        assert {f for c in cases for f in BC.FAULTS if BC.fault_applies(c, f)} == set(BC.FAULTS)
    long_random = [c for c in BC.RANDOM if c.m == 2600]
    assert long_random and all(BC.fault_applies(c, "drop_gs") and BC.fault_applies(c, "swap_R") for c in long_random)
    assert all(BC.fault_applies(c, "s_for_sk") for c in long_random if c.bits == 4)
    # row-local faults: on the long contraction by the exact cases
    for f in BC.ROW_LOCAL_FAULTS:
        assert any(BC.fault_applies(c, f) for c in BC.EXACT if c.m == 2600), f
        assert all(BC.fault_applies(c, f) for c in BC.RANDOM
                   if c.m * (c.r + 1) <= 25000 and c.T > 1 and c.r and (f != "pad_row" or c.m % BC.CHUNK_ROWS)), f


def test_single_fp16_rounding_of_u_fails_the_bar():
    """u rounded once to fp16 (what the contract forbids) is outside the dx bar at (33, 64, 8)."""
    for case in BC.RANDOM:
        if (case.m, case.n, case.r) != (33, 64, 8) or case.bias:
            continue
        d = BC.inputs(case)
        dy, L, R, c = (d[key].astype(np.float64) for key in ("dy", "L", "R", "c"))
        u16 = (dy @ L).astype(np.float16).astype(np.float64)
        dx = np.float64(d["gs"]) * (np.float64(d["s"] / np.float32(case.k)) * (dy @ c) + u16 @ R)
        dx64, _, bar, _ = BC.reference(case)
        assert (np.abs(dx - dx64) / bar).max() > 1


# ---------------------------------------------------------------------------- the ABI
def _struct_fields(name):
    txt = open(HEADER).read()
    body = txt[txt.index(f"typedef struct {name}"):txt.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*[;,]", body.split("{", 1)[1])


def test_backward_args_struct_matches_header():
    fields = [f for f, _ in K.LinearBackwardArgs._fields_]
    assert fields == _struct_fields("cq_linear_backward_args")
    assert fields == ["dy", "lddy", "tokens", "m", "n", "r", "bits", "codes", "code_stride", "qscale", "gscale",
                      "L", "ldl", "R", "ldr", "dx", "dx_dtype", "lddx", "u_out", "ldu"]
    txt = open(HEADER).read()
    assert int(re.search(r"#define CQ_ABI_VERSION (\d+)", txt).group(1)) == K.ABI_VERSION == 5
    assert K.load().cq_abi_version() == 5
    assert {"cq_linear_backward_workspace", "cq_linear_backward_input"} <= set(K.EXPORTS)


def _args(base, **kw):
    a = K.LinearBackwardArgs()
    a.dy, a.lddy, a.tokens, a.m, a.n, a.r, a.bits = base, 16, 1, 16, 64, 0, 2
    a.codes, a.code_stride, a.qscale, a.gscale = base + 256, 16, 1.0, 1.0
    a.dx, a.dx_dtype, a.lddx = base + 1024, K.CQ_F32, 64
    for key, v in kw.items():
        setattr(a, key, v)
    return a


def test_backward_entry_rejects_bad_arguments_without_a_device():
    """Validation runs before any HIP call: CQ_EINVAL with a message."""
    lib = K.load()
    buf = torch.zeros(8192, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16
    fac = dict(r=8, L=base + 2048, ldl=8, R=base + 3072, ldr=64)
    for kw, word in ((dict(bits=3), "bits"), (dict(bits=8), "bits"), (dict(r=K.LINEAR_MAX_RANK + 1), "rank"),
                     (dict(codes=base + 260), "aligned"), (dict(code_stride=24), "aligned"),
                     (dict(dy=base + 1), "misaligned"), (dict(dx=base + 1026), "misaligned"),
                     (dict(fac, L=base + 2049), "misaligned"), (dict(fac, R=base + 3073), "misaligned"),
                     (dict(fac, u_out=base + 4098, ldu=8), "misaligned"),
                     (dict(lddy=15), "leading"), (dict(lddx=63), "leading"), (dict(fac, ldl=7), "leading"),
                     (dict(fac, ldr=63), "leading"), (dict(fac, u_out=base + 4096, ldu=7), "leading"),
                     (dict(dx_dtype=7), "dtype")):
        a = _args(base, **kw)
        assert lib.cq_linear_backward_input(ctypes.byref(a), base + 6144, 2048, None) == K.CQ_EINVAL, kw
        assert word in lib.cq_last_error().decode(), (kw, lib.cq_last_error())
    # fp16 dx needs only 2-byte alignment; a workspace that is too small is refused as well
    a = _args(base, **fac)
    need = lib.cq_linear_backward_workspace(ctypes.byref(a))
    assert need == 2 * 1 * 32 * 2
    assert lib.cq_linear_backward_input(ctypes.byref(a), base + 6144, need - 1, None) == K.CQ_EINVAL
    assert "workspace" in lib.cq_last_error().decode()
    assert lib.cq_linear_backward_input(ctypes.byref(a), None, 0, None) == K.CQ_EINVAL
    # tokens = 0: nothing to do, no launch (there is no device here to launch on)
    assert lib.cq_linear_backward_input(ctypes.byref(_args(base, tokens=0)), None, 0, None) == 0
    assert lib.cq_linear_backward_input(ctypes.byref(_args(base, tokens=0, **fac)), None, 0, None) == 0


def test_workspace_depends_on_tokens_and_rank_alone():
    """No image of the codes or of the dense weight: the workspace does not grow with m or n."""
    lib = K.load()

    def ws(**kw):
        a = _args(0, tokens=512, r=128)
        for key, v in kw.items():
            setattr(a, key, v)
        return lib.cq_linear_backward_workspace(ctypes.byref(a))

    base = ws(m=64, n=64)
    assert base == ws(m=8192, n=64) == ws(m=64, n=8192) == ws(m=8192, n=8192)
    assert 0 < base <= 512 * 128 * 4 * 2           # u as halves, or one fp32 copy or two
    assert ws(r=0) == 0 and ws(tokens=0) == 0
    assert ws(tokens=1024) > base and ws(r=256) > base


# ---------------------------------------------------------------------------- CalderaLinear
def _layer(m=12, n=198, r=5, bits=2, seed=0, coded=False, bias=True):
    rng = np.random.default_rng(seed)
    k = 2 ** (bits - 1) - 1
    c = torch.from_numpy(rng.integers(-k, k + 1, (m, n)).astype(np.int8))
    L = torch.from_numpy(rng.standard_normal((m, r)).astype(np.float32))
    R = torch.from_numpy(rng.standard_normal((r, n)).astype(np.float32))
    b = torch.arange(m, dtype=torch.float32) if bias else None
    if coded:
        cl = torch.from_numpy(rng.integers(-1, 2, (m, r)).astype(np.int8))
        return CalderaLinear.from_codes(c, None, R, b, qscale=0.37, gscale=1.25, bits=bits, L_codes=(cl, 0.5, 2))
    return CalderaLinear.from_codes(c, L if r else None, R if r else None, b, qscale=0.37, gscale=1.25, bits=bits)


@pytest.mark.parametrize("master", [torch.float32, torch.float64, torch.bfloat16])
def test_enable_and_freeze_round_trip(master):
    lin = _layer()
    keys = list(lin.state_dict())
    L16, R16 = lin.L.clone(), lin.R.clone()
    params = lin.enable_factor_training(master)
    assert [name for name, _ in lin.named_parameters()] == ["L", "R"]
    assert params[0] is lin.L and params[1] is lin.R and lin.factors_trainable
    assert all(isinstance(p, torch.nn.Parameter) and p.requires_grad and p.dtype == master for p in params)
    if master != torch.bfloat16:       # widened exactly
        assert torch.equal(lin.L.detach().to(torch.float16), L16) and torch.equal(lin.L.detach().double(), L16.double())
        assert torch.equal(lin.R.detach().double(), R16.double())
    assert set(lin.state_dict()) == set(keys)
    assert {name for name, _ in lin.named_buffers()} == {"codes", "bias"}
    assert lin.enable_factor_training(master)[0] is params[0]        # idempotent
    # dtype casts of the model still leave the codes and the bias (and the masters) as stored
    torch.nn.Sequential(lin).half()
    assert (lin.codes.dtype, lin.bias.dtype, lin.L.dtype) == (torch.uint8, torch.float32, master)
    assert lin.freeze_factors() is lin and not lin.factors_trainable
    assert not list(lin.parameters()) and set(lin.state_dict()) == set(keys)
    assert lin.L.dtype == lin.R.dtype == torch.float16
    if master != torch.bfloat16:
        assert torch.equal(lin.L, L16) and torch.equal(lin.R, R16)
    lin.freeze_factors()                                              # idempotent


def test_freeze_rounds_the_masters_to_nearest_even():
    lin = _layer()
    L, R = lin.enable_factor_training()
    with torch.no_grad():
        L.fill_(1.0 + 2.0 ** -11)             # a tie between 1 and 1 + 2^-10: to even
        L[0, 0] = 1.0 + 3 * 2.0 ** -11        # a tie between 1 + 2^-10 and 1 + 2^-9: to even
        R.mul_(1.0 + 2.0 ** -13)
        want_R = R.detach().to(torch.float16)
    lin.freeze_factors()
    assert lin.L[0, 1] == 1.0 and lin.L[0, 0] == 1.0 + 2.0 ** -9 and torch.equal(lin.R, want_R)
    res = lin.to_result("layer")
    again = CalderaLinear.from_result(res, bias=lin.bias)
    assert torch.equal(again.L, lin.L) and torch.equal(again.R, lin.R) and torch.equal(again.codes, lin.codes)
    assert lin.packed_bytes() == again.packed_bytes()


def test_state_dict_moves_between_training_and_frozen_layers():
    train, frozen = _layer(seed=1), _layer(seed=2)
    L, R = train.enable_factor_training()
    with torch.no_grad():
        L.add_(0.001)
    sd = train.state_dict()
    assert set(sd) == set(frozen.state_dict()) and sd["L"].dtype == torch.float32
    frozen.load_state_dict(sd)                       # masters -> fp16 buffers: rounded
    assert frozen.L.dtype == torch.float16 and torch.equal(frozen.L, L.detach().to(torch.float16))
    assert torch.equal(frozen.codes, train.codes) and torch.equal(frozen.R, R.detach().to(torch.float16))
    other = _layer(seed=3)
    other.enable_factor_training()
    other.load_state_dict(frozen.state_dict())       # fp16 buffers -> masters: widened exactly
    assert other.L.dtype == torch.float32 and torch.equal(other.L.detach(), frozen.L.float())
    assert isinstance(other.L, torch.nn.Parameter) and torch.equal(other.codes, frozen.codes)


def test_documented_errors():
    with pytest.raises(ValueError, match="coded"):
        _layer(coded=True).enable_factor_training()
    with pytest.raises(ValueError, match="rank 0"):
        _layer(r=0).enable_factor_training()
    lin = _layer()
    lin.enable_factor_training()
    with pytest.raises(RuntimeError, match="HIP"):
        lin(torch.zeros(2, 198, requires_grad=True))
    dy, dx = torch.zeros(2, 12, dtype=torch.float16), torch.zeros(2, 198)
    frozen = _layer()
    for kw, word in ((dict(dy=dy.float()), "dy must be fp16"), (dict(dx=dx.double()), "dx must be"),
                     (dict(L=frozen.L.float()), "fp16"), (dict(dx=dx[:, :5]), "do not fit"),
                     (dict(u_out=torch.zeros(2, 4)), "u_out")):
        ops = dict(dy=dy, codes=frozen.codes, L=frozen.L, R=frozen.R, dx=dx, u_out=None)
        ops.update(kw)
        with pytest.raises(ValueError, match=word):
            K.linear_backward_args(ops["dy"], ops["codes"], 1.0, 1.0, ops["L"], ops["R"], ops["dx"], m=12, n=198,
                                   bits=2, u_out=ops["u_out"])


# ---------------------------------------------------------------------------- model.py
class _Net(torch.nn.Module):
    def __init__(self, extra=None):
        super().__init__()
        self.a = _layer(m=12, n=198, r=5, seed=4)
        self.act = torch.nn.ReLU()
        self.b = _layer(m=7, n=12, r=3, bits=4, seed=5, bias=False)
        self.codes_only = _layer(m=7, n=7, r=0, seed=6)
        self.dense = torch.nn.Linear(7, 3)
        if extra is not None:
            self.extra = extra


def test_prepare_and_finish_factor_finetuning():
    net = _Net()
    keys = list(net.state_dict())
    params = M.prepare_factor_finetuning(net)
    assert len(params) == 4 and all(p.dtype == torch.float32 for p in params)
    assert [id(p) for p in params] == [id(p) for p in (net.a.L, net.a.R, net.b.L, net.b.R)]
    assert not net.codes_only.factors_trainable           # rank 0: nothing to train, still back-propagates dx
    names = {name for name, _ in net.named_parameters()}
    assert names == {"a.L", "a.R", "b.L", "b.R", "dense.weight", "dense.bias"}
    assert M.prepare_factor_finetuning(net, torch.float64)[0] is params[0]   # already enabled: kept
    assert M.finish_factor_finetuning(net) is net
    assert {name for name, _ in net.named_parameters()} == {"dense.weight", "dense.bias"}
    assert set(net.state_dict()) == set(keys) and net.a.L.dtype == torch.float16


def test_prepare_names_the_layers_without_a_backward():
    had = HadamardCalderaLinear(_layer(m=8, n=16, r=2, bias=False), 13, 6)
    net = _Net(extra=torch.nn.Sequential(_layer(coded=True), had))
    with pytest.raises(ValueError) as err:
        M.prepare_factor_finetuning(net)
    assert "extra.0" in str(err.value) and "extra.1" in str(err.value) and "extra.1.inner" not in str(err.value)
    assert not list(net.a.parameters()) and not net.a.factors_trainable     # nothing was changed
