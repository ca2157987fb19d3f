"""Host-side checks of the packed backward with coded factors: the cases of
linear_packed_backward_cases.py are exact where they claim to be and can see the faults they are
meant to catch (planted in the reference), the ctypes struct matches the header, the C entry
refuses bad arguments before any HIP call and sizes its workspace by tokens and r alone, and the
fine-tuning surface of HadamardCalderaLinear / model.py on CPU tensors.  No GPU.

Every claimed (random case, fault) pair measures >= 10 bars; the smallest is 12.2 ("flip_first" on
random-m160n256r128b2L2R2T17), the smallest of a fault that is new here 22.8 ("flip_L")."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import linear_packed_backward_cases as PC
from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import model as M
from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear, HadamardCalderaLinear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "caldera_hip.h")
f64 = np.float64


# ---------------------------------------------------------------------------- the cases
def test_case_table():
    for cases in (PC.EXACT, PC.RANDOM):
        assert {(c.m, c.n, c.r) for c in cases} == set(PC.SHAPES)
        for shape in PC.SHAPES:
            here = [c for c in cases if (c.m, c.n, c.r) == shape]
            for combo in ((2, 4, 4), (2, 2, 2)):
                assert {c.T for c in here if (c.bits, c.lb, c.rb) == combo} >= {1, 5, 17, 64}
            if shape in PC.ALIGNED:
                assert 130 in {c.T for c in here}
        for shape in ((48, 198, 40), (160, 256, 128)):
            assert {(c.bits, c.lb, c.rb) for c in cases if (c.m, c.n, c.r) == shape} == set(PC.COMBOS)
        # the mask-free loops: u at T = 64 (whole workgroups of 64 tokens), main at T = 130 (of 128)
        assert {c.T for c in cases if c.m == 160 and (c.lb, c.rb) == (4, 16)} >= {64, 130}
    assert len(PC.COMBOS) == 16 and 160 // PC.CHUNK_ROWS - 2 > 0 and 128 // PC.CHUNK_ROWS - 2 > 0 and 128 >= 113
    assert PC.SHAPES[1] == (48, 198, 40) and PC.SHAPES[4] == (160, 256, 128)


@pytest.mark.parametrize("shape", PC.SHAPES, ids=lambda s: "m%dn%dr%d" % s)
def test_exact_references_are_exact_in_fp32_and_as_hi_plus_lo(shape):
    for case in (c for c in PC.EXACT + PC.EXACT16 if (c.m, c.n, c.r) == shape):
        dx, u, _, _ = _reference(case)
        d = PC.inputs(case)
        sk, uscale = PC.scales(case, d)
        assert sk == 0.5 and (uscale in (0.25, 0.5) or not case.r), case.id
        assert np.array_equal(dx * 4, np.rint(dx * 4)) and np.array_equal(u * 4, np.rint(u * 4)), case.id
        # u~ is exact as hi + lo in fp16 ...
        uh = u.astype(np.float16).astype(f64)
        ul = (u - uh).astype(np.float16).astype(f64)
        assert np.array_equal(uh + ul, u), case.id
        # ... and every partial sum, in any order, is an exact fp32 value: sums of absolute terms in
        # units of 0.25 stay below 2^24 (the unscaled u sum is a sum of integers below that too)
        ady, ac, al, ar = (np.abs(d[key].astype(f64)) for key in ("dy", "c", "lam", "rho"))
        worst = 4.0 * (0.5 * (ady @ ac) + (np.abs(uh) + np.abs(ul)) @ ar)
        assert worst.max() * 4 < 2 ** 24 and (ady @ al).max(initial=0) < 2 ** 24, case.id
        if case.kind == "exact16":
            assert np.abs(dx).max() <= 2048 and np.array_equal(dx, dx.astype(np.float16).astype(f64)), case.id


def test_hostile_operands_hold_what_the_faults_need():
    for case in PC.EXACT + PC.RANDOM:
        d = PC.inputs(case)
        if case.r and case.lb != 16:
            assert (d["ltail"] != 0).all() and d["ltail"].shape[1] >= case.r16 - case.r
            assert np.array_equal(PC.unpack(PC.l_codes(case), case.lb)[:, :case.r], d["lam"])
            assert np.array_equal(PC.unpack(PC.l_codes(case), case.lb)[:, case.r:], d["ltail"])
        if case.r and case.rb != 16:
            buf = PC.r_codes(case)
            assert buf.shape == (case.r32, PC.row_bytes(case.n, case.rb))
            assert np.array_equal(PC.unpack(buf, case.rb)[:case.r, :case.n], d["rho"])
            if case.r32 > case.r:
                assert d["rrows"].any()


_REF = {}


def _reference(case):
    """The fault-free reference of a case, computed once for all the faults held against it."""
    if case not in _REF:
        _REF[case] = PC.reference(case)
    return _REF[case]


# one test per fault, over every case the fault is claimed on: the suite runs for every later change
@pytest.mark.parametrize("fault", PC.FAULTS)
def test_planted_fault_changes_every_exact_case(fault):
    cases = [c for c in PC.EXACT if PC.fault_applies(c, fault)]
    assert cases
    for case in cases:
        dx, u, _, _ = _reference(case)
        dxf, uf, _, _ = PC.reference(case, fault)
        assert (dx != dxf).any(), case.id
        if case.r and fault in ("drop_last_rows", "drop_L_last", "drop_uscale", "flip_L", "lscale_for_lk",
                                "rscale_for_rk"):
            assert (u != uf).any(), case.id


@pytest.mark.parametrize("fault", PC.FAULTS)
def test_planted_fault_exceeds_ten_bars_on_random_cases(fault):
    cases = [c for c in PC.RANDOM if PC.fault_applies(c, fault)]
    assert cases
    worst = {}
    for case in cases:
        dx, _, bar, _ = _reference(case)
        dxf, _, _, _ = PC.reference(case, fault)
        worst[case.id] = (np.abs(dxf - dx) / bar).max()
    low = min(worst, key=worst.get)
    print(f"{fault}: {len(cases)} random cases, smallest {worst[low]:.1f} bars ({low})")
    assert worst[low] >= 10, (low, worst[low])


def test_every_fault_meets_exact_and_random_cases():
    new = ("drop_uscale", "lscale_for_lk", "rscale_for_rk", "flip_L", "flip_R", "tr_block_R", "L_tail", "R_rows")
    assert set(new) <= set(PC.FAULTS)
    for cases in (PC.EXACT, PC.RANDOM):
        assert {f for c in cases for f in PC.FAULTS if PC.fault_applies(c, f)} == set(PC.FAULTS)
    # the scale faults on every case that has the scale; the tail faults where a piece straddles r
    for c in PC.EXACT + PC.RANDOM:
        assert PC.fault_applies(c, "drop_uscale") == (c.r > 0)
        assert PC.fault_applies(c, "lscale_for_lk") == (c.r > 0 and c.lb == 4)
        assert PC.fault_applies(c, "rscale_for_rk") == (c.r > 0 and c.rb == 4)
        assert PC.fault_applies(c, "L_tail") == (c.r % 16 != 0 and c.lb != 16)
        assert PC.fault_applies(c, "R_rows") == (c.r % 16 != 0 and c.lb != 16 and c.rb != 16)


# ---------------------------------------------------------------------------- the ABI
def _struct_fields(name):
    txt = open(HEADER).read()
    body = txt[txt.index(f"typedef struct {name}"):txt.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*[;,]", body.split("{", 1)[1])


def test_packed_backward_args_struct_matches_header():
    fields = [f for f, _ in K.LinearPackedBackwardArgs._fields_]
    assert fields == _struct_fields("cq_linear_packed_backward_args")
    plain = [f for f, _ in K.LinearBackwardArgs._fields_]
    assert fields == plain + ["l_bits", "r_bits", "L_codes", "l_code_stride", "R_codes", "r_code_stride", "lscale",
                              "rscale"]
    assert fields[len(plain):] == [f for f, _ in K.LinearPackedArgs._fields_][len(K.LinearArgs._fields_):]
    for f, _ in K.LinearBackwardArgs._fields_:     # the plain struct is the leading part
        assert getattr(K.LinearPackedBackwardArgs, f).offset == getattr(K.LinearBackwardArgs, f).offset
    txt = open(HEADER).read()
    assert int(re.search(r"#define CQ_ABI_VERSION (\d+)", txt).group(1)) == K.ABI_VERSION == 5
    assert K.load().cq_abi_version() == 5
    assert {"cq_linear_packed_backward_workspace", "cq_linear_packed_backward_input"} <= set(K.EXPORTS)


def _args(base, **kw):
    a = K.LinearPackedBackwardArgs()
    a.dy, a.lddy, a.tokens, a.m, a.n, a.r, a.bits = base, 16, 1, 16, 64, 8, 2
    a.codes, a.code_stride, a.qscale, a.gscale = base + 256, 16, 1.0, 1.0
    a.dx, a.dx_dtype, a.lddx = base + 1024, K.CQ_F32, 64
    a.l_bits, a.r_bits = 4, 2
    a.L_codes, a.l_code_stride, a.lscale = base + 2048, 16, 1.0
    a.R_codes, a.r_code_stride, a.rscale = base + 3072, 16, 1.0
    for key, v in kw.items():
        setattr(a, key, v)
    return a


def test_packed_backward_entry_rejects_bad_arguments_without_a_device():
    """Validation runs before any HIP call: CQ_EINVAL with a message."""
    lib = K.load()
    buf = torch.zeros(8192, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16
    ws = base + 6144
    fp16 = dict(l_bits=16, r_bits=16, L=base + 2048, ldl=8, R=base + 3072, ldr=64)
    bad = (  # the plain entry's cases ...
        (dict(bits=3), "bits"), (dict(r=K.LINEAR_MAX_RANK + 1), "rank"), (dict(codes=base + 260), "aligned"),
        (dict(code_stride=24), "aligned"), (dict(dy=base + 1), "misaligned"), (dict(dx=base + 1026), "misaligned"),
        (dict(u_out=base + 4098, ldu=8), "misaligned"), (dict(lddy=15), "leading"), (dict(lddx=63), "leading"),
        (dict(u_out=base + 4096, ldu=7), "leading"), (dict(dx_dtype=7), "dtype"),
        (dict(fp16, L=base + 2049), "misaligned"), (dict(fp16, ldr=63), "leading"),
        (dict(fp16, l_bits=4, L_codes=0, ldr=63), "L codes"),
        # ... and those cq_linear_packed_forward adds for factor codes
        (dict(l_bits=3), "factor bits"), (dict(r_bits=8), "factor bits"), (dict(l_bits=0), "factor bits"),
        (dict(L_codes=0), "null L codes"), (dict(R_codes=0), "null R codes"),
        (dict(L_codes=base + 2052), "L codes and their row stride"), (dict(R_codes=base + 3080), "R codes and their"),
        (dict(l_code_stride=24), "L codes and their row stride"), (dict(r_code_stride=8), "R codes and their"),
        (dict(l_code_stride=0), "L code row stride"), (dict(n=128, lddx=128, code_stride=32), "R code row stride"),
        (dict(lscale=-1.0), "L scale"), (dict(lscale=float("inf")), "L scale"), (dict(rscale=float("nan")), "R scale"))
    for kw, word in bad:
        a = _args(base, **kw)
        assert lib.cq_linear_packed_backward_input(ctypes.byref(a), ws, 2048, None) == K.CQ_EINVAL, kw
        msg = lib.cq_last_error().decode()
        assert word in msg and "cq_linear_packed_backward_input" in msg, (kw, msg)
    # a coded factor's fp16 pointer and leading dimension are ignored, an fp16 factor's code fields too
    for kw in (dict(L=base + 1, ldl=0, R=base + 3, ldr=0), dict(fp16, L_codes=base + 1, l_code_stride=3, lscale=-1.0,
                                                                 R_codes=0, r_code_stride=-5, rscale=float("nan"))):
        assert lib.cq_linear_packed_backward_input(ctypes.byref(_args(base, tokens=0, **kw)), None, 0, None) == 0, kw
    # r = 0: the factor fields are not looked at
    assert lib.cq_linear_packed_backward_input(ctypes.byref(_args(base, tokens=0, r=0, L_codes=0, R_codes=0)),
                                               None, 0, None) == 0
    a = _args(base)
    need = lib.cq_linear_packed_backward_workspace(ctypes.byref(a))
    assert need == 2 * 1 * 32 * 2
    assert lib.cq_linear_packed_backward_input(ctypes.byref(a), ws, need - 1, None) == K.CQ_EINVAL
    assert "workspace" in lib.cq_last_error().decode()
    assert lib.cq_linear_packed_backward_input(ctypes.byref(a), None, 0, None) == K.CQ_EINVAL
    assert lib.cq_linear_packed_backward_input(None, None, 0, None) == K.CQ_EINVAL


def test_workspace_depends_on_tokens_and_rank_alone():
    """The same function as cq_linear_backward_workspace, whatever m, n and the factor formats."""
    lib = K.load()

    def ws(**kw):
        return lib.cq_linear_packed_backward_workspace(ctypes.byref(_args(0, **dict(dict(tokens=512, r=128), **kw))))

    plain = K.LinearBackwardArgs()
    plain.tokens, plain.m, plain.n, plain.r, plain.bits = 512, 64, 64, 128, 2
    base = ws(m=64, n=64)
    assert base == lib.cq_linear_backward_workspace(ctypes.byref(plain)) == 2 * 512 * 128 * 2
    assert base == ws(m=8192, n=8192) == ws(m=8192, n=64) == ws(m=64, n=8192)
    assert base == ws(l_bits=16) == ws(r_bits=4) == ws(l_bits=2, r_bits=16)
    assert ws(r=0) == 0 and ws(tokens=0) == 0 and ws(tokens=1024) == 2 * base and ws(r=256) == 2 * base


def test_python_wrapper_raises_value_errors():
    dy, dx = torch.zeros(2, 12, dtype=torch.float16), torch.zeros(2, 198)
    codes = torch.zeros(12, 64, dtype=torch.uint8)
    Lc, Rc = torch.zeros(12, 16, dtype=torch.uint8), torch.zeros(5, 64, dtype=torch.uint8)
    L, R = torch.zeros(12, 5, dtype=torch.float16), torch.zeros(5, 198, dtype=torch.float16)
    ok = dict(dy=dy, dx=dx, L=None, R=None, r=5, L_codes=(Lc, 0.5, 4), R_codes=(Rc, 0.5, 2), u_out=None)

    def call(**kw):
        o = dict(ok, **kw)
        return K.linear_packed_backward_args(o["dy"], codes, 1.0, 1.0, o["L"], o["R"], o["dx"], m=12, n=198, bits=2,
                                             r=o["r"], L_codes=o["L_codes"], R_codes=o["R_codes"], u_out=o["u_out"])

    a = call()
    assert (a.l_bits, a.r_bits, a.r, a.l_code_stride, a.r_code_stride) == (4, 2, 5, 16, 64) and not a.L and not a.R
    a = call(L=L, L_codes=None, r=None)
    assert (a.l_bits, a.r_bits, a.r, a.ldl) == (16, 2, 5, 5) and not a.L_codes
    for kw, word in ((dict(dy=dy.float()), "dy must be fp16"), (dict(dx=dx.double()), "dx must be"),
                     (dict(dx=dx[:, :5]), "do not fit"), (dict(u_out=torch.zeros(2, 4)), "u_out"),
                     (dict(r=None), "r is needed"), (dict(L=L), "exactly one of L"), (dict(R_codes=None), "exactly one of R"),
                     (dict(R=R.float(), R_codes=None), "fp16"), (dict(L=L[:, :4], L_codes=None), "do not fit"),
                     (dict(L_codes=(Lc[:5], 0.5, 4)), "L_codes must be"), (dict(R_codes=(Rc.int(), 0.5, 2)), "R_codes must be")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    with pytest.raises(RuntimeError, match="HIP"):
        K.linear_packed_backward_input(dy, codes, 1.0, 1.0, None, None, dx, m=12, n=198, bits=2, r=5,
                                       L_codes=(Lc, 0.5, 4), R_codes=(Rc, 0.5, 2))


# ---------------------------------------------------------------------------- the layers, model.py
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
    return CalderaLinear.from_codes(c, L, R, b, qscale=0.37, gscale=1.25, bits=bits)


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.dense = torch.nn.Linear(13, 13)
        self.had = HadamardCalderaLinear(_layer(m=8, n=16, r=2, bias=False, seed=1), 13, 6)
        self.coded = _layer(m=7, n=6, r=3, coded=True, seed=2)
        self.had_coded = HadamardCalderaLinear(_layer(m=8, n=8, r=2, bias=False, coded=True, seed=3), 7, 5)
        self.plain = _layer(m=4, n=5, r=2, bits=4, seed=4)


def test_hadamard_layer_delegates_the_training_surface():
    had = _Net().had
    keys = list(had.state_dict())
    L16 = had.inner.L.clone()
    assert not had.factors_trainable
    params = had.enable_factor_training()
    assert had.factors_trainable and params[0] is had.inner.L and params[1] is had.inner.R
    assert [name for name, _ in had.named_parameters()] == ["inner.L", "inner.R"]
    assert all(p.dtype == torch.float32 and p.requires_grad for p in params)
    assert had.freeze_factors() is had and not had.factors_trainable and not list(had.parameters())
    assert set(had.state_dict()) == set(keys) and torch.equal(had.inner.L, L16)
    with pytest.raises(ValueError, match="coded"):
        _Net().had_coded.enable_factor_training()
    with pytest.raises(RuntimeError, match="HIP"):
        had(torch.zeros(2, 13, requires_grad=True))


def test_prepare_factor_finetuning_keywords():
    net = _Net()
    keys = list(net.state_dict())
    # the defaults refuse as before, naming the layers and changing nothing
    with pytest.raises(ValueError) as err:
        M.prepare_factor_finetuning(net)
    msg = str(err.value)
    assert "packed layers without a backward" in msg and "had (Hadamard basis)" in msg and "coded (coded factors)" in msg
    assert "had_coded" in msg and "inner" not in msg and "plain" not in msg
    assert not net.plain.factors_trainable
    # one keyword alone still refuses what it does not admit
    with pytest.raises(ValueError) as err:
        M.prepare_factor_finetuning(net, hadamard=True)
    assert "coded (coded factors)" in str(err.value) and "had_coded (Hadamard basis, coded factors)" in str(err.value)
    assert "had (" not in str(err.value)
    with pytest.raises(ValueError) as err:
        M.prepare_factor_finetuning(net, coded_factors="freeze")
    assert "had (Hadamard basis)" in str(err.value) and "had_coded (Hadamard basis)" in str(err.value)
    assert "coded factors" not in str(err.value) and not net.plain.factors_trainable
    for value in ("train", None, True, ""):
        with pytest.raises(ValueError, match="coded_factors"):
            M.prepare_factor_finetuning(net, coded_factors=value)
    params = M.prepare_factor_finetuning(net, torch.float64, hadamard=True, coded_factors="freeze")
    assert [id(p) for p in params] == [id(p) for p in (net.had.inner.L, net.had.inner.R, net.plain.L, net.plain.R)]
    assert all(p.dtype == torch.float64 for p in params)
    names = {name for name, _ in net.named_parameters()}
    assert names == {"dense.weight", "dense.bias", "had.inner.L", "had.inner.R", "plain.L", "plain.R"}
    assert not net.coded.factors_trainable and not net.had_coded.factors_trainable
    assert net.coded.R.dtype == torch.float16 and not isinstance(net.coded.R, torch.nn.Parameter)
    with torch.no_grad():
        net.had.inner.L.add_(2.0 ** -12)
        want = net.had.inner.L.detach().to(torch.float16)
    assert M.finish_factor_finetuning(net) is net
    assert {name for name, _ in net.named_parameters()} == {"dense.weight", "dense.bias"}
    assert set(net.state_dict()) == set(keys) and net.had.inner.L.dtype == torch.float16
    assert torch.equal(net.had.inner.L, want) and not net.had.factors_trainable
