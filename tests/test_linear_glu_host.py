"""CPU side of the gated pair (cq_linear_glu_forward, CalderaGatedMLP, model.fuse_gated_mlps): the C ABI
and its argument checks without a device, the workspace, the cases of linear_glu_cases.py (all there, the
exact ones exact, the planted faults beyond ten bars), and fuse / unfuse on CPU tensors."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import linear_glu_cases as UC
from linear_glu_cases import ACT_IDENTITY, ACT_SILU, f32, f64
from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import model as M
from ee274_convexcaldera_llm_quantization_amd.linear import (CalderaGatedMLP, CalderaLinear, CalderaLinearGroup,
                                                              HadamardCalderaLinear, row_bytes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "caldera_hip.h")


# ---------------------------------------------------------------------------- the ABI
def _struct_fields(name):
    txt = open(HEADER).read()
    body = txt[txt.index(f"typedef struct {name}"):txt.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*[;,]", body.split("{", 1)[1])


def test_glu_abi_is_additive():
    txt = open(HEADER).read()
    assert int(re.search(r"#define CQ_ABI_VERSION (\d+)", txt).group(1)) == K.ABI_VERSION == 5
    assert int(re.search(r"#define CQ_ACT_IDENTITY\s+(\d+)", txt).group(1)) == K.ACT_IDENTITY == ACT_IDENTITY == 0
    assert int(re.search(r"#define CQ_ACT_SILU\s+(\d+)", txt).group(1)) == K.ACT_SILU == ACT_SILU == 1
    new = {"cq_linear_glu_workspace", "cq_linear_glu_forward"}
    assert new <= set(K.EXPORTS)
    lib = K.load()                      # raises for a missing export
    assert lib.cq_abi_version() == 5
    assert _struct_fields("cq_linear_glu_args") == [f for f, _ in K.LinearGluArgs._fields_] \
        == ["gate", "up", "q_format", "act", "h", "h_dtype", "ldh"]
    P = ctypes.sizeof(K.LinearPackedArgs)
    assert P % 8 == 0
    G = K.LinearGluArgs
    assert (G.gate.offset, G.up.offset, G.q_format.offset, G.act.offset, G.h.offset, G.h_dtype.offset, G.ldh.offset) \
        == (0, P, 2 * P, 2 * P + 4, 2 * P + 8, 2 * P + 16, 2 * P + 24) and ctypes.sizeof(G) == 2 * P + 32
    assert G._fields_[0][1] is K.LinearPackedArgs and G._fields_[1][1] is K.LinearPackedArgs
    assert [f for f, _ in K.LinearPackedArgs._fields_] == _struct_fields("cq_linear_packed_args")   # unchanged
    assert _struct_fields("cq_linear_group_args") == ["count", "q_format", "members"]               # unchanged


def _raw(ranks=(8, 8), q_format=K.QFMT_UNIFORM, act=K.ACT_SILU, h_dtype=K.CQ_F32, **member_kw):
    """A valid pair on host memory (never launched); member_kw: {field: (member name, value)}."""
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16
    a = K.LinearGluArgs()
    for i, name in enumerate(("gate", "up")):
        p = getattr(a, name)
        p.x, p.ldx, p.tokens, p.m, p.n, p.r, p.bits = base, 64, 1, 24, 64, ranks[i], 4
        p.codes, p.code_stride, p.qscale, p.gscale = base + 256 + 1024 * i, 32, 1.0, 1.0
        p.L, p.ldl, p.R, p.ldr = base + 4096, 8, base + 6144, 64
        p.l_bits = p.r_bits = 16               # y, y_dtype, ldy stay zero: not used, not checked
    for key, (name, v) in member_kw.items():
        setattr(getattr(a, name), key, v)
    a.q_format, a.act = q_format, act
    a.h, a.h_dtype, a.ldh = base + 16384, h_dtype, 24
    a._keep = buf
    return a, base


def test_glu_entry_rejects_bad_arguments_without_a_device():
    """Decided on the host before any launch: CQ_EINVAL with a message naming the member and the field."""
    lib = K.load()

    def refused(a, *words):
        assert lib.cq_linear_glu_forward(ctypes.byref(a), None, 0, None) == K.CQ_EINVAL, words
        msg = lib.cq_last_error().decode()
        for w in words:
            assert w in msg, (w, msg)

    assert lib.cq_linear_glu_forward(None, None, 0, None) == K.CQ_EINVAL
    ok, _ = _raw()
    ok.gate.tokens = ok.up.tokens = 0
    assert lib.cq_linear_glu_forward(ctypes.byref(ok), None, 0, None) == 0          # tokens == 0: CQ_OK, no launch
    assert ok.gate.y is None and ok.up.y is None and ok.gate.ldy == 0                # the y fields are not checked
    refused(_raw(q_format=2)[0], "q_format")
    refused(_raw(act=2)[0], "act 2")
    refused(_raw(act=-1)[0], "act")
    refused(_raw(h_dtype=7)[0], "h_dtype")
    for field, value in (("x", lambda b: b + 16), ("ldx", lambda b: 72), ("tokens", lambda b: 2), ("n", lambda b: 48),
                         ("m", lambda b: 16), ("bits", lambda b: 2)):
        a, base = _raw()
        setattr(a.up, field, value(base))
        refused(a, "up", field, "gate's")
    # the pair's own fields
    a, _ = _raw()
    a.ldh = 23
    refused(a, "ldh")
    a, _ = _raw()
    a.h = None
    refused(a, "null h")
    a, _ = _raw()
    a.h = a.h + 2
    refused(a, "misaligned h")
    a, _ = _raw(h_dtype=K.CQ_F16)
    a.h = a.h + 1
    refused(a, "misaligned h")
    a, _ = _raw(h_dtype=K.CQ_F16)
    a.h = a.h + 2                                       # fp16 h needs 2-byte alignment only
    a.gate.tokens = a.up.tokens = 0
    assert lib.cq_linear_glu_forward(ctypes.byref(a), None, 0, None) == 0
    # the factor formats: only where both members have r > 0
    a, base = _raw(l_bits=("up", 4), L_codes=("up", 0), l_code_stride=("up", 16), lscale=("up", 1.0))
    a.up.L_codes = base + 8192
    refused(a, "up", "l_bits")
    a, base = _raw(r_bits=("up", 4), r_code_stride=("up", 32), rscale=("up", 1.0))
    a.up.R_codes = base + 8192
    refused(a, "up", "r_bits")
    a, _ = _raw(ranks=(8, 0), l_bits=("up", 4), r_bits=("up", 2))   # a member with r = 0 fits any factor format
    assert lib.cq_linear_glu_workspace(ctypes.byref(a)) > 0
    a.gate.tokens = a.up.tokens = 0
    assert lib.cq_linear_glu_forward(ctypes.byref(a), None, 0, None) == 0
    # a member's own check, with the member named
    refused(_raw(code_stride=("up", 17))[0], "up", "aligned")
    refused(_raw(r=("gate", K.LINEAR_MAX_RANK + 1))[0], "gate", "rank")
    refused(_raw(bits=("gate", 3))[0], "gate", "bits")
    refused(_raw(codes=("gate", None))[0], "gate", "null")
    refused(_raw(q_format=K.QFMT_NF, qscale=("up", float("nan")))[0], "up", "NF scale")
    refused(_raw(q_format=K.QFMT_NF, qscale=("gate", -1.0))[0], "gate", "NF scale")


@pytest.mark.parametrize("tokens", [1, 16, 17, 130])
@pytest.mark.parametrize("ranks", [(8, 8), (40, 0), (0, 264), (0, 0)], ids=str)
def test_glu_workspace_is_the_two_member_groups(tokens, ranks):
    lib = K.load()
    a, _ = _raw(ranks=ranks)
    arr = (K.LinearPackedArgs * 2)()
    total = 0
    for i, name in enumerate(("gate", "up")):
        p = getattr(a, name)
        p.tokens, p.ldl = tokens, 264
        own = lib.cq_linear_packed_workspace(ctypes.byref(p))
        assert (own == 0) == (p.r == 0)
        total += (own + 15) // 16 * 16
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(p), ctypes.sizeof(K.LinearPackedArgs))
    g = K.LinearGroupArgs()
    g.count, g.q_format = 2, K.QFMT_UNIFORM
    g.members = ctypes.cast(arr, ctypes.POINTER(K.LinearPackedArgs))
    assert lib.cq_linear_glu_workspace(ctypes.byref(a)) == total == lib.cq_linear_group_workspace(ctypes.byref(g))
    assert lib.cq_linear_glu_workspace(None) == 0
    if total:   # too small a workspace is refused before any launch
        buf = torch.zeros(64, dtype=torch.uint8)
        ws = (buf.data_ptr() + 15) // 16 * 16
        assert lib.cq_linear_glu_forward(ctypes.byref(a), ws, 16, None) == K.CQ_EWORKSPACE


def test_glu_args_builder_checks_like_the_c_entry():
    x = torch.zeros(2, 198, dtype=torch.float16)

    def member(m=12, r=5, bits=4, n=198, **kw):
        d = dict(codes=torch.zeros(m, row_bytes(n, bits), dtype=torch.uint8), qscale=1.0, gscale=1.0,
                 L=torch.zeros(m, r, dtype=torch.float16) if r else None,
                 R=torch.zeros(r, n, dtype=torch.float16) if r else None, bias=None, m=m, n=n, bits=bits, r=r)
        d.update(kw)
        return d

    h = torch.zeros(2, 12)
    a = K.linear_glu_args(x, member(), member(r=0), h, K.QFMT_UNIFORM, K.ACT_SILU)
    assert (a.gate.m, a.gate.r, a.up.m, a.up.r, a.gate.x, a.up.x) == (12, 5, 12, 0, x.data_ptr(), x.data_ptr())
    assert (a.q_format, a.act, a.h, a.h_dtype, a.ldh) == (K.QFMT_UNIFORM, K.ACT_SILU, h.data_ptr(), K.CQ_F32, 12)
    assert a.gate.y is None and a.up.y is None and a.gate.ldy == a.up.ldy == 0
    view = torch.zeros(2, 20, dtype=torch.float16)[:, 3:15]
    a = K.linear_glu_args(x, member(), member(), view, K.QFMT_NF, K.ACT_IDENTITY)
    assert (a.act, a.h_dtype, a.ldh, a.h) == (K.ACT_IDENTITY, K.CQ_F16, 20, view.data_ptr())
    lib = K.load()
    assert lib.cq_linear_glu_workspace(ctypes.byref(a)) == 2 * 16 * 16 * 32 * 4
    coded = member(L=None, L_codes=(torch.zeros(12, 16, dtype=torch.uint8), 1.0, 4))
    for gate, up, out, qf, act, words in (
            (member(), member(), h, 5, 1, ("q_format",)),
            (member(), member(), h, 0, 2, ("act",)),
            (member(), member(), torch.zeros(2, 12, dtype=torch.bfloat16), 0, 1, ("h must be fp32 or fp16",)),
            (member(), member(), torch.zeros(2, 13), 0, 1, ("h (2, 13)",)),
            (member(), member(), torch.zeros(12, 2).t(), 0, 1, ("unit column stride",)),
            (member(), member(), torch.zeros(1, 12).expand(2, 12), 0, 1, ("ldh",)),
            (member(), member(m=20), h, 0, 1, ("up", "m 20")),
            (member(), member(bits=2), h, 0, 1, ("up", "bits")),
            (member(), member(n=64), h, 0, 1, ("up",)),
            (member(), coded, h, 0, 1, ("up", "l_bits")),
            (member(), member(qscale=float("inf")), h, K.QFMT_NF, 1, ("up", "NF scale")),
            (member(L=torch.zeros(12, 5)), member(), h, 0, 1, ("gate", "fp16"))):
        with pytest.raises(ValueError) as e:
            K.linear_glu_args(x, gate, up, out, qf, act)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        assert str(e.value).count("cq_linear:") == 1, str(e.value)
    K.linear_glu_args(x, member(r=0), coded, h, 0, 1)          # a member with r = 0 fits any factor format
    with pytest.raises(RuntimeError, match="HIP device"):
        K.linear_glu_forward(x, member(), member(), h, K.QFMT_UNIFORM)


# ---------------------------------------------------------------------------- the cases
def test_the_issues_cases_are_all_there():
    assert UC.SHAPES == ((33, 64, 8, 8), (48, 198, 40, 0), (80, 898, 200, 8), (272, 512, 16, 16), (48, 2600, 40, 40))
    q = {("uniform", 2), ("uniform", 4), ("nf", 4), ("nf", 2)}
    for s in UC.SHAPES:
        mine = [c for c in UC.ALL if (c.m, c.n, c.rg, c.ru) == s and c.lb == c.rb == 16 and c.bias == 0]
        assert {(c.fmt, c.bits, c.T) for c in mine} == {(f, b, T) for f, b in q for T in (1, 5, 16, 17, 64, 130)}
    fac = [c for c in UC.ALL if (c.lb, c.rb) != (16, 16)]
    assert {(c.m, c.n, c.rg, c.ru, c.lb, c.rb, c.T, c.fmt, c.bits) for c in fac} == \
        {(48, 198, 40, 40, lb, rb, T, f, b) for lb, rb in ((4, 4), (2, 16)) for T in (16, 17) for f, b in q}
    biased = [c for c in UC.ALL if c.bias]
    assert {(c.m, c.n, c.rg, c.ru) for c in biased} == {(33, 64, 8, 8)}
    assert {(c.bias, c.fmt, c.bits) for c in biased} == {(b, f, bb) for b in (1, 2) for f, bb in q}
    assert {c.T <= 16 for c in biased} == {True, False}
    for c in biased:
        d = UC.inputs(c)["members"]
        assert d[0]["bias"] is not None and (d[1]["bias"] is not None) == (c.bias == 2)
        assert c.bias < 2 or not np.array_equal(d[0]["bias"], d[1]["bias"])
    assert {(c.m, c.n) for c in UC.ALL if UC.has_f16(c)} == {(33, 64), (48, 198)}
    assert len({c.id for c in UC.ALL + UC.EXACT}) == len(UC.ALL) + len(UC.EXACT)
    # the shapes do what the issue picked them for: a partial third prefill workgroup of 128 rows, fewer rows
    # than one, two chunks per decode wave
    assert -(-272 // 128) == 3 and 272 % 128 and 80 < 128 and -(-2600 // 256) > 8
    # x is shared, the members differ, and the pad tails hold nonzero codes
    c = next(c for c in UC.ALL if (c.n, c.lb, c.fmt, c.bits) == (198, 4, "uniform", 2))
    d = UC.inputs(c)
    g, u = d["members"]
    assert not np.array_equal(g["V"], u["V"]) and g["gs"] != u["gs"]
    from ee274_convexcaldera_llm_quantization_amd.linear import unpack_bytes
    for codes, bits, cols in ((UC.packed_codes(c, g), 2, 198), (UC.factor_operand(c, g, "l")[1], 4, 40),
                              (UC.factor_operand(c, g, "rho")[1], 4, 198)):
        full = unpack_bytes(torch.from_numpy(codes), bits).numpy()
        assert full.shape[1] > cols and (full[:, cols:] != 0).all()
    assert np.array_equal(unpack_bytes(torch.from_numpy(UC.packed_codes(c, g)), 2).numpy()[:, :198], g["V"])
    nf = next(c for c in UC.ALL if (c.n, c.fmt, c.bits) == (198, "nf", 2))
    from ee274_convexcaldera_llm_quantization_amd.linear import unpack_index_bytes
    full = unpack_index_bytes(torch.from_numpy(UC.packed_codes(nf, UC.inputs(nf)["members"][0])), 2).numpy()
    assert (full[:, 198:] == 3).all() and np.array_equal(full[:, :198], UC.inputs(nf)["members"][0]["V"])


@pytest.mark.parametrize("case", UC.EXACT, ids=lambda c: c.id)
def test_the_reference_is_exact_on_the_integer_identity_cases(case):
    """Per member the sum of absolute terms stays below 2^24 units and z~ splits exactly, so v_g and v_u are
    fp32 values in every summation order; their product is one, too: the fp64 reference is what an exact
    kernel gives, bit for bit."""
    for (units, unit, split), mem in zip(UC.exact_units(case), UC.inputs(case)["members"]):
        assert units < 2 ** 24 and split and unit in (0.25, 0.5, 1.0)
        assert mem["bias"] is None and float(mem["gs"]) in (2.0, 4.0)
    (g, u), _ = UC.preactivations(case)
    h, _ = UC.reference(case, ACT_IDENTITY)
    for a in (g, u, h):
        assert np.array_equal(a.astype(f32).astype(f64), a)
    assert np.array_equal((g.astype(f32) * u.astype(f32)).astype(f64), h) and np.abs(h).max() > 0
    assert {c.T <= 16 for c in UC.EXACT} == {True, False}


@pytest.mark.parametrize("case", UC.ALL, ids=lambda c: c.id)
def test_every_planted_fault_exceeds_ten_bars(case):
    """On every random case, for both activations, every fault that applies to it."""
    for act in (ACT_SILU, ACT_IDENTITY):
        good, bar = UC.reference(case, act)
        assert (bar > 0).all()
        for fault in UC.FAULTS:
            if UC.fault_applies(case, act, fault):
                bad, _ = UC.reference(case, act, fault)
                assert (np.abs(bad - good) / bar).max() > 10, (act, fault)


def test_every_fault_meets_decode_and_prefill():
    for fault in UC.FAULTS:
        hit = [c for c in UC.ALL if UC.fault_applies(c, ACT_SILU, fault)]
        assert hit and {c.T <= 16 for c in hit} == {True, False}, fault
    # the bound the end-to-end bar rests on
    v = np.linspace(-20, 20, 400001)
    s = 1 / (1 + np.exp(-v))
    assert 1.09 < (s * (1 + v * (1 - s))).max() <= 1.1


# ---------------------------------------------------------------------------- the module
def _layer(m=12, n=40, r=3, bits=2, seed=0, **kw):
    g = torch.Generator().manual_seed(seed + m)
    k = 2 ** (bits - 1) - 1
    c = torch.randint(-k, k + 1, (m, n), generator=g).to(torch.int8)
    L = torch.randn(m, r, generator=g).half() if r and "L_codes" not in kw else None
    R = torch.randn(r, n, generator=g).half() if r else None
    return CalderaLinear.from_codes(c, L, R, None, qscale=0.05, gscale=1.5, bits=bits, **kw)


class _MLP(torch.nn.Module):
    def __init__(self, gate, up, down, act_fn):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj, self.act_fn = gate, up, down, act_fn

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


def _hadamard():
    return HadamardCalderaLinear(_layer(m=16, n=64), 40, 12)


def _model():
    net = torch.nn.Module()
    net.a = _MLP(_layer(seed=1), _layer(seed=2, r=0), _layer(m=40, n=12, seed=3), torch.nn.SiLU())
    net.b = _MLP(_layer(seed=4), _layer(seed=5), torch.nn.Linear(12, 40), torch.nn.functional.silu)
    net.dense = _MLP(torch.nn.Linear(40, 12), _layer(seed=6), torch.nn.Linear(12, 40), torch.nn.SiLU())
    net.had = _MLP(_layer(seed=7), _hadamard(), torch.nn.Linear(12, 40), torch.nn.SiLU())
    net.gelu = _MLP(_layer(seed=8), _layer(seed=9), torch.nn.Linear(12, 40), torch.nn.GELU())
    net.misfit = _MLP(_layer(seed=10), _layer(seed=11, bits=4), torch.nn.Linear(12, 40), torch.nn.SiLU())
    net.other = torch.nn.Linear(4, 4)
    return net


def test_construction_errors_name_the_attribute():
    good = (_layer(seed=1), _layer(seed=2), torch.nn.Linear(12, 40))
    mlp = CalderaGatedMLP(*good)
    assert [n for n, _ in mlp.named_children()] == ["gate_proj", "up_proj", "down_proj"] and mlp.act == "silu"
    assert CalderaGatedMLP(*good, act="identity").act == "identity"
    coded = _layer(seed=3, L_codes=(torch.zeros(12, 3, dtype=torch.int8), 1.0, 4))
    for args, kw, words in (
            ((torch.nn.Linear(40, 12), good[1], good[2]), {}, ("gate_proj", "Linear")),
            ((good[0], _hadamard(), good[2]), {}, ("up_proj", "HadamardCalderaLinear")),
            ((good[0], good[0], good[2]), {}, ("same layer",)),
            ((good[0], _layer(seed=2, bits=4), good[2]), {}, ("up_proj", "bits")),
            ((good[0], _layer(m=13, seed=2), good[2]), {}, ("up_proj", "out_features")),
            ((good[0], _layer(n=48, seed=2), good[2]), {}, ("up_proj", "in_features")),
            ((good[0], coded, good[2]), {}, ("up_proj", "L_bits")),
            ((good[0], good[1], lambda x: x), {}, ("down_proj",)),
            (good, {"act": "gelu"}, ("act", "gelu"))):
        with pytest.raises(ValueError) as e:
            CalderaGatedMLP(*args, **kw)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
    with pytest.raises(ValueError, match="max_fused_tokens"):
        CalderaGatedMLP(*good, max_fused_tokens=1.5)
    CalderaGatedMLP(good[0], _layer(seed=2, r=0), good[2])
    CalderaGatedMLP(_layer(seed=1, r=0), coded, good[2])           # r = 0 fits any factor format
    with pytest.raises(RuntimeError, match="HIP device"):           # the fused path has no CPU fallback
        with torch.no_grad():
            mlp(torch.zeros(2, 40))


def test_fuse_and_unfuse_gated_mlps():
    net = _model()
    before = copy.deepcopy(net.state_dict())
    keys = list(before)
    originals = {name: getattr(net, name) for name in ("a", "b")}
    layers = {name: (getattr(net, name).gate_proj, getattr(net, name).up_proj) for name in ("a", "b")}
    fused, skipped = M.fuse_gated_mlps(net)
    assert fused == ["a", "b"]
    reasons = dict(skipped)
    assert set(reasons) == {"dense", "had", "gelu", "misfit"}
    assert "gate_proj is dense (Linear)" in reasons["dense"]
    assert "up_proj is a HadamardCalderaLinear" in reasons["had"]
    assert "unknown activation" in reasons["gelu"] and "GELU" in reasons["gelu"]
    assert "incompatible" in reasons["misfit"] and "bits" in reasons["misfit"]
    for name in ("a", "b"):
        mod = getattr(net, name)
        assert isinstance(mod, CalderaGatedMLP) and mod.act == "silu"
        assert (mod.gate_proj, mod.up_proj) == layers[name]
        assert mod.__dict__["_original"][0] is originals[name]
        assert "_original" not in mod._modules and all(m is not originals[name] for m in net.modules())
    # the state dict: the same keys, loads in both directions
    assert list(net.state_dict()) == keys
    plain = _model()
    for p in plain.parameters():
        p.data.zero_()
    plain.load_state_dict(net.state_dict())                      # fused -> original
    assert all(torch.equal(v, before[k]) for k, v in plain.state_dict().items() if torch.is_tensor(v))
    net.load_state_dict(before)                                   # original -> fused
    # a second pass fuses nothing more
    again, skipped2 = M.fuse_gated_mlps(net)
    assert again == [] and dict(skipped2)["a"] == "already fused"
    # an explicit act overrides; a block with state of its own and the model itself are left alone
    net2 = _model()
    net2.gelu.extra = torch.nn.Linear(2, 2)
    fused2, skipped2 = M.fuse_gated_mlps(net2, act="identity")
    assert fused2 == ["a", "b"] and net2.a.act == "identity" and "extra" in dict(skipped2)["gelu"]
    root = _MLP(_layer(seed=1), _layer(seed=2), torch.nn.Linear(12, 40), torch.nn.SiLU())
    assert M.fuse_gated_mlps(root) == ([], [("<model>", "the model itself is the block (nothing to replace it in)")])
    with pytest.raises(ValueError):
        M.fuse_gated_mlps(net2, act="gelu")
    # unfuse: the original modules by identity, with the layers the fused modules hold now
    new_up = _layer(seed=99)
    net.a.up_proj = new_up
    assert M.unfuse_gated_mlps(net) == ["a", "b"]
    assert net.a is originals["a"] and net.b is originals["b"] and net.a.up_proj is new_up
    assert list(net.state_dict()) == keys
    assert M.unfuse_gated_mlps(net) == []


def test_the_model_helpers_work_on_a_fused_model(monkeypatch):
    net = _model()
    M.fuse_gated_mlps(net)
    names = M.set_dense_prefill(net, 64)
    assert {"a.gate_proj", "a.up_proj", "a.down_proj", "b.gate_proj", "b.up_proj"} <= set(names)
    assert net.a.gate_proj.dense_prefill_tokens == 64
    x = torch.zeros(64, 40)
    with torch.no_grad():
        assert not net.a._fused(x) and net.a._fused(x[:63])
    M.set_dense_prefill(net, None)
    # a group of gate / up is neither used nor disturbed by the fused module
    grouped, _ = M.group_shared_input_layers(net, sets=(("gate_proj", "up_proj"),))
    assert ("a.gate_proj", "a.up_proj") in grouped and isinstance(net.a.gate_proj.group, CalderaLinearGroup)
    calls = []
    monkeypatch.setattr(K, "linear_glu_forward", lambda x2, g, u, h, qf, act, ws=None: (calls.append((g["m"], act)),
                                                                                     h.fill_(2.0))[1])
    with torch.no_grad():
        h = net.a.glu(torch.zeros(2, 3, 40, dtype=torch.bfloat16))
    assert calls == [(12, K.ACT_SILU)] and h.shape == (2, 3, 12) and h.dtype == torch.bfloat16 and (h == 2).all()
    assert net.a.gate_proj.group is not None and net.a.gate_proj.group._kept == {}
    monkeypatch.undo()
    # the token limit: none at 2 bits, 64 tokens at 4 bits by default (where the fused launch was measured slower)
    from ee274_convexcaldera_llm_quantization_amd.linear import FUSED_TOKEN_LIMIT
    assert FUSED_TOKEN_LIMIT == {2: None, 4: 64} and net.a._fused(torch.zeros(4096, 40))
    four = (_layer(seed=1, bits=4), _layer(seed=2, bits=4), torch.nn.Identity())
    mlp4 = CalderaGatedMLP(*four)
    assert mlp4._fused(torch.zeros(64, 40)) and not mlp4._fused(torch.zeros(65, 40))
    assert CalderaGatedMLP(*four, max_fused_tokens=None)._fused(torch.zeros(4096, 40))
    assert not CalderaGatedMLP(*four, max_fused_tokens=16)._fused(torch.zeros(17, 40))
    # trainable factors: the fallback; frozen again: fused
    params = M.prepare_factor_finetuning(net.a)
    assert len(params) == 4 and not net.a._fused(torch.zeros(2, 40))
    M.finish_factor_finetuning(net.a)
    assert net.a._fused(torch.zeros(2, 40)) and not net.a._fused(torch.zeros(2, 40, requires_grad=True))
    # unpacking: the fused module holds dense layers then and takes the formula
    M.ungroup_shared_input_layers(net)
    monkeypatch.setattr(CalderaLinear, "materialize", lambda self, dtype=torch.float16, out=None:
                        torch.zeros(self.out_features, self.in_features, dtype=dtype))
    done = M.unpack_packed_layers(net.a, torch.float32)
    assert set(done) == {"gate_proj", "up_proj", "down_proj"} and isinstance(net.a.gate_proj, torch.nn.Linear)
    x = torch.randn(3, 40)
    want = net.a.down_proj(torch.nn.functional.silu(net.a.gate_proj(x)) * net.a.up_proj(x))
    assert not net.a._fused(x) and torch.equal(net.a(x), want)
