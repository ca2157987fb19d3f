"""CPU side of the grouped and gated Hadamard launches (cq_hadamard_group_rows, cq_hadamard_glu_rows,
HadamardLinearGroup, HadamardGatedMLP, model.group_shared_input_layers / fuse_gated_mlps with hadamard=True):
the C ABI and its argument checks without a device, the cases of hadamard_group_cases.py (the planted
faults beyond ten bars), the classes' construction errors, state dicts, the launch sequences with the
`_lib` entries replaced by recorders, and the model helpers on a toy model."""
import copy
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

import hadamard_group_cases as GC
from hadamard_group_cases import ACT_IDENTITY, ACT_SILU
from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import linear as LN
from ee274_convexcaldera_llm_quantization_amd import model as M
from ee274_convexcaldera_llm_quantization_amd.linear import (CalderaGatedMLP, CalderaLinear, CalderaLinearGroup,
                                                              HadamardCalderaLinear, HadamardGatedMLP,
                                                              HadamardLinearGroup)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "caldera_hip.h")


# ---------------------------------------------------------------------------- the ABI
def _struct_fields(name):
    txt = open(HEADER).read()
    body = txt[txt.index(f"typedef struct {name}"):txt.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*[;,]", body.split("{", 1)[1])


def test_the_abi_is_additive():
    txt = open(HEADER).read()
    assert int(re.search(r"#define CQ_ABI_VERSION (\d+)", txt).group(1)) == K.ABI_VERSION == 5
    assert int(re.search(r"#define CQ_HADAMARD_GROUP_MAX (\d+)", txt).group(1)) == K.HADAMARD_GROUP_MAX == 8
    assert int(re.search(r"#define CQ_HADAMARD_GLU_MAX_N (\d+)", txt).group(1)) == K.HADAMARD_GLU_MAX_N == 16384
    assert {"cq_hadamard_group_rows", "cq_hadamard_glu_rows"} <= set(K.EXPORTS)
    lib = K.load()                      # raises for a missing export
    assert lib.cq_abi_version() == 5
    H = K.HadamardArgs
    assert [f for f, _ in H._fields_] == _struct_fields("cq_hadamard_args")                      # unchanged
    assert ctypes.sizeof(H) == 88
    G = K.HadamardGroupArgs
    assert _struct_fields("cq_hadamard_group_args") == [f for f, _ in G._fields_] == ["count", "members"]
    assert (G.count.offset, G.members.offset, ctypes.sizeof(G)) == (0, 8, 16)
    U = K.HadamardGluArgs
    names = ["g", "g_dtype", "ldg", "u", "u_dtype", "ldu", "h", "h_dtype", "ldh", "rows", "n_in", "n_out", "P",
             "bias_g", "bias_u", "act"]
    assert _struct_fields("cq_hadamard_glu_args") == [f for f, _ in U._fields_] == names
    assert [getattr(U, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 112, 120]
    assert ctypes.sizeof(U) == 128


def _raw_group(count=3, rows=4, P=64):
    """Valid members on host memory (never launched)."""
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16
    arr = (K.HadamardArgs * max(count, 1))()
    for i in range(count):
        a = arr[i]
        a.x, a.x_dtype, a.ldx = base + 2048 * i, K.CQ_F32, P
        a.y, a.y_dtype, a.ldy = base + 32768 + 2048 * i, K.CQ_F16, P
        a.rows, a.n_in, a.n_out, a.P = rows, P, P - 3, P
    g = K.HadamardGroupArgs()
    g.count, g.members = count, ctypes.cast(arr, ctypes.POINTER(K.HadamardArgs))
    g._keep = (buf, arr)
    return g, arr, base


def test_the_group_entry_rejects_bad_arguments_without_a_device():
    lib = K.load()

    def refused(g, *words):
        assert lib.cq_hadamard_group_rows(ctypes.byref(g), None) == K.CQ_EINVAL, words
        msg = lib.cq_last_error().decode()
        for w in words:
            assert w in msg, (w, msg)

    assert lib.cq_hadamard_group_rows(None, None) == K.CQ_EINVAL
    for count in (0, 9, -1):
        g, _, _ = _raw_group()
        g.count = count
        refused(g, "count", str(count))
    g, _, _ = _raw_group()
    g.members = None
    refused(g, "members")
    g, arr, _ = _raw_group()
    arr[2].rows = 5
    refused(g, "member 2", "rows", "member 0's")
    g, arr, _ = _raw_group()
    arr[1].P = 128
    arr[1].ldx = arr[1].ldy = 128
    refused(g, "member 1", "P", "member 0's")
    # each member passes the single entry's validation, with the member named
    for i, field, value, words in ((1, "P", 48, ("P",)), (2, "n_in", 65, ("n_in",)), (0, "n_in", 0, ("n_in",)),
                                   (1, "n_out", 65, ("n_out",)), (2, "x_dtype", 9, ("x dtype",)),
                                   (0, "y_dtype", 9, ("y dtype",)), (1, "ldx", 63, ("leading dimension",)),
                                   (2, "ldy", 60, ("leading dimension",)), (1, "rows", -1, ("rows",))):
        g, arr, _ = _raw_group()
        setattr(arr[i], field, value)
        refused(g, f"member {i}", *words)
    g, arr, base = _raw_group()
    arr[1].x = base + 2
    refused(g, "member 1", "x is not aligned")
    g, arr, base = _raw_group()
    arr[2].y = base + 32769
    refused(g, "member 2", "y is not aligned")
    g, arr, base = _raw_group()
    arr[0].bias = base + 2
    refused(g, "member 0", "bias")
    g, arr, _ = _raw_group()
    arr[1].x = None
    refused(g, "member 1", "null")
    # rows == 0: CQ_OK without a launch; so is a group whose members all have nothing to write
    g, arr, _ = _raw_group(rows=0)
    assert lib.cq_hadamard_group_rows(ctypes.byref(g), None) == 0
    g, arr, _ = _raw_group()
    for a in arr:
        a.n_out = 0
    arr[1].x = None                      # a skipped member's pointers are not looked at, as in cq_hadamard_rows
    assert lib.cq_hadamard_group_rows(ctypes.byref(g), None) == 0


def _raw_glu(P=64, rows=4, **kw):
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16
    a = K.HadamardGluArgs()
    a.g, a.g_dtype, a.ldg = base, K.CQ_F32, P
    a.u, a.u_dtype, a.ldu = base + 8192, K.CQ_F32, P
    a.h, a.h_dtype, a.ldh = base + 16384, K.CQ_F16, P
    a.rows, a.n_in, a.n_out, a.P, a.act = rows, P, P - 3, P, K.ACT_SILU
    for k, v in kw.items():
        setattr(a, k, v(base) if callable(v) else v)
    a._keep = buf
    return a


def test_the_glu_entry_rejects_bad_arguments_without_a_device():
    lib = K.load()

    def refused(a, *words):
        assert lib.cq_hadamard_glu_rows(ctypes.byref(a), None) == K.CQ_EINVAL, words
        msg = lib.cq_last_error().decode()
        for w in words:
            assert w in msg, (w, msg)

    assert lib.cq_hadamard_glu_rows(None, None) == K.CQ_EINVAL
    assert lib.cq_hadamard_glu_rows(ctypes.byref(_raw_glu(rows=0)), None) == 0       # rows == 0: CQ_OK, no launch
    assert lib.cq_hadamard_glu_rows(ctypes.byref(_raw_glu(n_out=0, h=None)), None) == 0
    refused(_raw_glu(act=2), "act 2")
    refused(_raw_glu(act=-1), "act")
    for field in ("g_dtype", "u_dtype", "h_dtype"):
        refused(_raw_glu(**{field: 9}), field[0] + " dtype")
    refused(_raw_glu(P=48), "P = 48")
    refused(_raw_glu(P=32768, ldg=32768, ldu=32768, ldh=32768), "P = 32768", "16384")
    refused(_raw_glu(n_in=65), "n_in")
    refused(_raw_glu(n_in=0), "n_in")
    refused(_raw_glu(n_out=65), "n_out")
    refused(_raw_glu(n_out=-1), "n_out")
    refused(_raw_glu(rows=-1), "rows")
    refused(_raw_glu(ldg=63), "ldg")
    refused(_raw_glu(ldu=63), "ldu")
    refused(_raw_glu(ldh=60), "ldh")
    for field in ("g", "u", "h"):
        refused(_raw_glu(**{field: None}), "null")
    refused(_raw_glu(g=lambda b: b + 2), "g is not aligned")
    refused(_raw_glu(u=lambda b: b + 8194), "u is not aligned")
    refused(_raw_glu(h=lambda b: b + 16385), "h is not aligned")
    refused(_raw_glu(bias_g=lambda b: b + 2), "bias_g")
    refused(_raw_glu(bias_u=lambda b: b + 2), "bias_u")


def test_the_args_builders_check_like_the_c_entries():
    x = torch.zeros(4, 60)
    y = torch.zeros(4, 64, dtype=torch.float16)
    mem = dict(x=x, y=y, n_in=60, n_out=64, P=64)
    g = K.hadamard_group_args([mem, dict(mem, y=torch.zeros(4, 10), n_out=10, bias=torch.zeros(10))])
    assert g.count == 2 and g.members[1].n_out == 10 and g.members[1].bias and not g.members[0].bias
    assert g.members[0].x_dtype == K.CQ_F32 and g.members[0].y_dtype == K.CQ_F16
    with pytest.raises(ValueError, match="count 0"):
        K.hadamard_group_args([])
    with pytest.raises(ValueError, match="count 9"):
        K.hadamard_group_args([mem] * 9)
    with pytest.raises(ValueError, match=r"member 1: rows 5 differs from member 0's 4"):
        K.hadamard_group_args([mem, dict(mem, x=torch.zeros(5, 60), y=torch.zeros(5, 64))])
    with pytest.raises(ValueError, match=r"member 1: P 128 differs from member 0's 64"):
        K.hadamard_group_args([mem, dict(mem, P=128)])
    with pytest.raises(ValueError, match=r"member 1: .*bias"):
        K.hadamard_group_args([mem, dict(mem, bias=torch.zeros(3))])
    a = K.hadamard_glu_args(x, x, y, n_in=60, n_out=64, P=64, bias_u=torch.zeros(64), act=K.ACT_IDENTITY)
    assert (a.rows, a.n_in, a.n_out, a.P, a.act) == (4, 60, 64, 64, 0) and a.bias_u and not a.bias_g
    with pytest.raises(ValueError, match="P = 32768"):
        K.hadamard_glu_args(x, x, y, n_in=60, n_out=64, P=32768)
    with pytest.raises(ValueError, match="act"):
        K.hadamard_glu_args(x, x, y, n_in=60, n_out=64, P=64, act=3)
    with pytest.raises(ValueError, match="rows"):
        K.hadamard_glu_args(x, torch.zeros(5, 60), y, n_in=60, n_out=64, P=64)
    with pytest.raises(RuntimeError, match="HIP device"):
        K.hadamard_glu_rows(x, x, y, n_in=60, n_out=64, P=64)
    with pytest.raises(RuntimeError, match="HIP device"):
        K.hadamard_group_rows([mem])


# ---------------------------------------------------------------------------- the cases
def test_the_issues_cases_are_all_there():
    assert {c.P for c in GC.GROUP} == set(GC.PS) == {4, 64, 512, 1024, 2048, 4096, 8192, 16384, 32768}
    assert {c.P for c in GC.GLU} == set(GC.PS) - {32768}
    for cases in (GC.GROUP, GC.GLU):
        assert {c.rows for c in cases} == {1, 5, 17}
        assert len({c.id for c in cases}) == len(cases)
    for P in GC.PS:
        assert {len(c.members) for c in GC.GROUP if c.P == P} == {1, 2, 3, 8}
    mems = [m for c in GC.GROUP for m in c.members]
    assert {m.xdt for m in mems} == {m.ydt for m in mems} == set(GC.XDT)
    assert {m.bias for m in mems} == {False, True} and {m.pad_x > 0 for m in mems} == {m.pad_y > 0 for m in mems}
    assert any(m.n_in < c.P for c in GC.GROUP for m in c.members) and any(m.n_out < c.P for c in GC.GROUP for m in c.members)
    assert any(len({m.n_out for m in c.members}) > 1 for c in GC.GROUP)
    assert {c.bias for c in GC.GLU} == {0, 1, 2} and {c.hdt for c in GC.GLU} == set(GC.XDT)
    assert any(c.pad for c in GC.GLU) and any(c.n_in < c.P for c in GC.GLU) and any(c.n_out < c.P for c in GC.GLU)
    for fault in GC.GROUP_FAULTS:
        assert sum(GC.group_fault_applies(c, fault) for c in GC.GROUP) >= 5, fault
    for fault in GC.GLU_FAULTS:
        assert sum(GC.glu_fault_applies(c, ACT_SILU, fault) for c in GC.GLU) >= 5, fault


@pytest.mark.parametrize("case", GC.GROUP, ids=lambda c: c.id)
def test_every_planted_group_fault_exceeds_ten_bars(case):
    ref = GC.group_reference(case)
    for fault in GC.GROUP_FAULTS:
        if not GC.group_fault_applies(case, fault):
            continue
        bad = GC.group_reference(case, fault)
        worst = max(float((np.abs(b[0] - r[0]) / r[1]).max()) for b, r in zip(bad, ref))
        assert worst > 10, (fault, worst)


@pytest.mark.parametrize("case", GC.GLU, ids=lambda c: c.id)
@pytest.mark.parametrize("act", [ACT_IDENTITY, ACT_SILU], ids=["identity", "silu"])
def test_every_planted_glu_fault_exceeds_ten_bars(case, act):
    h, bar = GC.glu_reference(case, act)
    assert np.isfinite(h).all() and (bar > 0).all()
    for fault in GC.GLU_FAULTS:
        if not GC.glu_fault_applies(case, act, fault):
            continue
        bad, _ = GC.glu_reference(case, act, fault)
        assert float((np.abs(bad - h) / bar).max()) > 10, fault


# ---------------------------------------------------------------------------- the classes
def _inner(m, n, r=3, bits=2, seed=0, **kw):
    g = torch.Generator().manual_seed(seed * 131 + m)
    k = 2 ** (bits - 1) - 1
    c = torch.randint(-k, k + 1, (m, n), generator=g).to(torch.int8)
    L = torch.randn(m, r, generator=g).half() if r and "L_codes" not in kw else None
    R = torch.randn(r, n, generator=g).half() if r else None
    return CalderaLinear.from_codes(c, L, R, None, qscale=0.05, gscale=1.5, bits=bits, **kw)


def _had(out=12, inp=40, seed=0, bias=False, **kw):
    pr, pc = 1 << (out - 1).bit_length(), 1 << (inp - 1).bit_length()
    return HadamardCalderaLinear(_inner(pr, pc, seed=seed, **kw), inp, out,
                                 torch.arange(out, dtype=torch.float32) if bias else None)


def test_group_construction_errors_name_the_member_and_the_attribute():
    q, k, v = _had(seed=1), _had(out=6, seed=2, r=0), _had(seed=3, bias=True)
    group = HadamardLinearGroup([q, k, v])
    assert len(group) == 3 and q.group is group and k.group is group and group.members == (q, k, v)
    assert "_group" not in q._modules and "_group" not in q.state_dict()
    coded = dict(L_codes=(torch.zeros(16, 3, dtype=torch.int8), 1.0, 4))
    grouped_inner = _had(seed=9)
    CalderaLinearGroup([grouped_inner.inner])
    for members, words in (
            ([], ("0 members",)),
            ([_had(seed=i) for i in range(9)], ("9 members",)),
            ([_had(seed=1), _inner(16, 64)], ("member 1", "CalderaLinear", "not a HadamardCalderaLinear")),
            ([_had(seed=1), torch.nn.Linear(40, 12)], ("member 1", "Linear")),
            ([q], ("member 0", "already in a group")),
            ([_had(seed=1), grouped_inner], ("member 1", "inner", "CalderaLinearGroup")),
            ([_had(seed=1), _had(inp=70, seed=2)], ("member 1", "in_features")),
            ([_had(seed=1), _had(seed=2, bits=4)], ("member 1", "bits")),
            ([_had(seed=1), _had(seed=2, r=0), _had(seed=3, **coded)], ("member 2", "L_bits", "member 0's"))):
        with pytest.raises(ValueError) as e:
            HadamardLinearGroup(members)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
    twice = _had(seed=5)
    with pytest.raises(ValueError, match="member 1 is given twice"):
        HadamardLinearGroup([twice, twice])
    assert twice.group is None
    # a plain group still refuses a Hadamard layer, and a rank-0 member fits any factor format
    with pytest.raises(ValueError, match="HadamardCalderaLinear"):
        CalderaLinearGroup([_had(seed=1)])
    HadamardLinearGroup([_had(seed=1, r=0), _had(seed=3, **coded)])
    group.dissolve()
    assert q.group is None and k.group is None and v.group is None
    group2 = HadamardLinearGroup([q, k])
    state = pickle.loads(pickle.dumps(group2)).__dict__
    assert state["_key"] is None and state["_kept"] == {} and len(state["members"]) == 2


def test_mlp_construction_errors_name_the_attribute():
    good = (_had(seed=1), _had(seed=2), torch.nn.Linear(12, 40))
    mlp = HadamardGatedMLP(*good)
    assert [n for n, _ in mlp.named_children()] == ["gate_proj", "up_proj", "down_proj"] and mlp.act == "silu"
    assert mlp.max_fused_tokens is None and HadamardGatedMLP(*good, act="identity").act == "identity"
    coded = dict(L_codes=(torch.zeros(16, 3, dtype=torch.int8), 1.0, 4))
    for args, kw, words in (
            ((_inner(16, 64), good[1], good[2]), {}, ("gate_proj", "CalderaLinear", "not a HadamardCalderaLinear")),
            ((good[0], torch.nn.Linear(40, 12), good[2]), {}, ("up_proj", "Linear")),
            ((good[0], good[0], good[2]), {}, ("same layer",)),
            ((good[0], _had(seed=2, bits=4), good[2]), {}, ("up_proj", "bits")),
            ((good[0], _had(out=13, seed=2), good[2]), {}, ("up_proj", "out_features")),
            ((good[0], _had(inp=48, seed=2), good[2]), {}, ("up_proj", "in_features")),
            ((good[0], _had(seed=3, **coded), good[2]), {}, ("up_proj", "L_bits")),
            ((good[0], good[1], lambda x: x), {}, ("down_proj",)),
            (good, {"act": "gelu"}, ("act", "gelu")),
            (good, {"max_fused_tokens": 1.5}, ("max_fused_tokens",))):
        with pytest.raises(ValueError) as e:
            HadamardGatedMLP(*args, **kw)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
    with pytest.raises(ValueError, match="HadamardCalderaLinear"):
        CalderaGatedMLP(*good)                                       # the plain block still refuses them
    with pytest.raises(RuntimeError, match="HIP device"):            # the fused path has no CPU fallback
        with torch.no_grad():
            mlp(torch.zeros(2, 40))


# ---------------------------------------------------------------------------- launch sequences
@pytest.fixture
def calls(monkeypatch):
    """The `_lib` entries the Hadamard paths use, replaced by recorders that fill their outputs."""
    log = []

    def hadamard_rows(x, y, *, n_in, n_out, P, bias=None):
        log.append(("hadamard_rows", tuple(x.shape), tuple(y.shape), P))
        return y.fill_(1.0)

    def linear_group_forward(x, members, ys, q_format, ws=None):
        log.append(("linear_group_forward", tuple(x.shape), [tuple(y.shape) for y in ys], [m["m"] for m in members]))
        assert x.dtype == torch.float16 and all(y.dtype == torch.float32 for y in ys)
        assert all(m["bias"] is None for m in members)
        for i, y in enumerate(ys):
            y.fill_(10.0 + i)
        return ys

    def hadamard_group_rows(members):
        members = list(members)
        log.append(("hadamard_group_rows", [(tuple(m["x"].shape), tuple(m["y"].shape), m["P"]) for m in members]))
        for m in members:
            assert m["n_in"] == m["P"] == m["x"].shape[1] and m["n_out"] == m["y"].shape[1]
            m["y"].copy_(m["x"][:, :1].expand_as(m["y"]))       # the member's inner output, so they can be told apart
        return [m["y"] for m in members]

    def hadamard_glu_rows(g, u, h, *, n_in, n_out, P, bias_g=None, bias_u=None, act=K.ACT_SILU):
        log.append(("hadamard_glu_rows", tuple(g.shape), tuple(u.shape), tuple(h.shape), P, act,
                    bias_g is not None, bias_u is not None))
        return h.copy_((g[:, :1] * u[:, :1]).expand_as(h))

    for fn in (hadamard_rows, linear_group_forward, hadamard_group_rows, hadamard_glu_rows):
        monkeypatch.setattr(K, fn.__name__, fn)
    return log


def _names(log):
    return [c[0] for c in log]


def test_the_qkv_set_is_three_launch_groups(calls):
    q, k, v = _had(seed=1), _had(seed=2), _had(seed=3, bias=True)
    group = HadamardLinearGroup([q, k, v])
    x = torch.zeros(2, 5, 40, dtype=torch.bfloat16)
    with torch.no_grad():
        ys = group(x)
    assert _names(calls) == ["hadamard_rows", "linear_group_forward", "hadamard_group_rows"]
    assert calls[0] == ("hadamard_rows", (10, 40), (10, 64), 64)
    assert calls[1] == ("linear_group_forward", (10, 64), [(10, 16)] * 3, [16, 16, 16])
    assert calls[2] == ("hadamard_group_rows", [((10, 16), (10, 12), 16)] * 3)
    assert [tuple(y.shape) for y in ys] == [(2, 5, 12)] * 3 and all(y.dtype == torch.bfloat16 for y in ys)
    assert [float(y[0, 0, 0]) for y in ys] == [10.0, 11.0, 12.0]
    assert q.inner.group is None                      # no inner group is made


def test_differing_padded_widths_take_one_output_launch_each(calls):
    # (40, 100), (12, 100), (40, 100): pr 64, 16, 64 and pc 128
    q, k, v = _had(out=40, inp=100, seed=1), _had(out=12, inp=100, seed=2), _had(out=40, inp=100, seed=3)
    group = HadamardLinearGroup([q, k, v])
    with torch.no_grad():
        ys = group(torch.zeros(3, 100))
    assert _names(calls) == ["hadamard_rows", "linear_group_forward", "hadamard_group_rows", "hadamard_group_rows"]
    assert calls[1][2] == [(3, 64), (3, 16), (3, 64)]
    assert calls[2][1] == [((3, 64), (3, 40), 64)] * 2 and calls[3][1] == [((3, 16), (3, 12), 16)]
    assert [float(y[0, 0]) for y in ys] == [10.0, 11.0, 12.0] and [y.shape[1] for y in ys] == [40, 12, 40]


def test_the_member_protocol_keeps_and_claims(calls, monkeypatch):
    q, k, v = _had(seed=1), _had(seed=2), _had(seed=3)
    group = HadamardLinearGroup([q, k, v])
    alone = []
    monkeypatch.setattr(HadamardCalderaLinear, "_forward_alone", lambda self, x: alone.append(self) or "alone")
    x = torch.zeros(4, 40)
    with torch.no_grad():
        yq = q(x)
        assert _names(calls) == ["hadamard_rows", "linear_group_forward", "hadamard_group_rows"]
        assert set(group._kept) == {id(k), id(v)} and float(yq[0, 0]) == 10.0
        yv, yk = v(x), k(x)                                   # claimed in any order, no further launch
        assert len(calls) == 3 and float(yk[0, 0]) == 11.0 and float(yv[0, 0]) == 12.0 and group._kept == {}
        q(x)                                                  # a second call with this x starts over
        assert len(calls) == 6
        k(torch.zeros(4, 40))                                 # a new x restarts and releases what was kept
        assert len(calls) == 9 and set(group._kept) == {id(q), id(v)}
        x2 = torch.zeros(4, 40)
        q(x2)
        x2.add_(1)                                            # a bumped version: the kept outputs are stale
        k(x2)
        assert len(calls) == 15 and not alone
        # inference tensors and shallow copies run alone; so does x requiring grad
        with torch.inference_mode():
            assert q(torch.zeros(4, 40)) == "alone"
        assert alone == [q] and group._kept == {}
        replica = copy.copy(q)
        assert replica.group is group and replica(x) == "alone" and alone == [q, replica]
    xg = torch.zeros(4, 40, requires_grad=True)
    assert k(xg) == "alone" and len(calls) == 15
    with torch.no_grad():
        k(xg)                                                 # no graph needed: grouped again
    assert len(calls) == 18
    # group(x) keeps nothing; the dense threshold and trainable factors send every member alone
    with torch.no_grad():
        group(x)
        assert group._kept == {} and len(calls) == 21
        q.dense_prefill_tokens = 64
        assert group(torch.zeros(64, 40)) == ("alone",) * 3 and len(group(torch.zeros(63, 40))) == 3
        q.dense_prefill_tokens = None
        k.enable_factor_training()
        assert group(x) == ("alone",) * 3
        k.freeze_factors()
        monkeypatch.setattr(LN, "HADAMARD_GROUP_TOKEN_LIMIT", 8)
        assert group(torch.zeros(9, 40)) == ("alone",) * 3 and len(group(torch.zeros(8, 40))) == 3
    group.dissolve()
    assert q(x) == "alone"


def test_the_mlp_is_three_launch_groups_and_falls_back(calls, monkeypatch):
    gate, up = _had(seed=1, bias=True), _had(seed=2)
    mlp = HadamardGatedMLP(gate, up, torch.nn.Identity())
    with torch.no_grad():
        h = mlp(torch.zeros(2, 3, 40, dtype=torch.float16))
    assert _names(calls) == ["hadamard_rows", "linear_group_forward", "hadamard_glu_rows"]
    assert calls[1] == ("linear_group_forward", (6, 64), [(6, 16)] * 2, [16, 16])
    assert calls[2] == ("hadamard_glu_rows", (6, 16), (6, 16), (6, 12), 16, K.ACT_SILU, True, False)
    assert h.shape == (2, 3, 12) and h.dtype == torch.float16 and (h == 110).all()
    assert gate.group is None and gate.inner.group is None
    ident = HadamardGatedMLP(gate, up, torch.nn.Identity(), act="identity")
    with torch.no_grad():
        ident.glu(torch.zeros(1, 40, dtype=torch.float64))
    assert calls[-1][5] == K.ACT_IDENTITY and calls[-3][1] == (1, 40)
    # the fallbacks: the formula through the layers' own forwards
    monkeypatch.setattr(HadamardCalderaLinear, "_forward_alone",
                        lambda self, x: torch.full((*x.shape[:-1], self.out_features), 2.0) + 0 * x.sum())
    n = len(calls)
    want = torch.nn.functional.silu(torch.full((4, 12), 2.0)) * 2.0
    xg = torch.zeros(4, 40, requires_grad=True)
    out = mlp.glu(xg)                                                     # x requiring grad
    assert torch.equal(out, want) and out.requires_grad and len(calls) == n
    with torch.no_grad():
        assert mlp._fused(xg)
        limited = HadamardGatedMLP(gate, up, torch.nn.Identity(), max_fused_tokens=4)
        assert torch.equal(limited.glu(torch.zeros(5, 40)), want[:1].expand(5, 12)) and len(calls) == n
        limited.glu(torch.zeros(4, 40))
        assert len(calls) == n + 3
        gate.dense_prefill_tokens = 17
        assert not mlp._fused(torch.zeros(17, 40)) and mlp._fused(torch.zeros(16, 40))
        gate.dense_prefill_tokens = None
        up.enable_factor_training()
        assert not mlp._fused(torch.zeros(2, 40))
        up.freeze_factors()
        mlp.up_proj = torch.nn.Linear(40, 12)                             # the layers no longer fit
        assert not mlp._fused(torch.zeros(2, 40))
    # pr = 32768 is past the gated entry: the block is built, and takes the formula
    big = [HadamardCalderaLinear.__new__(HadamardCalderaLinear) for _ in range(2)]
    for i, had in enumerate(big):
        torch.nn.Module.__init__(had)
        had.in_features, had.out_features = 40, 20000
        inner = _inner(16, 64, seed=20 + i)
        inner.out_features = 32768                                        # the shape only: nothing is launched
        had.inner = inner
        had.register_buffer("bias", None)
    wide = HadamardGatedMLP(big[0], big[1], torch.nn.Identity())
    m = len(calls)
    with torch.no_grad():
        assert not wide._fused(torch.zeros(1, 40))
        assert wide.glu(torch.zeros(1, 40)).shape == (1, 20000) and len(calls) == m
        big[0].inner.out_features = big[1].inner.out_features = 16384
        assert wide._fused(torch.zeros(1, 40))


# ---------------------------------------------------------------------------- state dicts and model.py
class _Attn(torch.nn.Module):
    def __init__(self, q, k, v):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj = q, k, v


class _MLP(torch.nn.Module):
    def __init__(self, gate, up, down, act_fn):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj, self.act_fn = gate, up, down, act_fn

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


def _model():
    net = torch.nn.Module()
    net.attn = _Attn(_had(seed=1), _had(out=6, seed=2), _had(out=6, seed=3, bias=True))
    net.mlp = _MLP(_had(seed=4), _had(seed=5), _had(out=40, inp=12, seed=6), torch.nn.SiLU())
    net.mixed = _Attn(_had(seed=7), _inner(12, 40, seed=8), _inner(12, 40, seed=9))
    net.mixed_mlp = _MLP(_inner(12, 40, seed=10), _had(seed=11), torch.nn.Linear(12, 40), torch.nn.SiLU())
    net.plain = _Attn(_inner(12, 40, seed=12), _inner(12, 40, seed=13), _inner(12, 40, seed=14))
    net.plain_mlp = _MLP(_inner(12, 40, seed=15), _inner(12, 40, seed=16), torch.nn.Linear(12, 40), torch.nn.SiLU())
    net.misfit = _MLP(_had(seed=17), _had(seed=18, bits=4), torch.nn.Linear(12, 40), torch.nn.SiLU())
    return net


def test_the_default_arguments_leave_hadamard_sets_alone():
    net = _model()
    grouped, skipped = M.group_shared_input_layers(net)
    assert grouped == [("plain.q_proj", "plain.k_proj", "plain.v_proj"), ("plain_mlp.gate_proj", "plain_mlp.up_proj")]
    reasons = dict(skipped)
    assert reasons[("attn.q_proj", "attn.k_proj", "attn.v_proj")] == "q_proj is a HadamardCalderaLinear"
    assert reasons[("mlp.gate_proj", "mlp.up_proj")] == "gate_proj is a HadamardCalderaLinear"
    assert reasons[("mixed.q_proj", "mixed.k_proj", "mixed.v_proj")] == "q_proj is a HadamardCalderaLinear"
    assert reasons[("mixed_mlp.gate_proj", "mixed_mlp.up_proj")] == "up_proj is a HadamardCalderaLinear"
    assert reasons[("misfit.gate_proj", "misfit.up_proj")] == "gate_proj is a HadamardCalderaLinear"
    assert net.attn.q_proj.group is None and all(mod.group is None for mod in net.mlp.children()
                                                 if isinstance(mod, HadamardCalderaLinear))
    M.ungroup_shared_input_layers(net)
    fused, skipped = M.fuse_gated_mlps(net)
    assert fused == ["plain_mlp"]
    reasons = dict(skipped)
    assert reasons["mlp"] == "gate_proj is a HadamardCalderaLinear" == reasons["misfit"]
    assert reasons["mixed_mlp"] == "up_proj is a HadamardCalderaLinear"
    assert isinstance(net.mlp, _MLP) and isinstance(net.plain_mlp, CalderaGatedMLP)


def test_hadamard_true_groups_and_fuses_and_both_are_undone():
    net = _model()
    before = copy.deepcopy(net.state_dict())
    keys = list(before)
    grouped, skipped = M.group_shared_input_layers(net, hadamard=True)
    assert grouped == [("attn.q_proj", "attn.k_proj", "attn.v_proj"), ("mlp.gate_proj", "mlp.up_proj"),
                       ("plain.q_proj", "plain.k_proj", "plain.v_proj"), ("plain_mlp.gate_proj", "plain_mlp.up_proj")]
    reasons = dict(skipped)
    assert reasons[("mixed.q_proj", "mixed.k_proj", "mixed.v_proj")] == "q_proj is a HadamardCalderaLinear"
    assert reasons[("mixed_mlp.gate_proj", "mixed_mlp.up_proj")] == "up_proj is a HadamardCalderaLinear"
    assert "incompatible" in reasons[("misfit.gate_proj", "misfit.up_proj")] and "bits" in reasons[
        ("misfit.gate_proj", "misfit.up_proj")]
    assert isinstance(net.attn.q_proj.group, HadamardLinearGroup) and len(net.attn.q_proj.group) == 3
    assert net.attn.k_proj.group is net.attn.q_proj.group and isinstance(net.plain.q_proj.group, CalderaLinearGroup)
    assert net.attn.q_proj.inner.group is None
    again, skipped2 = M.group_shared_input_layers(net, hadamard=True)
    assert again == [] and dict(skipped2)[("attn.q_proj", "attn.k_proj", "attn.v_proj")] == "q_proj is already grouped"
    assert list(net.state_dict()) == keys                             # grouping changes no key
    original = net.mlp
    fused, skipped = M.fuse_gated_mlps(net, hadamard=True)
    assert fused == ["mlp", "plain_mlp"]
    reasons = dict(skipped)
    assert reasons["mixed_mlp"] == "up_proj is a HadamardCalderaLinear"
    assert "incompatible" in reasons["misfit"] and "bits" in reasons["misfit"]
    assert isinstance(net.mlp, HadamardGatedMLP) and net.mlp.act == "silu" and net.mlp.gate_proj is original.gate_proj
    assert dict(M.fuse_gated_mlps(net, hadamard=True)[1])["mlp"] == "already fused"
    # the state dict: the same keys, loads in both directions
    assert list(net.state_dict()) == keys
    plain = _model()
    plain.load_state_dict(net.state_dict())
    net.load_state_dict(before)
    assert all(torch.equal(v, before[k]) for k, v in plain.state_dict().items() if torch.is_tensor(v))
    # undo
    assert M.unfuse_gated_mlps(net) == ["mlp", "plain_mlp"] and net.mlp is original
    done = M.ungroup_shared_input_layers(net)
    assert ("attn.q_proj", "attn.k_proj", "attn.v_proj") in done and ("mlp.gate_proj", "mlp.up_proj") in done
    assert all(mod.group is None for mod in net.modules() if isinstance(mod, (CalderaLinear, HadamardCalderaLinear)))
    assert list(net.state_dict()) == keys


def test_replacing_a_grouped_hadamard_layer_dissolves_its_group(monkeypatch):
    net = _model()
    M.group_shared_input_layers(net, hadamard=True)
    k = net.attn.k_proj
    for cls in (CalderaLinear, HadamardCalderaLinear):
        monkeypatch.setattr(cls, "materialize", lambda self, dtype=torch.float16, out=None:
                            torch.zeros(self.out_features, self.in_features, dtype=dtype))
    M.unpack_packed_layers(net.attn, torch.float32)
    assert isinstance(net.attn.q_proj, torch.nn.Linear) and k.group is None
    net2 = _model()
    M.group_shared_input_layers(net2, hadamard=True)
    q, k2, v = net2.attn.q_proj, net2.attn.k_proj, net2.attn.v_proj
    res = k2.to_result("attn.k_proj")
    with pytest.raises(ValueError, match="attn.k_proj"):       # a packed layer holds no weight: refused, group kept
        M.apply_packed_results(net2, [res])
    assert k2.group is not None and k2.group.members == (q, k2, v)

    class Weighted(HadamardCalderaLinear):
        weight = property(lambda self: torch.zeros(self.out_features, self.in_features))

    k2.__class__ = Weighted
    assert M.apply_packed_results(net2, [res]) == ["attn.k_proj"]
    assert type(net2.attn.k_proj) is HadamardCalderaLinear and net2.attn.k_proj is not k2
    assert q.group is None and v.group is None and k2.group is None and net2.attn.k_proj.group is None
    assert net2.mlp.gate_proj.group is not None                # the other set keeps its group
