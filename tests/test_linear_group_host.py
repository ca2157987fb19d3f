"""CPU side of the grouped packed forward (cq_linear_group_forward, CalderaLinearGroup,
model.group_shared_input_layers): that the groups of linear_group_cases.py are exact and can see the
planted member-lookup faults, the C ABI and its argument checks without a device, and the grouping
surface of linear.py / model.py on CPU tensors with the launch replaced by a recording stand-in."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import linear_group_cases as GC
from linear_group_cases import f32, f64
from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import linear as LIN
from ee274_convexcaldera_llm_quantization_amd import model as M
from ee274_convexcaldera_llm_quantization_amd.linear import (CalderaLinear, CalderaLinearGroup, HadamardCalderaLinear,
                                                              row_bytes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "caldera_hip.h")


# ---------------------------------------------------------------------------- the cases
def test_the_issues_groups_are_all_there():
    shapes = {(g.n, g.members) for g in GC.ALL}
    assert shapes == {(198, ((33, 8), (272, 40), (48, 0))), (898, ((80, 200), (33, 40))),
                      (2600, ((48, 40), (33, 264))), (64, ((33, 8),)), (64, tuple((16 + i, 8) for i in range(8)))}
    assert GC.GROUP_MAX == K.LINEAR_GROUP_MAX == 8
    for n, members in shapes:
        for bits in (2, 4):
            Ts = {g.T for g in GC.ALL if (g.n, g.members, g.bits, g.fmt, g.lb) == (n, members, bits, "uniform", 16)}
            assert Ts == {1, 5, 16, 17} | ({130} if n == 198 else set())
    for n in (198, 898):
        for bits in (2, 4):
            mine = [g for g in GC.ALL if g.n == n and g.bits == bits]
            nf_coded = {("nf", 4, 4), ("nf", 2, 16)} if n == 198 else set()
            assert {(g.fmt, g.lb, g.rb) for g in mine} == {("uniform", 16, 16), ("uniform", 4, 4), ("uniform", 2, 16),
                                                           ("nf", 16, 16)} | nf_coded
    assert any(g.bias >= 0 for g in GC.ALL)
    assert len({g.id for g in GC.ALL}) == len(GC.ALL)
    # the boundaries fall inside tiles: rows unaligned, a rank-0 member, different r32, two decode chunks
    m198 = [m for m, _ in GC.SHAPES[198]]
    assert m198[0] % 16 and all(m % 256 for m in m198) and max(m198) > 256
    assert [(-(-r // 32)) * 32 for _, r in GC.SHAPES[198]] == [32, 64, 0]
    assert -(-2600 // 256) > 8 and 264 > 8 * 32


@pytest.mark.parametrize("group", GC.ALL, ids=lambda g: g.id)
def test_every_member_is_exact_in_fp32(group):
    """Per member: the sum of the absolute terms stays below 2^24 units, z~ splits exactly into fp16
    halves, and the reference is an fp32 value."""
    d = GC.inputs(group)
    assert np.abs(d["x"].astype(f64)).max() <= GC.xamp(group)
    for mem, y in zip(d["members"], GC.reference(group)):
        qs, zscale = GC.scales(group, mem)
        assert qs == f32(0.5) and zscale in (f32(0.25), f32(0.5), f32(1.0))
        assert float(mem["gs"]) in (4.0, 8.0, 16.0)
        units, unit, split_exact = GC.exact_units(group, mem)
        assert units < 2 ** 24, units
        assert split_exact
        assert np.array_equal(y.astype(f32).astype(f64), y)
        core = (y - (0 if mem["bias"] is None else mem["bias"].astype(f64))) / f64(mem["gs"])
        assert np.array_equal(np.round(core / unit), core / unit)


def _fault_params():
    out = []
    for g in GC.ALL:
        for tag, order in (("", None), ("-reversed", g.reversed_order)):
            if tag and g.count == 1:
                continue
            for f in GC.FAULTS:
                if GC.fault_applies(g, f, order):
                    out.append(pytest.param(g, f, order, id=f"{g.id}{tag}-{f}"))
    return out


@pytest.mark.parametrize("group,fault,order", _fault_params())
def test_planted_fault_changes_every_group_it_applies_to(group, fault, order):
    good, bad = GC.reference(group, order=order), GC.reference(group, fault, order)
    assert any(not np.array_equal(a, b) for a, b in zip(good, bad))


def test_every_fault_meets_a_group():
    for fault in GC.FAULTS:
        hit = [g for g in GC.ALL if GC.fault_applies(g, fault) or GC.fault_applies(g, fault, g.reversed_order)]
        assert hit, fault
        assert {g.T <= 16 for g in hit} == {True, False}, fault       # decode and prefill
    # the order the GPU test permutes to is a different one, and the outputs follow it
    g = next(g for g in GC.ALL if g.n == 198)
    a, b = GC.reference(g), GC.reference(g, order=g.reversed_order)
    assert all(np.array_equal(a[i], b[j]) for j, i in enumerate(g.reversed_order))


# ---------------------------------------------------------------------------- the ABI
def _struct_fields(name):
    txt = open(HEADER).read()
    body = txt[txt.index(f"typedef struct {name}"):txt.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*[;,]", body.split("{", 1)[1])


def test_group_abi_is_additive():
    txt = open(HEADER).read()
    assert int(re.search(r"#define CQ_ABI_VERSION (\d+)", txt).group(1)) == K.ABI_VERSION == 5
    assert int(re.search(r"#define CQ_LINEAR_GROUP_MAX (\d+)", txt).group(1)) == K.LINEAR_GROUP_MAX == 8
    new = {"cq_linear_group_workspace", "cq_linear_group_forward"}
    assert new <= set(K.EXPORTS)
    lib = K.load()                      # raises for a missing export
    assert lib.cq_abi_version() == 5
    for name in new:
        assert getattr(lib, name) is not None
    assert _struct_fields("cq_linear_group_args") == [f for f, _ in K.LinearGroupArgs._fields_] \
        == ["count", "q_format", "members"]
    assert K.LinearGroupArgs.members.offset == 8 and ctypes.sizeof(K.LinearGroupArgs) == 16
    assert K.LinearGroupArgs._fields_[2][1] is ctypes.POINTER(K.LinearPackedArgs)
    assert [f for f, _ in K.LinearPackedArgs._fields_] == _struct_fields("cq_linear_packed_args")   # unchanged


def _raw_group(count=3, q_format=K.QFMT_UNIFORM, ranks=(8, 0, 8), **member_kw):
    """A valid group of `count` members on host memory (never launched); member_kw: {field: (i, value)}."""
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16
    arr = (K.LinearPackedArgs * max(count, 1))()
    for i in range(max(count, 1)):
        p = arr[i]
        r = ranks[i % len(ranks)]
        p.x, p.ldx, p.tokens, p.m, p.n, p.r, p.bits = base, 64, 1, 16 + i, 64, r, 4
        p.codes, p.code_stride, p.qscale, p.gscale = base + 256, 32, 1.0, 1.0
        p.L, p.ldl, p.R, p.ldr = base + 2048, 8, base + 3072, 64
        p.y, p.y_dtype, p.ldy = base + 8192 + 512 * i, K.CQ_F32, 32
        p.l_bits = p.r_bits = 16
    for key, (i, v) in member_kw.items():
        setattr(arr[i], key, v)
    g = K.LinearGroupArgs()
    g.count, g.q_format = count, q_format
    g.members = ctypes.cast(arr, ctypes.POINTER(K.LinearPackedArgs))
    g._keep = (arr, buf)
    return g, base


def test_group_entry_rejects_bad_arguments_without_a_device():
    """The decision is made on the host before any launch: CQ_EINVAL with a message that names the
    member and the field."""
    lib = K.load()

    def refused(g, *words):
        assert lib.cq_linear_group_forward(ctypes.byref(g), None, 0, None) == K.CQ_EINVAL, words
        msg = lib.cq_last_error().decode()
        for w in words:
            assert w in msg, (w, msg)

    assert lib.cq_linear_group_forward(None, None, 0, None) == K.CQ_EINVAL
    refused(_raw_group(count=0)[0], "count 0")
    refused(_raw_group(count=9)[0], "count 9")
    g, base = _raw_group()
    g.members = ctypes.POINTER(K.LinearPackedArgs)()
    refused(g, "null members")
    refused(_raw_group(q_format=2)[0], "q_format")
    for field, value in (("x", lambda b: b + 16), ("ldx", lambda b: 72), ("tokens", lambda b: 2), ("n", lambda b: 48),
                         ("bits", lambda b: 2), ("y_dtype", lambda b: K.CQ_F16)):
        g, base = _raw_group()
        setattr(g.members[1], field, value(base))
        refused(g, "member 1", field)
    # the factor formats: among the members with r > 0 only
    g, base = _raw_group(l_bits=(2, 4), L_codes=(2, 0), l_code_stride=(2, 16), lscale=(2, 1.0))
    g.members[2].L_codes = base + 4096
    refused(g, "member 2", "l_bits")
    g, base = _raw_group(r_bits=(2, 4), r_code_stride=(2, 32), rscale=(2, 1.0))
    g.members[2].R_codes = base + 4096
    refused(g, "member 2", "r_bits")
    g, _ = _raw_group(l_bits=(1, 4), r_bits=(1, 2))           # member 1 has r = 0: fits any factor format
    assert lib.cq_linear_group_workspace(ctypes.byref(g)) > 0
    g.members[0].tokens = g.members[1].tokens = g.members[2].tokens = 0
    assert lib.cq_linear_group_forward(ctypes.byref(g), None, 0, None) == 0         # tokens == 0: CQ_OK, no launch
    # a member's own check, with the member named
    refused(_raw_group(code_stride=(2, 17))[0], "member 2", "aligned")
    refused(_raw_group(r=(0, K.LINEAR_MAX_RANK + 1))[0], "member 0", "rank")
    # q_format with a bad NF scale
    refused(_raw_group(q_format=K.QFMT_NF, qscale=(1, float("nan")))[0], "member 1", "NF scale")
    refused(_raw_group(q_format=K.QFMT_NF, qscale=(2, -1.0))[0], "member 2", "NF scale")


@pytest.mark.parametrize("tokens", [1, 16, 17, 130])
def test_group_workspace_is_the_aligned_sum_of_the_members(tokens):
    lib = K.load()
    g, _ = _raw_group(count=4, ranks=(8, 0, 40, 264))
    total = 0
    for i in range(4):
        g.members[i].tokens = tokens
        g.members[i].ldl = 264
        own = lib.cq_linear_packed_workspace(ctypes.byref(g.members[i]))
        assert (own == 0) == (g.members[i].r == 0)
        total += (own + 15) // 16 * 16
    assert lib.cq_linear_group_workspace(ctypes.byref(g)) == total > 0
    assert lib.cq_linear_group_workspace(None) == 0
    # too small a workspace is refused before any launch
    buf = torch.zeros(64, dtype=torch.uint8)
    ws = (buf.data_ptr() + 15) // 16 * 16
    assert lib.cq_linear_group_forward(ctypes.byref(g), ws, 16, None) == K.CQ_EWORKSPACE


def test_group_args_builder_checks_like_the_packed_one():
    x = torch.zeros(2, 198, dtype=torch.float16)

    def member(m=12, r=5, bits=4, n=198, **kw):
        d = dict(codes=torch.zeros(m, row_bytes(n, bits), dtype=torch.uint8), qscale=1.0, gscale=1.0,
                 L=torch.zeros(m, r, dtype=torch.float16) if r else None,
                 R=torch.zeros(r, n, dtype=torch.float16) if r else None, bias=None, m=m, n=n, bits=bits, r=r)
        d.update(kw)
        return d

    def ys(*ms, dtype=torch.float32):
        return [torch.zeros(2, m, dtype=dtype) for m in ms]

    g = K.linear_group_args(x, [member(), member(m=20, r=0), member(m=7, r=9)], ys(12, 20, 7), K.QFMT_UNIFORM)
    assert (g.count, g.q_format) == (3, K.QFMT_UNIFORM)
    assert [(g.members[i].m, g.members[i].r, g.members[i].tokens, g.members[i].x) for i in range(3)] == \
        [(12, 5, 2, x.data_ptr()), (20, 0, 2, x.data_ptr()), (7, 9, 2, x.data_ptr())]
    lib = K.load()
    assert lib.cq_linear_group_workspace(ctypes.byref(g)) == 2 * 16 * 16 * 32 * 4
    coded = member(m=7, r=9, L=None, L_codes=(torch.zeros(7, 16, dtype=torch.uint8), 1.0, 4))
    for members, outs, qf, words in (
            ([], [], 0, ("count 0",)),
            ([member()] * 9, ys(*[12] * 9), 0, ("count 9",)),
            ([member(), member()], ys(12), 0, ("outputs",)),
            ([member()], ys(12), 5, ("q_format",)),
            ([member(), member(bits=2)], ys(12, 12), 0, ("member 1", "bits")),
            ([member(), member(n=64)], ys(12, 12), 0, ("member 1",)),
            ([member(), member()], ys(12, 12)[:1] + ys(12, dtype=torch.float16), 0, ("member 1", "y_dtype")),
            ([member(), member(r=0), coded], ys(12, 12, 7), 0, ("member 2", "l_bits")),
            ([member(), member(qscale=float("inf"))], ys(12, 12), K.QFMT_NF, ("member 1", "NF scale")),
            ([member(), member(L=torch.zeros(12, 5))], ys(12, 12), 0, ("member 1", "fp16"))):
        with pytest.raises(ValueError) as e:
            K.linear_group_args(x, members, outs, qf)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        assert str(e.value).count("cq_linear:") == 1, str(e.value)   # a member's own message is not prefixed twice
    with pytest.raises(RuntimeError, match="HIP device"):
        K.linear_group_forward(x, [member()], ys(12), K.QFMT_UNIFORM)


# ---------------------------------------------------------------------------- CalderaLinearGroup
def _layer(m=12, n=40, r=3, bits=2, seed=0, **kw):
    g = torch.Generator().manual_seed(seed + m)
    k = 2 ** (bits - 1) - 1
    c = torch.randint(-k, k + 1, (m, n), generator=g).to(torch.int8)
    L = torch.randn(m, r, generator=g).half() if r else None
    R = torch.randn(r, n, generator=g).half() if r else None
    return CalderaLinear.from_codes(c, L, R, None, qscale=0.05, gscale=1.5, bits=bits, **kw)


class _Recorder:
    """Stands in for `_lib.linear_group_forward`: records the call and fills y_i with i + 1."""

    def __init__(self):
        self.calls = []

    def __call__(self, x, members, ys, q_format, ws=None):
        self.calls.append((x, [mem["m"] for mem in members], q_format))
        for i, y in enumerate(ys):
            y.fill_(i + 1)
        return ys


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(K, "linear_group_forward", rec)
    return rec


def test_group_construction_errors():
    a, b = _layer(12), _layer(20)
    for members, words in (
            ([], ("0 members",)),
            ([_layer(8 + i) for i in range(9)], ("9 members",)),
            ([a, torch.nn.Linear(40, 4)], ("member 1", "Linear")),
            ([a, a], ("member 1", "twice")),
            ([a, _layer(20, n=48)], ("member 1", "in_features")),
            ([a, _layer(20, bits=4)], ("member 1", "bits")),
            ([a, CalderaLinear.from_codes(torch.zeros(5, 40, dtype=torch.int64), None, None, None, qscale=1.0,
                                          gscale=1.0, bits=2, q_format=LIN.Q_FORMAT_NF)], ("member 1", "q_format")),
            ([a, _layer(9, r=0), CalderaLinear.from_codes(
                torch.zeros(5, 40, dtype=torch.int8), None, torch.zeros(3, 40).half(), None, qscale=1.0, gscale=1.0,
                bits=2, L_codes=(torch.zeros(5, 3, dtype=torch.int8), 1.0, 4))], ("member 2", "L_bits")),
            ([a, HadamardCalderaLinear(_layer(16, n=64), 40, 12)], ("member 1", "HadamardCalderaLinear"))):
        with pytest.raises(ValueError) as e:
            CalderaLinearGroup(members)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        assert a.group is None and b.group is None      # a refused group leaves no back-reference
    grp = CalderaLinearGroup([a, _layer(9, r=0), b])     # a rank-0 member fits
    assert a.group is grp and b.group is grp and len(grp) == 3
    with pytest.raises(ValueError, match="already in a group"):
        CalderaLinearGroup([b])
    grp.dissolve()
    assert a.group is None and b.group is None
    CalderaLinearGroup([b]).dissolve()                   # a group of one


def test_three_member_calls_on_one_x_are_one_launch(recorder):
    q, k, v = _layer(12), _layer(20), _layer(7, r=0)
    grp = CalderaLinearGroup([q, k, v])
    x = torch.randn(2, 3, 40)
    with torch.no_grad():
        yq, yk, yv = q(x), k(x), v(x)
    assert len(recorder.calls) == 1 and recorder.calls[0][1] == [12, 20, 7]
    assert recorder.calls[0][0].dtype == torch.float16 and tuple(recorder.calls[0][0].shape) == (6, 40)
    for y, m, val in ((yq, 12, 1.0), (yk, 20, 2.0), (yv, 7, 3.0)):
        assert tuple(y.shape) == (2, 3, m) and y.dtype == x.dtype and bool((y == val).all())
    assert grp._kept == {}                                # every kept output was claimed
    # the order of the calls does not matter, and a second call of the same member starts over
    with torch.no_grad():
        assert bool((v(x) == 3.0).all()) and bool((q(x) == 1.0).all())
        assert len(recorder.calls) == 2
        q(x)
        assert len(recorder.calls) == 3
    # a version change and another x start over; no strong reference to x is kept
    with torch.no_grad():
        k(x)
        n0 = len(recorder.calls)
        x.add_(0)
        k(x)
        assert len(recorder.calls) == n0 + 1
        x2 = x.clone()
        v(x2)
        assert len(recorder.calls) == n0 + 2 and set(grp._kept) == {id(q), id(k)}
        import weakref
        ref = weakref.ref(x2)
        del x2
        assert ref() is None
        q(x)
        assert len(recorder.calls) == n0 + 3
    # bf16 / fp16 activations: y in x's dtype; the group called directly: a tuple in member order
    with torch.no_grad():
        for dt in (torch.float16, torch.bfloat16):
            ys = grp(x.to(dt))
            assert [tuple(y.shape) for y in ys] == [(2, 3, 12), (2, 3, 20), (2, 3, 7)] and all(y.dtype == dt for y in ys)
    with pytest.raises(ValueError, match="in_features"):
        with torch.no_grad():
            q(torch.randn(2, 41))


def test_group_falls_back_to_the_members_own_path(recorder, monkeypatch):
    q, k = _layer(12), _layer(20)
    grp = CalderaLinearGroup([q, k])
    alone = []
    monkeypatch.setattr(CalderaLinear, "_forward_alone", lambda self, x: alone.append(self) or "alone")
    x = torch.randn(5, 40)
    with torch.no_grad():
        q(x)
    assert len(recorder.calls) == 1 and alone == []
    # a graph is needed
    xg = x.clone().requires_grad_()
    assert q(xg) == "alone" and k(xg) == "alone" and grp(xg) == ("alone", "alone")
    assert alone == [q, k, q, k] and len(recorder.calls) == 1 and grp._kept == {}
    with torch.no_grad():
        q(xg)                                            # grad mode off: the grouped launch again
    assert len(recorder.calls) == 2
    # a member trains
    k.enable_factor_training()
    del alone[:]
    with torch.no_grad():
        assert q(x) == "alone" and grp(x) == ("alone", "alone")
    assert alone == [q, q, k] and len(recorder.calls) == 2
    k.freeze_factors()
    # the dense prefill threshold of any member, at the token counts it applies to
    k.dense_prefill_tokens = 32
    x40 = torch.randn(2, 20, 40)
    del alone[:]
    with torch.no_grad():
        assert q(x40) == "alone"
        q(x)
    assert alone == [q] and len(recorder.calls) == 3
    # dissolve(): every layer runs alone
    grp.dissolve()
    with torch.no_grad():
        assert q(x) == "alone" and k(x) == "alone"
    assert len(recorder.calls) == 3


def test_an_inference_tensor_is_never_served_a_kept_output(recorder, monkeypatch):
    """An inference tensor has no version counter (reading it raises) and can be written in place
    unseen: member(x) keeps nothing for it and runs alone; group(x) launches grouped."""
    q, k = _layer(12), _layer(20)
    grp = CalderaLinearGroup([q, k])
    alone = []
    monkeypatch.setattr(CalderaLinear, "_forward_alone", lambda self, x: alone.append(self) or "alone")
    x = torch.randn(5, 40)
    with torch.no_grad():
        q(x)
    assert set(grp._kept) == {id(k)} and len(recorder.calls) == 1
    with torch.inference_mode():
        xi = torch.randn(5, 40)
        assert xi.is_inference()
        assert q(xi) == "alone" and grp._kept == {} and grp._key is None   # and the stale output is released
        assert k(xi) == "alone"
        xi.add_(1)
        assert k(xi) == "alone" and alone == [q, k, k] and len(recorder.calls) == 1
        ys = grp(xi)                                      # nothing is kept by a direct call: grouped
        assert len(recorder.calls) == 2 and [tuple(y.shape) for y in ys] == [(5, 12), (5, 20)] and grp._kept == {}
        # a tensor from outside the block keeps its version counter: the transparent path
        q(x), k(x)
        assert len(recorder.calls) == 3 and grp._kept == {}
    assert alone == [q, k, k]


def test_a_shallow_copy_of_a_member_runs_alone(recorder, monkeypatch):
    """`nn.DataParallel` replicas copy a module's `__dict__`, back-reference included, without being
    members: they run their own operands, and the group's kept outputs are not touched."""
    q, k = _layer(12), _layer(20)
    grp = CalderaLinearGroup([q, k])
    alone = []
    monkeypatch.setattr(CalderaLinear, "_forward_alone", lambda self, x: alone.append(self) or "alone")
    x = torch.randn(5, 40)
    rep = q._replicate_for_data_parallel()
    assert rep is not q and rep.group is grp
    with torch.no_grad():
        q(x)
        assert rep(x) == "alone" and alone == [rep]
        assert set(grp._kept) == {id(k)} and len(recorder.calls) == 1
        k(x)
    assert len(recorder.calls) == 1 and alone == [rep]


def test_a_layer_without_a_group_runs_todays_forward():
    lin = _layer(12)
    assert "_group" not in lin.__dict__ and lin.group is None
    with pytest.raises(RuntimeError, match="HIP device"):
        lin(torch.randn(2, 40))


def test_grouping_leaves_the_state_dict_and_the_extra_state_alone():
    a, b = _layer(12), _layer(20)
    plain = copy.deepcopy(a)
    grp = CalderaLinearGroup([a, b])
    sa, sp = a.state_dict(), plain.state_dict()
    assert list(sa) == list(sp) and a.get_extra_state() == plain.get_extra_state()
    assert all(torch.equal(sa[key], sp[key]) for key in sa if torch.is_tensor(sa[key]))
    assert a.packed_bytes() == plain.packed_bytes() and [n for n, _ in a.named_modules()] == [""]
    assert list(dict(a.named_buffers())) == list(dict(plain.named_buffers()))
    r1, r2 = a.to_result("w"), plain.to_result("w")
    assert torch.equal(r1.codes, r2.codes) and torch.equal(r1.L, r2.L)
    # a copy of the model carries its own group over its own layers
    net = torch.nn.ModuleDict(dict(a=a, b=b))
    twin = copy.deepcopy(net)
    assert twin["a"].group is not grp and twin["a"].group.members == (twin["a"], twin["b"])
    plain.load_state_dict(sa)
    assert plain.group is None


# ---------------------------------------------------------------------------- model.py
class _Attn(torch.nn.Module):
    def __init__(self, layers):
        super().__init__()
        for name, lin in layers.items():
            setattr(self, name, lin)


def _toy():
    net = torch.nn.Module()
    net.attn = _Attn(dict(q_proj=_layer(12), k_proj=_layer(6), v_proj=_layer(6, r=0), o_proj=_layer(40, n=12)))
    net.mlp = _Attn(dict(gate_proj=_layer(24), up_proj=_layer(24, seed=1), down_proj=_layer(40, n=24)))
    net.dense = _Attn(dict(q_proj=_layer(12), k_proj=torch.nn.Linear(40, 6), v_proj=_layer(6)))
    net.had = _Attn(dict(gate_proj=HadamardCalderaLinear(_layer(16, n=64), 40, 12), up_proj=_layer(12)))
    net.part = _Attn(dict(gate_proj=_layer(12)))
    net.mixed = _Attn(dict(gate_proj=_layer(12), up_proj=_layer(12, bits=4)))
    return net


def test_group_and_ungroup_shared_input_layers(recorder):
    net = _toy()
    keys = list(net.state_dict())
    grouped, skipped = M.group_shared_input_layers(net)
    assert grouped == [("attn.q_proj", "attn.k_proj", "attn.v_proj"), ("mlp.gate_proj", "mlp.up_proj")]
    reasons = dict(skipped)
    assert set(reasons) == {("dense.q_proj", "dense.k_proj", "dense.v_proj"), ("had.gate_proj", "had.up_proj"),
                            ("part.gate_proj", "part.up_proj"), ("mixed.gate_proj", "mixed.up_proj")}
    assert "dense" in reasons[("dense.q_proj", "dense.k_proj", "dense.v_proj")]
    assert "Hadamard" in reasons[("had.gate_proj", "had.up_proj")]
    assert "missing" in reasons[("part.gate_proj", "part.up_proj")]
    assert "incompatible" in reasons[("mixed.gate_proj", "mixed.up_proj")] and "bits" in reasons[
        ("mixed.gate_proj", "mixed.up_proj")]
    assert net.attn.q_proj.group.members == (net.attn.q_proj, net.attn.k_proj, net.attn.v_proj)
    assert net.attn.o_proj.group is None and net.mixed.gate_proj.group is None and net.dense.q_proj.group is None
    assert list(net.state_dict()) == keys
    # again: what is grouped already is skipped with that reason, nothing raises
    again, skipped2 = M.group_shared_input_layers(net)
    assert again == [] and "already grouped" in dict(skipped2)[("attn.q_proj", "attn.k_proj", "attn.v_proj")]
    x = torch.randn(3, 40)
    with torch.no_grad():
        net.attn.q_proj(x), net.attn.k_proj(x), net.attn.v_proj(x)
    assert len(recorder.calls) == 1
    # other sets
    assert M.group_shared_input_layers(net, sets=(("o_proj",),)) == ([("attn.o_proj",)], [])
    done = M.ungroup_shared_input_layers(net)
    assert sorted(done) == sorted(grouped + [("attn.o_proj",)])
    assert all(mod.group is None for mod in net.modules() if isinstance(mod, CalderaLinear))
    assert M.ungroup_shared_input_layers(net) == []


def test_replacing_a_grouped_layer_dissolves_its_group(monkeypatch):
    net = _toy()
    M.group_shared_input_layers(net)
    q, k = net.attn.q_proj, net.attn.k_proj
    assert q.group is not None
    # unpack_packed_layers replaces every packed layer by nn.Linear (materialize stands in on CPU)
    for cls in (CalderaLinear, HadamardCalderaLinear):
        monkeypatch.setattr(cls, "materialize",
                            lambda self, dtype=torch.float16, out=None: torch.zeros(self.out_features, self.in_features,
                                                                                     dtype=dtype))
    names = M.unpack_packed_layers(net, torch.float32)
    assert "attn.q_proj" in names and isinstance(net.attn.q_proj, torch.nn.Linear)
    assert q.group is None and k.group is None


def test_apply_packed_results_and_a_grouped_layer():
    """apply_packed_results replaces modules that hold a dense `weight`.  A packed layer holds none, so
    a result naming a grouped layer is refused by the shape check with the model and the group as they
    were; a layer that does expose one (here a subclass) is replaced, and its group dissolved."""
    net = _toy()
    M.group_shared_input_layers(net)
    q, k = net.attn.q_proj, net.attn.k_proj
    res = _layer(12, seed=5).to_result("attn.q_proj")
    with pytest.raises(ValueError, match="attn.q_proj"):
        M.apply_packed_results(net, [res])
    assert net.attn.q_proj is q and q.group is not None and q.group.members == (q, k, net.attn.v_proj)

    class Weighted(CalderaLinear):
        weight = property(lambda self: torch.zeros(self.out_features, self.in_features))

    q.__class__ = Weighted
    assert M.apply_packed_results(net, [res]) == ["attn.q_proj"]
    new = net.attn.q_proj
    assert new is not q and type(new) is CalderaLinear and new.group is None
    assert q.group is None and k.group is None and net.attn.v_proj.group is None
    assert net.mlp.gate_proj.group is not None            # the other set keeps its group
    assert M.group_shared_input_layers(net)[0] == [("attn.q_proj", "attn.k_proj", "attn.v_proj")]
