"""Host-side checks of the randomised Hadamard basis: the pinned sign vector, the additive ABI (three new
entries, ABI still 5), the bindings' refusals, the incoherence the signs buy, and the plumbing of
HadamardCalderaLinear, its group and its fused block and of model.py with the `_lib` entries stubbed, as
test_hadamard_group_host.py stubs them.  No GPU."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

import hadamard_sign_cases as SC
from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import linear as LIN
from ee274_convexcaldera_llm_quantization_amd import model as M
from ee274_convexcaldera_llm_quantization_amd.linear import (CalderaLinear, HadamardCalderaLinear, HadamardGatedMLP,
                                                              HadamardLinearGroup, hadamard_sign_vector)
from ee274_convexcaldera_llm_quantization_amd.sharding import pack_results, unpack_results
from test_hadamard_group_host import _had, _inner
from test_hadamard_host import _header_layout
from test_linear_host import _Dec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "caldera_hip.h")


# ---------------------------------------------------------------------------- the vector
def test_sign_vector_golden():
    v = hadamard_sign_vector(7, 4096)
    assert v.dtype == torch.int8 and v.device.type == "cpu" and v.shape == (4096,)
    assert v[:32].tolist() == SC.SEED7_FIRST32 and int(v.sum()) == SC.SEED7_SUM4096
    assert set(v.tolist()) == {-1, 1}
    for n in (0, 1, 31, 100):                                   # a prefix of any longer one
        assert torch.equal(hadamard_sign_vector(7, n), v[:n])
    # element i is -1 iff bit 63 of mix(mix(seed) + i) is set, in plain integer arithmetic
    big = (1 << 53) - 1
    w = hadamard_sign_vector(big, 50)
    assert w.tolist() == [-1 if LIN.mix64((LIN.mix64(big) + i) & (2 ** 64 - 1)) >> 63 else 1 for i in range(50)]
    assert not torch.equal(hadamard_sign_vector(8, 64), v[:64])
    for bad in (-1, 1 << 53, 1.0, True, None):
        with pytest.raises(ValueError, match="2\\^53"):
            hadamard_sign_vector(bad, 4)


# ---------------------------------------------------------------------------- the ABI
def test_the_abi_is_additive_and_still_5():
    txt = open(HEADER).read()
    assert int(re.search(r"#define CQ_ABI_VERSION (\d+)", txt).group(1)) == 5 == K.ABI_VERSION
    lib = K.load()
    assert lib.cq_abi_version() == 5
    for name in ("cq_hadamard_signed_rows", "cq_hadamard_signed_group_rows", "cq_hadamard_signed_glu_rows"):
        assert name in K.EXPORTS and getattr(lib, name) is not None
        assert re.search(rf"int {name}\(const {name.replace('_rows', '_args')}\* \w+, void\* stream\);", txt), name
    # the unsigned structs are where they were
    assert ctypes.sizeof(K.HadamardArgs) == _header_layout("cq_hadamard_args")[1] == 88
    assert ctypes.sizeof(K.HadamardGluArgs) == _header_layout("cq_hadamard_glu_args")[1]
    # the signed ones: the unsigned struct first, then two pointers
    for cls, inner, fields in ((K.HadamardSignedArgs, K.HadamardArgs, ("sign_in", "sign_out")),
                               (K.HadamardSignedGluArgs, K.HadamardGluArgs, ("sign_g", "sign_u"))):
        base = ctypes.sizeof(inner)
        assert base % 8 == 0 and [f for f, _ in cls._fields_] == ["a", *fields]
        assert [getattr(cls, f).offset for f in ("a", *fields)] == [0, base, base + 8]
        assert ctypes.sizeof(cls) == base + 16
    body = txt[txt.index("typedef struct cq_hadamard_signed_args"):txt.index("} cq_hadamard_signed_args;")]
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == ["a", "sign_in", "sign_out"]
    body = txt[txt.index("typedef struct cq_hadamard_signed_glu_args"):txt.index("} cq_hadamard_signed_glu_args;")]
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == ["a", "sign_g", "sign_u"]
    assert [f for f, _ in K.HadamardSignedGroupArgs._fields_] == ["count", "members"]
    assert K.HadamardSignedGroupArgs.members.offset == 8 and ctypes.sizeof(K.HadamardSignedGroupArgs) == 16


def test_the_signed_entries_validate_like_the_unsigned_ones_without_a_device():
    lib = K.load()
    buf = torch.zeros(8192, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16

    def args(**kw):
        s = K.HadamardSignedArgs()
        a = s.a
        a.x, a.x_dtype, a.ldx = base, K.CQ_F16, 64
        a.y, a.y_dtype, a.ldy = base + 4096, K.CQ_F32, 64
        a.rows, a.n_in, a.n_out, a.P = 2, 64, 64, 64
        s.sign_in, s.sign_out = base + 1, base + 3          # any alignment is accepted
        for key, v in kw.items():
            setattr(a, key, v)
        return s

    for kw, word in ((dict(P=48), "power of two"), (dict(n_in=65, ldx=128), "n_in"), (dict(n_out=65, ldy=128), "n_out"),
                     (dict(x_dtype=K.CQ_F64), "x dtype"), (dict(x=base + 1), "x is not aligned"),
                     (dict(bias=base + 2), "bias is not aligned"), (dict(ldy=10), "leading dimension"),
                     (dict(rows=-1), "rows")):
        s = args(**kw)
        assert lib.cq_hadamard_signed_rows(ctypes.byref(s), None) == K.CQ_EINVAL, kw
        msg = lib.cq_last_error().decode()
        assert word in msg and "cq_hadamard_signed_rows" in msg, (kw, msg)
    assert lib.cq_hadamard_signed_rows(None, None) == K.CQ_EINVAL
    assert lib.cq_hadamard_signed_rows(ctypes.byref(args(rows=0)), None) == 0      # no launch, no device needed
    # the group entry names the member; the gated entry keeps its own maximum
    arr = (K.HadamardSignedArgs * 2)(args(), args(P=128, n_in=64, n_out=64))
    g = K.HadamardSignedGroupArgs(2, ctypes.cast(arr, ctypes.POINTER(K.HadamardSignedArgs)))
    assert lib.cq_hadamard_signed_group_rows(ctypes.byref(g), None) == K.CQ_EINVAL
    assert "member 1" in lib.cq_last_error().decode() and "P" in lib.cq_last_error().decode()
    g.count = 9
    assert lib.cq_hadamard_signed_group_rows(ctypes.byref(g), None) == K.CQ_EINVAL
    assert "count" in lib.cq_last_error().decode()
    assert lib.cq_hadamard_signed_group_rows(None, None) == K.CQ_EINVAL
    u = K.HadamardSignedGluArgs()
    u.a.g = u.a.u = base
    u.a.h = base + 4096
    u.a.g_dtype = u.a.u_dtype = u.a.h_dtype = K.CQ_F32
    u.a.ldg = u.a.ldu = u.a.ldh = 64
    u.a.rows, u.a.n_in, u.a.n_out, u.a.P, u.a.act = 0, 64, 64, 64, K.ACT_SILU
    assert lib.cq_hadamard_signed_glu_rows(ctypes.byref(u), None) == 0
    u.a.P = u.a.n_in = u.a.n_out = u.a.ldg = u.a.ldu = u.a.ldh = 2 * K.HADAMARD_GLU_MAX_N
    assert lib.cq_hadamard_signed_glu_rows(ctypes.byref(u), None) == K.CQ_EINVAL
    assert "power of two" in lib.cq_last_error().decode()
    u.a.P = u.a.n_in = u.a.n_out = 64
    u.a.act = 9
    assert lib.cq_hadamard_signed_glu_rows(ctypes.byref(u), None) == K.CQ_EINVAL
    assert "act" in lib.cq_last_error().decode()
    assert lib.cq_hadamard_signed_glu_rows(None, None) == K.CQ_EINVAL


def test_the_bindings_refuse_wrong_sign_vectors_with_a_message():
    x, y = torch.zeros(3, 60, dtype=torch.float16), torch.zeros(3, 64)
    ok = dict(n_in=60, n_out=64, P=64)
    s60, s64 = torch.ones(60, dtype=torch.int8), torch.ones(64, dtype=torch.int8)
    a = K.hadamard_signed_args(x, y, sign_in=s60, sign_out=s64, **ok)
    assert (a.sign_in, a.sign_out, a.a.ldx, a.a.P) == (s60.data_ptr(), s64.data_ptr(), 60, 64)
    longer = K.hadamard_signed_args(x, y, sign_in=s64, **ok)        # a longer vector serves: the prefix is read
    assert longer.sign_in == s64.data_ptr() and not longer.sign_out
    for kw, words in ((dict(sign_in=s60.float()), ("sign_in", "int8")),
                      (dict(sign_out=s64.to(torch.uint8)), ("sign_out", "int8")),
                      (dict(sign_in=s60[:59]), ("sign_in", "59", "60")),
                      (dict(sign_out=s60), ("sign_out", "60", "64")),
                      (dict(sign_in=torch.ones(120, dtype=torch.int8)[::2]), ("sign_in", "contiguous")),
                      (dict(sign_in=torch.ones(60, 1, dtype=torch.int8)), ("sign_in", "vector")),
                      (dict(sign_out=torch.ones(64, dtype=torch.int8, device="meta")), ("sign_out", "meta")),
                      (dict(sign_in=[1] * 60), ("sign_in", "int8"))):
        for call in (K.hadamard_signed_args, K.hadamard_signed_rows):   # the wrapper refuses before any device check
            with pytest.raises(ValueError) as e:
                call(x, y, **ok, **kw)
            assert all(w in str(e.value) for w in ("cq_hadamard_signed_rows", *words)), str(e.value)
    with pytest.raises(ValueError, match="cq_hadamard_signed_rows: P = 48"):     # the unsigned checks, under this name
        K.hadamard_signed_args(x, y, n_in=60, n_out=64, P=48)
    with pytest.raises(RuntimeError, match="HIP"):
        K.hadamard_signed_rows(x, y, sign_in=s60, **ok)
    # the group builder names the member, the gated one its own vectors
    mem = dict(x=x, y=y, sign_in=s60, **ok)
    g = K.hadamard_signed_group_args([mem, dict(mem, sign_out=s64)])
    assert g.count == 2 and g.members[1].sign_out == s64.data_ptr() and not g.members[0].sign_out
    with pytest.raises(ValueError, match="cq_hadamard_signed_group_rows: member 1: sign_out .*int8"):
        K.hadamard_signed_group_rows([mem, dict(mem, sign_out=s64.short())])
    with pytest.raises(ValueError, match="member 1: P 128 differs"):
        K.hadamard_signed_group_args([mem, dict(mem, P=128)])
    with pytest.raises(ValueError, match="count 0"):
        K.hadamard_signed_group_args([])
    gg = torch.zeros(3, 64)
    u = K.hadamard_signed_glu_args(gg, gg.clone(), y, n_in=64, n_out=64, P=64, sign_g=s64)
    assert u.sign_g == s64.data_ptr() and not u.sign_u and u.a.act == K.ACT_SILU
    with pytest.raises(ValueError, match="cq_hadamard_signed_glu_rows: sign_u has 60 entries"):
        K.hadamard_signed_glu_rows(gg, gg.clone(), y, n_in=64, n_out=64, P=64, sign_u=s60)
    with pytest.raises(ValueError, match="cq_hadamard_signed_glu_rows: unknown act"):
        K.hadamard_signed_glu_args(gg, gg.clone(), y, n_in=64, n_out=64, P=64, act=5)


# ---------------------------------------------------------------------------- incoherence
def _mu(Wt):
    return float(Wt.abs().max() / Wt.pow(2).mean().sqrt())


@pytest.mark.parametrize("shape", [(48, 100), (64, 128)])
def test_signs_spread_a_common_offset(shape):
    """W = 0.02 N(0, 1) + 0.05: without signs the offset lands on one entry of H1 pad(W) H2 and sets the absmax
    scale; with them mu = max |W~| / rms(W~) falls at least threefold (measured with these seeds: 6.2x at
    (48, 100), 12.4x at (64, 128)).  The inverse recovers W to fp32 round-off: orthogonal transforms of
    log2(pr pc) <= 13 stages each way, so 64 2^-24 max |W| is a wide bound."""
    m, n = shape
    W = 0.02 * torch.randn(m, n, generator=torch.Generator().manual_seed(0)) + 0.05
    su, sv = hadamard_sign_vector(11, m), hadamard_sign_vector(12, n)
    pr, pc = 1 << (m - 1).bit_length(), 1 << (n - 1).bit_length()
    H1, H2 = M.normalized_hadamard(pr, "cpu"), M.normalized_hadamard(pc, "cpu")
    Wp = torch.zeros(pr, pc)
    Wp[:m, :n] = W
    plain = H1 @ Wp @ H2
    Ws = torch.zeros(pr, pc)
    Ws[:m, :n] = su.float()[:, None] * W * sv.float()[None, :]
    signed = H1 @ Ws @ H2
    print(f"{shape}: mu {_mu(plain):.1f} plain, {_mu(signed):.1f} signed, ratio {_mu(plain) / _mu(signed):.2f}")
    assert _mu(plain) >= 3 * _mu(signed)
    back = (H1 @ signed @ H2)[:m, :n] * su.float()[:, None] * sv.float()[None, :]
    assert float((back - W).abs().max()) <= 64 * 2.0 ** -24 * float(W.abs().max())


def test_hadamard_transform_takes_the_signs(monkeypatch):
    monkeypatch.setattr(K, "gemm", lambda A, B, *, C=None: A @ B if C is None else C.copy_(A @ B))
    W = torch.randn(12, 40, generator=torch.Generator().manual_seed(1))
    su, sv = hadamard_sign_vector(5, 12), hadamard_sign_vector(6, 40)
    plain, shape = M.hadamard_transform(W)
    signed, shape2 = M.hadamard_transform(W, signs=(su, sv))
    flipped, _ = M.hadamard_transform(su.float()[:, None] * W * sv.float()[None, :])
    assert shape == shape2 == (12, 40) and torch.equal(signed, flipped) and not torch.equal(signed, plain)
    back = M.hadamard_transform(signed, inverse=True, original_shape=shape, signs=(su, sv))
    assert float((back - W).abs().max()) <= 64 * 2.0 ** -24 * float(W.abs().max())
    assert torch.equal(back, M.hadamard_transform(signed, inverse=True, original_shape=shape)
                       * su.float()[:, None] * sv.float()[None, :])
    longer = (hadamard_sign_vector(5, 16), hadamard_sign_vector(6, 64))            # prefixes: the same transform
    assert torch.equal(M.hadamard_transform(W, signs=longer)[0], signed)
    with pytest.raises(ValueError, match="do not cover"):
        M.hadamard_transform(W, signs=(su[:11], sv))


# ---------------------------------------------------------------------------- the layer
def _signed(out=12, inp=40, seed=0, bias=False, seeds=(21, 22), **kw):
    base = _had(out, inp, seed, bias, **kw)
    return HadamardCalderaLinear(base.inner, inp, out, base.bias, sign_seeds=seeds)


@pytest.fixture
def calls(monkeypatch):
    """The `_lib` entries and the inner launches the Hadamard layers use, replaced by recorders."""
    log = []

    def hadamard_rows(x, y, *, n_in, n_out, P, bias=None):
        log.append(("hadamard_rows", dict(x=x, y=y, n_in=n_in, n_out=n_out, P=P, bias=bias)))
        return y.fill_(1.0)

    def hadamard_signed_rows(x, y, *, n_in, n_out, P, bias=None, sign_in=None, sign_out=None):
        log.append(("hadamard_signed_rows", dict(x=x, y=y, n_in=n_in, n_out=n_out, P=P, bias=bias, sign_in=sign_in,
                                                 sign_out=sign_out)))
        return y.fill_(1.0)

    def hadamard_group_rows(members):
        log.append(("hadamard_group_rows", list(members)))

    def hadamard_signed_group_rows(members):
        log.append(("hadamard_signed_group_rows", list(members)))

    def hadamard_glu_rows(g, u, h, *, n_in, n_out, P, bias_g=None, bias_u=None, act=K.ACT_SILU):
        log.append(("hadamard_glu_rows", dict(n_in=n_in, n_out=n_out, P=P, bias_g=bias_g, bias_u=bias_u, act=act)))
        return h.fill_(2.0)

    def hadamard_signed_glu_rows(g, u, h, *, n_in, n_out, P, bias_g=None, bias_u=None, act=K.ACT_SILU, sign_g=None,
                                 sign_u=None):
        log.append(("hadamard_signed_glu_rows", dict(n_in=n_in, n_out=n_out, P=P, bias_g=bias_g, bias_u=bias_u, act=act,
                                                     sign_g=sign_g, sign_u=sign_u)))
        return h.fill_(2.0)

    def linear_group_forward(x, members, ys, q_format, ws=None):
        log.append(("linear_group_forward", [m["m"] for m in members]))
        return [y.fill_(3.0) for y in ys]

    for fn in (hadamard_rows, hadamard_signed_rows, hadamard_group_rows, hadamard_signed_group_rows, hadamard_glu_rows,
               hadamard_signed_glu_rows, linear_group_forward):
        monkeypatch.setattr(K, fn.__name__, fn)
    monkeypatch.setattr(LIN, "_launch_packed", lambda lin, x2, y, L16=None, R16=None: log.append(("inner",)) or y.fill_(3.0))

    def packed_backward(lin, dy16, x2, L16, R16, needs, dx_dtype, factor_dtypes):
        log.append(("inner_backward",))
        return torch.ones((dy16.shape[0], lin.in_features), dtype=dx_dtype), None, None

    monkeypatch.setattr(LIN, "_packed_backward", packed_backward)
    return log


def _names(log):
    return [c[0] for c in log]


def test_an_unsigned_layer_is_what_it_was(calls):
    lin = _had(bias=True)
    assert lin.sign_seeds is None and lin.get_extra_state() == {"in_features": 40, "out_features": 12}
    assert set(lin.state_dict()) == {"bias", "_extra_state", "inner.codes", "inner.L", "inner.R", "inner._extra_state"}
    assert "sign" not in lin.extra_repr() and "hadamard_signs" not in lin.to_result("x").extra
    x = torch.zeros(5, 40, requires_grad=True)
    y = LIN._HadamardLinearFunction.apply(x, None, None, lin)
    y.backward(torch.ones(5, 12))
    assert _names(calls) == ["hadamard_rows", "inner", "hadamard_rows", "hadamard_rows", "inner_backward", "hadamard_rows"]
    shapes = [(c[1]["n_in"], c[1]["n_out"], c[1]["P"]) for c in calls if c[0] == "hadamard_rows"]
    assert shapes == [(40, 64, 64), (16, 12, 16), (12, 16, 16), (64, 40, 64)]
    assert calls[2][1]["bias"] is lin.bias and all(c[1]["bias"] is None for c in (calls[0], calls[3], calls[5]))
    assert all(set(c[1]) == {"x", "y", "n_in", "n_out", "P", "bias"} for c in calls if c[0] == "hadamard_rows")


def test_a_signed_layer_calls_the_signed_entries_with_its_vectors(calls):
    lin = _signed(bias=True, seeds=(21, 22))
    assert lin.sign_seeds == (21, 22)
    assert lin.sign_out.dtype == lin.sign_in.dtype == torch.int8
    assert torch.equal(lin.sign_out, hadamard_sign_vector(21, 12)) and torch.equal(lin.sign_in, hadamard_sign_vector(22, 40))
    assert lin.get_extra_state() == {"in_features": 40, "out_features": 12, "sign_seeds": (21, 22)}
    assert set(lin.state_dict()) == {"bias", "sign_out", "sign_in", "_extra_state", "inner.codes", "inner.L", "inner.R",
                                     "inner._extra_state"}
    assert "sign_seeds=(21, 22)" in lin.extra_repr() and not list(lin.parameters())
    x = torch.zeros(5, 40, requires_grad=True)
    y = LIN._HadamardLinearFunction.apply(x, None, None, lin)
    y.backward(torch.ones(5, 12))
    assert _names(calls) == ["hadamard_signed_rows", "inner", "hadamard_signed_rows", "hadamard_signed_rows",
                             "inner_backward", "hadamard_signed_rows"]
    t = [c[1] for c in calls if c[0] == "hadamard_signed_rows"]
    assert [(c["n_in"], c["n_out"], c["P"]) for c in t] == [(40, 64, 64), (16, 12, 16), (12, 16, 16), (64, 40, 64)]
    # forward: sv on the way in, su (and the bias) on the way out; backward: su on dy, sv on dx
    assert t[0]["sign_in"] is lin.sign_in and t[0]["sign_out"] is None and t[0]["bias"] is None
    assert t[1]["sign_out"] is lin.sign_out and t[1]["sign_in"] is None and t[1]["bias"] is lin.bias
    assert t[2]["sign_in"] is lin.sign_out and t[2]["sign_out"] is None and t[2]["bias"] is None
    assert t[3]["sign_out"] is lin.sign_in and t[3]["sign_in"] is None and t[3]["bias"] is None
    # the state dict loads into a layer built with other seeds, and the casts of a model leave the vectors alone
    other = _signed(bias=True, seeds=(1, 2))
    other.load_state_dict(lin.state_dict())
    assert other.sign_seeds == (21, 22) and torch.equal(other.sign_in, lin.sign_in)
    lin.half()
    assert lin.sign_in.dtype == torch.int8 and torch.equal(lin.sign_out, hadamard_sign_vector(21, 12))
    with pytest.raises(RuntimeError, match="missing|Missing|Unexpected|unexpected"):
        _had(bias=True).load_state_dict(lin.state_dict())
    for bad in ((1,), (1, 2, 3), (-1, 2), (1, 1 << 53), (1.5, 2)):
        with pytest.raises(ValueError, match="sign_seeds|seed_out|seed_in"):
            _signed(seeds=bad)


def test_dense_weight_and_materialize_carry_the_signs(calls):
    plain, lin = _had(seed=3), _signed(seed=3, seeds=(5, 6))
    su, sv = hadamard_sign_vector(5, 12).float(), hadamard_sign_vector(6, 40).float()
    assert torch.equal(lin.dense_weight(), plain.dense_weight() * su[:, None] * sv[None, :])
    # y = su * (H1 (W~ (H2 (sv * pad(x))))) is x dense_weight()^T
    x = torch.randn(3, 40, generator=torch.Generator().manual_seed(2))
    H1, H2 = M.normalized_hadamard(16, "cpu"), M.normalized_hadamard(64, "cpu")
    xp = torch.zeros(3, 64)
    xp[:, :40] = x * sv
    y = ((xp @ H2) @ lin.inner.dense_weight().t() @ H1)[:, :12] * su
    torch.testing.assert_close(y, x @ lin.dense_weight().t(), rtol=1e-4, atol=1e-5)
    # materialize: sv on the first transform's outputs, su on the second's (the stubs see the arguments only)
    lin.inner.materialize = lambda dtype: torch.zeros(16, 64)
    calls.clear()
    lin.materialize(torch.float32)
    t = [c[1] for c in calls]
    assert _names(calls) == ["hadamard_signed_rows"] * 2
    assert t[0]["sign_out"] is lin.sign_in and t[0]["sign_in"] is None and (t[0]["n_in"], t[0]["n_out"]) == (64, 40)
    assert t[1]["sign_out"] is lin.sign_out and t[1]["sign_in"] is None and (t[1]["n_in"], t[1]["n_out"]) == (16, 12)
    plain.inner.materialize = lin.inner.materialize
    calls.clear()
    plain.materialize(torch.float32)
    assert _names(calls) == ["hadamard_rows"] * 2


def test_results_round_trip_keeps_the_seeds():
    lin, plain = _signed(bias=True, seeds=(2 ** 53 - 1, 7)), _had(seed=4)
    res = lin.to_result("proj")
    assert res.extra["hadamard"] == [12, 40] and res.extra["hadamard_signs"] == [2 ** 53 - 1, 7]
    back = unpack_results(pack_results([res, plain.to_result("other")]))
    assert back[0].extra["hadamard_signs"] == [2 ** 53 - 1, 7] and "hadamard_signs" not in back[1].extra
    again = HadamardCalderaLinear.from_result(back[0], bias=lin.bias)
    assert again.sign_seeds == lin.sign_seeds
    sa, sb = lin.state_dict(), again.state_dict()
    assert set(sa) == set(sb)
    for key, v in sa.items():
        assert torch.equal(v, sb[key]) if torch.is_tensor(v) else v == pytest.approx(sb[key]), key
    assert HadamardCalderaLinear.from_result(back[1]).sign_seeds is None           # a file without the key: as before
    model = torch.nn.Module()
    model.proj, model.other = torch.nn.Linear(40, 12), torch.nn.Linear(40, 12, bias=False)
    assert M.apply_packed_results(model, back) == ["proj", "other"]
    assert model.proj.sign_seeds == lin.sign_seeds and torch.equal(model.proj.sign_in, lin.sign_in)
    assert model.other.sign_seeds is None and "sign_in" not in model.other.state_dict()
    res.extra["hadamard_signs"] = [1]
    with pytest.raises(ValueError, match="hadamard_signs"):
        HadamardCalderaLinear.from_result(res)


# ---------------------------------------------------------------------------- groups and fused blocks
def test_groups_and_blocks_refuse_mixed_sets_and_differing_seed_in():
    for members, words in (([_signed(seed=1), _had(seed=2)], ("member 1", "sign_seeds None", "member 0")),
                           ([_had(seed=1), _had(seed=2), _signed(seed=3)], ("member 2", "sign_seeds (21, 22)")),
                           ([_signed(seed=1), _signed(seed=2, seeds=(21, 23))], ("member 1", "seed_in 23", "22"))):
        with pytest.raises(ValueError) as e:
            HadamardLinearGroup(members)
        assert all(w in str(e.value) for w in ("HadamardLinearGroup", *words)), str(e.value)
        assert all(had.group is None for had in members)
    down = torch.nn.Linear(12, 40)
    for gate, up, words in ((_signed(seed=1), _had(seed=2), ("up_proj", "sign_seeds None")),
                            (_had(seed=1), _signed(seed=2), ("up_proj", "sign_seeds (21, 22)")),
                            (_signed(seed=1), _signed(seed=2, seeds=(9, 23)), ("up_proj", "seed_in 23"))):
        with pytest.raises(ValueError) as e:
            HadamardGatedMLP(gate, up, down)
        assert all(w in str(e.value) for w in ("HadamardGatedMLP", *words)), str(e.value)
    # seed_out may differ: they share x^ only
    HadamardLinearGroup([_signed(seed=1, seeds=(1, 22)), _signed(out=6, seed=2, seeds=(2, 22))]).dissolve()
    HadamardGatedMLP(_signed(seed=1, seeds=(1, 22)), _signed(seed=2, seeds=(2, 22)), down)


def test_signed_sets_take_the_signed_launches_and_unsigned_ones_todays(calls):
    q, k, v = _signed(seed=1, seeds=(1, 22)), _signed(out=6, seed=2, seeds=(2, 22)), _signed(seed=3, bias=True, seeds=(3, 22))
    group = HadamardLinearGroup([q, k, v])
    with torch.no_grad():
        group(torch.zeros(5, 40))
    assert _names(calls) == ["hadamard_signed_rows", "linear_group_forward", "hadamard_signed_group_rows",
                             "hadamard_signed_group_rows"]
    assert calls[0][1]["sign_in"] is q.sign_in and calls[0][1]["sign_out"] is None
    first, second = calls[2][1], calls[3][1]
    assert [m["sign_out"] for m in first] == [q.sign_out, v.sign_out] and [m["sign_out"] for m in second] == [k.sign_out]
    assert all(torch.equal(a, b) for a, b in zip([m["sign_out"] for m in first], [q.sign_out, v.sign_out]))
    assert first[1]["bias"] is v.bias and all("sign_in" not in m for m in first + second)
    group.dissolve()
    calls.clear()
    mlp = HadamardGatedMLP(q, v, torch.nn.Identity())
    with torch.no_grad():
        mlp(torch.zeros(5, 40))
    assert _names(calls) == ["hadamard_signed_rows", "linear_group_forward", "hadamard_signed_glu_rows"]
    assert calls[2][1]["sign_g"] is q.sign_out and calls[2][1]["sign_u"] is v.sign_out and calls[2][1]["bias_u"] is v.bias
    # unsigned sets: the unsigned wrappers with the arguments they always had
    calls.clear()
    a, b = _had(seed=1), _had(seed=2, bias=True)
    g2 = HadamardLinearGroup([a, b])
    with torch.no_grad():
        g2(torch.zeros(5, 40))
    assert _names(calls) == ["hadamard_rows", "linear_group_forward", "hadamard_group_rows"]
    assert all(set(m) == {"x", "y", "n_in", "n_out", "P", "bias"} for m in calls[2][1])
    g2.dissolve()
    calls.clear()
    with torch.no_grad():
        HadamardGatedMLP(a, b, torch.nn.Identity())(torch.zeros(5, 40))
    assert _names(calls) == ["hadamard_rows", "linear_group_forward", "hadamard_glu_rows"]
    assert set(calls[2][1]) == {"n_in", "n_out", "P", "bias_g", "bias_u", "act"}


# ---------------------------------------------------------------------------- model.py
class _Block(torch.nn.Module):
    def __init__(self, h=24, i=40):
        super().__init__()
        self.self_attn = torch.nn.Module()
        for name in ("q_proj", "k_proj", "v_proj"):
            setattr(self.self_attn, name, torch.nn.Linear(h, h if name == "q_proj" else 12, bias=name == "v_proj"))
        self.mlp = torch.nn.Module()
        self.mlp.gate_proj, self.mlp.up_proj = torch.nn.Linear(h, i, bias=False), torch.nn.Linear(h, i, bias=False)
        self.mlp.down_proj = torch.nn.Linear(i, h, bias=False)
        self.mlp.act_fn = torch.nn.SiLU()


def _toy():
    torch.manual_seed(4)
    net = torch.nn.Module()
    net.language = torch.nn.Module()
    net.language.layers = torch.nn.ModuleList([_Block(), _Block()])
    return net


def _quantise(monkeypatch, net, **kw):
    def gemm(A, B, *, C=None, D=None, gamma=0.0):
        out = A @ B if D is None else A @ B + gamma * D
        return out if C is None else C.copy_(out)

    monkeypatch.setattr(K, "gemm", gemm)
    monkeypatch.setattr(M, "_rel_error",
                        lambda W, out: float(torch.linalg.norm(W.float() - out) / torch.linalg.norm(W.float())))
    seen = []

    def decompose(qp, Ws, H):
        seen.extend(W.clone() for W in Ws)
        return [_Dec(W, 0.5) for W in Ws]

    rep = M.apply_caldera_quantization(net, None, M.driver_params(), decompose=decompose, device="cpu",
                                       selection=M.LayerSelection(layers=None, min_dim=1), packed=True,
                                       packed_hadamard=True, **kw)
    return rep, seen


def test_seed_derivation_is_the_documented_one():
    b = LIN.mix64(3)
    out, inn = M.hadamard_sign_seeds(3, "a.b.q_proj", 24)
    assert inn == LIN.mix64((b + 48) % 2 ** 64) >> 11
    assert out == LIN.mix64((b + 2 * zlib.crc32(b"a.b.q_proj") + 1) % 2 ** 64) >> 11
    assert 0 <= out < 2 ** 53 and 0 <= inn < 2 ** 53
    assert M.hadamard_sign_seeds(3, "other", 24)[1] == inn and M.hadamard_sign_seeds(3, "other", 24)[0] != out
    assert M.hadamard_sign_seeds(3, "a.b.q_proj", 25)[1] != inn and M.hadamard_sign_seeds(4, "a.b.q_proj", 24) != (out, inn)


def test_the_caller_raises_the_documented_errors():
    net = _toy()
    nothing = dict(decompose=lambda *a: pytest.fail("decomposed"), device="cpu")
    with pytest.raises(ValueError, match="hadamard_signs needs packed_hadamard=True"):
        M.apply_caldera_quantization(net, None, M.driver_params(), packed=True, hadamard_signs=3, **nothing)
    with pytest.raises(ValueError, match="hadamard_signs needs packed_hadamard=True"):
        M.apply_caldera_quantization(net, None, M.driver_params(), hadamard=True, hadamard_signs=3, **nothing)
    for bad in (-1, 1 << 53, 2.0, True):
        with pytest.raises(ValueError, match="2\\^53"):
            M.apply_caldera_quantization(net, None, M.driver_params(), packed=True, packed_hadamard=True,
                                         hadamard_signs=bad, **nothing)
    # padding changes n under a Hessian: as without signs
    with pytest.raises(ValueError, match="padding changes n"):
        M.apply_caldera_quantization(net, {n: torch.ones(m.weight.shape[1]) for n, m in net.named_modules()
                                           if isinstance(m, torch.nn.Linear)}, M.driver_params(), packed=True,
                                     packed_hadamard=True, hadamard_signs=3, device="cpu", decompose=nothing["decompose"],
                                     selection=M.LayerSelection(layers=None, min_dim=1))


def test_the_caller_builds_signed_layers_that_share_seed_in(monkeypatch):
    ref, net = _toy(), _toy()
    rep, seen = _quantise(monkeypatch, net, hadamard_signs=3)
    assert all(o.applied for o in rep.layers) and len(rep.layers) == 12
    mods, orig = dict(net.named_modules()), dict(ref.named_modules())
    for o in rep.layers:
        lin = mods[o.name]
        assert isinstance(lin, HadamardCalderaLinear)
        assert lin.sign_seeds == M.hadamard_sign_seeds(3, o.name, lin.in_features)
        # the decomposition, the recovered weight and the gate are the signed transform's
        W = orig[o.name].weight.data
        err = float(torch.linalg.norm(W - lin.dense_weight()) / torch.linalg.norm(W))
        assert abs(err - o.rel_error) < 1e-5, (o.name, err, o.rel_error)
    signed_in = M.hadamard_transform(orig[rep.layers[0].name].weight.data,
                                     signs=(mods[rep.layers[0].name].sign_out, mods[rep.layers[0].name].sign_in))[0]
    assert any(torch.equal(signed_in, W) for W in seen)
    for blk in net.language.layers:
        att, mlp = blk.self_attn, blk.mlp
        assert att.q_proj.sign_seeds[1] == att.k_proj.sign_seeds[1] == att.v_proj.sign_seeds[1] == mlp.gate_proj.sign_seeds[1]
        assert mlp.gate_proj.sign_seeds[1] == mlp.up_proj.sign_seeds[1] != mlp.down_proj.sign_seeds[1]
        assert len({lin.sign_seeds[0] for lin in (att.q_proj, att.k_proj, att.v_proj, mlp.gate_proj, mlp.up_proj)}) == 5
        assert att.v_proj.bias is not None
    # so the grouped and fused launches stay available
    grouped, skipped = M.group_shared_input_layers(net, hadamard=True)
    assert len(grouped) == 4 and not skipped
    M.ungroup_shared_input_layers(net)
    fused, skipped = M.fuse_gated_mlps(net, hadamard=True)
    assert fused == ["language.layers.0.mlp", "language.layers.1.mlp"] and not skipped
    # a set that does not fit is skipped with the reason, not raised
    M.unfuse_gated_mlps(net)
    blk = net.language.layers[0]
    blk.mlp.up_proj = HadamardCalderaLinear(blk.mlp.up_proj.inner, 24, 40)          # unsigned beside a signed gate
    grouped, skipped = M.group_shared_input_layers(net, hadamard=True)
    why = dict(skipped)[("language.layers.0.mlp.gate_proj", "language.layers.0.mlp.up_proj")]
    assert "incompatible" in why and "sign_seeds" in why and len(grouped) == 3
    fused, skipped = M.fuse_gated_mlps(net, hadamard=True)
    assert fused == ["language.layers.1.mlp"] and "sign_seeds" in dict(skipped)["language.layers.0.mlp"]


def test_without_the_keyword_nothing_changes(monkeypatch):
    a, b = _toy(), _toy()
    rep_a, seen_a = _quantise(monkeypatch, a)
    rep_b, seen_b = _quantise(monkeypatch, b, hadamard_signs=None)
    assert all(torch.equal(x, y) for x, y in zip(seen_a, seen_b)) and len(seen_a) == len(seen_b) == 12
    assert [o.rel_error for o in rep_a.layers] == [o.rel_error for o in rep_b.layers]
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and "sign" not in ka
        assert torch.equal(va, vb) if torch.is_tensor(va) else va == vb
    assert all(m.sign_seeds is None for m in a.modules() if isinstance(m, HadamardCalderaLinear))
