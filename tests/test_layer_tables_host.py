"""Host-side tables of what the packed and Hadamard-basis layers hand to the `_lib` entries: which operands
each factor format passes to each entry (forward, input gradient, dequant, group member dicts), the ordered
launch sequences of the layers alone, grouped, gated, materialised and on the dense prefill path, and the
construction errors of the groups and the gated blocks, each against its full text.  The entries are replaced
by recorders (as test_hadamard_signs_host.py replaces them) and CPU tensors pass for device tensors; the
expectations are literal tables.  No GPU."""
import itertools
import re

import pytest
import torch

from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import linear as LIN
from ee274_convexcaldera_llm_quantization_amd.linear import (CalderaGatedMLP, CalderaLinear, CalderaLinearGroup,
                                                              HadamardCalderaLinear, HadamardGatedMLP,
                                                              HadamardLinearGroup)

f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64

# entry -> (positional parameters, required keywords, optional keywords with their defaults): the signatures of _lib
_FACTOR_KW = dict(r=None, L_codes=None, R_codes=None)
SIGNATURES = {
    "linear_forward": ("x codes qscale gscale L R bias y", "m n bits", dict(ws=None)),
    "linear_packed_forward": ("x codes qscale gscale L R bias y", "m n bits", dict(_FACTOR_KW, ws=None)),
    "linear_codebook_forward": ("x codes qscale gscale L R bias y", "m n bits q_format", dict(_FACTOR_KW, ws=None)),
    "linear_backward_input": ("dy codes qscale gscale L R dx", "m n bits", dict(u_out=None, ws=None)),
    "linear_packed_backward_input": ("dy codes qscale gscale L R dx", "m n bits", dict(_FACTOR_KW, u_out=None, ws=None)),
    "linear_codebook_backward_input": ("dy codes qscale gscale L R dx", "m n bits q_format",
                                       dict(_FACTOR_KW, u_out=None, ws=None)),
    "linear_dequant": ("codes qscale gscale L R w", "m n bits q_format", dict(_FACTOR_KW)),
    "linear_group_forward": ("x members ys q_format", "", dict(ws=None)),
    "linear_glu_forward": ("x gate up h q_format act", "", dict(act=K.ACT_SILU, ws=None)),
    "hadamard_rows": ("x y", "n_in n_out P", dict(bias=None)),
    "hadamard_signed_rows": ("x y", "n_in n_out P", dict(bias=None, sign_in=None, sign_out=None)),
    "hadamard_group_rows": ("members", "", {}),
    "hadamard_signed_group_rows": ("members", "", {}),
    "hadamard_glu_rows": ("g u h", "n_in n_out P", dict(bias_g=None, bias_u=None, act=K.ACT_SILU)),
    "hadamard_signed_glu_rows": ("g u h", "n_in n_out P", dict(bias_g=None, bias_u=None, act=K.ACT_SILU, sign_g=None,
                                                               sign_u=None)),
}


@pytest.fixture
def calls(monkeypatch):
    """Every `_lib` entry the layers launch, replaced on `K` by a recorder with the entry's signature (an unknown
    or a missing keyword raises); torch.mm recorded too; CPU tensors answer `is_cuda` with True."""
    log = []

    def recorder(name, pos, req, opt):
        pos, req = pos.split(), req.split()

        def entry(*args, **kw):
            assert len(args) <= len(pos), (name, len(args))
            rec = dict(zip(pos, args))
            assert not set(kw) & set(rec), (name, kw)
            assert set(kw) <= set(pos[len(args):]) | set(req) | set(opt), (name, sorted(kw))
            assert (set(pos[len(args):]) - set(opt)) | set(req) <= set(kw), (name, sorted(kw))
            rec = dict(opt, **rec, **kw)
            for key in ("members", "ys"):
                if key in rec:
                    rec[key] = list(rec[key])
            log.append((name, rec))
            return next((rec[key] for key in ("w", "y", "h", "dx", "ys") if key in rec), None)   # the entry's output
        return entry

    for name, sig in SIGNATURES.items():
        assert callable(getattr(K, name))
        monkeypatch.setattr(K, name, recorder(name, *sig))
    real_mm = torch.mm

    def mm(a, b, *, out=None, out_dtype=None):
        log.append(("mm", dict(a=a, b=b, out=out, out_dtype=out_dtype)))
        if out is not None:
            return out.copy_(real_mm(a.float(), b.float()))
        return real_mm(a.float(), b.float()).to(out_dtype or a.dtype)

    monkeypatch.setattr(torch, "mm", mm)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    return log


def _names(log):
    return [c[0] for c in log]


def _table(**axes):
    """One test that runs `case(calls, **row)` for every row of the product of `axes`, the log emptied before
    each row; a failure names its row."""
    def wrap(case):
        def test(calls):
            for row in itertools.product(*axes.values()):
                calls.clear()
                row = dict(zip(axes, row))
                try:
                    case(calls, **row)
                except AssertionError as e:
                    raise AssertionError(f"{row}: {e}") from e
        test.__name__, test.__doc__ = case.__name__, case.__doc__
        return test
    return wrap


# ---------------------------------------------------------------------------- layers
M_, N_, RANK = 12, 40, 3


def _codes(m, n, bits, seed, nf=False):
    g = torch.Generator().manual_seed(seed)
    k = 2 ** (bits - 1) - 1
    return torch.randint(0, 2 ** bits, (m, n), generator=g) if nf else torch.randint(-k, k + 1, (m, n), generator=g)


def _layer(kind, m=M_, n=N_, seed=0, bias=False, bits=None):
    """A CalderaLinear of one of the issue's seven factor / Q formats."""
    g = torch.Generator().manual_seed(100 + seed)
    L, R = torch.randn(m, RANK, generator=g).half(), torch.randn(RANK, n, generator=g).half()
    Lc, Rc = (_codes(m, RANK, 4, seed + 1), 0.75, 4), (_codes(RANK, n, 2, seed + 2), 1.25, 2)
    b = torch.arange(m, dtype=f32) if bias else None
    kw = dict(qscale=0.05, gscale=1.5)
    if kind == "rank0":
        return CalderaLinear.from_codes(_codes(m, n, bits or 2, seed), None, None, b, bits=bits or 2, **kw)
    if kind == "fp16":
        return CalderaLinear.from_codes(_codes(m, n, bits or 2, seed), L, R, b, bits=bits or 2, **kw)
    if kind == "coded_L":
        return CalderaLinear.from_codes(_codes(m, n, 2, seed), None, R, b, bits=2, L_codes=Lc, **kw)
    if kind == "coded_R":
        return CalderaLinear.from_codes(_codes(m, n, 4, seed), L, None, b, bits=4, R_codes=Rc, **kw)
    if kind == "coded_LR":
        return CalderaLinear.from_codes(_codes(m, n, 2, seed), None, None, b, bits=2, L_codes=Lc, R_codes=Rc, **kw)
    if kind == "nf4_fp16":
        return CalderaLinear.from_codes(_codes(m, n, 4, seed, nf=True), L, R, b, bits=4, q_format=LIN.Q_FORMAT_NF, **kw)
    assert kind == "nf2_coded"
    return CalderaLinear.from_codes(_codes(m, n, 2, seed, nf=True), None, None, b, bits=2, L_codes=Lc, R_codes=Rc,
                                    q_format=LIN.Q_FORMAT_NF, **kw)


# kind -> (forward entry, input-gradient entry, L operand, R operand, bits, q_format, rank, L bits, R bits);
# an operand is "fp16" (the fp16 tensor), "codes" (the (codes, scale, bits) triple) or None (rank 0)
OPERANDS = {
    "rank0":     ("linear_forward", "linear_backward_input", None, None, 2, 0, 0, 16, 16),
    "fp16":      ("linear_forward", "linear_backward_input", "fp16", "fp16", 2, 0, 3, 16, 16),
    "coded_L":   ("linear_packed_forward", "linear_packed_backward_input", "codes", "fp16", 2, 0, 3, 4, 16),
    "coded_R":   ("linear_packed_forward", "linear_packed_backward_input", "fp16", "codes", 4, 0, 3, 16, 2),
    "coded_LR":  ("linear_packed_forward", "linear_packed_backward_input", "codes", "codes", 2, 0, 3, 4, 2),
    "nf4_fp16":  ("linear_codebook_forward", "linear_codebook_backward_input", "fp16", "fp16", 4, 1, 3, 16, 16),
    "nf2_coded": ("linear_codebook_forward", "linear_codebook_backward_input", "codes", "codes", 2, 1, 3, 4, 2),
}
# the keywords each entry family receives beside m, n, bits (None: the wrapper's default is left alone)
FAMILY_KW = {
    "linear_forward": (), "linear_backward_input": (),
    "linear_packed_forward": ("r", "L_codes", "R_codes"), "linear_packed_backward_input": ("r", "L_codes", "R_codes"),
    "linear_codebook_forward": ("q_format", "r", "L_codes", "R_codes"),
    "linear_codebook_backward_input": ("q_format", "r", "L_codes", "R_codes"),
}


def _check_operands(rec, lin, kind, L16, R16, family):
    """The factor operands of one recorded call: fp16 tensors by identity, code triples by their parts."""
    _, _, l_op, r_op, bits, fmt, rank, l_bits, r_bits = OPERANDS[kind]
    want_L = (lin.L if L16 is None else L16) if l_op == "fp16" else None
    want_R = (lin.R if R16 is None else R16) if r_op == "fp16" else None
    assert rec["L"] is want_L and rec["R"] is want_R, (kind, rec["L"], rec["R"])
    assert rec["codes"] is lin.codes and (rec["qscale"], rec["gscale"]) == (0.05, 1.5)
    assert (rec["m"], rec["n"], rec["bits"]) == (M_, N_, bits)
    if "q_format" in family:
        assert rec["q_format"] == fmt
    if "r" not in family:                         # the uniform fp16 entries take the rank from the factors
        assert "r" not in rec and "L_codes" not in rec
        return
    assert rec["r"] == rank
    for key, op, codes, scale, fbits in (("L_codes", l_op, lin.L_codes, 0.75, l_bits),
                                         ("R_codes", r_op, lin.R_codes, 1.25, r_bits)):
        if op == "codes":
            assert rec[key][0] is codes and tuple(rec[key][1:]) == (scale, fbits) and len(rec[key]) == 3, (kind, key)
        else:
            assert rec[key] is None, (kind, key)


def _masters(lin, kind, masters):
    """(L16, R16) as the callers pass them: None with the layer's buffers, and for a coded factor or rank 0."""
    if not masters:
        return None, None
    l_op, r_op = OPERANDS[kind][2:4]
    return (lin.L.clone() if l_op == "fp16" else None), (lin.R.clone() if r_op == "fp16" else None)


@_table(kind=list(OPERANDS), masters=[False, True])
def test_operand_table_forward_and_dequant(calls, kind, masters):
    lin = _layer(kind, bias=True)
    fwd, _, l_op, r_op, bits, fmt, rank, l_bits, r_bits = OPERANDS[kind]
    assert (lin.bits, lin.q_format, lin.rank, lin.L_bits, lin.R_bits) == (bits, fmt, rank, l_bits, r_bits)
    assert (lin.L is None) == (l_op == "codes") and (lin.R is None) == (r_op == "codes")
    assert rank or (tuple(lin.L.shape), tuple(lin.R.shape)) == ((M_, 0), (0, N_))     # rank 0 keeps empty buffers
    L16, R16 = _masters(lin, kind, masters)
    x2, y = torch.zeros(5, N_, dtype=f16), torch.empty(5, M_)
    assert LIN._launch_packed(lin, x2, y, L16, R16) is y
    assert _names(calls) == [fwd]
    rec = calls[0][1]
    assert set(rec) == set("x codes qscale gscale L R bias y m n bits ws".split()) | set(FAMILY_KW[fwd])
    assert rec["x"] is x2 and rec["y"] is y and rec["bias"] is lin.bias and rec["ws"] is None
    _check_operands(rec, lin, kind, L16, R16, FAMILY_KW[fwd])
    # cq_linear_dequant: one entry for every format, always with q_format, r and both code triples
    calls.clear()
    w = torch.empty(M_, N_, dtype=f16)
    LIN._dequant(lin, w, L16, R16)
    assert _names(calls) == ["linear_dequant"]
    rec = calls[0][1]
    assert set(rec) == set("codes qscale gscale L R w m n bits q_format r L_codes R_codes".split()) and rec["w"] is w
    _check_operands(rec, lin, kind, L16, R16, ("q_format", "r", "L_codes", "R_codes"))
    # the member dict of cq_linear_group_forward (always the layer's buffers: a group does not train)
    with torch.no_grad():
        CalderaLinearGroup([lin])(torch.zeros(5, N_))
    mem = calls[-1][1]["members"][0]
    assert calls[-1][0] == "linear_group_forward" and calls[-1][1]["q_format"] == fmt
    assert set(mem) == set("codes qscale gscale L R bias m n bits r L_codes R_codes".split()) and mem["bias"] is lin.bias
    _check_operands(mem, lin, kind, None, None, ("r", "L_codes", "R_codes"))


# kind -> whether u_out (T, r) fp32 is allocated when the R gradient is wanted
U_OUT = {"rank0": False, "fp16": True, "nf4_fp16": True}


@_table(kind=list(OPERANDS), masters=[False, True])
def test_operand_table_input_gradient(calls, kind, masters):
    lin = _layer(kind)
    bwd, l_op, r_op = OPERANDS[kind][1], OPERANDS[kind][2], OPERANDS[kind][3]
    # the saved fp16 factors: the buffers' or the masters' fp16 values; None for a coded factor and at rank 0
    L16 = (lin.L.clone() if masters else lin.L) if l_op == "fp16" else None
    R16 = (lin.R.clone() if masters else lin.R) if r_op == "fp16" else None
    dy16, x2 = torch.zeros(5, M_, dtype=f16), torch.zeros(5, N_, dtype=f16)
    trains = l_op == r_op == "fp16"
    for needs in ((True, False, False), (True, True, True)) if trains else ((True, False, False),):
        calls.clear()
        dx2, dL, dR = LIN._packed_backward(lin, dy16, x2, L16, R16, needs, f32, (f32, f32))
        assert _names(calls) == [bwd]
        rec = calls[0][1]
        extra = set(FAMILY_KW[bwd]) | {"u_out", "ws"}
        assert set(rec) == set("dy codes qscale gscale L R dx m n bits".split()) | extra
        assert rec["dy"] is dy16 and rec["dx"] is dx2 and tuple(dx2.shape) == (5, N_) and dx2.dtype == f32
        assert rec["L"] is L16 and rec["R"] is R16 and rec["ws"] is None
        _check_operands(dict(rec, L=rec["L"], R=rec["R"]), lin, kind, L16, R16, FAMILY_KW[bwd])
        if needs[2] and U_OUT[kind]:
            assert tuple(rec["u_out"].shape) == (5, RANK) and rec["u_out"].dtype == f32
            assert tuple(dL.shape) == (M_, RANK) and tuple(dR.shape) == (RANK, N_) and dL.dtype == dR.dtype == f32
        else:
            assert rec["u_out"] is None and dL is None and dR is None
    assert LIN._packed_backward(lin, dy16, x2, L16, R16, (False, False, False), f32, (None, None)) == (None, None, None)


# ---------------------------------------------------------------------------- sequences
OUT, INP, PR, PC = 12, 40, 16, 64
Y_PLAIN = {bf16: f32, f16: f16, f32: f32, f64: f32}     # the packed launch's output dtype for an x dtype
X_HAD = {bf16: bf16, f16: f16, f32: f32, f64: f32}      # the dtype the transforms read x in and write y in
DTYPES = [bf16, f16, f32, f64]


def _variant(variant, out=OUT, seed=0, bias=False, kind="fp16"):
    """A plain, an unsigned or a signed Hadamard layer of (out, 40): (layer, its packed layer)."""
    b = torch.arange(out, dtype=f32) if bias else None
    if variant == "plain":
        lin = _layer(kind, out, INP, seed, bias)
        return lin, lin
    inner = _layer(kind, LIN._next_pow2(out), PC, seed)
    return HadamardCalderaLinear(inner, INP, out, b, sign_seeds=(21 + seed, 22) if variant == "signed" else None), inner


def _resolve(v, layers):
    """"bias" / "sign_in" / "sign_out", optionally "@i" for the i-th layer -> that attribute, for `is`."""
    if not isinstance(v, str):
        return v
    name, _, i = v.partition("@")
    return getattr(layers[int(i or 0)], name)


def _check_sequence(log, want, layers):
    """want: (entry, {key: value}) in order; a value (shape, dtype) stands for a tensor, a string for a layer's
    attribute (by identity), a list for a list of tensors or of member dicts."""
    assert _names(log) == [w[0] for w in want], _names(log)
    for (name, rec), (_, fields) in zip(log, want):
        for key, v in fields.items():
            got = rec[key]
            if isinstance(v, tuple):
                assert (tuple(got.shape), got.dtype) == v, (name, key, tuple(got.shape), got.dtype)
            elif isinstance(v, list) and v and isinstance(v[0], tuple):
                assert [(tuple(t.shape), t.dtype) for t in got] == v, (name, key)
            elif isinstance(v, list):
                assert len(got) == len(v), (name, key)
                for g, w in zip(got, v):
                    assert set(g) == set(w), (name, key, sorted(g))
                    _check_sequence([(name, g)], [(name, w)], layers)
            elif isinstance(v, str):
                assert got is _resolve(v, layers), (name, key)
            else:
                assert got == v and type(got) is type(v), (name, key, got)


def _rows_entry(variant):
    return "hadamard_rows" if variant == "unsigned" else "hadamard_signed_rows"


def _signs(variant, **kw):
    """The sign keywords of a signed transform: absent from an unsigned entry's record."""
    return kw if variant == "signed" else {}


def _alone_forward(variant, dt, T=5, i=0, bias="bias"):
    """The launches of one layer alone on a (T, 40) x of dtype dt."""
    if variant == "plain":
        return [("linear_forward", dict(x=((T, INP), f16), y=((T, OUT), Y_PLAIN[dt]), bias=f"{bias}@{i}", m=OUT, n=INP))]
    rows, xd = _rows_entry(variant), X_HAD[dt]
    return [(rows, dict(x=((T, INP), xd), y=((T, PC), f16), n_in=INP, n_out=PC, P=PC, bias=None,
                        **_signs(variant, sign_in=f"sign_in@{i}", sign_out=None))),
            ("linear_forward", dict(x=((T, PC), f16), y=((T, PR), f32), bias=None, m=PR, n=PC)),
            (rows, dict(x=((T, PR), f32), y=((T, OUT), xd), n_in=PR, n_out=OUT, P=PR, bias=f"{bias}@{i}",
                        **_signs(variant, sign_in=None, sign_out=f"sign_out@{i}")))]


def _alone_backward(variant, dt, T=5):
    if variant == "plain":
        return [("linear_backward_input", dict(dy=((T, OUT), f16), dx=((T, INP), Y_PLAIN[dt]), u_out=None, m=OUT, n=INP))]
    rows, xd = _rows_entry(variant), X_HAD[dt]
    return [(rows, dict(x=((T, OUT), xd), y=((T, PR), f16), n_in=OUT, n_out=PR, P=PR, bias=None,
                        **_signs(variant, sign_in="sign_out", sign_out=None))),
            ("linear_backward_input", dict(dy=((T, PR), f16), dx=((T, PC), f32), u_out=None, m=PR, n=PC)),
            (rows, dict(x=((T, PC), f32), y=((T, INP), xd), n_in=PC, n_out=INP, P=PC, bias=None,
                        **_signs(variant, sign_in=None, sign_out="sign_in")))]


@_table(variant=["plain", "unsigned", "signed"], dt=DTYPES)
def test_sequence_alone_without_and_with_a_graph(calls, variant, dt):
    layer, packed = _variant(variant, bias=True)
    x = torch.zeros(1, 5, INP, dtype=dt)
    with torch.no_grad():
        y = layer(x)
    assert y.dtype == dt and tuple(y.shape) == (1, 5, OUT) and not y.requires_grad
    _check_sequence(calls, _alone_forward(variant, dt), [layer])
    assert calls[-2 if variant != "plain" else 0][1]["L"] is packed.L           # the buffers themselves
    # with a graph: the same forward launches, and the mirrored backward
    calls.clear()
    xg = torch.zeros(1, 5, INP, dtype=dt, requires_grad=True)
    y = layer(xg)
    assert y.dtype == dt and tuple(y.shape) == (1, 5, OUT) and y.requires_grad
    _check_sequence(calls, _alone_forward(variant, dt), [layer])
    calls.clear()
    y.backward(torch.ones_like(y))
    assert xg.grad.dtype == dt and tuple(xg.grad.shape) == (1, 5, INP)
    _check_sequence(calls, _alone_backward(variant, dt), [layer])


@_table(variant=["plain", "unsigned", "signed"])
def test_sequence_with_trainable_factors(calls, variant):
    """The masters rounded to fp16 reach the launches, with and without a graph; u_out is allocated for dR."""
    layer, packed = _variant(variant)
    layer.enable_factor_training()
    x = torch.zeros(5, INP)
    with torch.no_grad():
        layer(x)
    rec = calls[0 if variant == "plain" else 1][1]
    assert rec["L"].dtype == f16 and rec["L"] is not packed.L and packed.L.dtype == f32
    calls.clear()
    y = layer(x)                                   # the factors alone ask for a graph; no dx, so no input-gradient launch
    assert y.requires_grad and _names(calls) == _names(_alone_forward(variant, f32))
    calls.clear()
    y.backward(torch.ones_like(y))
    assert _names(calls) == ([] if variant == "plain" else [_rows_entry(variant)])
    calls.clear()
    y = layer(x.clone().requires_grad_())
    calls.clear()
    y.backward(torch.ones_like(y))
    assert _names(calls) == _names(_alone_backward(variant, f32))
    rec = calls[0 if variant == "plain" else 1][1]
    rows = 5
    assert tuple(rec["u_out"].shape) == (rows, RANK) and rec["u_out"].dtype == f32 and rec["L"].dtype == f16
    assert packed.L.grad.dtype == f32 and tuple(packed.R.grad.shape) == tuple(packed.R.shape)


def _member(i, pr, out, variant, bias):
    return dict(x=((5, pr), f32), y=((5, out), None), n_in=pr, n_out=out, P=pr, bias=bias,
                **_signs(variant, sign_out=f"sign_out@{i}"))


@_table(variant=["plain", "unsigned", "signed"], outs=[(12, 12, 12), (12, 6, 12)], dt=DTYPES)
def test_sequence_group_of_three(calls, variant, outs, dt):
    pairs = [_variant(variant, out, seed=i, bias=i == 2) for i, out in enumerate(outs)]
    layers, packed = [p[0] for p in pairs], [p[1] for p in pairs]
    group = (CalderaLinearGroup if variant == "plain" else HadamardLinearGroup)(layers)
    x = torch.zeros(1, 5, INP, dtype=dt)
    with torch.no_grad():
        ys = group(x)
    assert [(tuple(y.shape), y.dtype) for y in ys] == [((1, 5, out), dt) for out in outs]
    prs = [LIN._next_pow2(out) for out in outs]
    if variant == "plain":
        want = [("linear_group_forward", dict(x=((5, INP), f16), ys=[((5, out), Y_PLAIN[dt]) for out in outs], q_format=0))]
        biases = [None, None, "bias@2"]
    else:
        xd = X_HAD[dt]
        want = [(_rows_entry(variant), dict(x=((5, INP), xd), y=((5, PC), f16), n_in=INP, n_out=PC, P=PC, bias=None,
                                            **_signs(variant, sign_in="sign_in@0", sign_out=None))),
                ("linear_group_forward", dict(x=((5, PC), f16), ys=[((5, pr), f32) for pr in prs], q_format=0))]
        grouped = "hadamard_group_rows" if variant == "unsigned" else "hadamard_signed_group_rows"
        order = [[0, 1, 2]] if outs == (12, 12, 12) else [[0, 2], [1]]     # one launch per distinct pr, member order
        for bucket in order:
            mems = [_member(i, prs[i], outs[i], variant, "bias@2" if i == 2 else None) for i in bucket]
            for mem in mems:
                mem["y"] = (mem["y"][0], xd)
            want.append((grouped, dict(members=mems)))
        biases = [None, None, None]                                        # the output transform adds the bias
    _check_sequence(calls, want, layers)
    launch = calls[0 if variant == "plain" else 1][1]
    assert [m["m"] for m in launch["members"]] == (list(outs) if variant == "plain" else prs)
    for mem, lin, b in zip(launch["members"], packed, biases):
        assert mem["codes"] is lin.codes and mem["L"] is lin.L and mem["R"] is lin.R and mem["r"] == RANK
        assert mem["bias"] is _resolve(b, layers) and mem["L_codes"] is None and mem["R_codes"] is None
    if variant != "plain":                                                 # the transforms read the inner outputs
        flat = [m for c in calls[2:] for m in c[1]["members"]]
        inner_ys = launch["ys"]
        order = [0, 1, 2] if outs == (12, 12, 12) else [0, 2, 1]
        assert all(m["x"] is inner_ys[i] for m, i in zip(flat, order))


@_table(variant=["plain", "unsigned", "signed"], dt=DTYPES)
def test_sequence_gated_mlp_fused_and_falling_back(calls, variant, dt):
    (gate, gp), (up, upk) = _variant(variant, seed=0, bias=True), _variant(variant, seed=1)
    if variant == "signed":
        up = HadamardCalderaLinear(upk, INP, OUT, None, sign_seeds=(5, 22))
    cls = CalderaGatedMLP if variant == "plain" else HadamardGatedMLP
    mlp = cls(gate, up, torch.nn.Identity())
    x = torch.zeros(1, 5, INP, dtype=dt)
    with torch.no_grad():
        h = mlp(x)
    assert h.dtype == dt and tuple(h.shape) == (1, 5, OUT)
    if variant == "plain":
        want = [("linear_glu_forward", dict(x=((5, INP), f16), h=((5, OUT), Y_PLAIN[dt]), q_format=0, act=K.ACT_SILU))]
        _check_sequence(calls, want, [gate, up])
        g, u = calls[0][1]["gate"], calls[0][1]["up"]
        assert g["bias"] is gate.bias and u["bias"] is None
    else:
        xd = X_HAD[dt]
        glu = "hadamard_glu_rows" if variant == "unsigned" else "hadamard_signed_glu_rows"
        want = [(_rows_entry(variant), dict(x=((5, INP), xd), y=((5, PC), f16), n_in=INP, n_out=PC, P=PC, bias=None,
                                            **_signs(variant, sign_in="sign_in@0", sign_out=None))),
                ("linear_group_forward", dict(x=((5, PC), f16), ys=[((5, PR), f32)] * 2, q_format=0)),
                (glu, dict(g=((5, PR), f32), u=((5, PR), f32), h=((5, OUT), xd), n_in=PR, n_out=OUT, P=PR,
                           bias_g="bias@0", bias_u=None, act=K.ACT_SILU,
                           **_signs(variant, sign_g="sign_out@0", sign_u="sign_out@1")))]
        _check_sequence(calls, want, [gate, up])
        g, u = calls[1][1]["members"]
        assert g["bias"] is None and calls[2][1]["g"] is calls[1][1]["ys"][0] and calls[2][1]["u"] is calls[1][1]["ys"][1]
    for mem, lin in ((g, gp), (u, upk)):
        assert set(mem) == set("codes qscale gscale L R bias m n bits r L_codes R_codes".split())
        assert mem["codes"] is lin.codes and mem["L"] is lin.L and mem["R"] is lin.R and mem["r"] == RANK
    # past max_fused_tokens: the formula through the layers' own launches, gate then up
    calls.clear()
    limited = cls(gate, up, torch.nn.Identity(), act="identity", max_fused_tokens=4)
    with torch.no_grad():
        h = limited.glu(x)
    assert h.dtype == dt and tuple(h.shape) == (1, 5, OUT)
    _check_sequence(calls, _alone_forward(variant, dt, i=0) + _alone_forward(variant, dt, i=1), [gate, up])
    calls.clear()
    with torch.no_grad():
        limited.glu(x[:, :4])
    assert _names(calls) == [w[0] for w in want] and calls[-1][1]["act"] == K.ACT_IDENTITY


@_table(variant=["plain", "unsigned", "signed"], dt=[f16, bf16, f32])
def test_sequence_materialize(calls, variant, dt):
    layer, packed = _variant(variant, bias=True)
    W = layer.materialize(dt)
    assert W.dtype == dt and tuple(W.shape) == (OUT, INP)
    if variant == "plain":
        want = [("linear_dequant", dict(w=((OUT, INP), dt), m=OUT, n=INP, r=RANK, q_format=0))]
    else:
        rows = _rows_entry(variant)
        want = [("linear_dequant", dict(w=((PR, PC), f32), m=PR, n=PC, r=RANK, q_format=0)),
                (rows, dict(x=((PR, PC), f32), y=((PR, INP), f32), n_in=PC, n_out=INP, P=PC, bias=None,
                            **_signs(variant, sign_in=None, sign_out="sign_in"))),
                (rows, dict(x=((INP, PR), f32), y=((INP, OUT), dt), n_in=PR, n_out=OUT, P=PR, bias=None,
                            **_signs(variant, sign_in=None, sign_out="sign_out")))]
    _check_sequence(calls, want, [layer])
    assert calls[0][1]["L"] is packed.L and calls[0][1]["codes"] is packed.codes
    out = torch.empty(OUT, INP, dtype=dt)
    assert layer.materialize(out=out) is out and _names(calls) == [w[0] for w in want] * 2


@_table(variant=["plain", "unsigned", "signed"], dt=DTYPES)
def test_sequence_dense_prefill(calls, variant, dt):
    """At dense_prefill_tokens the packed launch becomes cq_linear_dequant into the fp16 scratch weight and one
    GEMM; the transforms around it stay.  A layer in a group or a gated block runs alone there."""
    layer, packed = _variant(variant)
    layer.dense_prefill_tokens = 17
    assert packed.dense_prefill_tokens == 17
    T = 17
    x = torch.zeros(T, INP, dtype=dt)
    with torch.no_grad():
        y = layer(x)
    assert y.dtype == dt and tuple(y.shape) == (T, OUT)
    pm, pn = (OUT, INP) if variant == "plain" else (PR, PC)
    ydt = Y_PLAIN[dt] if variant == "plain" else f32
    dense = [("linear_dequant", dict(w=((pm, pn), f16), m=pm, n=pn, r=RANK, q_format=0)),
             ("mm", dict(a=((T, pn), f16), b=((pn, pm), f16), out=None if ydt == f16 else None,
                         out_dtype=None if ydt == f16 else f32))]
    if ydt == f16:
        dense[1][1]["out"] = ((T, pm), f16)
    alone = _alone_forward(variant, dt, T=T, bias="bias")
    want = dense if variant == "plain" else [alone[0], *dense, alone[2]]
    _check_sequence(calls, want, [layer])
    calls.clear()
    with torch.no_grad():
        layer(x[:16])
    assert _names(calls) == _names(alone)
    # the input gradient at that length: a fresh materialisation and the GEMM dy16 W16
    calls.clear()
    xg = torch.zeros(T, INP, dtype=dt, requires_grad=True)
    y = layer(xg)
    calls.clear()
    y.backward(torch.ones_like(y))
    back = _alone_backward(variant, dt, T=T)
    dxdt = Y_PLAIN[dt] if variant == "plain" else f32
    gemm = [("linear_dequant", dict(w=((pm, pn), f16), m=pm, n=pn)),
            ("mm", dict(a=((T, pm), f16), b=((pm, pn), f16), out_dtype=None if dxdt == f16 else f32))]
    _check_sequence(calls, gemm if variant == "plain" else [back[0], *gemm, back[2]], [layer])
    # a group and a gated block leave such a call to the members' own launches
    other, _ = _variant(variant, seed=1)
    if variant == "signed":
        other = HadamardCalderaLinear(other.inner, INP, OUT, None, sign_seeds=(7, 22))
    group = (CalderaLinearGroup if variant == "plain" else HadamardLinearGroup)([layer, other])
    calls.clear()
    with torch.no_grad():
        group(x)
    plain_other = _alone_forward(variant, dt, T=T, i=1)
    _check_sequence(calls, want + plain_other, [layer, other])
    group.dissolve()
    mlp = (CalderaGatedMLP if variant == "plain" else HadamardGatedMLP)(layer, other, torch.nn.Identity())
    calls.clear()
    with torch.no_grad():
        mlp(x)
    _check_sequence(calls, want + plain_other, [layer, other])


# ---------------------------------------------------------------------------- messages
def _had(out=OUT, inp=INP, seed=0, seeds=None, kind="fp16", bits=None):
    inner = _layer(kind, LIN._next_pow2(out), LIN._next_pow2(inp), seed, bits=bits)
    return HadamardCalderaLinear(inner, inp, out, None, sign_seeds=seeds)


def _raises(text, fn, *args, **kw):
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        fn(*args, **kw)


def test_message_table_of_the_groups():
    a = _layer("fp16")
    grouped = _layer("fp16", seed=1)
    CalderaLinearGroup([grouped])
    G = CalderaLinearGroup
    _raises("CalderaLinearGroup: 0 members, not 1 .. 8", G, [])
    _raises("CalderaLinearGroup: 9 members, not 1 .. 8", G, [_layer("rank0", seed=i) for i in range(9)])
    _raises("CalderaLinearGroup: member 0 is a HadamardCalderaLinear: its input and output transforms are per layer, "
            "it cannot be grouped", G, [_had()])
    _raises("CalderaLinearGroup: member 1 is a Linear, not a CalderaLinear", G, [a, torch.nn.Linear(INP, OUT)])
    _raises("CalderaLinearGroup: member 1 is given twice", G, [a, a])
    _raises("CalderaLinearGroup: member 1 is already in a group (dissolve() it first)", G, [a, grouped])
    _raises("CalderaLinearGroup: member 1: device meta differs from member 0's cpu", G, [a, _layer("fp16", seed=2).to("meta")])
    _raises("CalderaLinearGroup: member 1: in_features 48 differs from member 0's 40", G, [a, _layer("fp16", n=48, seed=2)])
    _raises("CalderaLinearGroup: member 1: bits 4 differs from member 0's 2", G, [a, _layer("fp16", seed=2, bits=4)])
    _raises("CalderaLinearGroup: member 1: q_format 1 differs from member 0's 0", G, [a, _layer("nf2_coded", seed=2)])
    _raises("CalderaLinearGroup: member 2: L_bits 4 differs from member 1's 16", G,
            [_layer("rank0", seed=3), a, _layer("coded_L", seed=2)])
    _raises("CalderaLinearGroup: member 1: R_bits 2 differs from member 0's 16", G, [_layer("coded_L", seed=3),
                                                                                    _layer("coded_LR", seed=2)])
    # a member's format is judged as it is reached: the earlier member's fault is the one reported
    _raises("CalderaLinearGroup: member 1: bits 4 differs from member 0's 2", G, [a, _layer("fp16", seed=2, bits=4), a])
    assert a.group is None
    h = _had()
    in_group = _had(seed=1)
    HadamardLinearGroup([in_group])
    inner_grouped = _had(seed=2)
    CalderaLinearGroup([inner_grouped.inner])
    G = HadamardLinearGroup
    _raises("HadamardLinearGroup: 0 members, not 1 .. 8", G, [])
    _raises("HadamardLinearGroup: 9 members, not 1 .. 8", G, [_had(seed=i, kind="rank0") for i in range(9)])
    _raises("HadamardLinearGroup: member 1 is a CalderaLinear, not a HadamardCalderaLinear", G, [h, a])
    _raises("HadamardLinearGroup: member 1 is given twice", G, [h, h])
    _raises("HadamardLinearGroup: member 1 is already in a group (dissolve() it first)", G, [h, in_group])
    _raises("HadamardLinearGroup: member 1: inner is in a CalderaLinearGroup (dissolve() it first)", G, [h, inner_grouped])
    _raises("HadamardLinearGroup: member 1: device meta differs from member 0's cpu", G, [h, _had(seed=3).to("meta")])
    _raises("HadamardLinearGroup: member 1: in_features 70 differs from member 0's 40", G, [h, _had(inp=70, seed=3)])
    _raises("HadamardLinearGroup: member 1: inner bits 4 differs from member 0's 2", G, [h, _had(seed=3, bits=4)])
    _raises("HadamardLinearGroup: member 2: inner L_bits 4 differs from member 1's 16", G,
            [_had(seed=4, kind="rank0"), h, _had(seed=3, kind="coded_L")])
    _raises("HadamardLinearGroup: member 1: sign_seeds None but member 0's are (21, 22): signed and unsigned layers "
            "do not share the input transform", G, [_had(seed=4, seeds=(21, 22)), h])
    _raises("HadamardLinearGroup: member 1: sign seed_in 23 differs from member 0's 22", G,
            [_had(seed=4, seeds=(21, 22)), _had(seed=5, seeds=(21, 23))])
    # the formats and the signs are judged on the whole set, after every member's own rules
    _raises("HadamardLinearGroup: member 2 is given twice", G, [h, _had(seed=3, bits=4), h])
    assert h.group is None


def test_message_table_of_the_gated_blocks():
    down = torch.nn.Linear(OUT, INP)
    a, b = _layer("fp16"), _layer("fp16", seed=1)
    B = CalderaGatedMLP
    _raises("CalderaGatedMLP: act 'gelu' not in ('silu', 'identity')", B, a, b, down, act="gelu")
    _raises("CalderaGatedMLP: gate_proj is a HadamardCalderaLinear: its input and output transforms are per layer, it "
            "does not fit the fused launch", B, _had(), b, down)
    _raises("CalderaGatedMLP: up_proj is a Linear, not a CalderaLinear", B, a, torch.nn.Linear(INP, OUT), down)
    _raises("CalderaGatedMLP: gate_proj and up_proj are the same layer", B, a, a, down)
    _raises("CalderaGatedMLP: up_proj: device meta differs from gate_proj's cpu", B, a, _layer("fp16", seed=2).to("meta"), down)
    _raises("CalderaGatedMLP: up_proj: in_features 48 differs from gate_proj's 40", B, a, _layer("fp16", n=48, seed=2), down)
    _raises("CalderaGatedMLP: up_proj: out_features 13 differs from gate_proj's 12", B, a, _layer("fp16", m=13, seed=2), down)
    _raises("CalderaGatedMLP: up_proj: bits 4 differs from gate_proj's 2", B, a, _layer("fp16", seed=2, bits=4), down)
    _raises("CalderaGatedMLP: up_proj: L_bits 4 differs from gate_proj's 16", B, a, _layer("coded_L", seed=2), down)
    _raises("CalderaGatedMLP: down_proj is a function, not a module", B, a, b, lambda x: x)
    _raises("CalderaGatedMLP: max_fused_tokens 1.5 is not \"auto\", None or an int", B, a, b, down, max_fused_tokens=1.5)
    _raises("CalderaGatedMLP: max_fused_tokens True is not \"auto\", None or an int", B, a, b, down, max_fused_tokens=True)
    assert B(a, b, down).max_fused_tokens == "auto" and B(a, b, down, max_fused_tokens=None).max_fused_tokens is None
    g, u = _had(), _had(seed=1)
    B = HadamardGatedMLP
    _raises("HadamardGatedMLP: act 'gelu' not in ('silu', 'identity')", B, g, u, down, act="gelu")
    _raises("HadamardGatedMLP: gate_proj is a CalderaLinear, not a HadamardCalderaLinear", B, a, u, down)
    _raises("HadamardGatedMLP: gate_proj and up_proj are the same layer", B, g, g, down)
    _raises("HadamardGatedMLP: up_proj: device meta differs from gate_proj's cpu", B, g, _had(seed=2).to("meta"), down)
    _raises("HadamardGatedMLP: up_proj: in_features 48 differs from gate_proj's 40", B, g, _had(inp=48, seed=2), down)
    _raises("HadamardGatedMLP: up_proj: out_features 13 differs from gate_proj's 12", B, g, _had(out=13, seed=2), down)
    _raises("HadamardGatedMLP: up_proj: inner bits 4 differs from gate_proj's 2", B, g, _had(seed=2, bits=4), down)
    _raises("HadamardGatedMLP: up_proj: inner R_bits 2 differs from gate_proj's 16", B, _had(seed=3, bits=4),
            _had(seed=2, kind="coded_R"), down)
    _raises("HadamardGatedMLP: up_proj: sign_seeds (21, 22) but gate_proj's are None: signed and unsigned layers do "
            "not share the input transform", B, g, _had(seed=2, seeds=(21, 22)), down)
    _raises("HadamardGatedMLP: up_proj: sign seed_in 23 differs from gate_proj's 22", B, _had(seed=3, seeds=(1, 22)),
            _had(seed=2, seeds=(1, 23)), down)
    _raises("HadamardGatedMLP: down_proj is a function, not a module", B, g, u, lambda x: x)
    _raises("HadamardGatedMLP: max_fused_tokens 'auto' is not None or an int", B, g, u, down, max_fused_tokens="auto")
    assert B(g, u, down).max_fused_tokens is None and B(g, u, down).extra_repr() == "act=silu"
    # the limits' meanings: "auto" looks FUSED_TOKEN_LIMIT up by the Q bits, None is no limit
    four = CalderaGatedMLP(_layer("fp16", seed=5, bits=4), _layer("fp16", seed=6, bits=4), down)
    with torch.no_grad():
        assert LIN.FUSED_TOKEN_LIMIT == {2: None, 4: 64} and LIN.HADAMARD_GROUP_TOKEN_LIMIT is None
        assert four._fused(torch.zeros(64, INP)) and not four._fused(torch.zeros(65, INP))
        assert CalderaGatedMLP(a, b, down)._fused(torch.zeros(4096, INP)) and B(g, u, down)._fused(torch.zeros(4096, INP))
