"""Host-side checks of the Hadamard transform entry and of HadamardCalderaLinear: the cases of
hadamard_cases.py are what they claim (exact references are representable, planted faults
show), the ctypes struct matches the header, cq_hadamard_rows validates before any device call,
and the layer / model.py surface (constructors, state, results files, errors, the inputs the
decomposition receives) on CPU tensors.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg
import torch

import hadamard_cases as HC
import linear_cases as LC
from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import model as M
from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear, HadamardCalderaLinear
from ee274_convexcaldera_llm_quantization_amd.sharding import load_results, save_results
from test_linear_host import _Dec, _decomposition, _tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "caldera_hip.h")


# ---------------------------------------------------------------------------- the cases
def test_case_lists_cover_every_regime():
    for cases, Ps in ((HC.EXACT, {1, 4, 64, 1024, 4096, 16384}), (HC.RANDOM, {2, 32, 128, 512, 2048, 8192, 32768})):
        assert {c.P for c in cases} == Ps
        assert {c.rows for c in cases} == {1, 3, 17, 70}
        assert {c.xdt for c in cases} == set(HC.XDT)
    assert {c.ydt for c in HC.EXACT16} == {"f16", "bf16"}
    assert max(c.P for c in HC.EXACT16 if c.ydt == "bf16") == 64 and max(c.P for c in HC.EXACT16) == 1024
    big = [c for c in HC.ALL if c.P >= 64]
    for pick in (lambda c: c.n_in, lambda c: c.n_out):
        assert {(pick(c) == c.P, pick(c) == c.P - 5, pick(c) == c.P // 2 + 1, pick(c) == 1) for c in big} == \
            {(True, False, False, False), (False, True, False, False), (False, False, True, False),
             (False, False, False, True)}
    assert any(c.bias for c in HC.EXACT) and len({c.id for c in HC.ALL}) == len(HC.ALL)


def test_kronecker_reference_is_scipys_matrix():
    rng = np.random.default_rng(0)
    for P in (1, 2, 64, 512, 2048):
        X = rng.standard_normal((3, P))
        np.testing.assert_allclose(HC.hadamard64(X, P), X @ scipy.linalg.hadamard(P).astype(np.float64),
                                   rtol=0, atol=1e-9)
    i, j = 37, 1234                  # entry (i, j) is (-1)^popcount(i & j)
    e = np.zeros((1, 4096))
    e[0, j] = 1.0
    assert HC.hadamard64(e, 4096)[0, i] == (-1) ** bin(i & j).count("1")


@pytest.mark.parametrize("case", HC.EXACT + HC.EXACT16, ids=lambda c: c.id)
def test_exact_references_are_representable(case):
    y, _ = HC.reference(case)
    d = HC.inputs(case)
    assert round(np.log2(case.P)) % 2 == 0                      # c is a power of two
    x = d["x"].astype(np.float64)
    assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= (4 if case.kind == "exact" else 1)
    # every partial sum of any stage order is an integer bounded by sum |x|
    assert np.abs(x).sum(1).max() <= (65536 if case.kind == "exact" else 1024)
    assert np.array_equal(y, y.astype(np.float32).astype(np.float64))
    unscaled = (y - (0 if d["bias"] is None else d["bias"].astype(np.float64))) * np.sqrt(case.P)
    assert np.array_equal(unscaled, np.rint(unscaled))
    if d["bias"] is not None:
        assert np.array_equal(d["bias"] * 2, np.rint(d["bias"] * 2))
    if case.ydt == "f16":
        assert np.array_equal(y, y.astype(np.float16).astype(np.float64))
    if case.ydt == "bf16":
        assert np.array_equal(y, HC.from_bf16_bits(HC.to_bf16_bits(y.astype(np.float32))).astype(np.float64))
    # x is exact in the dtype it is handed over in
    if case.xdt == "f16":
        assert np.array_equal(d["x"], d["x"].astype(np.float16).astype(np.float32))
    if case.xdt == "bf16":
        assert np.array_equal(d["x"], HC.from_bf16_bits(HC.to_bf16_bits(d["x"])))


@pytest.mark.parametrize("fault", HC.FAULTS)
@pytest.mark.parametrize("case", HC.ALL, ids=lambda c: c.id)
def test_planted_fault_shows_in_every_case(case, fault):
    y, bar = HC.reference(case)
    yf, _ = HC.reference(case, fault)
    if case.kind == "random":
        assert (np.abs(yf - y) / bar).max() >= 10
    else:
        assert (y != yf).any()


def test_random_inputs_are_exact_in_their_dtype():
    for case in HC.RANDOM:
        x = HC.inputs(case)["x"]
        if case.xdt == "f16":
            assert np.array_equal(x, x.astype(np.float16).astype(np.float32))
        if case.xdt == "bf16":
            assert np.array_equal(x, HC.from_bf16_bits(HC.to_bf16_bits(x)))


# ---------------------------------------------------------------------------- the ABI
_CTYPE = {"const void*": 8, "void*": 8, "const float*": 8, "int": 4, "int64_t": 8, "float": 4}


def _header_layout(name):
    """[(field, offset)] and the size of a struct of the header, by C's natural alignment."""
    txt = open(HEADER).read()
    body = txt[txt.index(f"typedef struct {name}"):txt.index(f"}} {name};")].split("{", 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, out = 0, []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        mt = re.match(r"((?:const\s+)?[A-Za-z_0-9]+\s*\*?)\s*(.*)", decl)
        ctype = re.sub(r"\s*\*", "*", mt.group(1).strip())
        size = _CTYPE[ctype]
        for field in (f.strip() for f in mt.group(2).split(",")):
            off = -(-off // size) * size
            out.append((field, off))
            off += size
    return out, -(-off // 8) * 8


def test_hadamard_args_struct_matches_header():
    layout, size = _header_layout("cq_hadamard_args")
    assert [f for f, _ in K.HadamardArgs._fields_] == [f for f, _ in layout]
    assert [(f, getattr(K.HadamardArgs, f).offset) for f, _ in K.HadamardArgs._fields_] == layout
    assert ctypes.sizeof(K.HadamardArgs) == size == 88
    txt = open(HEADER).read()
    assert int(re.search(r"#define CQ_HADAMARD_MAX_N (\d+)", txt).group(1)) == K.HADAMARD_MAX_N == 32768
    assert "cq_hadamard_rows" in K.EXPORTS


def test_abi_version_is_still_5():
    txt = open(HEADER).read()
    assert int(re.search(r"#define CQ_ABI_VERSION (\d+)", txt).group(1)) == 5 == K.ABI_VERSION
    assert K.load().cq_abi_version() == 5


def test_entry_rejects_bad_arguments_without_a_device():
    """Validation runs before any HIP call: CQ_EINVAL with a message; rows == 0 returns 0."""
    lib = K.load()
    buf = torch.zeros(8192, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16

    def args(**kw):
        a = K.HadamardArgs()
        a.x, a.x_dtype, a.ldx = base, K.CQ_F16, 64
        a.y, a.y_dtype, a.ldy = base + 4096, K.CQ_F32, 64
        a.rows, a.n_in, a.n_out, a.P = 2, 64, 64, 64
        for key, v in kw.items():
            setattr(a, key, v)
        return a

    for kw, word in ((dict(P=48), "power of two"), (dict(P=0), "power of two"),
                     (dict(P=2 * K.HADAMARD_MAX_N, n_in=64, n_out=64), "power of two"),
                     (dict(n_in=65, ldx=128), "n_in"), (dict(n_in=0), "n_in"), (dict(n_out=65, ldy=128), "n_out"),
                     (dict(x_dtype=K.CQ_F64), "x dtype"), (dict(y_dtype=7), "y dtype"),
                     (dict(x=base + 1), "x is not aligned"), (dict(y=base + 4098), "y is not aligned"),
                     (dict(x=base + 2, x_dtype=K.CQ_F32), "x is not aligned"),
                     (dict(bias=base + 2), "bias is not aligned"),
                     (dict(ldx=63), "leading dimension"), (dict(ldy=10), "leading dimension"),
                     (dict(rows=-1), "rows")):
        a = args(**kw)
        assert lib.cq_hadamard_rows(ctypes.byref(a), None) == K.CQ_EINVAL, kw
        assert word in lib.cq_last_error().decode(), (kw, lib.cq_last_error())
    assert lib.cq_hadamard_rows(None, None) == K.CQ_EINVAL
    assert lib.cq_hadamard_rows(ctypes.byref(args(rows=0)), None) == 0          # no launch, no device needed
    assert lib.cq_hadamard_rows(ctypes.byref(args(rows=0, x=None, y=None)), None) == 0


def test_binding_refuses_wrong_operands_with_a_message():
    x, y = torch.zeros(3, 60, dtype=torch.float16), torch.zeros(3, 64)
    ok = dict(n_in=60, n_out=64, P=64)
    assert K.hadamard_args(x, y, **ok).ldx == 60
    for xs, ys, kw, word in ((x.double(), y, ok, "x must be fp16, bf16 or fp32"),
                             (x, y.to(torch.int32), ok, "y must be fp16, bf16 or fp32"),
                             (x[0], y, ok, "x must be a matrix"), (x.t().contiguous().t(), y, ok, "unit column stride"),
                             (x, y[:2], ok, "differ in rows"), (x, y, dict(ok, n_in=64), "does not have 64 columns"),
                             (x, y, dict(ok, P=48), "power of two"), (x, y, dict(ok, P=32), "do not fit"),
                             (x, y, dict(ok, P=2 * K.HADAMARD_MAX_N), "power of two"),
                             (x, y, dict(ok, bias=torch.zeros(64, dtype=torch.float16)), "bias"),
                             (x, y, dict(ok, bias=torch.zeros(60)), "bias")):
        with pytest.raises(ValueError, match=word):
            K.hadamard_args(xs, ys, **kw)
    with pytest.raises(RuntimeError, match="HIP"):
        K.hadamard_rows(x, y, **ok)


# ---------------------------------------------------------------------------- HadamardCalderaLinear
def _padded_layer(m=12, n=198, r=5, bits=2, seed=0):
    """Operands of a layer on the padded (pr, pc) grid of an (m, n) weight."""
    pr, pc = 1 << (m - 1).bit_length(), 1 << (n - 1).bit_length()
    rng = np.random.default_rng(seed)
    k = 2 ** (bits - 1) - 1
    c = rng.integers(-k, k + 1, (pr, pc)).astype(np.int8)
    L = rng.standard_normal((pr, r)).astype(np.float32)
    R = rng.standard_normal((r, pc)).astype(np.float32)
    return c, L, R, 0.37, 1.25


@pytest.mark.parametrize("bits,m,n", [(2, 12, 198), (4, 12, 198), (2, 16, 64), (4, 33, 130)])
def test_constructors_agree_and_dense_weight_is_the_recovered_matrix(bits, m, n):
    c, L, R, s, gs = _padded_layer(m, n, bits=bits)
    pr, pc = c.shape
    bias = torch.arange(m, dtype=torch.float32) / 7
    a = HadamardCalderaLinear.from_decomposition(_decomposition(c, L, R, s, gs, bits), bits, (m, n), bias=bias)
    assert (a.in_features, a.out_features, a.padded_shape) == (n, m, (pr, pc))
    assert isinstance(a.inner, CalderaLinear) and a.inner.bias is None and a.bias.dtype == torch.float32
    assert a.get_extra_state() == {"in_features": n, "out_features": m}
    assert not list(a.parameters())
    assert a.packed_bytes() == a.inner.packed_bytes() + 4 * m
    k = 2 ** (bits - 1) - 1
    Wt = gs * (c.astype(np.float64) * (s / k) + a.inner.L.double().numpy() @ a.inner.R.double().numpy())
    H1 = scipy.linalg.hadamard(pr) / np.sqrt(pr)
    H2 = scipy.linalg.hadamard(pc) / np.sqrt(pc)
    np.testing.assert_allclose(a.dense_weight().double().numpy(), (H1 @ Wt @ H2)[:m, :n], rtol=1e-5, atol=1e-5)
    assert a.dense_weight().shape == (m, n)
    # to_result -> from_result reproduces the buffers bit for bit
    res = a.to_result("layer")
    assert res.extra["hadamard"] == [m, n] and (res.m, res.n) == (pr, pc)
    b = HadamardCalderaLinear.from_result(res, bias=bias)
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb) and {"inner.codes", "inner.L", "inner.R", "bias"} <= set(sa)
    for key, v in sa.items():
        if torch.is_tensor(v):
            assert v.dtype == sb[key].dtype and torch.equal(v, sb[key]), key
        else:
            assert v == pytest.approx(sb[key]), key
    assert np.array_equal(a.inner.codes.numpy(), LC.inference_codes(c, bits))


def test_coded_factors_pass_through_to_the_inner_layer():
    c, L, R, s, gs = _padded_layer()
    dec = _decomposition(c, L, R, s, gs, 2)
    rng = np.random.default_rng(3)
    dec.L_idxs = torch.from_numpy(rng.integers(-7, 8, (1, 5 * 16)).astype(np.int8))
    dec.R_idxs = torch.from_numpy(rng.integers(-1, 2, (1, 5 * 256)).astype(np.int8))
    dec.L_scale, dec.R_scale = torch.tensor([[0.5]]), torch.tensor([[0.25]])
    a = HadamardCalderaLinear.from_decomposition(dec, 2, (12, 198), L_bits=4, R_bits=2)
    direct = CalderaLinear.from_decomposition(dec, 2, L_bits=4, R_bits=2)
    assert (a.inner.L_bits, a.inner.R_bits) == (4, 2) and a.inner.L is None and a.inner.R is None
    assert torch.equal(a.inner.L_codes, direct.L_codes) and torch.equal(a.inner.R_codes, direct.R_codes)
    b = HadamardCalderaLinear.from_result(a.to_result("x"))
    assert torch.equal(b.inner.L_codes, a.inner.L_codes) and torch.equal(b.inner.R_codes, a.inner.R_codes)
    assert (b.inner.lscale, b.inner.rscale) == (a.inner.lscale, a.inner.rscale)


def test_state_dict_round_trips(tmp_path):
    c, L, R, s, gs = _padded_layer()
    a = HadamardCalderaLinear.from_decomposition(_decomposition(c, L, R, s, gs, 2), 2, (12, 198),
                                                 bias=torch.arange(12, dtype=torch.float32))
    c2, L2, R2, _, _ = _padded_layer(seed=1)
    b = HadamardCalderaLinear.from_decomposition(_decomposition(c2, L2, R2, 9.0, 9.0, 2), 2, (12, 198),
                                                 bias=torch.zeros(12))
    torch.save(a.state_dict(), tmp_path / "sd.pt")
    b.load_state_dict(torch.load(tmp_path / "sd.pt"))
    for key in ("codes", "L", "R"):
        assert torch.equal(getattr(a.inner, key), getattr(b.inner, key))
    assert torch.equal(a.bias, b.bias)
    assert (b.inner.qscale, b.inner.gscale, b.in_features, b.out_features) == (a.inner.qscale, a.inner.gscale, 198, 12)


def test_dtype_casts_leave_the_stored_operands_alone():
    c, L, R, s, gs = _padded_layer()
    lin = HadamardCalderaLinear.from_decomposition(_decomposition(c, L, R, s, gs, 2), 2, (12, 198),
                                                   bias=torch.arange(12, dtype=torch.float32) / 3)
    before = {key: v.clone() for key, v in lin.state_dict().items() if torch.is_tensor(v)}
    model = torch.nn.Sequential(lin, torch.nn.Linear(12, 4))
    for cast in (lambda mod: mod.half(), lambda mod: mod.to(torch.bfloat16), lambda mod: mod.double()):
        cast(model)
        assert (lin.inner.codes.dtype, lin.inner.L.dtype, lin.inner.R.dtype, lin.bias.dtype) == \
            (torch.uint8, torch.float16, torch.float16, torch.float32)
        for key, v in lin.state_dict().items():
            if torch.is_tensor(v):
                assert torch.equal(v, before[key]), key
    assert model[1].weight.dtype == torch.float64


def test_results_file_round_trip_into_a_model(tmp_path):
    c, L, R, s, gs = _padded_layer(bits=4)
    direct = HadamardCalderaLinear.from_decomposition(_decomposition(c, L, R, s, gs, 4), 4, (12, 198))
    c0, L0, R0, _, _ = _padded_layer(m=16, n=256, seed=2)      # a plain packed layer beside it
    plain = CalderaLinear.from_decomposition(_decomposition(c0, L0, R0, s, gs, 2), 2)
    path = str(tmp_path / "res.cqrs")
    save_results(path, [direct.to_result("proj"), plain.to_result("other")])
    model = torch.nn.Module()
    model.proj = torch.nn.Linear(198, 12, bias=True)
    model.other = torch.nn.Linear(256, 16, bias=False)
    assert M.apply_packed_results(model, load_results(path)) == ["proj", "other"]
    assert isinstance(model.proj, HadamardCalderaLinear) and type(model.other) is CalderaLinear
    assert torch.equal(model.proj.inner.codes, direct.inner.codes) and torch.equal(model.proj.inner.L, direct.inner.L)
    assert (model.proj.in_features, model.proj.out_features) == (198, 12)
    assert model.proj.bias is not None and model.proj.bias.shape == (12,) and model.proj.inner.bias is None
    assert torch.equal(model.other.codes, plain.codes)
    # a Hadamard result is matched against the original shape, not the padded one
    wrong = torch.nn.Module()
    wrong.proj = torch.nn.Linear(256, 16)
    with pytest.raises(ValueError, match="weight"):
        M.apply_packed_results(wrong, [direct.to_result("proj")])


def test_documented_errors():
    c, L, R, s, gs = _padded_layer()
    dec = _decomposition(c, L, R, s, gs, 2)
    lin = HadamardCalderaLinear.from_decomposition(dec, 2, (12, 198))
    with pytest.raises(RuntimeError, match="HIP"):
        lin(torch.zeros(2, 198))
    with pytest.raises(ValueError, match="padded shape"):          # the decomposition is not on (12, 64)'s grid
        HadamardCalderaLinear.from_decomposition(dec, 2, (12, 64))
    with pytest.raises(ValueError, match=str(K.HADAMARD_MAX_N)):
        HadamardCalderaLinear.from_decomposition(dec, 2, (12, K.HADAMARD_MAX_N + 1))
    with pytest.raises(ValueError, match=str(K.HADAMARD_MAX_N)):
        HadamardCalderaLinear(lin.inner, K.HADAMARD_MAX_N + 1, 12)
    with pytest.raises(ValueError, match="no bias"):
        HadamardCalderaLinear(CalderaLinear.from_decomposition(dec, 2, bias=torch.zeros(16)), 198, 12)
    with pytest.raises(ValueError, match="hadamard"):
        HadamardCalderaLinear.from_result(lin.inner.to_result("x"))
    model = torch.nn.Sequential(torch.nn.Linear(198, 12))
    nothing = dict(decompose=lambda *a: [])
    with pytest.raises(ValueError, match="needs packed=True"):
        M.apply_caldera_quantization(model, None, object(), packed_hadamard=True, **nothing)
    with pytest.raises(ValueError, match="packed_hadamard"):
        M.apply_caldera_quantization(model, None, object(), packed=True, hadamard=True, **nothing)
    with pytest.raises(ValueError, match="hadamard=True"):
        M.apply_caldera_quantization(model, None, object(), packed=True, packed_hadamard=True, hadamard=True, **nothing)
    with pytest.raises(ValueError, match="scale_W"):
        M.apply_caldera_quantization(model, None, object(), packed=True, packed_hadamard=True, scale_W=True, **nothing)
    # a layer whose padded size is over the transform's maximum
    wide = torch.nn.Module()
    wide.language = torch.nn.Module()
    wide.language.q_proj = torch.nn.Linear(K.HADAMARD_MAX_N + 1, 2, bias=False, device="meta")
    sel = M.LayerSelection(layers=None, min_dim=1)
    with pytest.raises(ValueError, match=str(K.HADAMARD_MAX_N)):
        M.apply_caldera_quantization(wide, None, object(), packed=True, packed_hadamard=True, selection=sel, **nothing)
    # padding changes n under a Hessian: the hadamard branch's own error
    odd = torch.nn.Module()
    odd.language = torch.nn.Module()
    odd.language.q_proj = torch.nn.Linear(6, 4, bias=False)
    with pytest.raises(ValueError, match="padding changes n"):
        M.apply_caldera_quantization(odd, {"language.q_proj": torch.ones(6)}, object(), packed=True,
                                     packed_hadamard=True, selection=sel, **nothing)


# ---------------------------------------------------------------------------- model.py
def _cpu_caller(monkeypatch):
    def gemm(A, B, *, C=None, D=None, gamma=0.0, **kw):
        assert not kw
        out = A @ B if D is None else A @ B + gamma * D
        return out if C is None else C.copy_(out)

    monkeypatch.setattr(K, "gemm", gemm)
    monkeypatch.setattr(M, "_rel_error",
                        lambda W, out: float(torch.linalg.norm(W.float() - out) / torch.linalg.norm(W.float())))


def _run(monkeypatch, **kw):
    _cpu_caller(monkeypatch)
    m = _tiny()
    names = [n for n, _, _ in M.select_layers(m, None)[0]]
    seen = []

    def decompose(qp, Ws, H):
        seen.append(([W.clone() for W in Ws], H))
        # the second layer's decomposition is all zeros: relative error 1 > the 0.99 gate
        return [_Dec(W, 0.0 if len(seen) == 1 and i == 1 else 0.5) for i, W in enumerate(Ws)]

    rep = M.apply_caldera_quantization(m, None, M.driver_params(), decompose=decompose, device="cpu", **kw)
    return m, rep, names, seen


def _same_inputs(a, b):
    assert len(a) == len(b)
    for (Wa, Ha), (Wb, Hb) in zip(a, b):
        assert Ha is None and Hb is None and len(Wa) == len(Wb)
        for x, y in zip(Wa, Wb):
            assert x.shape == y.shape and torch.equal(x, y)


def test_decomposition_receives_the_same_inputs(monkeypatch):
    """Without packed_hadamard the decomposition sees the weights themselves, as before;
    packed_hadamard=True sends it what hadamard=True sends."""
    ref = _tiny()
    mods = dict(ref.named_modules())
    m0, rep0, names, plain = _run(monkeypatch, packed=True)
    flat = [W for Ws, _ in plain for W in Ws]
    by_shape = {}
    for n in names:
        by_shape.setdefault(tuple(mods[n].weight.shape), []).append(mods[n].weight.data)
    expect = [W for group in by_shape.values() for W in group]
    assert len(flat) == len(expect) and all(torch.equal(a, b) for a, b in zip(flat, expect))
    _, _, _, dense = _run(monkeypatch, hadamard=True, hadamard_gate=True)
    _, _, _, packed = _run(monkeypatch, packed=True, packed_hadamard=True)
    _same_inputs(dense, packed)
    assert {tuple(W.shape) for Ws, _ in packed for W in Ws} == {(512, 512), (1024, 512), (512, 1024)}


def test_packed_hadamard_keeps_gate_and_counters_and_replaces_layers(monkeypatch):
    m0, rep0, names, _ = _run(monkeypatch, hadamard=True, hadamard_gate=True)
    m1, rep1, _, _ = _run(monkeypatch, packed=True, packed_hadamard=True)
    assert [(o.name, o.shape, o.rel_error, o.applied) for o in rep0.layers] == \
        [(o.name, o.shape, o.rel_error, o.applied) for o in rep1.layers]
    for attr in ("quantized_param_count", "unquantized_language_param_count", "vision_param_count", "total_bits"):
        assert getattr(rep0, attr) == getattr(rep1, attr)
    assert sum(not o.applied for o in rep1.layers) == 1 and rep1.quantized_param_count > 0
    mods0, mods1 = dict(m0.named_modules()), dict(m1.named_modules())
    for o in rep1.layers:
        if not o.applied:
            assert isinstance(mods1[o.name], torch.nn.Linear)
            assert torch.equal(mods1[o.name].weight, mods0[o.name].weight)
            continue
        lin = mods1[o.name]
        assert isinstance(lin, HadamardCalderaLinear) and lin.inner.bits == 2
        assert (lin.out_features, lin.in_features) == o.shape
        assert lin.padded_shape == tuple(1 << (d - 1).bit_length() for d in o.shape)
        torch.testing.assert_close(lin.dense_weight(), mods0[o.name].weight.float(), rtol=1e-5, atol=1e-6)
