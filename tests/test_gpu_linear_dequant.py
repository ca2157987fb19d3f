"""The materialise kernel and the dense-GEMM path of the packed layers on the GPU (cq_linear_dequant,
CalderaLinear.materialize / dense_prefill_tokens, HadamardCalderaLinear.materialize,
model.set_dense_prefill / unpack_packed_layers) against the fp64 reference of
linear_dequant_cases.py: exact cases bit for bit, narrow outputs as the fp32 output rounded once,
random cases within the bar, nothing written outside w, nothing depending on tails and pads, repeat
calls and graph capture; the layer's dense path against fp64 products of the reference weight with
a bar made of its named roundings.

Measured on an MI355X (the figures DESIGN 9.6 quotes): the random cases' worst error is 0.153 of the
bar, materialize() against dense_weight() 0.127 of the doubled bar, and the dense path's worst
0.248 (forward) / 0.330 (x.grad) of its bar."""
import copy

import numpy as np
import pytest
import torch

import linear_codebook_cases as CC
import linear_dequant_cases as DC
from weight_stride_cases import pack_codes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
U24, U11 = 2.0 ** -24, 2.0 ** -11
DTYPES = {torch.float32: np.float32, torch.float16: np.float16}


def _K():
    from ee274_convexcaldera_llm_quantization_amd import _lib as K
    K.load()
    return K


def _t(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def _operands(case):
    """dict(codes, L, R, L_codes, R_codes) device operands of the entry."""
    out = dict(codes=_t(DC.q_operand(case)), L=None, R=None, L_codes=None, R_codes=None)
    if case.r:
        for which, key in (("l", "L"), ("rho", "R")):
            op = DC.factor_operand(case, which)
            if op[0] == "fp16":
                out[key] = _t(op[1])
            else:
                out[key + "_codes"] = (_t(op[1]), float(op[2]), op[3])
    return out


def _entry(case, dtype=torch.float32, **over):
    """The case through cq_linear_dequant, w at ldw = n + 5 in the middle of a NaN-filled buffer: the
    pad must stay NaN and no NaN may appear inside.  over: operands to use instead of the case's."""
    K = _K()
    d = DC.inputs(case)
    ops = _operands(case)
    ops.update(over)
    buf = torch.full((case.m + 2, case.n + 5), NAN, dtype=dtype, device=DEV)
    w = buf[1:case.m + 1, 2:case.n + 2]
    K.linear_dequant(ops["codes"], d["s"], d["gs"], ops["L"], ops["R"], w, m=case.m, n=case.n, bits=case.bits,
                     q_format=case.fmt, r=case.r, L_codes=ops["L_codes"], R_codes=ops["R_codes"])
    out = w.clone()
    assert not torch.isnan(out).any(), "NaN inside w"
    buf[1:case.m + 1, 2:case.n + 2] = NAN
    assert torch.isnan(buf).all(), "the entry wrote outside w"
    return out.cpu()


def _module(case, bias=None):
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
    d = DC.inputs(case)
    f = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    spec = {}
    for which, key in (("l", "L"), ("rho", "R")):
        bits = case.lb if which == "l" else case.rb
        spec[key] = None if bits == 16 or not case.r else (f(d[which]), float(d["sl" if which == "l" else "sr"]), bits)
    return CalderaLinear.from_codes(f(d["q"]), None if spec["L"] or not case.r else f(d["l"]),
                                    None if spec["R"] or not case.r else f(d["rho"]), bias, qscale=float(d["s"]),
                                    gscale=float(d["gs"]), bits=case.bits, L_codes=spec["L"], R_codes=spec["R"],
                                    q_format=case.fmt).to(DEV)


def _frac(err, bar):
    """The largest err / bar; 0 / 0 (a zero weight with a zero bar) counts as 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(err == 0, 0.0, err / bar)
    return float(f.max())


# ---------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("case", DC.EXACT, ids=lambda c: c.id)
def test_exact_cases_bit_for_bit(case):
    ref, _ = DC.reference(case)
    w = _entry(case).numpy()
    print(f"{case.id}: mismatches {(w != ref).sum()} of {ref.size}")
    assert w.dtype == np.float32 and np.array_equal(w.astype(np.float64), ref)


@pytest.mark.parametrize("case", DC.ALL, ids=lambda c: c.id)
def test_narrow_outputs_are_the_fp32_output_rounded_once(case):
    w32 = _entry(case)
    for dt in (torch.float16, torch.bfloat16):
        w = _entry(case, dt)
        assert w.dtype == dt and torch.equal(w, w32.to(dt)), dt


@pytest.mark.parametrize("case", DC.RANDOM, ids=lambda c: c.id)
def test_random_cases_within_the_bar(case):
    ref, bar = DC.reference(case)
    w = _entry(case).numpy().astype(np.float64)
    err = np.abs(w - ref)
    print(f"{case.id}: worst {_frac(err, bar):.4f} bars")
    assert np.isfinite(w).all() and (err <= bar).all()


def _garbage_codes(case, rng):
    """The Q codes with random fields in every row's tail."""
    q = DC.inputs(case)["q"]
    per = 8 // case.bits
    width = DC.row_bytes(case.n, case.bits) * per
    if case.fmt == DC.NF:
        full = rng.integers(0, 2 ** case.bits, (case.m, width)).astype(np.uint8)
        full[:, :case.n] = q
        return CC.index_codes(full, case.bits)
    return _garbage_uniform(q, case.bits, rng)


def _garbage_uniform(c, bits, rng, extra_rows=0):
    """(rows, cols) uniform codes in the inference layout with random fields (every bit pattern) in the
    rows' tails and `extra_rows` rows of random bytes after the last one."""
    rows, cols = c.shape
    k, per = 2 ** (bits - 1) - 1, 8 // bits
    width = DC.row_bytes(cols, bits) * per
    full = rng.integers(-k, k + 2, (rows + extra_rows, width)).astype(np.int8)
    full[:rows, :cols] = c
    return pack_codes(full, bits).reshape(rows + extra_rows, width // per)


@pytest.mark.parametrize("case", [c for c in DC.ALL if c.m in (12, 48, 130)], ids=lambda c: c.id)
def test_tails_pads_and_bytes_after_the_last_row_change_nothing(case):
    """Random fields in the Q code rows' tails, in the L codes' pad columns (q >= r), in the R code
    rows' tails and random bytes after the last R-code row, against the clean operands."""
    rng = np.random.default_rng(case.seed + 5)
    d = DC.inputs(case)
    clean = _entry(case)
    over = dict(codes=_t(_garbage_codes(case, rng)))
    assert not torch.equal(over["codes"], _t(DC.q_operand(case)))
    if case.r and case.lb != 16:
        over["L_codes"] = (_t(_garbage_uniform(d["l"], case.lb, rng)), float(d["sl"]), case.lb)
    if case.r and case.rb != 16:
        full = _t(_garbage_uniform(d["rho"], case.rb, rng, extra_rows=3))
        over["R_codes"] = (full[:case.r], float(d["sr"]), case.rb)
    assert torch.equal(_entry(case, **over), clean)
    if case.r and case.rb == 16:          # an fp16 R followed by NaN rows and with a NaN pad inside ldr
        buf = torch.full((case.r + 2, case.n + 3), NAN, dtype=torch.float16, device=DEV)
        buf[:case.r, :case.n] = _t(d["rho"])
        assert torch.equal(_entry(case, R=buf[:case.r, :case.n]), clean)
    if case.r and case.lb == 16:
        buf = torch.full((case.m + 2, case.r + 3), NAN, dtype=torch.float16, device=DEV)
        buf[:case.m, :case.r] = _t(d["l"])
        assert torch.equal(_entry(case, L=buf[:case.m, :case.r]), clean)


@pytest.mark.parametrize("case", [c for c in DC.RANDOM if (c.m, c.lb, c.rb) in ((130, 16, 16), (130, 4, 4))],
                         ids=lambda c: c.id)
def test_second_call_and_captured_graph_give_the_same_bits(case):
    K = _K()
    d = DC.inputs(case)
    ops = _operands(case)
    kw = dict(m=case.m, n=case.n, bits=case.bits, q_format=case.fmt, r=case.r, L_codes=ops["L_codes"],
              R_codes=ops["R_codes"])
    first = _entry(case, torch.float16)
    assert torch.equal(_entry(case, torch.float16), first)
    w = torch.zeros((case.m, case.n), dtype=torch.float16, device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        K.linear_dequant(ops["codes"], d["s"], d["gs"], ops["L"], ops["R"], w, **kw)       # warm-up
    torch.cuda.current_stream().wait_stream(stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.linear_dequant(ops["codes"], d["s"], d["gs"], ops["L"], ops["R"], w, **kw)
    for _ in range(2):
        w.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(w.cpu(), first)


@pytest.mark.parametrize("case", DC.RANDOM, ids=lambda c: c.id)
def test_materialize_against_dense_weight(case):
    """torch fp32 ops against the kernel: each within the bar of the fp64 reference, so the doubled
    bar between them; the narrow types are the kernel's fp32 rounded once, `out` may be strided."""
    _, bar = DC.reference(case)
    lin = _module(case)
    w32 = lin.materialize(torch.float32)
    err = (w32.double() - lin.dense_weight().double()).abs().cpu().numpy()
    print(f"{case.id}: worst {_frac(err, 2 * bar):.4f} doubled bars")
    assert tuple(w32.shape) == (case.m, case.n) and (err <= 2 * bar).all()
    assert torch.equal(w32.cpu(), _entry(case))
    assert lin.materialize().dtype == torch.float16 and torch.equal(lin.materialize(), w32.to(torch.float16))
    buf = torch.full((case.m, case.n + 3), NAN, dtype=torch.bfloat16, device=DEV)
    out = lin.materialize(out=buf[:, 1:case.n + 1])
    assert out.data_ptr() == buf[:, 1:].data_ptr() and torch.equal(out, w32.to(torch.bfloat16))
    assert torch.isnan(buf[:, 0]).all() and torch.isnan(buf[:, case.n + 1:]).all()


def test_materialize_uses_the_rounded_masters_while_training():
    case = next(c for c in DC.RANDOM if (c.m, c.fmt, c.bits, c.lb, c.rb) == (48, DC.UNIFORM, 4, 16, 16))
    lin = _module(case)
    lin.enable_factor_training()
    with torch.no_grad():
        lin.L.add_(1e-3 * torch.randn_like(lin.L))
    got = lin.materialize(torch.float32)
    frozen = copy.deepcopy(lin).freeze_factors()
    assert torch.equal(got, frozen.materialize(torch.float32))
    assert not torch.equal(got.cpu(), _entry(case))


# ---------------------------------------------------------------------------- the layer's dense path
LAYER_CASES = [c for c in DC.RANDOM if (c.m, c.n, c.r) == (160, 256, 128)
               and (c.fmt, c.bits, c.lb, c.rb) in ((DC.UNIFORM, 2, 16, 16), (DC.UNIFORM, 4, 4, 4), (DC.NF, 4, 16, 2),
                                                   (DC.NF, 2, 2, 16))]


def _x(case, T, cols, seed=0):
    rng = np.random.default_rng(case.seed + 31 * T + seed)
    return rng.standard_normal((T, cols)).astype(np.float16)


def _product_bar(a64, W64, out64, K, fp16_out):
    """The dense path's named roundings against the fp64 product a W: each weight to fp16
    (2^-11 sum |a| |W|), the GEMM's fp32 sum over K terms (K 2^-24 sum |a| |W|), and the output to
    fp16 where it is fp16 (2^-11 |out|)."""
    S = np.abs(a64) @ np.abs(W64)
    return (U11 + K * U24) * S + (U11 * np.abs(out64) if fp16_out else 0.0)


@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: c.id)
def test_below_the_threshold_nothing_changes(case):
    lin, ref = _module(case), _module(case)
    lin.dense_prefill_tokens = 17
    for dt in (torch.float16, torch.float32):
        x = _t(_x(case, 16, case.n)).to(dt)
        with torch.no_grad():
            assert torch.equal(lin(x), ref(x))
        xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
        dy = _t(_x(case, 16, case.m, 1)).to(dt)
        lin(xa).backward(dy)
        ref(xb).backward(dy)
        assert torch.equal(xa.grad, xb.grad)


@pytest.mark.parametrize("T", [17, 64])
@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: c.id)
def test_dense_forward_and_x_grad_against_fp64(case, T):
    W64, _ = DC.reference(case)          # from the codes, never from the kernel's output
    lin, unset = _module(case), _module(case)
    lin.dense_prefill_tokens = 17
    x16, dy16 = _x(case, T, case.n), _x(case, T, case.m, 1)
    y64, dx64 = x16.astype(np.float64) @ W64.T, dy16.astype(np.float64) @ W64
    for dt in (torch.float16, torch.float32):
        half = dt == torch.float16
        x = _t(x16).to(dt).requires_grad_()
        y = lin(x)
        assert y.dtype == dt and tuple(y.shape) == (T, case.m)
        with torch.no_grad():
            assert torch.equal(lin(x.detach()), y)              # the inference launch: the same path
            assert not torch.equal(unset(x.detach()), y)        # and not the packed kernels
        y.backward(_t(dy16).to(dt))
        ey = np.abs(y.detach().double().cpu().numpy() - y64)
        ex = np.abs(x.grad.double().cpu().numpy() - dx64)
        fy = _frac(ey, _product_bar(x16.astype(np.float64), W64.T, y64, case.n, half))
        fx = _frac(ex, _product_bar(dy16.astype(np.float64), W64, dx64, case.m, half))
        print(f"{case.id} T={T} {dt}: y worst {fy:.4f} bars, x.grad worst {fx:.4f} bars")
        assert x.grad.dtype == dt and fy <= 1 and fx <= 1


def test_dense_path_adds_the_bias_in_fp32():
    case = LAYER_CASES[0]
    rng = np.random.default_rng(5)
    bias = torch.from_numpy(rng.standard_normal(case.m).astype(np.float32))
    lin = _module(case, bias)
    lin.dense_prefill_tokens = 17
    x16 = _x(case, 17, case.n)
    W16 = lin.materialize().float().cpu().numpy().astype(np.float64)
    y64 = x16.astype(np.float64) @ W16.T
    with torch.no_grad():
        y32, y16 = lin(_t(x16).float()), lin(_t(x16))
    # from the kernel's own fp16 weight: the fp32 sum, the fp32 bias addition, fp16 y rounded once
    bar = (case.n + 2) * U24 * (np.abs(x16.astype(np.float64)) @ np.abs(W16.T) + np.abs(bias.numpy()))
    assert (np.abs(y32.double().cpu().numpy() - (y64 + bias.numpy())) <= bar).all()
    assert torch.equal(y16, y32.to(torch.float16))


@pytest.mark.parametrize("T", [17, 64])
def test_factor_gradients_equal_the_unset_layers_within_their_bars(T):
    """dL and dR of the dense path (u = dy L by torch) and of the packed backward (u from the kernel),
    each against fp64 within test_gpu_linear_backward.py's bars, and so within a bar of each other."""
    case = LAYER_CASES[0]
    d = DC.inputs(case)
    x16, dy16 = _x(case, T, case.n), _x(case, T, case.m, 1)
    gs = float(d["gs"])
    ax, ady = np.abs(x16.astype(np.float64)), np.abs(dy16.astype(np.float64))
    L64, R64 = d["l"].astype(np.float64), d["rho"].astype(np.float64)
    dL64 = gs * dy16.astype(np.float64).T @ (x16.astype(np.float64) @ R64.T)
    dR64 = gs * (dy16.astype(np.float64) @ L64).T @ x16.astype(np.float64)
    barL = (T + case.n + 64) * U24 * gs * (ady.T @ (ax @ np.abs(R64).T))
    barR = (T + case.m + 64) * U24 * gs * ((ady @ np.abs(L64)).T @ ax)
    grads = []
    for tokens in (17, None):
        lin = _module(case)
        lin.enable_factor_training()
        lin.dense_prefill_tokens = tokens
        x = _t(x16).requires_grad_()
        lin(x).backward(_t(dy16))
        gL, gR = lin.L.grad.double().cpu().numpy(), lin.R.grad.double().cpu().numpy()
        print(f"T={T} dense_prefill_tokens={tokens}: dL worst {_frac(np.abs(gL - dL64), barL):.4f} bars, "
              f"dR worst {_frac(np.abs(gR - dR64), barR):.4f} bars")
        assert (np.abs(gL - dL64) <= barL).all() and (np.abs(gR - dR64) <= barR).all()
        grads.append((gL, gR))
    assert (np.abs(grads[0][0] - grads[1][0]) <= barL).all() and (np.abs(grads[0][1] - grads[1][1]) <= barR).all()


def _hadamard_layer(seed=3):
    """A 100 x 198 layer in the Hadamard basis: inner 128 x 256, 4-bit codes, r = 16."""
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear, HadamardCalderaLinear
    rng = np.random.default_rng(seed)
    c = torch.from_numpy(rng.integers(-7, 8, (128, 256)).astype(np.int8))
    L = torch.from_numpy((0.15 * rng.standard_normal((128, 16))).astype(np.float16))
    R = torch.from_numpy((0.15 * rng.standard_normal((16, 256))).astype(np.float16))
    inner = CalderaLinear.from_codes(c, L, R, None, qscale=0.05, gscale=1.7, bits=4)
    bias = torch.from_numpy(rng.standard_normal(100).astype(np.float32))
    A = 1.7 * (np.float32(0.05) / np.float32(7) * np.abs(c.numpy()) + np.abs(L.numpy().astype(np.float64))
               @ np.abs(R.numpy().astype(np.float64)))
    return HadamardCalderaLinear(inner, 198, 100, bias).to(DEV), float(np.linalg.norm(A))


def test_hadamard_layer_dense_path_and_materialize():
    """Against the layer's dense_weight() product, with the two transforms of dense_weight() redone in
    fp64 (H1 inner.dense_weight() H2) so that the reference's own error is the inner torch-ops
    weight's alone.  H is orthogonal, so the bars are norm bars: an entrywise error of eps sum |x^| |W~|
    in the inner product is at most eps ||x|| ||W~||_F after the output transform (Cauchy-Schwarz)."""
    from ee274_convexcaldera_llm_quantization_amd.model import normalized_hadamard
    (had, Anorm), (unset, _) = _hadamard_layer(), _hadamard_layer()
    had.dense_prefill_tokens = 17
    assert had.inner.dense_prefill_tokens == 17 and unset.dense_prefill_tokens is None
    Wt = had.inner.dense_weight().double()
    W = (normalized_hadamard(128, DEV, torch.float64) @ Wt @ normalized_hadamard(256, DEV, torch.float64))
    W = W[:100, :198].cpu().numpy()
    assert np.abs(W - had.dense_weight().double().cpu().numpy()).max() <= 400 * U24 * Anorm
    x16 = np.random.default_rng(9).standard_normal((17, 198)).astype(np.float16)
    y64 = x16.astype(np.float64) @ W.T + had.bias.double().cpu().numpy()
    with torch.no_grad():
        y, y0 = had(_t(x16).float()), unset(_t(x16).float())
    assert not torch.equal(y, y0)
    # x^ to fp16 and W~ to fp16 (2^-11 each), the GEMM's 256 fp32 terms, and 64 for the fp32
    # transforms (10 + 9 roundings), the bias addition and the inner reference's r + 8 = 24
    xn = np.linalg.norm(x16.astype(np.float64), axis=1, keepdims=True)
    bar = np.broadcast_to((2 * U11 + (256 + 64) * U24) * xn * Anorm + U24 * np.abs(y64), y64.shape)
    err = np.abs(y.double().cpu().numpy() - y64)
    print(f"hadamard dense path: worst {_frac(err, bar):.4f} bars, "
          f"unset layer {_frac(np.abs(y0.double().cpu().numpy() - y64), bar):.4f}")
    assert (err <= bar).all()
    # materialize: kernels alone.  Two weights within (r + 8) 2^-24 A of the truth, and two fp32
    # transforms of 8 + 1 and 7 + 1 roundings
    Wm = had.materialize(torch.float32)
    assert tuple(Wm.shape) == (100, 198) and Wm.is_contiguous()
    wbar = (2 * (16 + 8) + 17) * U24 * Anorm
    werr = np.abs(Wm.double().cpu().numpy() - W)
    print(f"hadamard materialize: worst {werr.max() / wbar:.4f} bars")
    assert (werr <= wbar).all()
    assert torch.equal(had.materialize(), Wm.to(torch.float16))
    out = torch.empty((100, 198), dtype=torch.bfloat16, device=DEV)
    assert torch.equal(had.materialize(out=out), Wm.to(torch.bfloat16))


def test_unpack_packed_layers_gives_plain_linears():
    from ee274_convexcaldera_llm_quantization_amd import model as M
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
    a, b = LAYER_CASES[1], LAYER_CASES[2]          # the layers are used one by one: a container, not a chain
    bias = torch.from_numpy(np.random.default_rng(2).standard_normal(b.m).astype(np.float32))
    net = torch.nn.ModuleDict({"first": _module(a), "second": _module(b, bias), "had": _hadamard_layer()[0]})
    packed = copy.deepcopy(net)
    assert M.set_dense_prefill(net, 32) == ["first", "second", "had"]
    assert all(isinstance(mod, CalderaLinear) and mod.dense_prefill_tokens == 32
               for mod in (net["first"], net["second"], net["had"].inner))
    assert M.set_dense_prefill(net, None) == ["first", "second", "had"] and net["first"].dense_prefill_tokens is None
    assert M.unpack_packed_layers(net) == ["first", "second", "had"]
    for name in ("first", "second", "had"):
        lin = net[name]
        assert type(lin) is torch.nn.Linear and lin.weight.dtype == torch.float16
        assert torch.equal(lin.weight.detach(), packed[name].materialize())
        assert (lin.bias is None) == (packed[name].bias is None)
    assert torch.equal(net["second"].bias.detach(), bias.to(DEV).to(torch.float16))
    assert not any(isinstance(mod, CalderaLinear) for mod in net.modules())
    # the plain layer's forward: the dense path's roundings against the fp64 product
    W64, _ = DC.reference(a)
    x16 = _x(a, 17, a.n)
    y64 = x16.astype(np.float64) @ W64.T
    with torch.no_grad():
        y = net["first"](_t(x16))
    assert _frac(np.abs(y.double().cpu().numpy() - y64), _product_bar(x16.astype(np.float64), W64.T, y64, a.n, True)) <= 1
    net32 = copy.deepcopy(packed)
    M.unpack_packed_layers(net32, torch.float32)
    assert torch.equal(net32["first"].weight.detach(), packed["first"].materialize(torch.float32))


def test_dense_path_forward_in_a_captured_graph():
    case = LAYER_CASES[1]
    lin = _module(case)
    lin.dense_prefill_tokens = 17
    x = _t(_x(case, 64, case.n))
    with torch.no_grad():
        want = lin(x).clone()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            lin(x)                                              # warm-up on the capture's side stream
        torch.cuda.current_stream().wait_stream(stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = lin(x)
    for _ in range(2):
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, want)
