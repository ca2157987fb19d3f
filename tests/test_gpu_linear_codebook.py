"""The packed linear layer with an NF4 / NF2 codebook Q on the GPU (cq_linear_codebook_forward,
cq_linear_codebook_backward_input, CalderaLinear / HadamardCalderaLinear with q_format NF) against
the fp64 reference of linear_codebook_cases.py: exact cases bit for bit, random cases within the
bar, through the C entries and through the module; the uniform format through the codebook
entries; row independence, strided operands and a garbage index tail, graph capture; autograd and
an optimiser step; layers built from real NF decompositions, a whole tiny model and a results
file."""
import copy

import numpy as np
import pytest
import torch

import linear_backward_cases as BC
import linear_cases as LC
import linear_codebook_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
U24 = 2.0 ** -24


def _K():
    from ee274_convexcaldera_llm_quantization_amd import _lib as K
    K.load()
    return K


def _t(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def _factors(case):
    """(L, R, L_codes, R_codes) device operands of the entries."""
    out = {}
    for which in ("l", "rho"):
        op = CC.factor_operand(case, which)
        out[which] = (_t(op[1]), None) if op[0] == "fp16" else (None, (_t(op[1]), float(op[2]), op[3]))
    if not case.r:
        return None, None, None, None
    return out["l"][0], out["rho"][0], out["l"][1], out["rho"][1]


def _in_nan_buffer(a_np):
    """a at ld = K inside a NaN-filled buffer."""
    T, n = a_np.shape
    buf = torch.full((T * n + 24,), NAN, dtype=torch.float16, device=DEV)
    a = buf[8:8 + T * n].view(T, n)
    a.copy_(torch.from_numpy(a_np))
    return a


def _entry(case, odtype=torch.float32, a=None, codes=None, L=None, R=None):
    """The case through its C entry, the output written into the middle of a NaN-filled buffer that
    must stay NaN.  a / codes / L / R: operands to use instead of the case's."""
    K = _K()
    d = CC.inputs(case)
    L0, R0, Lc, Rc = _factors(case)
    L, R = (L0 if L is None else L), (R0 if R is None else R)
    codes = _t(CC.index_codes(d["idx"], case.bits)) if codes is None else codes
    a = _in_nan_buffer(d["a"]) if a is None else a
    T = a.shape[0]
    cols = case.m if case.dirn == "fwd" else case.n
    obuf = torch.full((T + 2, cols + 5), NAN, dtype=odtype, device=DEV)
    o = obuf[1:T + 1, 2:cols + 2]
    kw = dict(m=case.m, n=case.n, bits=case.bits, q_format=K.QFMT_NF, r=case.r, L_codes=Lc, R_codes=Rc)
    if case.dirn == "fwd":
        K.linear_codebook_forward(a, codes, d["s"], d["gs"], L, R, _t(d["bias"]), o, **kw)
    else:
        K.linear_codebook_backward_input(a, codes, d["s"], d["gs"], L, R, o, **kw)
    out = o.clone()
    obuf[1:T + 1, 2:cols + 2] = NAN
    assert torch.isnan(obuf).all(), "the entry wrote outside its output"
    return out.cpu()


def _module(case, trainable=False):
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear, Q_FORMAT_NF
    d = CC.inputs(case)
    f = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    spec = {}
    for which, key in (("l", "L"), ("rho", "R")):
        bits = case.lb if which == "l" else case.rb
        spec[key] = None if bits == 16 or not case.r else (f(d[which]), float(d["sl" if which == "l" else "sr"]), bits)
    lin = CalderaLinear.from_codes(f(d["idx"]), None if spec["L"] or not case.r else f(d["l"]),
                                   None if spec["R"] or not case.r else f(d["rho"]), f(d["bias"]),
                                   qscale=float(d["s"]), gscale=float(d["gs"]), bits=case.bits, L_codes=spec["L"],
                                   R_codes=spec["R"], q_format=Q_FORMAT_NF).to(DEV)
    if trainable:
        lin.enable_factor_training()
    return lin


def _through_module(case, dtype):
    """The case's output through CalderaLinear: forward, or x.grad for the case's dy."""
    lin = _module(case)
    a = _t(CC.inputs(case)["a"]).to(dtype)
    if case.dirn == "fwd":
        with torch.no_grad():
            return lin(a.view(1, case.T, case.n))[0].cpu()
    x = torch.zeros((case.T, case.n), dtype=dtype, device=DEV, requires_grad=True)
    lin(x).backward(a)
    return x.grad.cpu()


def _report(case, y, ref, bar=None):
    if bar is None:
        print(f"{case.id}: mismatches {(y != ref).sum()} of {ref.size}")
    else:
        print(f"{case.id}: worst {np.nanmax(np.abs(y - ref) / bar):.4f} bars")


# ---------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("case", CC.EXACT, ids=lambda c: c.id)
def test_exact_cases_bit_for_bit(case):
    ref, _ = CC.reference(case)
    y = _entry(case).numpy()
    _report(case, y, ref)
    assert y.dtype == np.float32 and np.array_equal(y.astype(np.float64), ref)
    ym = _through_module(case, torch.float32)
    assert ym.dtype == torch.float32 and np.array_equal(ym.numpy(), y)


@pytest.mark.parametrize("case", CC.EXACT16, ids=lambda c: c.id)
def test_fp16_output_is_the_exact_fp32_result_rounded_once(case):
    ref, _ = CC.reference(case)
    y32, y16 = _entry(case), _entry(case, torch.float16)
    _report(case, y32.numpy(), ref)
    assert np.array_equal(y32.numpy().astype(np.float64), ref)
    assert y16.dtype == torch.float16 and np.array_equal(y16.numpy(), ref.astype(np.float16))
    ym = _through_module(case, torch.float16)
    assert ym.dtype == torch.float16 and torch.equal(ym, y16)


@pytest.mark.parametrize("case", CC.RANDOM, ids=lambda c: c.id)
def test_random_cases_within_the_bar(case):
    ref, bar = CC.reference(case)
    y = _entry(case).numpy().astype(np.float64)
    _report(case, y, ref, bar)
    assert np.isfinite(y).all() and (np.abs(y - ref) <= bar).all()
    ym = _through_module(case, torch.float32)
    assert np.array_equal(ym.numpy().astype(np.float64), y)    # same kernels, same bits


# ---------------------------------------------------------------------------- CQ_QFMT_UNIFORM
@pytest.mark.parametrize("case", [c for c in LC.RANDOM if (c.m, c.T) in ((80, 16), (80, 64)) and c.bits == 4],
                         ids=lambda c: c.id)
def test_uniform_format_through_the_codebook_forward_is_the_packed_entry(case):
    K = _K()
    d = LC.inputs(case)
    codes = _t(LC.inference_codes(d["c"], case.bits))
    x, L, R = _t(d["x"]), _t(d["L"]), _t(d["R"])
    ya = torch.empty((case.T, case.m), dtype=torch.float32, device=DEV)
    yb, yc = torch.empty_like(ya), torch.empty_like(ya)
    K.linear_forward(x, codes, d["s"], d["gs"], L, R, None, ya, m=case.m, n=case.n, bits=case.bits)
    K.linear_packed_forward(x, codes, d["s"], d["gs"], L, R, None, yb, m=case.m, n=case.n, bits=case.bits)
    K.linear_codebook_forward(x, codes, d["s"], d["gs"], L, R, None, yc, m=case.m, n=case.n, bits=case.bits,
                              q_format=K.QFMT_UNIFORM)
    assert torch.equal(ya, yb) and torch.equal(yb, yc)
    ref, bar = LC.reference(case)
    assert (np.abs(yc.double().cpu().numpy() - ref) <= bar).all()


@pytest.mark.parametrize("case", [c for c in BC.RANDOM if (c.m, c.n, c.T) == (80, 898, 17)], ids=lambda c: c.id)
def test_uniform_format_through_the_codebook_backward_is_the_packed_entry(case):
    K = _K()
    d = BC.inputs(case)
    codes = _t(BC.inference_codes(d["c"], case.bits))
    dy, L, R = _t(d["dy"]), _t(d["L"]), _t(d["R"])
    da = torch.empty((case.T, case.n), dtype=torch.float32, device=DEV)
    db = torch.empty_like(da)
    ua, ub = (torch.empty((case.T, case.r), dtype=torch.float32, device=DEV) for _ in range(2))
    K.linear_packed_backward_input(dy, codes, d["s"], d["gs"], L, R, da, m=case.m, n=case.n, bits=case.bits, u_out=ua)
    K.linear_codebook_backward_input(dy, codes, d["s"], d["gs"], L, R, db, m=case.m, n=case.n, bits=case.bits,
                                     q_format=K.QFMT_UNIFORM, u_out=ub)
    assert torch.equal(da, db) and torch.equal(ua, ub)
    ref, _, bar, _ = BC.reference(case)
    assert (np.abs(db.double().cpu().numpy() - ref) <= bar).all()


# ---------------------------------------------------------------------------- contract
@pytest.mark.parametrize("case", [c for c in CC.RANDOM if (c.m, c.n) == (80, 898) and c.lb == 16
                                  and c.T in (16, 17, 64)], ids=lambda c: c.id)
def test_rows_are_independent_and_calls_repeat(case):
    a0 = CC.inputs(case)["a"]
    y0 = _entry(case)
    assert torch.equal(_entry(case), y0)
    rng = np.random.default_rng(3)
    for t in sorted({0, 5, case.T - 1}):
        for fill in ("zeros", "other", "nan"):
            a = {"zeros": np.zeros_like(a0), "other": rng.standard_normal(a0.shape).astype(np.float16),
                 "nan": np.full_like(a0, np.nan)}[fill]
            a[t] = a0[t]
            y = _entry(case, a=_in_nan_buffer(a))
            assert torch.equal(y[t], y0[t]), (t, fill)


def _in_nan(t, pad_cols, fill=NAN):
    """t (rows, cols) as a view with row stride cols + pad_cols of a buffer filled with `fill`."""
    rows, cols = t.shape
    buf = torch.full((rows + 1, cols + pad_cols), fill, dtype=t.dtype, device=DEV)
    view = buf[:rows, :cols]
    view.copy_(t)
    return view


@pytest.mark.parametrize("case", [c for c in CC.EXACT if c.lb == 16 and not c.bias
                                  and (c.dirn, c.m, c.T) in (("fwd", 48, 3), ("fwd", 48, 16), ("fwd", 80, 17),
                                                             ("bwd", 80, 17), ("bwd", 198, 17))],
                         ids=lambda c: c.id)
def test_strided_operands_and_a_garbage_index_tail(case):
    """L, R and the codes as views with a row stride (ldl = r + 3, ldr = n + 5, code_stride = row
    bytes + 16) inside NaN / 0xFF-filled buffers, the activations in a NaN-filled buffer, and random
    indices in every row's pad tail -- NF2 has no level that would be neutral there: the result is
    still the reference bit for bit."""
    d = CC.inputs(case)
    m, n, per = case.m, case.n, 8 // case.bits
    rb = CC.row_bytes(n, case.bits)
    assert rb * per > n
    full = np.random.default_rng(9).integers(0, 2 ** case.bits, (m, rb * per)).astype(np.uint8)
    assert (full[:, n:] != CC.TAIL_INDEX[case.bits]).any()
    full[:, :n] = d["idx"]
    codes = _in_nan(torch.from_numpy(CC.index_codes(full, case.bits)), 16, 0xFF)
    assert codes.shape[1] == rb
    L = _in_nan(torch.from_numpy(d["l"]), 3) if case.r else None
    R = _in_nan(torch.from_numpy(d["rho"]), 5) if case.r else None
    assert codes.stride(0) == rb + 16 and (not case.r or (L.stride(0), R.stride(0)) == (case.r + 3, n + 5))
    y = _entry(case, codes=codes, L=L, R=R)
    ref, _ = CC.reference(case)
    assert np.array_equal(y.numpy().astype(np.float64), ref)
    # and every tail fill of the plain layout gives the same bits
    for tail in range(2 ** case.bits):
        yt = _entry(case, codes=_t(CC.index_codes(d["idx"], case.bits, tail=tail)))
        assert torch.equal(yt, y), tail


@pytest.mark.parametrize("bits", [4, 2])
def test_decode_forward_in_a_captured_graph(bits):
    """The entry neither allocates nor synchronises: a captured decode forward replays to the
    bits of the eager one."""
    case = next(c for c in CC.RANDOM if (c.dirn, c.m, c.bits, c.T, c.lb) == ("fwd", 80, bits, 16, 16))
    lin = _module(case)
    x = _t(CC.inputs(case)["a"])
    xs = torch.zeros_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        lin(xs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        ys = lin(xs)
    xs.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(ys, lin(x))


# ---------------------------------------------------------------------------- autograd
_TRAIN = [c for c in CC.RANDOM if c.dirn == "bwd" and c.lb == 16 and (c.m, c.T) in ((80, 17), (160, 64))]


@pytest.mark.parametrize("case", _TRAIN, ids=lambda c: c.id)
def test_autograd_gives_the_entrys_dx_and_factor_gradients_within_their_bars(case):
    """x.grad is the codebook backward entry's dx (held against fp64 above); dL = gs dy^T (x R^T) and
    dR = gs (dy L)^T x do not involve Q and keep test_gpu_linear_backward.py's bars."""
    d = CC.inputs(case)
    lin = _module(case, trainable=True)
    dy16 = _t(d["a"])
    x16 = torch.randn(case.T, case.n, generator=torch.Generator().manual_seed(case.seed)).half().to(DEV)
    x = x16.float().requires_grad_()
    lin(x).backward(dy16.float())
    assert torch.equal(x.grad.cpu(), _entry(case))
    xd, dyd = x16.double().cpu(), dy16.double().cpu()
    L, R = (torch.from_numpy(d[key]).double().requires_grad_() for key in ("l", "rho"))
    gs = float(d["gs"])
    ((xd @ (gs * (L @ R)).t()) * dyd).sum().backward()       # the Q term has no factor gradient
    barL = (case.T + case.n + 64) * U24 * gs * (dyd.abs().t() @ (xd.abs() @ R.detach().abs().t()))
    barR = (case.T + case.m + 64) * U24 * gs * ((dyd.abs() @ L.detach().abs()).t() @ xd.abs())
    eL = ((lin.L.grad.double().cpu() - L.grad).abs() / barL).max().item()
    eR = ((lin.R.grad.double().cpu() - R.grad).abs() / barR).max().item()
    print(f"{case.id}: dL worst {eL:.4f} bars, dR worst {eR:.4f} bars")
    assert lin.L.grad.dtype == torch.float32 and eL <= 1 and eR <= 1


@pytest.mark.parametrize("bits", [4, 2])
def test_hadamard_layer_with_an_nf_inner_layer_backpropagates_through_the_three_entries(bits):
    """forward = cq_hadamard_rows, the inner codebook forward, cq_hadamard_rows; x.grad = the same
    three entries mirrored, bit for bit (each entry is held against fp64 on its own)."""
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardCalderaLinear
    K = _K()
    m, n, T = 200, 300, 17
    inner = _module(CC.Case("random", "bwd", 256, 512, 16, bits, T))      # the padded grid of a (200, 300) layer
    had = HadamardCalderaLinear(inner, n, m, bias=torch.linspace(-1, 1, m)).to(DEV)
    pr, pc = had.padded_shape
    g = torch.Generator().manual_seed(bits)
    x = torch.randn(T, n, generator=g).to(DEV).requires_grad_()
    dy = torch.randn(T, m, generator=g).to(DEV)
    y = had(x)
    y.backward(dy)
    with torch.no_grad():
        assert torch.equal(y, had(x.detach()))
    xh = torch.empty((T, pc), dtype=torch.float16, device=DEV)
    K.hadamard_rows(x.detach(), xh, n_in=n, n_out=pc, P=pc)
    y32 = torch.empty((T, pr), dtype=torch.float32, device=DEV)
    kw = dict(m=pr, n=pc, bits=bits, q_format=K.QFMT_NF, r=inner.rank)
    K.linear_codebook_forward(xh, inner.codes, inner.qscale, inner.gscale, inner.L, inner.R, None, y32, **kw)
    yy = torch.empty((T, m), dtype=torch.float32, device=DEV)
    K.hadamard_rows(y32, yy, n_in=pr, n_out=m, P=pr, bias=had.bias)
    assert torch.equal(yy, y.detach())
    dyh = torch.empty((T, pr), dtype=torch.float16, device=DEV)
    K.hadamard_rows(dy, dyh, n_in=m, n_out=pr, P=pr)
    dxh = torch.empty((T, pc), dtype=torch.float32, device=DEV)
    K.linear_codebook_backward_input(dyh, inner.codes, inner.qscale, inner.gscale, inner.L, inner.R, dxh, **kw)
    dx = torch.empty((T, n), dtype=torch.float32, device=DEV)
    K.hadamard_rows(dxh, dx, n_in=pc, n_out=n, P=pc)
    assert torch.equal(dx, x.grad)
    # against fp64 dy (H1 W~ H2)[:m, :n]: test_gpu_hadamard_backward.py's bar restated for level
    # indices -- the fp16 rounding of dy^ (2^-11), the inner entry's bar (P pr + r + 32) 2^-24 A on
    # |dy^|, and the two transforms' (log2 P + 2) 2^-24 bars, carried through H2's 1 / sqrt(pc)
    from ee274_convexcaldera_llm_quantization_amd.linear import unpack_index_bytes
    from ee274_convexcaldera_llm_quantization_amd.model import normalized_hadamard
    H1, H2 = normalized_hadamard(pr, DEV, torch.float64), normalized_hadamard(pc, DEV, torch.float64)
    dyp = torch.zeros((T, pr), dtype=torch.float64, device=DEV)
    dyp[:, :m] = dy.double()
    dyh64 = dyp @ H1
    idx = unpack_index_bytes(inner.codes, bits)[:, :pc].long()
    lev = torch.from_numpy(CC.LEVELS[bits]).to(DEV)[idx]
    sd = float(np.float32(inner.qscale) / np.float32(CC.DENOM[bits]))
    L64, R64, gs = inner.L.double(), inner.R.double(), inner.gscale
    Wt = gs * (sd * lev + L64 @ R64)
    ref = ((dyh64 @ Wt) @ H2)[:, :n]
    aW = Wt.abs()
    dyh16 = dyh64.half().double().abs()
    A = gs * (sd * (dyh16 @ lev.abs()) + (dyh16 @ L64.abs()) @ R64.abs())
    dxbar = ((1 if bits == 4 else 2) * pr + inner.rank + 32) * U24 * A
    bar_in = 1.01 * (np.log2(pr) + 2) * U24 * dy.double().abs().sum(1, keepdim=True) / np.sqrt(pr)
    inner_terms = 2.0 ** -11 * (dyh64.abs() @ aW) + dxbar + bar_in * aW.sum(0)[None, :]
    bar_out = 1.01 * (np.log2(pc) + 2) * U24 * (dyh16 @ aW + dxbar).sum(1, keepdim=True) / np.sqrt(pc)
    bar = inner_terms.sum(1, keepdim=True) / np.sqrt(pc) + bar_out
    frac = ((x.grad.double() - ref).abs() / bar).max().item()
    print(f"nf{bits}: dx {frac:.4f} of the bar")
    assert torch.isfinite(x.grad).all() and frac <= 1.0


@pytest.mark.parametrize("bits", [4, 2])
def test_one_optimiser_step_on_l_and_r(bits):
    from ee274_convexcaldera_llm_quantization_amd import model as M
    case = next(c for c in CC.RANDOM if (c.dirn, c.m, c.n, c.bits, c.T, c.lb) == ("bwd", 160, 256, bits, 64, 16))
    net = torch.nn.Sequential(_module(case))
    codes0 = net[0].codes.clone()
    params = M.prepare_factor_finetuning(net)
    assert len(params) == 2
    opt = torch.optim.SGD(params, lr=1e-3)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(case.T, case.n, generator=g).to(DEV)
    target = torch.randn(case.T, case.m, generator=g).to(DEV)
    before = [p.detach().clone() for p in params]
    loss0 = ((net(x) - target) ** 2).mean()
    loss0.backward()
    opt.step()
    with torch.no_grad():
        loss1 = ((net(x) - target) ** 2).mean()
    assert all(not torch.equal(p.detach(), b) for p, b in zip(params, before))
    assert float(loss1) < float(loss0.detach()) and torch.equal(net[0].codes, codes0)
    M.finish_factor_finetuning(net)
    assert net[0].L.dtype == torch.float16 and not net[0].factors_trainable


# ---------------------------------------------------------------------------- end to end
def _bar_of(lin, x16):
    """(bar, lr_term) of an NF CalderaLinear for fp16 x (T, n), in fp64 from its buffers:
    test_gpu_linear.py::_bar_of restated for level indices, (P n + r + 32) 2^-24 A."""
    from ee274_convexcaldera_llm_quantization_amd.linear import unpack_index_bytes
    x = np.abs(x16.double().cpu().numpy())
    idx = unpack_index_bytes(lin.codes.cpu(), lin.bits)[:, :lin.in_features].numpy().astype(np.int64)
    c = np.abs(CC.LEVELS[lin.bits][idx])
    L, R = np.abs(lin.L.double().cpu().numpy()), np.abs(lin.R.double().cpu().numpy())
    sd = np.float64(np.float32(lin.qscale) / np.float32(CC.DENOM[lin.bits]))
    lr = lin.gscale * ((x @ R.T) @ L.T)
    A = lin.gscale * sd * (x @ c.T) + lr
    planes = 1 if lin.bits == 4 else 2
    return (planes * lin.in_features + lin.rank + 32) * U24 * A, lr


@pytest.mark.parametrize("method,bits", [("nf4", 4), ("nf2", 2)])
def test_layer_from_a_real_nf_decomposition(method, bits):
    """caldera() with an NF Q on a 128 x 256, r = 16 matrix: the layer from the decomposition and
    the one from engine.last_packed agree bit for bit; dense_weight() is gs (Q + fp16(L) fp16(R))
    within 4 * 2^-24 |gs Q| plus the fp32 rounding of the product L R, the sum and gs; forward stays
    within the bar plus the fp16 rounding of the stored factors (each <= 2^-11 relative)."""
    from ee274_convexcaldera_llm_quantization_amd.api import caldera_batch
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear, Q_FORMAT_NF
    from ee274_convexcaldera_llm_quantization_amd.sharding import MatrixResult
    from src.caldera.decomposition.alg import caldera
    from src.caldera.utils.dataclasses import CalderaParams
    from src.caldera.utils.quantization import QuantizerFactory
    torch.manual_seed(0)
    W = (torch.randn(128, 256) * 0.02).to(torch.float16)
    qp = CalderaParams(Q_bits=bits, L_bits=16, R_bits=16, rank=16, iters=2, update_order=["Q", "LR"], sigma_reg=1e-8,
                       quant_factory_Q=QuantizerFactory(method, 64))
    dec = caldera(qp, W.to(DEV), None, device=DEV, use_tqdm=False)
    assert dec.Q_idxs.dtype == torch.uint8 and dec.Q_scale.numel() == 1
    with pytest.raises(ValueError, match="uniform"):
        CalderaLinear.from_decomposition(dec, bits)
    a = CalderaLinear.from_decomposition(dec, bits, Q_method=method).to(DEV)
    assert a.q_format == Q_FORMAT_NF and (a.out_features, a.in_features, a.rank) == (128, 256, 16)
    # the compact form of the same run carries the indices and the scale
    decs, eng = caldera_batch(qp, [W.to(DEV)], None, device=DEV, return_engine=True, streams=1)
    lp = eng.last_packed[0]
    assert lp["Q_method"] == method and lp["codes"].numel() == 128 * 256 * bits // 8 and "n_padded" not in lp
    res = MatrixResult("w", 128, 256, 16, bits, lp["codes"], lp["Q_scale"], lp["L"], lp["R"], lp["global_scale"], {},
                       {}, Q_method=lp["Q_method"])
    b = CalderaLinear.from_result(res).to(DEV)
    c = CalderaLinear.from_decomposition(decs[0], bits, Q_method=method).to(DEV)
    assert torch.equal(b.codes, c.codes) and torch.equal(b.L, c.L) and b.qscale == c.qscale
    assert torch.equal(a.codes, c.codes) and torch.equal(a.L, c.L) and torch.equal(a.R, c.R)
    gs = float(dec.global_scale)
    Q = dec.Q.double().to(DEV)
    lr = a.L.double() @ a.R.double()
    ref = gs * (Q + lr)
    # the Q gap 4 * 2^-24 |gs Q|; the fp32 matmul L R, r roundings on |L| |R| alone (+ 1); the sum and
    # the product with gs, one rounding each on the result's terms
    absLR = a.L.double().abs() @ a.R.double().abs()
    tol = 4 * U24 * gs * Q.abs() + (a.rank + 1) * U24 * gs * absLR + 2 * U24 * gs * (Q.abs() + absLR)
    err = (a.dense_weight().double() - ref).abs()
    print(f"{method}: dense_weight worst {(err / tol.clamp_min(1e-300)).max().item():.4f} of the tolerance")
    assert (err <= tol).all()
    Wd = (gs * (Q + dec.L.double().to(DEV) @ dec.R.double().to(DEV))).cpu().numpy()
    g = torch.Generator().manual_seed(1)
    for T in (5, 40):
        x = torch.randn(T, 256, generator=g).half().to(DEV)
        with torch.no_grad():
            ya = a(x.float())
            assert torch.equal(ya, b(x.float()))
        ref = x.double().cpu().numpy() @ Wd.T
        bar, lrt = _bar_of(a, x)
        # Q itself differs from the reference's by 4 * 2^-24 relative: inside the bar's A by a factor n
        tolf = bar + 3 * 2.0 ** -11 * lrt
        e = np.abs(ya.double().cpu().numpy() - ref)
        print(f"{method} T {T}: worst {np.max(e / tolf):.4f} of the tolerance")
        assert (e <= tolf).all()


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1 = torch.nn.Linear(128, 256, bias=True)
        self.fc2 = torch.nn.Linear(256, 128, bias=False)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc1(x)))


@torch.no_grad()
@pytest.mark.parametrize("hadamard", [False, True], ids=["plain", "hadamard"])
def test_model_packed_nf4_and_results_file(tmp_path, hadamard):
    """apply_caldera_quantization(packed=True[, packed_hadamard=True]) with an nf4 factory on a
    two-layer model; engine.last_packed through save_results / load_results / apply_packed_results
    and the layers' own to_result give the output bits of the directly built layers."""
    from ee274_convexcaldera_llm_quantization_amd import model as M
    from ee274_convexcaldera_llm_quantization_amd.api import caldera_batch
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear, HadamardCalderaLinear, Q_FORMAT_NF
    from ee274_convexcaldera_llm_quantization_amd.sharding import MatrixResult, load_results, save_results
    from src.caldera.utils.quantization import QuantizerFactory
    torch.manual_seed(0)
    base = _Tiny()
    for p in base.parameters():
        torch.nn.init.normal_(p, std=0.05)
    base = base.to(DEV)
    sel = M.LayerSelection(scope="", keys=("fc",), layers=None, min_dim=8)
    qp = M.driver_params(16)
    qp.iters, qp.Q_bits, qp.quant_factory_Q = 2, 4, QuantizerFactory("nf4", 64)
    packed, fresh, fresh2 = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)
    rep = M.apply_caldera_quantization(packed, None, qp, selection=sel, device=DEV, packed=True,
                                       packed_hadamard=hadamard)
    assert [o.applied for o in rep.layers] == [True, True]
    cls = HadamardCalderaLinear if hadamard else CalderaLinear
    for lin in (packed.fc1, packed.fc2):
        assert isinstance(lin, cls) and (lin.inner if hadamard else lin).q_format == Q_FORMAT_NF
    x = torch.randn(7, 128, generator=torch.Generator().manual_seed(2)).to(DEV)
    out = packed(x)
    assert torch.isfinite(out).all()
    # against the dense weights the layers stand for: fp16 rounding of the activations dominates
    h = x
    for name in ("fc1", "fc2"):
        lin = getattr(packed, name)
        y = lin(h)
        Wd = lin.dense_weight().double()
        ref = h.half().double() @ Wd.T + (0 if lin.bias is None else lin.bias.double())
        tol = 3 * 2.0 ** -11 * (h.half().double().abs() @ Wd.abs().T)
        assert ((y.double() - ref).abs() <= tol).all(), name
        h = torch.relu(y)
    # the layers' own results through a file
    path = str(tmp_path / "layers.cqrs")
    save_results(path, [packed.fc1.to_result("fc1"), packed.fc2.to_result("fc2")])
    assert M.apply_packed_results(fresh, load_results(path)) == ["fc1", "fc2"]
    assert torch.equal(fresh(x), out)
    # engine.last_packed of the same decompositions through a file
    results = []
    for name in ("fc1", "fc2"):
        W = getattr(base, name).weight.data
        Wt, shape = M.hadamard_transform(W) if hadamard else (W, None)
        _, eng = caldera_batch(qp, [Wt], None, device=DEV, return_engine=True, streams=1, scale_W=False)
        lp = eng.last_packed[0]
        assert lp["Q_method"] == "nf4"
        extra = {"hadamard": list(shape)} if hadamard else {}
        results.append(MatrixResult(name, Wt.shape[0], Wt.shape[1], lp["L"].shape[1], 4, lp["codes"], lp["Q_scale"],
                                    lp["L"], lp["R"], lp["global_scale"], {}, extra, Q_method=lp["Q_method"]))
    path2 = str(tmp_path / "engine.cqrs")
    save_results(path2, results)
    assert [r.Q_method for r in load_results(path2)] == ["nf4", "nf4"]
    assert M.apply_packed_results(fresh2, load_results(path2)) == ["fc1", "fc2"]
    assert torch.equal(fresh2(x), out)
