"""The packed linear layer on the GPU (cq_linear_forward, CalderaLinear, model.py packed=True)
against the fp64 reference of linear_cases.py: exact cases bit for bit, random cases within the
worst-case fp32 bar, through the C entry and through the module; row independence and
repeatability; layers built from a real decomposition; a whole tiny model, also via a results
file; graph capture of a decode forward."""
import numpy as np
import pytest
import torch

import linear_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _K():
    from ee274_convexcaldera_llm_quantization_amd import _lib as K
    K.load()
    return K


def _operands(case):
    d = LC.inputs(case)
    t = lambda a: None if a is None else torch.from_numpy(a).to(DEV)  # noqa: E731
    codes = torch.from_numpy(LC.inference_codes(d["c"], case.bits)).to(DEV)
    L, R = (t(d["L"]), t(d["R"])) if case.r else (None, None)
    return d, codes, L, R, t(d["bias"])


def _x_in_nan_buffer(x_np):
    """x at ld = n inside a NaN-filled buffer (n = 198: rows 4-byte aligned only)."""
    T, n = x_np.shape
    buf = torch.full((T * n + 24,), NAN, dtype=torch.float16, device=DEV)
    x = buf[8:8 + T * n].view(T, n)
    x.copy_(torch.from_numpy(x_np))
    return x


def _entry(case, ydtype=torch.float32, x=None):
    """y through the C entry, written into the middle of a NaN-filled buffer that must stay NaN."""
    K = _K()
    d, codes, L, R, bias = _operands(case)
    x = _x_in_nan_buffer(d["x"]) if x is None else x
    T, m = x.shape[0], case.m
    ybuf = torch.full((T + 2, m + 5), NAN, dtype=ydtype, device=DEV)
    y = ybuf[1:T + 1, 2:m + 2]
    K.linear_forward(x, codes, d["s"], d["gs"], L, R, bias, y, m=m, n=case.n, bits=case.bits)
    out = y.clone()
    ybuf[1:T + 1, 2:m + 2] = NAN
    assert torch.isnan(ybuf).all(), "cq_linear_forward wrote outside y"
    return out.cpu()


def _module(case):
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
    d = LC.inputs(case)
    f = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    lin = CalderaLinear.from_codes(torch.from_numpy(d["c"]), f(d["L"]), f(d["R"]), f(d["bias"]),
                                   qscale=float(d["s"]), gscale=float(d["gs"]), bits=case.bits)
    return lin.to(DEV)


def _report(case, y, ref, bar=None):
    if bar is None:
        print(f"{case.id}: mismatches {(y != ref).sum()} of {ref.size}")
    else:
        print(f"{case.id}: worst {np.nanmax(np.abs(y - ref) / bar):.4f} bars")


@pytest.mark.parametrize("case", LC.EXACT, ids=lambda c: c.id)
def test_exact_cases_bit_for_bit(case):
    ref, _ = LC.reference(case)
    y = _entry(case).numpy()
    _report(case, y, ref)
    assert y.dtype == np.float32 and np.array_equal(y.astype(np.float64), ref)
    x = torch.from_numpy(LC.inputs(case)["x"]).to(DEV)
    ym = _module(case)(x.float().view(1, case.T, case.n))        # fp32 in -> fp32 out, leading dims kept
    assert ym.dtype == torch.float32 and ym.shape == (1, case.T, case.m)
    assert np.array_equal(ym[0].cpu().numpy(), y)


@pytest.mark.parametrize("case", LC.EXACT16, ids=lambda c: c.id)
def test_fp16_output_is_the_fp32_result_rounded_once(case):
    ref, _ = LC.reference(case)
    y32 = _entry(case)
    y16 = _entry(case, torch.float16)
    _report(case, y32.numpy(), ref)
    assert np.array_equal(y32.numpy().astype(np.float64), ref)
    assert y16.dtype == torch.float16 and torch.equal(y16, y32.half())
    ym = _module(case)(torch.from_numpy(LC.inputs(case)["x"]).to(DEV))
    assert ym.dtype == torch.float16 and torch.equal(ym.cpu(), y16)


@pytest.mark.parametrize("case", LC.RANDOM, ids=lambda c: c.id)
def test_random_cases_within_the_bar(case):
    ref, bar = LC.reference(case)
    y = _entry(case).numpy().astype(np.float64)
    _report(case, y, ref, bar)
    assert np.isfinite(y).all() and (np.abs(y - ref) <= bar).all()
    ym = _module(case)(torch.from_numpy(LC.inputs(case)["x"]).to(DEV).float())
    assert np.array_equal(ym.cpu().numpy().astype(np.float64), y)    # same kernels, same bits


@pytest.mark.parametrize("case", [c for c in LC.RANDOM if (c.m, c.bits) == (80, 2)], ids=lambda c: c.id)
def test_rows_are_independent_and_calls_repeat(case):
    """T = 16 (decode) and 17, 64 (prefill): row t has the same bits whatever the other rows hold."""
    x0 = LC.inputs(case)["x"]
    y0 = _entry(case)
    assert torch.equal(_entry(case), y0)
    rng = np.random.default_rng(3)
    for t in sorted({0, 5, case.T - 1}):
        for fill in ("zeros", "other", "nan"):
            x = {"zeros": np.zeros_like(x0), "other": rng.standard_normal(x0.shape).astype(np.float16),
                 "nan": np.full_like(x0, np.nan)}[fill]
            x[t] = x0[t]
            y = _entry(case, x=_x_in_nan_buffer(x))
            assert torch.equal(y[t], y0[t]), (t, fill)


def _in_nan(t, pad_cols, fill=NAN):
    """t (rows, cols) as a view with row stride cols + pad_cols of a buffer filled with `fill`."""
    rows, cols = t.shape
    buf = torch.full((rows + 1, cols + pad_cols), fill, dtype=t.dtype, device=DEV)
    view = buf[:rows, :cols]
    view.copy_(t)
    return view


@pytest.mark.parametrize("case", [c for c in LC.EXACT if (c.m, c.T) in ((48, 3), (48, 16), (80, 17)) and c.r],
                         ids=lambda c: c.id)
def test_strided_operands_and_nonzero_code_tail(case):
    """L, R and the codes as views with a row stride (ldl = r + 3 and ldr = n + 5: rows not 16-byte
    aligned; code_stride = row bytes + 16) inside NaN / 0xFF-filled buffers, and random nonzero codes in
    every row's pad tail: the result is still the reference bit for bit (pad columns contribute
    nothing whatever the tail holds)."""
    K = _K()
    d = LC.inputs(case)
    m, n, k, per = case.m, case.n, case.k, 8 // case.bits
    rb = LC.row_bytes(n, case.bits)
    assert rb * per > n
    full = np.random.default_rng(9).integers(-k, k + 1, (m, rb * per)).astype(np.int8)
    assert (full[:, n:] != 0).any()
    full[:, :n] = d["c"]
    codes = _in_nan(torch.from_numpy(LC.pack_codes(full, case.bits).reshape(m, rb)), 16, 0xFF)
    L = _in_nan(torch.from_numpy(d["L"]), 3)
    R = _in_nan(torch.from_numpy(d["R"]), 5)
    assert (codes.stride(0), L.stride(0), R.stride(0)) == (rb + 16, case.r + 3, n + 5)
    x = _x_in_nan_buffer(d["x"])
    y = torch.full((case.T, m), NAN, dtype=torch.float32, device=DEV)
    K.linear_forward(x, codes, d["s"], d["gs"], L, R, None, y, m=m, n=n, bits=case.bits)
    ref, _ = LC.reference(case)
    assert np.array_equal(y.cpu().numpy().astype(np.float64), ref)


def test_module_survives_dtype_casts_of_the_model():
    """model.half() / .to(bfloat16) after quantising: the layer keeps its operand types and the
    forward follows x's dtype."""
    case = next(c for c in LC.EXACT16 if (c.bits, c.T) == (2, 5))
    ref, _ = LC.reference(case)
    lin = _module(case)
    x = torch.from_numpy(LC.inputs(case)["x"]).to(DEV)
    for cast, dt in ((lambda mod: mod.half(), torch.float16), (lambda mod: mod.to(torch.bfloat16), torch.bfloat16)):
        cast(lin)
        y = lin(x.to(dt))          # x in {-1, 0, 1} is exact in bf16; y is the exact fp32 result rounded once
        assert y.dtype == dt and torch.equal(y.cpu(), torch.from_numpy(ref).to(dt))
    assert torch.equal(lin(x).double().cpu(), torch.from_numpy(ref))


def _bar_of(lin, x16):
    """(bar, lr_term) of a CalderaLinear for fp16 x (T, n), in fp64 from its buffers."""
    from ee274_convexcaldera_llm_quantization_amd.linear import unpack_bytes
    k = 2 ** (lin.bits - 1) - 1
    x = np.abs(x16.double().cpu().numpy())
    c = np.abs(unpack_bytes(lin.codes.cpu(), lin.bits)[:, :lin.in_features].numpy().astype(np.float64))
    L, R = np.abs(lin.L.double().cpu().numpy()), np.abs(lin.R.double().cpu().numpy())
    sk = np.float64(np.float32(lin.qscale) / np.float32(k))
    lr = lin.gscale * ((x @ R.T) @ L.T)
    A = lin.gscale * sk * (x @ c.T) + lr
    return (lin.in_features + lin.rank + 32) * 2.0 ** -24 * A, lr


@pytest.mark.parametrize("bits", [2, 4])
def test_layer_from_a_real_decomposition(bits):
    """The smoke shape (256 x 512 fp16, rank 16): the layer built from engine.last_packed and the
    one built from the returned decomposition agree bit for bit and match x (gs (Q + L R))^T in
    fp64 within the bar plus the fp16 rounding of the stored factors (each <= 2^-11 relative)."""
    from ee274_convexcaldera_llm_quantization_amd.api import caldera_batch
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
    from ee274_convexcaldera_llm_quantization_amd.sharding import MatrixResult
    from src.caldera.utils.dataclasses import CalderaParams
    torch.manual_seed(0)
    W = (torch.randn(256, 512) * 0.02).to(torch.float16)
    qp = CalderaParams(Q_bits=bits, L_bits=16, R_bits=16, rank=16, iters=2, update_order=["Q", "LR"], sigma_reg=1e-8)
    decs, eng = caldera_batch(qp, [W.to(DEV)], None, device=DEV, return_engine=True, streams=1)
    dec, lp = decs[0], eng.last_packed[0]
    extra = {"n_padded": lp["n_padded"]} if "n_padded" in lp else {}
    res = MatrixResult("w", 256, 512, lp["L"].shape[1], bits, lp["codes"], lp["Q_scale"], lp["L"], lp["R"],
                       lp["global_scale"], {}, extra)
    a = CalderaLinear.from_result(res).to(DEV)
    b = CalderaLinear.from_decomposition(dec, bits).to(DEV)
    assert torch.equal(a.codes, b.codes) and torch.equal(a.L, b.L) and torch.equal(a.R, b.R)
    Wd = float(dec.global_scale) * (dec.Q.double() + dec.L.double() @ dec.R.double()).cpu().numpy()
    g = torch.Generator().manual_seed(1)
    for T in (5, 40):
        x = torch.randn(T, 512, generator=g).half().to(DEV)
        ya, yb = a(x.float()), b(x.float())
        assert torch.equal(ya, yb)
        ref = x.double().cpu().numpy() @ Wd.T
        bar, lr = _bar_of(a, x)
        tol = bar + 3 * 2.0 ** -11 * lr
        err = np.abs(ya.double().cpu().numpy() - ref)
        print(f"bits {bits} T {T}: worst {np.max(err / tol):.4f} of the tolerance")
        assert (err <= tol).all()


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1 = torch.nn.Linear(128, 256, bias=True)
        self.fc2 = torch.nn.Linear(256, 128, bias=False)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc1(x)))


@torch.no_grad()
def test_model_packed_forward_and_results_file(tmp_path):
    import copy
    from ee274_convexcaldera_llm_quantization_amd import model as M
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
    from ee274_convexcaldera_llm_quantization_amd.sharding import load_results, save_results
    torch.manual_seed(0)
    base = _Tiny()
    for p in base.parameters():
        torch.nn.init.normal_(p, std=0.05)
    base = base.to(DEV)
    sel = M.LayerSelection(scope="", keys=("fc",), layers=None, min_dim=8)
    qp = M.driver_params(16)
    qp.iters = 2
    dense, packed, fresh = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)
    rep_d = M.apply_caldera_quantization(dense, None, qp, selection=sel, device=DEV)
    rep_p = M.apply_caldera_quantization(packed, None, qp, selection=sel, device=DEV, packed=True)
    assert [o.applied for o in rep_p.layers] == [True, True] == [o.applied for o in rep_d.layers]
    assert rep_p.quantized_param_count == rep_d.quantized_param_count == 2 * 128 * 256
    assert isinstance(packed.fc1, CalderaLinear) and isinstance(packed.fc2, CalderaLinear)
    assert isinstance(dense.fc1, torch.nn.Linear) and packed.fc1.bias is not None
    x = torch.randn(7, 128, generator=torch.Generator().manual_seed(2)).half().float().to(DEV)
    # layer by layer on the same input: packed forward vs the dense write-back in fp64
    h = x
    for name in ("fc1", "fc2"):
        lin, ref_mod = getattr(packed, name), getattr(dense, name)
        h16 = h.half()
        y = lin(h16.float())
        ref = h16.double() @ ref_mod.weight.double().T
        if ref_mod.bias is not None:
            ref = ref + ref_mod.bias.double()
        bar, lr = _bar_of(lin, h16)
        tol = bar + 3 * 2.0 ** -11 * lr
        err = (y.double() - ref).abs().cpu().numpy()
        print(f"{name}: worst {np.max(err / tol):.4f} of the tolerance")
        assert (err <= tol).all()
        h = torch.relu(y)
    out_p = packed(x)
    path = str(tmp_path / "layers.cqrs")
    save_results(path, [packed.fc1.to_result("fc1"), packed.fc2.to_result("fc2")])
    assert M.apply_packed_results(fresh, load_results(path)) == ["fc1", "fc2"]
    assert torch.equal(fresh(x), out_p)
    with pytest.raises(KeyError):
        M.apply_packed_results(fresh, [packed.fc1.to_result("nope")])


def test_decode_forward_in_a_captured_graph():
    """The entry neither allocates nor synchronises: a captured decode forward replays to the
    bits of the eager one."""
    case = next(c for c in LC.RANDOM if (c.m, c.bits, c.T) == (80, 4, 16))
    lin = _module(case)
    x = torch.from_numpy(LC.inputs(case)["x"]).to(DEV)
    xs = torch.zeros_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lin(xs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = lin(xs)
    xs.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ys, lin(x))
