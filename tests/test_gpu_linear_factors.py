"""The packed linear layer with coded factors on the GPU (cq_linear_packed_forward, CalderaLinear
with L_codes / R_codes, model.py packed_factors=True) against the fp64 reference of
linear_factor_cases.py: exact cases bit for bit, random cases within the worst-case fp32 bar,
through the C entry and through the module; row independence and repeatability; strided code
buffers with nonzero tails; fp16 factors through the new entry against cq_linear_forward;
layers built from a real decomposition; a tiny model through a results file; graph capture."""
import numpy as np
import pytest
import torch

import linear_cases as LC
import linear_factor_cases as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _K():
    from ee274_convexcaldera_llm_quantization_amd import _lib as K
    K.load()
    return K


def _factor(case, which):
    """(fp16 tensor | None, (codes, scale, bits) | None) of factor "l" / "rho" on the device."""
    op = FC.factor_operand(case, which)
    if op[0] == "fp16":
        return torch.from_numpy(op[1]).to(DEV), None
    return None, (torch.from_numpy(op[1]).to(DEV), float(op[2]), op[3])


def _x_in_nan_buffer(x_np):
    """x at ld = n inside a NaN-filled buffer (n = 198: rows 4-byte aligned only)."""
    T, n = x_np.shape
    buf = torch.full((T * n + 24,), NAN, dtype=torch.float16, device=DEV)
    x = buf[8:8 + T * n].view(T, n)
    x.copy_(torch.from_numpy(x_np))
    return x


def _entry(case, ydtype=torch.float32, x=None, operands=None):
    """y through the C entry, written into the middle of a NaN-filled buffer that must stay NaN."""
    K = _K()
    d = FC.inputs(case)
    if operands is None:
        codes = torch.from_numpy(FC.inference_codes(d["c"], case.bits)).to(DEV)
        (L, Lc), (R, Rc) = _factor(case, "l"), _factor(case, "rho")
    else:
        codes, L, Lc, R, Rc = operands
    bias = None if d["bias"] is None else torch.from_numpy(d["bias"]).to(DEV)
    x = _x_in_nan_buffer(d["x"]) if x is None else x
    T, m = x.shape[0], case.m
    ybuf = torch.full((T + 2, m + 5), NAN, dtype=ydtype, device=DEV)
    y = ybuf[1:T + 1, 2:m + 2]
    K.linear_packed_forward(x, codes, d["s"], d["gs"], L, R, bias, y, m=m, n=case.n, bits=case.bits, r=case.r,
                            L_codes=Lc, R_codes=Rc)
    out = y.clone()
    ybuf[1:T + 1, 2:m + 2] = NAN
    assert torch.isnan(ybuf).all(), "cq_linear_packed_forward wrote outside y"
    return out.cpu()


def _module(case):
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
    d = FC.inputs(case)
    f = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    lin = CalderaLinear.from_codes(
        torch.from_numpy(d["c"]), f(d["l"]) if case.lb == 16 else None, f(d["rho"]) if case.rb == 16 else None,
        f(d["bias"]), qscale=float(d["s"]), gscale=float(d["gs"]), bits=case.bits,
        L_codes=None if case.lb == 16 else (f(d["l"]), float(d["sl"]), case.lb),
        R_codes=None if case.rb == 16 else (f(d["rho"]), float(d["sr"]), case.rb))
    return lin.to(DEV)


def _report(case, y, ref, bar=None):
    if bar is None:
        print(f"{case.id}: mismatches {(y != ref).sum()} of {ref.size}")
    else:
        print(f"{case.id}: worst {np.nanmax(np.abs(y - ref) / bar):.4f} bars")


@pytest.mark.parametrize("case", FC.EXACT, ids=lambda c: c.id)
def test_exact_cases_bit_for_bit(case):
    ref, _ = FC.reference(case)
    y = _entry(case).numpy()
    _report(case, y, ref)
    assert y.dtype == np.float32 and np.array_equal(y.astype(np.float64), ref)
    x = torch.from_numpy(FC.inputs(case)["x"]).to(DEV)
    ym = _module(case)(x.float().view(1, case.T, case.n))        # fp32 in -> fp32 out, leading dims kept
    assert ym.dtype == torch.float32 and ym.shape == (1, case.T, case.m)
    assert np.array_equal(ym[0].cpu().numpy(), y)


@pytest.mark.parametrize("case", FC.EXACT16, ids=lambda c: c.id)
def test_fp16_output_is_the_fp32_result_rounded_once(case):
    ref, _ = FC.reference(case)
    y32 = _entry(case)
    y16 = _entry(case, torch.float16)
    _report(case, y32.numpy(), ref)
    assert np.array_equal(y32.numpy().astype(np.float64), ref)
    assert y16.dtype == torch.float16 and torch.equal(y16, y32.half())
    ym = _module(case)(torch.from_numpy(FC.inputs(case)["x"]).to(DEV))
    assert ym.dtype == torch.float16 and torch.equal(ym.cpu(), y16)


@pytest.mark.parametrize("case", FC.RANDOM, ids=lambda c: c.id)
def test_random_cases_within_the_bar(case):
    ref, bar = FC.reference(case)
    y = _entry(case).numpy().astype(np.float64)
    _report(case, y, ref, bar)
    assert np.isfinite(y).all() and (np.abs(y - ref) <= bar).all()
    ym = _module(case)(torch.from_numpy(FC.inputs(case)["x"]).to(DEV).float())
    assert np.array_equal(ym.cpu().numpy().astype(np.float64), y)    # same kernels, same bits


@pytest.mark.parametrize("case", [c for c in FC.RANDOM if (c.m, c.bits, c.lb, c.rb) == (80, 2, 4, 4) and c.T in (16, 17)],
                         ids=lambda c: c.id)
def test_rows_are_independent_and_calls_repeat(case):
    """T = 16 (decode) and 17 (prefill): row t has the same bits whatever the other rows hold."""
    x0 = FC.inputs(case)["x"]
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


def _strided_codes(c, bits, rng):
    """(rows, cols) codes in the inference layout with random nonzero codes in every row's pad tail,
    as a view with row stride row bytes + 16 of 0xFF-filled storage."""
    rows, cols = c.shape
    k, per = 2 ** (bits - 1) - 1, 8 // bits
    rb = LC.row_bytes(cols, bits)
    assert rb * per > cols
    full = rng.integers(-k, k + 1, (rows, rb * per)).astype(np.int8)
    assert (full[:, cols:] != 0).any()
    full[:, :cols] = c
    t = torch.from_numpy(LC.pack_codes(full, bits).reshape(rows, rb))
    buf = torch.full((rows + 1, rb + 16), 0xFF, dtype=torch.uint8, device=DEV)
    view = buf[:rows, :rb]
    view.copy_(t)
    assert view.stride(0) == rb + 16
    return view


@pytest.mark.parametrize("case", [c for c in FC.EXACT if (c.lb, c.rb) in ((4, 4), (2, 2)) and c.bits == 2
                                  and (c.m, c.r, c.T) in ((48, 40, 5), (48, 40, 64), (48, 264, 16), (80, 200, 17))],
                         ids=lambda c: c.id)
def test_strided_code_buffers_and_nonzero_tails(case):
    """Q, L and R codes as views with a row stride inside 0xFF-filled buffers, random nonzero codes in
    every row's pad tail (L: q >= r, R and Q: j >= n): still the reference bit for bit."""
    d = FC.inputs(case)
    rng = np.random.default_rng(9)
    codes = _strided_codes(d["c"], case.bits, rng)
    Lc = (_strided_codes(d["l"], case.lb, rng), float(d["sl"]), case.lb)
    Rc = (_strided_codes(d["rho"], case.rb, rng), float(d["sr"]), case.rb)
    y = _entry(case, operands=(codes, None, Lc, None, Rc)).numpy()
    ref, _ = FC.reference(case)
    _report(case, y, ref)
    assert np.array_equal(y.astype(np.float64), ref)


@pytest.mark.parametrize("case", [c for c in LC.RANDOM if (c.m, c.bits) == (80, 4) and c.T in (16, 64)],
                         ids=lambda c: c.id)
def test_fp16_factors_through_the_packed_entry_equal_cq_linear_forward(case):
    K = _K()
    d = LC.inputs(case)
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    x, codes, L, R = t(d["x"]), t(LC.inference_codes(d["c"], case.bits)), t(d["L"]), t(d["R"])
    y0 = torch.full((case.T, case.m), NAN, device=DEV)
    y1 = torch.full((case.T, case.m), NAN, device=DEV)
    K.linear_forward(x, codes, d["s"], d["gs"], L, R, None, y0, m=case.m, n=case.n, bits=case.bits)
    K.linear_packed_forward(x, codes, d["s"], d["gs"], L, R, None, y1, m=case.m, n=case.n, bits=case.bits)
    assert torch.isfinite(y0).all() and torch.equal(y0, y1)


def _bar_of(lin, x16):
    """The bar of a coded CalderaLinear for fp16 x (T, n), in fp64 from its buffers."""
    from ee274_convexcaldera_llm_quantization_amd.linear import unpack_bytes
    f32 = np.float32
    x = np.abs(x16.double().cpu().numpy())
    un = lambda t, bits, cols: np.abs(unpack_bytes(t.cpu(), bits)[:, :cols].numpy().astype(np.float64))  # noqa: E731
    c = un(lin.codes, lin.bits, lin.in_features)
    l, rho = un(lin.L_codes, lin.L_bits, lin.rank), un(lin.R_codes, lin.R_bits, lin.in_features)
    k = lambda bits: f32(2 ** (bits - 1) - 1)  # noqa: E731
    sk = np.float64(f32(lin.qscale) / k(lin.bits))
    zscale = np.float64(f32(f32(lin.lscale) / k(lin.L_bits)) * f32(f32(lin.rscale) / k(lin.R_bits)))
    A = lin.gscale * (sk * (x @ c.T) + zscale * (x @ rho.T) @ l.T)
    return (lin.in_features + lin.rank + 32) * 2.0 ** -24 * A


@pytest.mark.parametrize("bits", [2, 4])
def test_layer_from_a_real_decomposition(bits):
    """256 x 512 fp16, rank 16, 4-bit L and R: the layer built from engine.last_packed and the one
    built from the returned decomposition agree bit for bit and match x (gs (Q + L R))^T in fp64
    from dec.Q / L / R within the bar alone -- coded factors are not rounded to fp16, so there is
    no allowance for that."""
    from ee274_convexcaldera_llm_quantization_amd.api import caldera_batch
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
    from src.caldera.utils.dataclasses import CalderaParams
    torch.manual_seed(0)
    W = (torch.randn(256, 512) * 0.02).to(torch.float16)
    qp = CalderaParams(Q_bits=bits, L_bits=4, R_bits=4, rank=16, iters=2, update_order=["Q", "LR"], sigma_reg=1e-8)
    decs, eng = caldera_batch(qp, [W.to(DEV)], None, device=DEV, return_engine=True, streams=1)
    dec, lp = decs[0], eng.last_packed[0]
    assert lp["L_codes"].dtype == lp["R_codes"].dtype == torch.int8
    assert lp["L_codes"].shape == (256, 16) and lp["R_codes"].shape == (16, 512)
    from ee274_convexcaldera_llm_quantization_amd.linear import unpack_bytes
    npad = lp.get("n_padded", 512)
    c = unpack_bytes(lp["codes"].reshape(-1), bits).view(256, npad)[:, :512]
    a = CalderaLinear.from_codes(c, None, None, qscale=lp["Q_scale"], gscale=lp["global_scale"], bits=bits,
                                 L_codes=(lp["L_codes"], lp["L_scale"], 4), R_codes=(lp["R_codes"], lp["R_scale"], 4)).to(DEV)
    b = CalderaLinear.from_decomposition(dec, bits, L_bits=4, R_bits=4).to(DEV)
    assert a.L is None and b.R is None
    for key in ("codes", "L_codes", "R_codes"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert (a.qscale, a.lscale, a.rscale, a.gscale) == (b.qscale, b.lscale, b.rscale, b.gscale)
    Wd = float(dec.global_scale) * (dec.Q.double() + dec.L.double() @ dec.R.double()).cpu().numpy()
    g = torch.Generator().manual_seed(1)
    for T in (5, 40):
        x = torch.randn(T, 512, generator=g).half().to(DEV)
        ya, yb = a(x.float()), b(x.float())
        assert torch.equal(ya, yb)
        ref = x.double().cpu().numpy() @ Wd.T
        bar = _bar_of(a, x)
        err = np.abs(ya.double().cpu().numpy() - ref)
        print(f"bits {bits} T {T}: worst {np.max(err / bar):.4f} bars")
        assert (err <= bar).all()


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1 = torch.nn.Linear(128, 256, bias=True)
        self.fc2 = torch.nn.Linear(256, 128, bias=False)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc1(x)))


@torch.no_grad()
def test_model_packed_factors_and_results_file(tmp_path):
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
    qp.iters, qp.L_bits, qp.R_bits = 2, 4, 4
    dense, coded, fresh = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)
    rep_d = M.apply_caldera_quantization(dense, None, qp, selection=sel, device=DEV)
    rep_c = M.apply_caldera_quantization(coded, None, qp, selection=sel, device=DEV, packed=True, packed_factors=True)
    assert [o.applied for o in rep_c.layers] == [True, True] == [o.applied for o in rep_d.layers]
    assert rep_c.quantized_param_count == rep_d.quantized_param_count == 2 * 128 * 256
    x = torch.randn(7, 128, generator=torch.Generator().manual_seed(2)).half().float().to(DEV)
    # layer by layer on the same input: coded forward vs the dense write-back (Q + L R in fp32) in fp64
    h = x
    for name in ("fc1", "fc2"):
        lin, ref_mod = getattr(coded, name), getattr(dense, name)
        assert isinstance(lin, CalderaLinear) and (lin.L_bits, lin.R_bits, lin.L, lin.R) == (4, 4, None, None)
        h16 = h.half()
        y = lin(h16.float())
        ref = h16.double() @ ref_mod.weight.double().T
        if ref_mod.bias is not None:
            ref = ref + ref_mod.bias.double()
        # the dense write-back rounds Q + L R once to fp32: 2^-24 of |W| per element, inside the bar's A
        bar = _bar_of(lin, h16)
        err = (y.double() - ref).abs().cpu().numpy()
        print(f"{name}: worst {np.max(err / bar):.4f} bars")
        assert (err <= bar).all()
        h = torch.relu(y)
    out_c = coded(x)
    path = str(tmp_path / "layers.cqrs")
    save_results(path, [coded.fc1.to_result("fc1"), coded.fc2.to_result("fc2")])
    assert M.apply_packed_results(fresh, load_results(path)) == ["fc1", "fc2"]
    assert fresh.fc1.L is None and fresh.fc1.L_codes is not None
    assert torch.equal(fresh(x), out_c)


def test_coded_decode_forward_in_a_captured_graph():
    """The entry neither allocates nor synchronises: a captured decode forward (one stream)
    replays to the bits of the eager one."""
    case = next(c for c in FC.RANDOM if (c.m, c.bits, c.lb, c.rb, c.T) == (80, 2, 4, 4, 16))
    lin = _module(case)
    x = torch.from_numpy(FC.inputs(case)["x"]).to(DEV)
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
