"""The packed linear layer's backward on the GPU (cq_linear_backward_input, CalderaLinear's autograd
function, model.prepare_factor_finetuning) against the fp64 reference of linear_backward_cases.py:
exact cases bit for bit, random cases within the worst-case fp32 bars, through the C entry and
through the module; row independence, repeatability, graph capture; dL and dR against fp64
autograd; five SGD steps on a tiny packed model."""
import numpy as np
import pytest
import torch

import linear_backward_cases as BC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _K():
    from ee274_convexcaldera_llm_quantization_amd import _lib as K
    K.load()
    return K


def _in_nan(t, pad_cols, fill=NAN):
    """t (rows, cols) as a view with row stride cols + pad_cols of a buffer filled with `fill`."""
    rows, cols = t.shape
    buf = torch.full((rows + 1, cols + pad_cols), fill, dtype=t.dtype, device=DEV)
    view = buf[:rows, :cols]
    view.copy_(t)
    return view


def _dy_in_nan_buffer(dy_np):
    """dy at ld = m inside a NaN-filled buffer (m = 33: rows 2-byte aligned only)."""
    T, m = dy_np.shape
    buf = torch.full((T * m + 24,), NAN, dtype=torch.float16, device=DEV)
    dy = buf[8:8 + T * m].view(T, m)
    dy.copy_(torch.from_numpy(dy_np))
    return dy


def _operands(case, hostile=False):
    """codes, L, R on the device.  hostile: random nonzero codes in every row's pad columns and R
    at ldr = n + 5 inside a NaN-filled buffer (rows not 16-byte aligned), L at ldl = r + 3."""
    d = BC.inputs(case)
    m, n, k, per = case.m, case.n, case.k, 8 // case.bits
    if hostile:
        rb = BC.row_bytes(n, case.bits)
        from linear_cases import pack_codes
        full = np.random.default_rng(9).integers(-k, k + 1, (m, rb * per)).astype(np.int8)
        full[:, :n] = d["c"]
        codes = _in_nan(torch.from_numpy(pack_codes(full, case.bits).reshape(m, rb)), 16, 0xFF)
    else:
        codes = torch.from_numpy(BC.inference_codes(d["c"], case.bits)).to(DEV)
    if not case.r:
        return d, codes, None, None
    if hostile:
        return d, codes, _in_nan(torch.from_numpy(d["L"]), 3), _in_nan(torch.from_numpy(d["R"]), 5)
    return d, codes, torch.from_numpy(d["L"]).to(DEV), torch.from_numpy(d["R"]).to(DEV)


def _entry(case, dxdtype=torch.float32, dy=None, hostile=False, want_u=True):
    """(dx, u) through the C entry, each written into the middle of a NaN-filled buffer that must
    stay NaN around it."""
    K = _K()
    d, codes, L, R = _operands(case, hostile)
    dy = _dy_in_nan_buffer(d["dy"]) if dy is None else dy
    T, n, r = dy.shape[0], case.n, case.r
    dxbuf = torch.full((T + 2, n + 5), NAN, dtype=dxdtype, device=DEV)
    dx = dxbuf[1:T + 1, 2:n + 2]
    ubuf = torch.full((T + 2, r + 5), NAN, dtype=torch.float32, device=DEV)
    u = ubuf[1:T + 1, 2:r + 2] if r and want_u else None
    K.linear_backward_input(dy, codes, d["s"], d["gs"], L, R, dx, m=case.m, n=n, bits=case.bits, u_out=u)
    out, uo = dx.clone(), (ubuf[1:T + 1, 2:r + 2].clone() if u is not None else None)
    dxbuf[1:T + 1, 2:n + 2] = NAN
    ubuf[1:T + 1, 2:r + 2] = NAN
    assert torch.isnan(dxbuf).all(), "cq_linear_backward_input wrote outside dx"
    assert torch.isnan(ubuf).all(), "cq_linear_backward_input wrote outside u_out"
    return out.cpu(), None if uo is None else uo.cpu()


def _module(case, trainable=False):
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
    d = BC.inputs(case)
    f = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    lin = CalderaLinear.from_codes(torch.from_numpy(d["c"]), f(d["L"]) if case.r else None,
                                   f(d["R"]) if case.r else None, f(d["bias"]), qscale=float(d["s"]),
                                   gscale=float(d["gs"]), bits=case.bits).to(DEV)
    if trainable:
        lin.enable_factor_training()
    return lin


def _x_of(case, dtype=torch.float16):
    g = torch.Generator().manual_seed(case.seed)
    return torch.randn(case.T, case.n, generator=g).to(torch.float16).to(DEV).to(dtype)


def _report(case, got, ref, bar=None, what="dx"):
    if bar is None:
        print(f"{case.id} {what}: mismatches {(got != ref).sum()} of {ref.size}")
    elif ref.size:
        print(f"{case.id} {what}: worst {np.nanmax(np.abs(got - ref) / np.maximum(bar, 1e-300)):.4f} bars")


# ---------------------------------------------------------------------------- the C entry
@pytest.mark.parametrize("case", BC.EXACT, ids=lambda c: c.id)
def test_exact_cases_bit_for_bit(case):
    ref, uref, _, _ = BC.reference(case)
    dx, u = _entry(case)
    _report(case, dx.numpy(), ref)
    assert dx.dtype == torch.float32 and np.array_equal(dx.numpy().astype(np.float64), ref)
    if case.r:
        _report(case, u.numpy(), uref, what="u")
        assert np.array_equal(u.numpy().astype(np.float64), uref)
        dx2, _ = _entry(case, want_u=False)      # u_out = NULL: the same dx
        assert torch.equal(dx2, dx)


@pytest.mark.parametrize("case", BC.EXACT16, ids=lambda c: c.id)
def test_fp16_dx_is_the_fp32_result_rounded_once(case):
    ref, _, _, _ = BC.reference(case)
    dx32, _ = _entry(case)
    dx16, _ = _entry(case, torch.float16)
    _report(case, dx32.numpy(), ref)
    assert np.array_equal(dx32.numpy().astype(np.float64), ref)
    assert dx16.dtype == torch.float16 and torch.equal(dx16, dx32.half())
    assert np.array_equal(dx16.numpy().astype(np.float64), ref)


@pytest.mark.parametrize("case", BC.RANDOM, ids=lambda c: c.id)
def test_random_cases_within_the_bars(case):
    ref, uref, bar, ubar = BC.reference(case)
    dx, u = _entry(case)
    dx = dx.numpy().astype(np.float64)
    _report(case, dx, ref, bar)
    assert np.isfinite(dx).all() and (np.abs(dx - ref) <= bar).all()
    if case.r:
        u = u.numpy().astype(np.float64)
        _report(case, u, uref, ubar, what="u")
        assert np.isfinite(u).all() and (np.abs(u - uref) <= ubar).all()


@pytest.mark.parametrize("case", [c for c in BC.EXACT if c.T in (5, 64) and c.m in (33, 48, 80, 198, 272)],
                         ids=lambda c: c.id)
def test_pad_columns_and_strided_operands_change_nothing(case):
    """Random nonzero codes in every row's pad columns (code_stride = row bytes + 16 inside a
    0xFF-filled buffer), L at ldl = r + 3 and R at ldr = n + 5 inside NaN-filled buffers: still
    the reference bit for bit."""
    ref, uref, _, _ = BC.reference(case)
    dx, u = _entry(case, hostile=True)
    assert np.array_equal(dx.numpy().astype(np.float64), ref)
    if case.r:
        assert np.array_equal(u.numpy().astype(np.float64), uref)


@pytest.mark.parametrize("case", [c for c in BC.RANDOM if (c.m, c.bits) == (80, 2) and c.T in (17, 64)],
                         ids=lambda c: c.id)
def test_rows_are_independent_of_the_token_count_and_calls_repeat(case):
    """Row t of a T = 17 and a T = 64 call has the bits of the same row computed alone at T = 1."""
    dy0 = BC.inputs(case)["dy"]
    dx0, u0 = _entry(case)
    dx1, u1 = _entry(case)
    assert torch.equal(dx0, dx1) and torch.equal(u0, u1)
    for t in sorted({0, 5, 16, case.T - 1}):
        dxt, ut = _entry(case, dy=_dy_in_nan_buffer(dy0[t:t + 1]))
        assert torch.equal(dxt[0], dx0[t]) and torch.equal(ut[0], u0[t]), t
    rng = np.random.default_rng(3)
    for fill in ("other", "nan"):
        dy = rng.standard_normal(dy0.shape).astype(np.float16) if fill == "other" else np.full_like(dy0, np.nan)
        dy[5] = dy0[5]
        dxf, _ = _entry(case, dy=_dy_in_nan_buffer(dy))
        assert torch.equal(dxf[5], dx0[5]), fill


def test_backward_entry_in_a_captured_graph():
    """The entry neither allocates nor synchronises: a captured call replays to the bits of the
    eager one."""
    K = _K()
    case = next(c for c in BC.RANDOM if (c.m, c.bits, c.T) == (80, 4, 64))
    d, codes, L, R = _operands(case)
    dy = torch.from_numpy(d["dy"]).to(DEV)
    kw = dict(m=case.m, n=case.n, bits=case.bits)
    want = torch.empty((case.T, case.n), dtype=torch.float32, device=DEV)
    uwant = torch.empty((case.T, case.r), dtype=torch.float32, device=DEV)
    K.linear_backward_input(dy, codes, d["s"], d["gs"], L, R, want, u_out=uwant, **kw)
    dys, dxs, us = torch.zeros_like(dy), torch.zeros_like(want), torch.zeros_like(uwant)
    a = K.linear_backward_args(dys, codes, d["s"], d["gs"], L, R, dxs, u_out=us, **kw)
    import ctypes
    ws = K.workspace(K.load().cq_linear_backward_workspace(ctypes.byref(a)), DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.linear_backward_input(dys, codes, d["s"], d["gs"], L, R, dxs, u_out=us, ws=ws, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.linear_backward_input(dys, codes, d["s"], d["gs"], L, R, dxs, u_out=us, ws=ws, **kw)
    dys.copy_(dy)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dxs, want) and torch.equal(us, uwant)


# ---------------------------------------------------------------------------- the module
_MODULE_CASES = [c for c in BC.RANDOM if (c.m, c.n) in ((48, 198), (80, 898)) and c.T in (17, 64)]


@pytest.mark.parametrize("case", [c for c in BC.EXACT16 if c.T == 5] + [c for c in BC.RANDOM if c.m == 198 and c.T == 17]
                         + _MODULE_CASES[:2], ids=lambda c: c.id)
def test_frozen_layer_gives_x_grad_equal_to_the_entry(case):
    lin = _module(case)
    dy = torch.from_numpy(BC.inputs(case)["dy"]).to(DEV)
    for dt in (torch.float16, torch.float32):
        x = _x_of(case, dt).requires_grad_()
        y = lin(x)
        assert y.grad_fn is not None and y.dtype == dt
        with torch.no_grad():
            assert torch.equal(lin(x), y)                  # the graph's forward is the inference launch
        y.backward(dy.to(dt))
        want, _ = _entry(case, dt)
        assert x.grad.dtype == dt and torch.equal(x.grad.cpu(), want)
    assert not list(lin.parameters())


def test_bf16_x_gets_an_fp32_dx_cast_once():
    case = next(c for c in BC.EXACT16 if (c.bits, c.T) == (4, 5))
    lin = _module(case)
    x = _x_of(case, torch.bfloat16).requires_grad_()
    dy = torch.from_numpy(BC.inputs(case)["dy"]).to(DEV)      # -1..1: exact in bf16
    lin(x).backward(dy.to(torch.bfloat16))
    ref, _, _, _ = BC.reference(case)
    assert x.grad.dtype == torch.bfloat16
    assert torch.equal(x.grad.cpu(), torch.from_numpy(ref).to(torch.bfloat16))


def _factor_grads64(case, x16, dy16):
    """dL, dR of sum(dy * (x W^T)) with W = gs (c (s / k) + L R), L and R as fp64 leaves, and the bars."""
    d = BC.inputs(case)
    c = torch.from_numpy(d["c"]).double()
    L = torch.from_numpy(d["L"]).double().requires_grad_()
    R = torch.from_numpy(d["R"]).double().requires_grad_()
    sk, gs = float(np.float64(d["s"] / np.float32(case.k))), float(np.float64(d["gs"]))
    x, dy = x16.double().cpu(), dy16.double().cpu()
    ((x @ (gs * (c * sk + L @ R)).t()) * dy).sum().backward()
    ax, ady, aL, aR = x.abs(), dy.abs(), L.detach().abs(), R.detach().abs()
    T, m, n = case.T, case.m, case.n
    barL = (T + n + 64) * 2.0 ** -24 * gs * (ady.t() @ (ax @ aR.t()))
    barR = (T + m + 64) * 2.0 ** -24 * gs * ((ady @ aL).t() @ ax)
    return L.grad, R.grad, barL, barR


@pytest.mark.parametrize("case", _MODULE_CASES, ids=lambda c: c.id)
def test_factor_gradients_against_fp64_autograd(case):
    frozen, lin = _module(case), _module(case, trainable=True)
    x16 = _x_of(case)
    dy16 = torch.from_numpy(BC.inputs(case)["dy"]).to(DEV)
    with torch.no_grad():
        assert torch.equal(lin(x16), frozen(x16))   # no optimiser step yet: the frozen forward's bits
    # leading dimensions are kept, with fp16 and fp32 x
    lead = (case.T,) if case.T % 2 else (2, case.T // 2)
    for dt in (torch.float16, torch.float32):
        lin.zero_grad()
        x = x16.to(dt).reshape(*lead, case.n).clone().requires_grad_()
        y = lin(x)
        with torch.no_grad():
            y0 = frozen(x16.to(dt))
        assert y.shape == (*lead, case.m) and y.dtype == dt and torch.equal(y.reshape(case.T, case.m), y0)
        y.backward(dy16.to(dt).reshape(*lead, case.m))
        assert x.grad.shape == x.shape and x.grad.dtype == dt
        want, _ = _entry(case, dt)
        assert torch.equal(x.grad.reshape(case.T, case.n).cpu(), want)
        dL64, dR64, barL, barR = _factor_grads64(case, x16, dy16)
        assert lin.L.grad.dtype == lin.R.grad.dtype == torch.float32
        eL = ((lin.L.grad.double().cpu() - dL64).abs() / barL).max().item()
        eR = ((lin.R.grad.double().cpu() - dR64).abs() / barR).max().item()
        print(f"{case.id} {dt}: dL worst {eL:.4f} bars, dR worst {eR:.4f} bars")
        assert eL <= 1 and eR <= 1
    # factors alone (x without grad): the same dL and dR
    gL, gR = lin.L.grad.clone(), lin.R.grad.clone()
    lin.zero_grad()
    lin(x16.float()).backward(dy16.float())
    eL = ((lin.L.grad.double().cpu() - dL64).abs() / barL).max().item()
    eR = ((lin.R.grad.double().cpu() - dR64).abs() / barR).max().item()
    assert eL <= 1 and eR <= 1 and torch.equal(lin.L.grad, gL)


def test_single_fp16_rounding_of_z_or_u_would_fail_the_factor_bars():
    """The dL / dR bars force z and u to stay in fp32 between the two products."""
    case = _MODULE_CASES[0]
    x16 = _x_of(case).cpu()
    d = BC.inputs(case)
    dy, L, R = (torch.from_numpy(d[key]).double() for key in ("dy", "L", "R"))
    dL64, dR64, barL, barR = _factor_grads64(case, x16, torch.from_numpy(d["dy"]))
    gs = float(d["gs"])
    z16 = (x16.double() @ R.t()).half().double()
    u16 = (dy @ L).half().double()
    assert (((gs * dy.t() @ z16) - dL64).abs() / barL).max() > 1
    assert (((gs * u16.t() @ x16.double()) - dR64).abs() / barR).max() > 1


def test_no_grad_saves_nothing():
    case = _MODULE_CASES[0]
    lin = _module(case, trainable=True)
    x = _x_of(case).requires_grad_()
    with torch.no_grad():
        y = lin(x)
    assert y.grad_fn is None and not y.requires_grad
    y = lin(x.detach())                       # trainable factors alone make the graph
    assert y.grad_fn is not None
    lin.L.requires_grad_(False), lin.R.requires_grad_(False)
    assert lin(x.detach()).grad_fn is None


# ---------------------------------------------------------------------------- a tiny model
def _random_layer(m, n, r, bits, seed):
    """A layer with the random cases' distributions: codes in -k..k, L, R ~ 0.15 N(0, 1), s = 0.05, gs = 1.7."""
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
    rng = np.random.default_rng(seed)
    k = 2 ** (bits - 1) - 1
    c = torch.from_numpy(rng.integers(-k, k + 1, (m, n)).astype(np.int8))
    L = torch.from_numpy((0.15 * rng.standard_normal((m, r))).astype(np.float16))
    R = torch.from_numpy((0.15 * rng.standard_normal((r, n))).astype(np.float16))
    return CalderaLinear.from_codes(c, L, R, None, qscale=0.05, gscale=1.7, bits=bits)


class _Tiny(torch.nn.Module):
    """(48, 198, 40) at 2 bits -> ReLU -> (33, 48, 8) at 4 bits."""

    def __init__(self):
        super().__init__()
        self.fc1 = _random_layer(48, 198, 40, 2, 21)
        self.fc2 = _random_layer(33, 48, 8, 4, 22)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc1(x)))


# a CPU restatement in fp64 (masters rounded to fp16 in each forward) falls from 4.78 to 2.15 in five
# steps at this rate, monotonically, as it does at a quarter and at ten times the rate
TINY_LR = 0.02


def test_five_sgd_steps_on_a_tiny_packed_model():
    from ee274_convexcaldera_llm_quantization_amd import model as M
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
    net = _Tiny().to(DEV)
    keys = set(net.state_dict())
    codes = [net.fc1.codes.clone(), net.fc2.codes.clone()]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(32, 198, generator=g).to(DEV)
    target = torch.randn(32, 33, generator=g).to(DEV)
    params = M.prepare_factor_finetuning(net)
    assert len(params) == 4
    opt = torch.optim.SGD(params, lr=TINY_LR)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(net(x), target)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        losses.append(torch.nn.functional.mse_loss(net(x), target).item())
    print("losses", " ".join(f"{v:.5f}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert torch.equal(net.fc1.codes, codes[0]) and torch.equal(net.fc2.codes, codes[1])
    tuned = net(x).detach()
    M.finish_factor_finetuning(net)
    assert not list(net.parameters()) and set(net.state_dict()) == keys
    with torch.no_grad():
        y = net(x)
    assert y.grad_fn is None and torch.equal(y, tuned)
    for lin in (net.fc1, net.fc2):
        again = CalderaLinear.from_result(lin.to_result("layer")).to(DEV)
        assert torch.equal(again.L, lin.L) and torch.equal(again.R, lin.R) and torch.equal(again.codes, lin.codes)
        assert again.L.dtype == torch.float16

