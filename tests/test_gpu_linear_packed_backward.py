"""The packed backward with coded factors on the GPU (cq_linear_packed_backward_input and
CalderaLinear's autograd function on a layer with coded factors) against the fp64 reference of
linear_packed_backward_cases.py: exact cases bit for bit in dx and u_out, random cases within the
worst-case fp32 bars, the fp16-factor path against cq_linear_backward_input, hostile tails, row
independence, graph capture.  Every coded operand carries nonzero tail codes (L) and random bytes
behind its last row (R), see the case module."""
import ctypes

import numpy as np
import pytest
import torch

import linear_backward_cases as BC
import linear_packed_backward_cases as PC

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


def _operands(case, qtail=False, clean=False):
    """dict of the entry's weight operands on the device.  The coded factors are the case's hostile
    buffers (clean: proper tails and nothing behind R); an fp16 factor sits at ld + 3 / + 5 inside
    a NaN-filled buffer.  qtail: random nonzero codes in the pad columns of the layer's own codes,
    at code_stride = row bytes + 16 inside a 0xFF-filled buffer."""
    d = PC.inputs(case)
    m, n, k, per = case.m, case.n, case.k, 8 // case.bits
    if qtail:
        rb = PC.row_bytes(n, case.bits)
        full = np.random.default_rng(9).integers(-k, k + 1, (m, rb * per)).astype(np.int8)
        full[:, :n] = d["c"]
        codes = _in_nan(torch.from_numpy(PC.pack_codes(full, case.bits).reshape(m, rb)), 16, 0xFF)
    else:
        codes = torch.from_numpy(PC.inference_codes(d["c"], case.bits)).to(DEV)
    ops = dict(codes=codes, L=None, R=None, L_codes=None, R_codes=None)
    if not case.r:
        return d, ops
    if case.lb == 16:
        ops["L"] = _in_nan(torch.from_numpy(d["lam"]), 3)
    else:
        buf = PC.inference_codes(d["lam"], case.lb) if clean else PC.l_codes(case)
        ops["L_codes"] = (torch.from_numpy(buf).to(DEV), float(d["sl"]), case.lb)
    if case.rb == 16:
        ops["R"] = _in_nan(torch.from_numpy(d["rho"]), 5)
    else:
        buf = PC.inference_codes(d["rho"], case.rb) if clean else PC.r_codes(case)
        ops["R_codes"] = (torch.from_numpy(buf).to(DEV)[:case.r], float(d["sr"]), case.rb)
    return d, ops


def _entry(case, dxdtype=torch.float32, dy=None, want_u=True, **how):
    """(dx, u~) through the C entry, each written into the middle of a NaN-filled buffer that must
    stay NaN around it."""
    K = _K()
    d, ops = _operands(case, **how)
    dy = _dy_in_nan_buffer(d["dy"]) if dy is None else dy
    T, n, r = dy.shape[0], case.n, case.r
    dxbuf = torch.full((T + 2, n + 5), NAN, dtype=dxdtype, device=DEV)
    dx = dxbuf[1:T + 1, 2:n + 2]
    ubuf = torch.full((T + 2, r + 5), NAN, dtype=torch.float32, device=DEV)
    u = ubuf[1:T + 1, 2:r + 2] if r and want_u else None
    K.linear_packed_backward_input(dy, ops["codes"], d["s"], d["gs"], ops["L"], ops["R"], dx, m=case.m, n=n,
                                   bits=case.bits, r=r, L_codes=ops["L_codes"], R_codes=ops["R_codes"], u_out=u)
    out, uo = dx.clone(), (ubuf[1:T + 1, 2:r + 2].clone() if u is not None else None)
    dxbuf[1:T + 1, 2:n + 2] = NAN
    ubuf[1:T + 1, 2:r + 2] = NAN
    assert torch.isnan(dxbuf).all(), "cq_linear_packed_backward_input wrote outside dx"
    assert torch.isnan(ubuf).all(), "cq_linear_packed_backward_input wrote outside u_out"
    return out.cpu(), None if uo is None else uo.cpu()


def _report(case, got, ref, bar=None, what="dx"):
    if bar is None:
        print(f"{case.id} {what}: mismatches {(got != ref).sum()} of {ref.size}")
    elif ref.size:
        print(f"{case.id} {what}: worst {np.nanmax(np.abs(got - ref) / np.maximum(bar, 1e-300)):.4f} bars")


# ---------------------------------------------------------------------------- the C entry
@pytest.mark.parametrize("case", PC.EXACT, ids=lambda c: c.id)
def test_exact_cases_bit_for_bit(case):
    ref, uref, _, _ = PC.reference(case)
    dx, u = _entry(case)
    _report(case, dx.numpy(), ref)
    assert dx.dtype == torch.float32 and np.array_equal(dx.numpy().astype(np.float64), ref)
    if case.r:
        _report(case, u.numpy(), uref, what="u")
        assert np.array_equal(u.numpy().astype(np.float64), uref)
        dx2, _ = _entry(case, want_u=False)      # u_out = NULL: the same dx
        assert torch.equal(dx2, dx)


@pytest.mark.parametrize("case", PC.EXACT16, ids=lambda c: c.id)
def test_fp16_dx_is_the_fp32_result_rounded_once(case):
    ref, _, _, _ = PC.reference(case)
    dx32, _ = _entry(case)
    dx16, _ = _entry(case, torch.float16)
    _report(case, dx32.numpy(), ref)
    assert np.array_equal(dx32.numpy().astype(np.float64), ref)
    assert dx16.dtype == torch.float16 and torch.equal(dx16, dx32.half())
    assert np.array_equal(dx16.numpy().astype(np.float64), ref)


@pytest.mark.parametrize("case", PC.RANDOM, ids=lambda c: c.id)
def test_random_cases_within_the_bars(case):
    ref, uref, bar, ubar = PC.reference(case)
    dx, u = _entry(case)
    dx = dx.numpy().astype(np.float64)
    _report(case, dx, ref, bar)
    assert np.isfinite(dx).all() and (np.abs(dx - ref) <= bar).all()
    if case.r:
        u = u.numpy().astype(np.float64)
        _report(case, u, uref, ubar, what="u")
        assert np.isfinite(u).all() and (np.abs(u - uref) <= ubar).all()
    dx16, _ = _entry(case, torch.float16)
    assert torch.equal(dx16, torch.from_numpy(dx).float().half())


@pytest.mark.parametrize("case", [c for c in BC.RANDOM if (c.m, c.bits, c.T) in ((48, 2, 17), (80, 4, 64), (160, 2, 130))],
                         ids=lambda c: c.id)
def test_fp16_factor_path_has_the_bits_of_the_plain_entry(case):
    """l_bits = r_bits = 16: cq_linear_backward_input, which is this entry with those values."""
    K = _K()
    d = BC.inputs(case)
    codes = torch.from_numpy(BC.inference_codes(d["c"], case.bits)).to(DEV)
    dy, L, R = (torch.from_numpy(d[key]).to(DEV) for key in ("dy", "L", "R"))
    out = []
    for fn in (K.linear_backward_input, K.linear_packed_backward_input):
        for dt in (torch.float32, torch.float16):
            dx = torch.full((case.T, case.n), NAN, dtype=dt, device=DEV)
            u = torch.full((case.T, case.r), NAN, dtype=torch.float32, device=DEV)
            fn(dy, codes, d["s"], d["gs"], L, R, dx, m=case.m, n=case.n, bits=case.bits, u_out=u)
            out += [dx, u]
    assert not any(torch.isnan(t).any() for t in out)
    assert all(torch.equal(a, b) for a, b in zip(out[:4], out[4:]))


_TAIL_CASES = [c for c in PC.EXACT if c.T in (5, 64) and (c.bits, c.lb, c.rb) in ((2, 4, 4), (2, 2, 2))] + \
              [c for c in PC.EXACT if (c.m, c.T) == (48, 17)]


@pytest.mark.parametrize("case", _TAIL_CASES, ids=lambda c: c.id)
def test_nonzero_tails_in_the_q_l_and_r_codes_change_nothing(case):
    """Random nonzero codes in the pad columns of the Q codes as well (the L tails and the bytes
    behind R are there in every test): the reference bit for bit, and the bits of proper operands."""
    ref, uref, _, _ = PC.reference(case)
    dx, u = _entry(case, qtail=True)
    assert np.array_equal(dx.numpy().astype(np.float64), ref)
    dxc, uc = _entry(case, clean=True)
    assert torch.equal(dx, dxc)
    if case.r:
        assert np.array_equal(u.numpy().astype(np.float64), uref) and torch.equal(u, uc)


def test_hostile_tails_on_random_cases_give_the_bits_of_proper_operands():
    for case in (c for c in PC.RANDOM if (c.m, c.T) in ((48, 64), (80, 17))):
        dx, u = _entry(case, qtail=True)
        dxc, uc = _entry(case, clean=True)
        assert torch.equal(dx, dxc) and torch.equal(u, uc), case.id


@pytest.mark.parametrize("case", [c for c in PC.RANDOM if c.m == 80 and c.T in (17, 64)], ids=lambda c: c.id)
def test_rows_are_independent_of_the_token_count_and_calls_repeat(case):
    """Row t of a T = 17 and a T = 64 call has the bits of the same row computed alone at T = 1."""
    dy0 = PC.inputs(case)["dy"]
    dx0, u0 = _entry(case)
    dx1, u1 = _entry(case)
    assert torch.equal(dx0, dx1) and torch.equal(u0, u1)
    for t in sorted({0, 5, 16, case.T - 1}):
        dxt, ut = _entry(case, dy=_dy_in_nan_buffer(dy0[t:t + 1]))
        assert torch.equal(dxt[0], dx0[t]) and torch.equal(ut[0], u0[t]), t
    dy = np.full_like(dy0, np.nan)
    dy[5] = dy0[5]
    dxf, _ = _entry(case, dy=_dy_in_nan_buffer(dy))
    assert torch.equal(dxf[5], dx0[5])


def test_packed_backward_entry_in_a_captured_graph():
    """The entry neither allocates nor synchronises: a captured call replays to the bits of the
    eager one."""
    K = _K()
    case = next(c for c in PC.RANDOM if (c.m, c.lb, c.rb, c.T) == (80, 4, 4, 64))
    d, ops = _operands(case)
    dy = torch.from_numpy(d["dy"]).to(DEV)
    kw = dict(m=case.m, n=case.n, bits=case.bits, r=case.r, L_codes=ops["L_codes"], R_codes=ops["R_codes"])
    args = (ops["codes"], d["s"], d["gs"], None, None)
    want = torch.empty((case.T, case.n), dtype=torch.float32, device=DEV)
    uwant = torch.empty((case.T, case.r), dtype=torch.float32, device=DEV)
    K.linear_packed_backward_input(dy, *args, want, u_out=uwant, **kw)
    dys, dxs, us = torch.zeros_like(dy), torch.zeros_like(want), torch.zeros_like(uwant)
    a = K.linear_packed_backward_args(dys, *args, dxs, u_out=us, **kw)
    ws = K.workspace(K.load().cq_linear_packed_backward_workspace(ctypes.byref(a)), DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.linear_packed_backward_input(dys, *args, dxs, u_out=us, ws=ws, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.linear_packed_backward_input(dys, *args, dxs, u_out=us, ws=ws, **kw)
    dys.copy_(dy)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dxs, want) and torch.equal(us, uwant)


# ---------------------------------------------------------------------------- the module
def _module(case):
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
    d = PC.inputs(case)
    t = torch.from_numpy
    return CalderaLinear.from_codes(
        t(d["c"]), t(d["lam"]) if case.lb == 16 else None, t(d["rho"]) if case.rb == 16 else None, None,
        qscale=float(d["s"]), gscale=float(d["gs"]), bits=case.bits,
        L_codes=None if case.lb == 16 else (t(d["lam"]), float(d["sl"]), case.lb),
        R_codes=None if case.rb == 16 else (t(d["rho"]), float(d["sr"]), case.rb)).to(DEV)


def _x_of(case, dtype=torch.float16):
    g = torch.Generator().manual_seed(case.seed)
    return torch.randn(case.T, case.n, generator=g).to(torch.float16).to(DEV).to(dtype)


@pytest.mark.parametrize("case", [c for c in PC.RANDOM if (c.m, c.T) == (48, 17)], ids=lambda c: c.id)
def test_coded_layer_has_a_graph_and_x_grad_equals_the_entry(case):
    """Every factor format: the graph's forward is the inference launch, x.grad the entry's dx for
    fp16, fp32 and bf16 x (bf16: the fp32 dx cast once); nothing becomes a parameter."""
    lin = _module(case)
    dy = torch.from_numpy(PC.inputs(case)["dy"]).to(DEV)
    want32, _ = _entry(case)
    for dt in (torch.float16, torch.float32, torch.bfloat16):
        x = _x_of(case, dt).requires_grad_()
        y = lin(x)
        assert y.grad_fn is not None and y.dtype == dt
        with torch.no_grad():
            y0 = lin(x)
        assert y0.grad_fn is None and torch.equal(y0, y)
        y.backward(dy.to(dt))               # N(0, 1) in fp16 -> bf16 loses bits: the entry gets what the layer got
        seen = dy.to(dt).to(torch.float16)
        if dt == torch.bfloat16:
            want, _ = _entry(case, dy=seen.contiguous())
            want = want.to(dt)
        else:
            want = want32.to(dt) if dt == torch.float32 else _entry(case, dt)[0]
        assert x.grad.dtype == dt and torch.equal(x.grad.cpu(), want)
    assert not list(lin.parameters()) and not lin.factors_trainable
    with pytest.raises(ValueError, match="coded"):
        lin.enable_factor_training()
    with torch.no_grad():
        assert lin(_x_of(case).requires_grad_()).grad_fn is None
