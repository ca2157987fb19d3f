"""The gated pair on the GPU (cq_linear_glu_forward, CalderaGatedMLP, model.fuse_gated_mlps): with the
identity the output is bit for bit the fp32 product of the members' own fp32 outputs (fp16 h: that product
rounded once); with silu it is within the epilogue's bar of silu(v_g) v_u formed in fp64 from those
outputs, and within the end-to-end bar of the fp64 reference of linear_glu_cases.py; nothing is written
outside h; graph capture; ragged views; the module, its fallbacks and fuse / unfuse on a toy model."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import linear_glu_cases as UC
from linear_glu_cases import ACT_IDENTITY, ACT_SILU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _K():
    from ee274_convexcaldera_llm_quantization_amd import _lib as K
    K.load()
    return K


def _t(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


_OPS = {}


def _operands(case):
    """(x, [gate, up] member dicts of device operands, q_format) of a case, uploaded once."""
    if case in _OPS:
        return _OPS[case]
    K = _K()
    d = UC.inputs(case)
    mems = []
    for mem in d["members"]:
        op = dict(codes=_t(UC.packed_codes(case, mem)), qscale=float(mem["s"]), gscale=float(mem["gs"]),
                  bias=_t(mem["bias"]), m=mem["m"], n=case.n, bits=case.bits, r=mem["r"])
        if mem["r"]:
            for which, key in (("l", "L"), ("rho", "R")):
                f = UC.factor_operand(case, mem, which)
                if f[0] == "fp16":
                    op[key] = _t(f[1])
                else:
                    op[key + "_codes"] = (_t(f[1]), float(f[2]), f[3])
        mems.append(op)
    qf = K.QFMT_NF if case.fmt == "nf" else K.QFMT_UNIFORM
    _OPS[case] = (_t(d["x"]), mems, qf)
    return _OPS[case]


def _fused(case, act, dtype, x=None, ld_extra=5):
    """h of the fused entry as a host array; h is a strided view inside a NaN-filled buffer (the canary),
    which must be untouched around it."""
    K = _K()
    x0, mems, qf = _operands(case)
    x = x0 if x is None else x
    buf = torch.full((case.T + 2, case.m + ld_extra), NAN, dtype=dtype, device=DEV)
    h = buf[1:case.T + 1, 2:case.m + 2]
    K.linear_glu_forward(x, mems[0], mems[1], h, qf, act)
    out = h.clone()
    h.fill_(NAN)
    assert torch.isnan(buf).all(), "the entry wrote outside h"
    return out.cpu().numpy()


_ALONE = {}


def _alone(case):
    """(v_g, v_u): each member through cq_linear_codebook_forward with fp32 y, computed once per case."""
    if case not in _ALONE:
        K = _K()
        x, mems, qf = _operands(case)
        vs = []
        for op in mems:
            y = torch.full((case.T, case.m), NAN, dtype=torch.float32, device=DEV)
            K.linear_codebook_forward(x, op["codes"], op["qscale"], op["gscale"], op.get("L"), op.get("R"), op["bias"],
                                      y, m=op["m"], n=op["n"], bits=op["bits"], q_format=qf, r=op["r"],
                                      L_codes=op.get("L_codes"), R_codes=op.get("R_codes"))
            vs.append(y.cpu().numpy())
        assert all(np.isfinite(v).all() for v in vs)
        _ALONE[case] = tuple(vs)
    return _ALONE[case]


# ---------------------------------------------------------------------------- the entry
@pytest.mark.parametrize("case", UC.ALL + UC.EXACT, ids=lambda c: c.id)
def test_identity_is_the_product_of_the_members_own_outputs_bit_for_bit(case):
    vg, vu = _alone(case)
    want = vg * vu                                        # one fp32 multiply
    h = _fused(case, ACT_IDENTITY, torch.float32)
    print(f"{case.id}: {int((h != want).sum())} of {want.size} differ")
    assert h.dtype == np.float32 and np.array_equal(h, want)
    if UC.has_f16(case):
        h16 = _fused(case, ACT_IDENTITY, torch.float16)
        with np.errstate(over="ignore"):
            assert h16.dtype == np.float16 and np.array_equal(h16, want.astype(np.float16))
    if case.kind == "exact":                              # and the fp64 reference from the operands
        assert np.array_equal(h.astype(np.float64), UC.reference(case, ACT_IDENTITY)[0])


@pytest.mark.parametrize("case", UC.ALL, ids=lambda c: c.id)
def test_silu_against_the_members_own_outputs(case):
    vg, vu = _alone(case)
    hs, bar32, bar16 = UC.epilogue_reference(ACT_SILU, vg, vu)
    h = _fused(case, ACT_SILU, torch.float32)
    err = np.abs(h.astype(np.float64) - hs)
    print(f"{case.id}: worst error / bar {float((err / bar32).max()):.3f}")
    assert np.isfinite(h).all() and (err <= bar32).all()
    if UC.has_f16(case):
        h16 = _fused(case, ACT_SILU, torch.float16)
        err16 = np.abs(h16.astype(np.float64) - hs)
        print(f"{case.id}: fp16 worst error / bar {float((err16 / bar16).max()):.3f}")
        assert np.isfinite(h16).all() and (err16 <= bar16).all()


@pytest.mark.parametrize("act", [ACT_SILU, ACT_IDENTITY], ids=["silu", "identity"])
@pytest.mark.parametrize("case", UC.ALL, ids=lambda c: c.id)
def test_end_to_end_against_the_fp64_reference(case, act):
    ref, bar = UC.reference(case, act)
    h = _fused(case, act, torch.float32)
    err = np.abs(h.astype(np.float64) - ref)
    print(f"{case.id}: worst error / bar {float((err / bar).max()):.4f}")
    assert (err <= bar).all()


def test_the_entry_refuses_before_any_launch_and_accepts_zero_tokens():
    K = _K()
    case = next(c for c in UC.ALL if (c.m, c.T, c.fmt, c.bits, c.bias) == (33, 5, "uniform", 2, 0))
    x, mems, qf = _operands(case)
    buf = torch.full((case.T, case.m), NAN, device=DEV)
    with pytest.raises(ValueError, match="up"):
        K.linear_glu_forward(x, mems[0], dict(mems[1], bits=4), buf, qf, ACT_SILU)
    with pytest.raises(ValueError, match="act"):
        K.linear_glu_forward(x, mems[0], mems[1], buf, qf, 7)
    a = K.linear_glu_args(x, mems[0], mems[1], buf, qf, ACT_SILU)
    a.gate.tokens = a.up.tokens = 0
    lib = K.load()
    assert lib.cq_linear_glu_workspace(ctypes.byref(a)) == 0
    assert lib.cq_linear_glu_forward(ctypes.byref(a), None, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


@pytest.mark.parametrize("case", [c for c in UC.ALL if c.T in (16, 17) and c.n == 198 and c.lb == 16 and c.bits == 2],
                         ids=lambda c: c.id)
def test_a_captured_graph_replays_to_the_eager_bits(case):
    """The entry neither allocates nor synchronises nor copies: with its workspace preallocated a
    captured call allocates nothing and replays to the eager bits."""
    K = _K()
    x, mems, qf = _operands(case)
    lib = K.load()
    h = torch.empty((case.T, case.m), dtype=torch.float32, device=DEV)
    xs = torch.zeros_like(x)
    ws = K.workspace(lib.cq_linear_glu_workspace(ctypes.byref(K.linear_glu_args(xs, mems[0], mems[1], h, qf, ACT_SILU))),
                     DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.linear_glu_forward(xs, mems[0], mems[1], h, qf, ACT_SILU, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_allocated()            # after the capture's own bookkeeping (RNG state)
        K.linear_glu_forward(xs, mems[0], mems[1], h, qf, ACT_SILU, ws=ws)
        inside = torch.cuda.memory_allocated()
    assert inside == before
    xs.copy_(x)
    h.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(h.cpu().numpy(), _fused(case, ACT_SILU, torch.float32))


@pytest.mark.parametrize("case", [c for c in UC.ALL if (c.m, c.fmt, c.bits, c.bias) == (33, "uniform", 4, 2)]
                         + [c for c in UC.ALL if (c.m, c.n, c.fmt, c.bits) == (80, 898, "nf", 4) and c.T in (5, 64)],
                         ids=lambda c: c.id)
def test_ragged_views(case):
    """x as a view with ldx > n (odd: the element-wise loader) in a NaN-filled buffer, h with ldh > m and
    a canary around it, fp32 and fp16: the bits of the contiguous call."""
    x0 = _operands(case)[0]
    buf = torch.full((case.T + 1, case.n + 3), NAN, dtype=torch.float16, device=DEV)
    x = buf[:case.T, 1:case.n + 1]
    x.copy_(x0)
    assert x.stride(0) == case.n + 3
    for act in (ACT_SILU, ACT_IDENTITY):
        for dtype in (torch.float32, torch.float16):
            assert np.array_equal(_fused(case, act, dtype, x=x, ld_extra=9), _fused(case, act, dtype, ld_extra=4))


# ---------------------------------------------------------------------------- the module
def _layer(rng, m, n, r, bits):
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
    k = 2 ** (bits - 1) - 1
    c = torch.from_numpy(rng.integers(-k, k + 1, (m, n)).astype(np.int8))
    L = torch.from_numpy((0.15 * rng.standard_normal((m, r))).astype(np.float16)) if r else None
    R = torch.from_numpy((0.15 * rng.standard_normal((r, n))).astype(np.float16)) if r else None
    return CalderaLinear.from_codes(c, L, R, None, qscale=0.05, gscale=1.7, bits=bits)


class _MLP(torch.nn.Module):
    def __init__(self, rng, n=96, ff=200):
        super().__init__()
        self.gate_proj, self.up_proj = _layer(rng, ff, n, 16, 2), _layer(rng, ff, n, 8, 2)
        self.down_proj = _layer(rng, n, ff, 8, 2)
        self.act_fn = torch.nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        rng = np.random.default_rng(23)
        self.blocks = torch.nn.ModuleList([_MLP(rng), _MLP(rng)])

    def forward(self, x):
        for b in self.blocks:
            x = x + b(x)
        return x


def _count(monkeypatch):
    from ee274_convexcaldera_llm_quantization_amd import _lib as K
    calls = []
    real = K.linear_glu_forward
    monkeypatch.setattr(K, "linear_glu_forward", lambda *a, **kw: (calls.append(a[0].shape[0]), real(*a, **kw))[1])
    return calls


def _x(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.bfloat16], ids=str)
def test_module_against_the_formula_from_the_members_fp32_outputs(dtype, monkeypatch):
    """glu(x) is silu(v_g) v_u from the members' fp32 pre-activations rounded once: against that product
    formed by torch in fp32 from the members' fp32 outputs (on the fp16 x the kernel sees) it is within
    the epilogue's bar, plus the one rounding to x's dtype."""
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaGatedMLP
    mlp = _MLP(np.random.default_rng(5)).to(DEV)
    fused = CalderaGatedMLP(mlp.gate_proj, mlp.up_proj, mlp.down_proj)
    calls = _count(monkeypatch)
    for shape in ((1, 1, 96), (2, 3, 96), (1, 40, 96)):       # decode, decode, prefill
        x = _x(shape, 3, dtype)
        with torch.no_grad():
            h = fused.glu(x)
            x32 = x.to(torch.float16).float()                  # fp32 x: the members return their fp32 values
            vg, vu = mlp.gate_proj(x32), mlp.up_proj(x32)
            want = torch.nn.functional.silu(vg.double()) * vu.double()
            assert h.dtype == dtype and h.shape == vg.shape
            eps = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}[dtype]   # half an ulp: 2^-p, p = 11 / 8 bits
            bar = (8 * 2.0 ** -24 + eps) * want.abs() + 2.0 ** -25
            assert ((h.double() - want).abs() <= bar).all()
            # and the block: down_proj on that h
            assert torch.equal(fused(x), mlp.down_proj(h))
    assert calls == [1, 1, 6, 6, 40, 40]                      # glu(x) and forward(x), one launch pair each


def test_fallbacks_are_the_unfused_formula_and_gradients_flow(monkeypatch):
    from ee274_convexcaldera_llm_quantization_amd import model as M
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaGatedMLP
    mlp = _MLP(np.random.default_rng(7)).to(DEV)
    fused = CalderaGatedMLP(mlp.gate_proj, mlp.up_proj, mlp.down_proj)
    calls = _count(monkeypatch)
    # x requires grad
    grads = []
    for net in (mlp, fused):
        x = _x((2, 3, 96), 9).requires_grad_()
        y = net(x)
        y.square().sum().backward()
        grads.append((y.detach(), x.grad))
    assert calls == [] and torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert grads[0][1].abs().max() > 0
    # dense_prefill_tokens reached, and not reached
    M.set_dense_prefill(fused, 64)
    x = _x((1, 64, 96), 11, torch.float16)
    with torch.no_grad():
        assert torch.equal(fused(x), mlp(x)) and calls == []
        fused(x[:, :63])
    assert calls == [63]
    M.set_dense_prefill(fused, None)
    # trainable factors
    params = M.prepare_factor_finetuning(fused)
    assert len(params) == 6
    x = _x((2, 3, 96), 13)
    with torch.no_grad():
        assert torch.equal(fused(x), mlp(x))
    y = fused(x)
    y.square().sum().backward()
    assert calls == [63] and all(p.grad is not None and p.grad.abs().max() > 0 for p in params)
    M.finish_factor_finetuning(fused)
    with torch.no_grad():
        fused(x)
    assert calls == [63, 6]


def test_fuse_run_unfuse_run_on_a_toy_model(monkeypatch):
    from ee274_convexcaldera_llm_quantization_amd import model as M
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaGatedMLP
    plain = _Toy().to(DEV)
    model = copy.deepcopy(plain)
    originals = [model.blocks[0], model.blocks[1]]
    done, skipped = M.fuse_gated_mlps(model)
    assert done == ["blocks.0", "blocks.1"] and skipped == []
    assert all(isinstance(b, CalderaGatedMLP) for b in model.blocks)
    calls = _count(monkeypatch)
    x = _x((2, 3, 96), 17, torch.float16)
    with torch.no_grad():
        want = plain(x)
        got = model(x)
    assert calls == [6, 6] and got.shape == want.shape and torch.isfinite(got).all()
    # one rounding of h instead of three: not the unfused bits.  Each h differs by at most 3 * 2^-11
    # relative; a down_proj output sums 200 of them with random signs (sum |terms| ~ sqrt(200) ~ 14 times
    # the output's scale), so 0.02 of the largest output per block, and the second block passes the
    # first one's on: 0.05 is a sanity bound, the bit-level claims are the tests above
    ratio = float((got.float() - want.float()).abs().max() / want.float().abs().max())
    print(f"fused against unfused fp16: {ratio:.2e} of the largest output")
    assert ratio <= 0.05
    assert M.unfuse_gated_mlps(model) == done
    assert model.blocks[0] is originals[0] and model.blocks[1] is originals[1]
    with torch.no_grad():
        assert torch.equal(model(x), want)
    assert calls == [6, 6]
