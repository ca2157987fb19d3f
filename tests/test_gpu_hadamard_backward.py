"""HadamardCalderaLinear's backward on the device: the forward with a graph is the inference
forward, x.grad is exactly the three public entries (transform, the inner layer's input gradient,
transform), dx and the inner factors' gradients against fp64, five SGD steps on a tiny model of
every packed layer kind.

    out x in        padded           reaches
    6 x 13          8 x 16           small single-wave transforms
    100 x 198       128 x 256        mid-size single-wave transforms (also with a coded-factor inner)
    1000 x 4096     1024 x 4096      the block transform path

The dx bar mirrors test_gpu_hadamard_linear.py's, elementwise in fp64 for fp32 dy and x (dy^ = H1
pad(dy) exactly, W~ the inner layer's dense weight, pr x pc the padded grid):

    bar[j] = (1 / sqrt(pc)) sum_j' ( 2^-11 sum_i |dy^_i| |W~_ij'|  +  dxbar_j' )  +  the two transform bars

2^-11 |dy^| is the rounding of dy^ to fp16, dxbar the worst-case bound of
linear_backward_cases.py for the inner layer on the fp16 dy^ it receives ((pr + r + 32) 2^-24 A),
and each transform adds hadamard_cases' 1.01 (log2 P + 2) 2^-24 sum |input| / sqrt(P): the first
one's is carried through |W~| and H2 like the fp16 rounding, the second's is on the inner layer's
fp32 dx^.

The factor gradients are taken in the Hadamard basis, dL = gs dy^^T (x^ R^T) and dR = gs (dy^ L)^T x^,
and held against fp64 autograd through H1 gs (Q + L R) H2 on the fp32 x and dy.  The bars are the
worst-case fp32 bars of test_gpu_linear_backward.py on |x^|, |dy^| (factors (T + pc + 64) 2^-24 resp.
(T + pr + 64) 2^-24 of the sums of magnitudes) plus 2^-9 of the same sums: the reference goes
through H in fp64, so the kernels' fp16 x^ and dy^ differ from its operands by 2^-11 (1 + the
transforms' 1.01 (log2 P + 2) 2^-13 <= 0.002) each, and 2 (1.002) 2^-11 (1 + 2^-11) <= 2^-9."""
import numpy as np
import pytest
import torch

import hadamard_cases as HC
import test_gpu_hadamard_linear as HL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
u24 = 2.0 ** -24
SHAPES = [(6, 13), (100, 198), (1000, 4096)]
_CASES = [(m, n, "fp16") for m, n in SHAPES] + [(100, 198, "coded4")]


def _K():
    from ee274_convexcaldera_llm_quantization_amd import _lib as K
    K.load()
    return K


def _lin(m, n, factors="fp16", bias=True):
    return HL._layer(m, n, 8, 2 if m != 100 else 4, factors, bias)


def _xy(lin, T, dtype=torch.float32):
    g = torch.Generator().manual_seed(T + lin.in_features)
    x = torch.randn(T, lin.in_features, generator=g).to(dtype).to(DEV)
    dy = torch.randn(T, lin.out_features, generator=g).to(dtype).to(DEV)
    return x, dy


def _backward_by_hand(lin, dy2, dx_dtype):
    """The three public entries on dy2 (T, m): transform to the fp16 dy^, the inner layer's input
    gradient in fp32, transform to dx (T, n)."""
    K = _K()
    inner = lin.inner
    pr, pc = lin.padded_shape
    T = dy2.shape[0]
    dyh = torch.empty((T, pr), dtype=torch.float16, device=DEV)
    K.hadamard_rows(dy2, dyh, n_in=lin.out_features, n_out=pr, P=pr)
    dxh = torch.empty((T, pc), dtype=torch.float32, device=DEV)
    if inner.L_codes is not None or inner.R_codes is not None:
        K.linear_packed_backward_input(dyh, inner.codes, inner.qscale, inner.gscale, inner.L, inner.R, dxh, m=pr, n=pc,
                                       bits=inner.bits, r=inner.rank,
                                       L_codes=(inner.L_codes, inner.lscale, inner.L_bits),
                                       R_codes=(inner.R_codes, inner.rscale, inner.R_bits))
    else:
        K.linear_backward_input(dyh, inner.codes, inner.qscale, inner.gscale, inner.L, inner.R, dxh, m=pr, n=pc,
                                bits=inner.bits)
    dx = torch.empty((T, lin.in_features), dtype=dx_dtype, device=DEV)
    K.hadamard_rows(dxh, dx, n_in=pc, n_out=lin.in_features, P=pc)
    return dx, dyh


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("T", [1, 5, 17])
@pytest.mark.parametrize("m,n,factors", _CASES)
def test_graph_forward_is_the_inference_forward_and_x_grad_the_three_entries(m, n, factors, T):
    lin = _lin(m, n, factors)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        x, dy = _xy(lin, T, dt)
        x = x.reshape(1, T, n).requires_grad_()             # leading dimensions are kept
        y = lin(x)
        assert y.grad_fn is not None and y.dtype == dt and y.shape == (1, T, m)
        with torch.no_grad():
            y0 = lin(x)
        assert y0.grad_fn is None and torch.equal(_bits(y0), _bits(y.detach()))
        y.backward(dy.reshape(1, T, m))
        want, _ = _backward_by_hand(lin, dy, dt)
        assert x.grad.dtype == dt and x.grad.shape == x.shape
        assert torch.equal(_bits(x.grad.reshape(T, n)), _bits(want)), dt
    assert not list(lin.parameters())


# ---------------------------------------------------------------------------- fp64 references
def _operands64(lin):
    """(c, L, R, sk, gs) of the inner layer in fp64; a coded factor dequantised as the kernel does."""
    from ee274_convexcaldera_llm_quantization_amd.linear import unpack_bytes
    inner = lin.inner
    k = 2 ** (inner.bits - 1) - 1
    c = unpack_bytes(inner.codes.cpu(), inner.bits)[:, :inner.in_features].numpy().astype(np.float64)
    L, R = (t.double().cpu().numpy() for t in inner.factors())
    sk = np.float64(np.float32(inner.qscale) / np.float32(k))
    return c, L, R, sk, np.float64(np.float32(inner.gscale))


def _hat64(v, cols, P):
    """H_P pad(v) / sqrt(P) of the rows of v (T, cols) in fp64."""
    X = np.zeros((v.shape[0], P))
    X[:, :cols] = v
    return HC.hadamard64(X, P) / np.sqrt(np.float64(P))


def _dx_ref_and_bar(lin, dy):
    """fp64 dy W for fp32 dy (T, m) (numpy fp64), W = (H1 W~ H2)[:m, :n], and the bar of the module
    docstring, (T, n)."""
    pr, pc = lin.padded_shape
    c, L, R, sk, gs = _operands64(lin)
    dyh = _hat64(dy, lin.out_features, pr)
    Wt = gs * (sk * c + L @ R)
    ref = _hat64(dyh @ Wt, pc, pc)[:, :lin.in_features]
    aW = np.abs(Wt)
    dyh16 = np.abs(dyh.astype(np.float16).astype(np.float64))
    A = gs * (sk * (dyh16 @ np.abs(c)) + (dyh16 @ np.abs(L)) @ np.abs(R))
    dxbar = (pr + lin.inner.rank + 32) * u24 * A
    bar_in = 1.01 * (np.log2(pr) + 2) * u24 * np.abs(dy).sum(1, keepdims=True) / np.sqrt(pr)      # per element of dy^
    inner_terms = 2.0 ** -11 * (np.abs(dyh) @ aW) + dxbar + bar_in * aW.sum(0)[None, :]
    dxh = dyh16 @ aW + dxbar                    # |dx^| as the second transform sums it
    bar_out = 1.01 * (np.log2(pc) + 2) * u24 * dxh.sum(1, keepdims=True) / np.sqrt(pc)
    return ref, inner_terms.sum(1, keepdims=True) / np.sqrt(pc) + bar_out + np.zeros((1, lin.in_features))


_FRACTIONS = []


@pytest.mark.parametrize("T", [1, 5, 17])
@pytest.mark.parametrize("m,n,factors", _CASES)
def test_x_grad_against_fp64_within_the_bar(m, n, factors, T):
    lin = _lin(m, n, factors)
    x, dy = _xy(lin, T)
    x.requires_grad_()
    lin(x).backward(dy)
    ref, bar = _dx_ref_and_bar(lin, dy.double().cpu().numpy())
    got = x.grad.double().cpu().numpy()
    frac = (np.abs(got - ref) / bar).max()
    _FRACTIONS.append(frac)
    print(f"m{m} n{n} {factors} T{T}: dx {frac:.4f} of the bar (largest so far {max(_FRACTIONS):.4f})")
    assert np.isfinite(got).all() and frac <= 1.0


def _times_h(X, P):
    """X (rows, P) fp64 torch -> X H_P / sqrt(P), differentiable (hadamard64's factorisation)."""
    import scipy.linalg
    b = min(P, 256)
    a = P // b
    Ha, Hb = (torch.from_numpy(scipy.linalg.hadamard(v).astype(np.float64)) for v in (a, b))
    return torch.matmul(Ha, X.reshape(-1, a, b) @ Hb).reshape(-1, P) / float(np.sqrt(np.float64(P)))


@pytest.mark.parametrize("T", [5, 17])
@pytest.mark.parametrize("m,n", SHAPES)
def test_inner_factor_gradients_against_fp64_autograd_through_h(m, n, T):
    lin = _lin(m, n)
    pr, pc = lin.padded_shape
    L0, R0 = lin.inner.L.clone(), lin.inner.R.clone()
    params = lin.enable_factor_training()
    assert [name for name, _ in lin.named_parameters()] == ["inner.L", "inner.R"] and lin.factors_trainable
    x, dy = _xy(lin, T)
    x.requires_grad_()
    y = lin(x)
    frozen = _lin(m, n)
    with torch.no_grad():
        assert torch.equal(y.detach(), frozen(x))           # no step yet: the frozen forward's bits
    y.backward(dy)
    want, dyh16 = _backward_by_hand(frozen, dy, torch.float32)
    assert torch.equal(x.grad, want)
    # fp64 autograd through H1 gs (Q + L R) H2
    c, _, _, sk, gs = _operands64(frozen)
    L = L0.double().cpu().requires_grad_()
    R = R0.double().cpu().requires_grad_()
    Wt = float(gs) * (torch.from_numpy(c) * float(sk) + L @ R)
    W = _times_h(_times_h(Wt, pc).t().contiguous(), pr).t()[:m, :n]       # H1 W~ H2: H is symmetric
    x64, dy64 = x.detach().double().cpu(), dy.double().cpu()
    ((x64 @ W.t()) * dy64).sum().backward()
    xh = torch.from_numpy(np.abs(_hat64(x64.numpy(), n, pc)))
    dyh = torch.from_numpy(np.abs(_hat64(dy64.numpy(), m, pr)))
    aL, aR = L.detach().abs(), R.detach().abs()
    barL = ((T + pc + 64) * u24 + 2.0 ** -9) * float(gs) * (dyh.t() @ (xh @ aR.t()))
    barR = ((T + pr + 64) * u24 + 2.0 ** -9) * float(gs) * ((dyh @ aL).t() @ xh)
    gL, gR = params[0].grad, params[1].grad
    assert gL.dtype == gR.dtype == torch.float32 and gL.shape == (pr, 8) and gR.shape == (8, pc)
    eL = ((gL.double().cpu() - L.grad).abs() / barL).max().item()
    eR = ((gR.double().cpu() - R.grad).abs() / barR).max().item()
    print(f"m{m} n{n} T{T}: dL worst {eL:.4f} bars, dR worst {eR:.4f} bars")
    assert eL <= 1 and eR <= 1
    lin.freeze_factors()
    assert torch.equal(lin.inner.L, L0) and torch.equal(lin.inner.R, R0) and not list(lin.parameters())


# ---------------------------------------------------------------------------- a tiny model
class _Tiny(torch.nn.Module):
    """Linear(24, 198) -> Hadamard (100 x 198, padded 128 x 256) -> ReLU -> coded factors (48, 100, 8)
    -> ReLU -> plain packed (33, 48, 8)."""

    def __init__(self):
        super().__init__()
        from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
        torch.manual_seed(3)
        self.front = torch.nn.Linear(24, 198)
        self.had = HL._layer(100, 198, 8, 2, "fp16", True, seed=31)
        rng = np.random.default_rng(32)
        c = torch.from_numpy(rng.integers(-1, 2, (48, 100)).astype(np.int8))
        self.coded = CalderaLinear.from_codes(
            c, None, None, None, qscale=0.05, gscale=1.7, bits=2,
            L_codes=(torch.from_numpy(rng.integers(-7, 8, (48, 8)).astype(np.int8)), 0.3, 4),
            R_codes=(torch.from_numpy(rng.integers(-1, 2, (8, 100)).astype(np.int8)), 0.3, 2))
        c = torch.from_numpy(rng.integers(-7, 8, (33, 48)).astype(np.int8))
        L = torch.from_numpy((0.15 * rng.standard_normal((33, 8))).astype(np.float16))
        R = torch.from_numpy((0.15 * rng.standard_normal((8, 48))).astype(np.float16))
        self.plain = CalderaLinear.from_codes(c, L, R, None, qscale=0.05, gscale=1.7, bits=4)

    def forward(self, x):
        return self.plain(torch.relu(self.coded(torch.relu(self.had(self.front(x))))))


# the steepest step that a CPU restatement in fp64 (every layer as its dense weight, the masters
# rounded to fp16 in each forward) still takes monotonically is far above this rate: the loss
# falls monotonically there at this rate, at a quarter of it and at four times it
TINY_LR = 0.01


def test_five_sgd_steps_through_every_packed_layer_kind():
    from ee274_convexcaldera_llm_quantization_amd import model as M
    net = _Tiny().to(DEV)
    keys = set(net.state_dict())
    g = torch.Generator().manual_seed(12)
    x = torch.randn(32, 24, generator=g).to(DEV)
    target = torch.randn(32, 33, generator=g).to(DEV)
    with pytest.raises(ValueError, match="without a backward"):
        M.prepare_factor_finetuning(net)
    params = M.prepare_factor_finetuning(net, hadamard=True, coded_factors="freeze")
    assert [id(p) for p in params] == [id(p) for p in (net.had.inner.L, net.had.inner.R, net.plain.L, net.plain.R)]
    assert not net.coded.factors_trainable and not list(net.coded.parameters())
    opt = torch.optim.SGD(params + list(net.front.parameters()), lr=TINY_LR)
    losses = []
    for step in range(5):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(net(x), target)
        loss.backward()
        if step == 0:       # the dense layer in front is reached through all three packed layers
            gw = net.front.weight.grad
            assert torch.isfinite(gw).all() and gw.abs().max() > 0 and (gw != 0).float().mean() > 0.5
            assert all(torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for p in params)
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        last = net(x)
        losses.append(torch.nn.functional.mse_loss(last, target).item())
    print("losses", " ".join(f"{v:.5f}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:]))
    tuned = net(x).detach()                                  # the last training forward (with a graph)
    assert torch.equal(tuned, last)
    M.finish_factor_finetuning(net)
    assert {name for name, _ in net.named_parameters()} == {"front.weight", "front.bias"}
    assert set(net.state_dict()) == keys and net.had.inner.L.dtype == torch.float16
    with torch.no_grad():
        y = net(x)
    assert torch.equal(y, tuned)
