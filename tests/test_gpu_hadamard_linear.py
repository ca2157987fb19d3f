"""HadamardCalderaLinear on the device: the forward is exactly its three public entries, exact
and random end-to-end cases against fp64, a tiny model quantised with packed_hadamard=True
beside the dense Hadamard write-back, a results file, dtype casts and graph capture.

The random bar, elementwise in fp64 (x^ = H2 pad(x) exactly, W~ the inner layer's dense weight,
pr x pc the padded grid):

    bar[i] = (1 / sqrt(pr)) sum_i' ( 2^-11 sum_j |x^_j| |W~_i'j|  +  linbar_i' )  +  the two transform bars

2^-11 |x^| is the fp16 rounding of the transformed activations, linbar the worst-case bound of
linear_cases.py for the inner layer on the fp16 x^ it receives ((pc + r + 32) 2^-24 A), and each
transform adds hadamard_cases' 1.01 (log2 P + 2) 2^-24 sum |input| / sqrt(P): the input
transform's is carried through |W~| and H1 like the fp16 rounding, the output transform's is on
the inner layer's fp32 result.  fp32 x, so the output is not rounded again."""
import numpy as np
import pytest
import torch

import hadamard_cases as HC
import linear_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
u24 = 2.0 ** -24


def _K():
    from ee274_convexcaldera_llm_quantization_amd import _lib as K
    K.load()
    return K


def _pow2(n):
    return 1 << (n - 1).bit_length()


def _layer(m, n, r, bits, factors="fp16", bias=False, kind="random", seed=0):
    """A HadamardCalderaLinear of an (m, n) weight from host-seeded operands on the padded grid,
    on the device, and the operands."""
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear, HadamardCalderaLinear
    pr, pc = _pow2(m), _pow2(n)
    rng = np.random.default_rng(seed + 1000 * m + n + 7 * r + bits)
    k = 2 ** (bits - 1) - 1
    c = torch.from_numpy(rng.integers(-k, k + 1, (pr, pc)).astype(np.int8))
    kw = {}
    if kind == "exact":
        L = torch.from_numpy(rng.integers(-2, 3, (pr, r)).astype(np.float32))
        R = torch.from_numpy(rng.integers(-2, 3, (r, pc)).astype(np.float32))
        s, gs = k / 2, 4.0
        b = torch.from_numpy((rng.integers(-8, 9, m) * 0.5).astype(np.float32)) if bias else None
    else:
        L = torch.from_numpy((0.15 * rng.standard_normal((pr, r))).astype(np.float32))
        R = torch.from_numpy((0.15 * rng.standard_normal((r, pc))).astype(np.float32))
        s, gs = 0.05, 1.7
        b = torch.from_numpy(rng.standard_normal(m).astype(np.float32)) if bias else None
    if r == 0:
        L = R = None
    elif factors == "coded4":
        kw = dict(L_codes=(torch.from_numpy(rng.integers(-7, 8, (pr, r)).astype(np.int8)), 0.6, 4),
                  R_codes=(torch.from_numpy(rng.integers(-7, 8, (r, pc)).astype(np.int8)), 0.4, 4))
        L = R = None
    inner = CalderaLinear.from_codes(c, L, R, None, qscale=s, gscale=gs, bits=bits, **kw)
    return HadamardCalderaLinear(inner, n, m, b).to(DEV)


def _by_hand(lin, x2):
    """The three public entries on x2 (T, n): transform, the inner layer's entry, transform."""
    K = _K()
    inner = lin.inner
    pr, pc = lin.padded_shape
    T = x2.shape[0]
    xh = torch.empty((T, pc), dtype=torch.float16, device=DEV)
    K.hadamard_rows(x2, xh, n_in=lin.in_features, n_out=pc, P=pc)
    y32 = torch.empty((T, pr), dtype=torch.float32, device=DEV)
    if inner.rank and (inner.L_codes is not None or inner.R_codes is not None):
        K.linear_packed_forward(xh, inner.codes, inner.qscale, inner.gscale, inner.L, inner.R, None, y32, m=pr, n=pc,
                                bits=inner.bits, r=inner.rank,
                                L_codes=(inner.L_codes, inner.lscale, inner.L_bits),
                                R_codes=(inner.R_codes, inner.rscale, inner.R_bits))
    else:
        K.linear_forward(xh, inner.codes, inner.qscale, inner.gscale, inner.L if inner.rank else None,
                         inner.R if inner.rank else None, None, y32, m=pr, n=pc, bits=inner.bits)
    y = torch.empty((T, lin.out_features), dtype=x2.dtype, device=DEV)
    K.hadamard_rows(y32, y, n_in=pr, n_out=lin.out_features, P=pr, bias=lin.bias)
    return y


# ---------------------------------------------------------------------------- plumbing
@pytest.mark.parametrize("T", [1, 16, 17])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("factors,r", [("fp16", 8), ("coded4", 8), ("fp16", 0)], ids=["fp16", "coded4", "r0"])
@pytest.mark.parametrize("bits", [2, 4])
@pytest.mark.parametrize("m,n", [(48, 198), (80, 898)])
def test_forward_is_its_three_entries(m, n, bits, factors, r, bias, T):
    lin = _layer(m, n, r, bits, factors, bias)
    assert lin.padded_shape == {(48, 198): (64, 256), (80, 898): (128, 1024)}[(m, n)]
    g = torch.Generator().manual_seed(T + m)
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        x = torch.randn(2, T, n, generator=g).to(dt).to(DEV)       # leading dimensions are kept
        y = lin(x)
        assert y.dtype == dt and y.shape == (2, T, m)
        hand = _by_hand(lin, x.reshape(-1, n))
        assert torch.equal(y.reshape(-1, m).view(torch.int16 if dt != torch.float32 else torch.int32),
                           hand.view(torch.int16 if dt != torch.float32 else torch.int32)), dt
    with pytest.raises(ValueError, match="last dimension"):
        lin(torch.zeros(2, n + 1, device=DEV))


# ---------------------------------------------------------------------------- fp64 references
def _operands64(lin):
    """(c, L, R, sk, gs) of the inner layer in fp64 from its buffers (fp16 factors)."""
    from ee274_convexcaldera_llm_quantization_amd.linear import unpack_bytes
    inner = lin.inner
    k = 2 ** (inner.bits - 1) - 1
    c = unpack_bytes(inner.codes.cpu(), inner.bits)[:, :inner.in_features].numpy().astype(np.float64)
    r = inner.rank
    L = inner.L.double().cpu().numpy() if r else np.zeros((inner.out_features, 0))
    R = inner.R.double().cpu().numpy() if r else np.zeros((0, inner.in_features))
    sk = np.float64(np.float32(inner.qscale) / np.float32(k))
    return c, L, R, sk, np.float64(np.float32(inner.gscale))


def _xhat64(lin, x):
    pr, pc = lin.padded_shape
    X = np.zeros((x.shape[0], pc))
    X[:, :lin.in_features] = x
    return HC.hadamard64(X, pc) / np.sqrt(np.float64(pc))


def _bar(lin, x):
    """The elementwise bar of the module docstring for fp32 x (T, n) (numpy fp64), (T, m)."""
    pr, pc = lin.padded_shape
    c, L, R, sk, gs = _operands64(lin)
    xh = np.abs(_xhat64(lin, x))
    Wt = np.abs(gs * (sk * c + L @ R))
    xh16 = np.abs(_xhat64(lin, x).astype(np.float16).astype(np.float64))
    A = gs * (sk * (xh16 @ np.abs(c).T) + (xh16 @ np.abs(R).T) @ np.abs(L).T)
    linbar = (pc + lin.inner.rank + 32) * u24 * A
    bar_in = 1.01 * (np.log2(pc) + 2) * u24 * np.abs(x).sum(1, keepdims=True) / np.sqrt(pc)       # per element of x^
    inner_terms = 2.0 ** -11 * (xh @ Wt.T) + linbar + bar_in * Wt.sum(1)[None, :]
    # |y32| <= |x^16| |W~|^T + linbar: what the output transform sums
    y32 = xh16 @ Wt.T + linbar
    bar_out = 1.01 * (np.log2(pr) + 2) * u24 * y32.sum(1, keepdims=True) / np.sqrt(pr)
    return inner_terms.sum(1, keepdims=True) / np.sqrt(pr) + bar_out + np.zeros((1, lin.out_features))


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("bits", [2, 4])
@pytest.mark.parametrize("m,n,T", [(12, 60, 5), (50, 198, 17), (12, 198, 1), (50, 60, 16)])
def test_exact_end_to_end(m, n, T, bits, bias):
    """pc in {64, 256}, pr in {16, 64}: x with at most 8 nonzeros of +-1..+-4 per row makes H2 x
    exact in fp16; integer codes with s / k = 0.5, integer L, R in -2..2, gs = 4: every
    intermediate is a dyadic rational below 2^24 units (asserted), so y matches fp64 bit for bit."""
    lin = _layer(m, n, 4, bits, bias=bias, kind="exact")
    pr, pc = lin.padded_shape
    rng = np.random.default_rng(T * 31 + n)
    x = np.zeros((T, n), dtype=np.float32)
    for t in range(T):
        j = rng.choice(n, size=8, replace=False)
        x[t, j] = rng.integers(1, 5, 8) * rng.choice([-1, 1], 8)
    xh = _xhat64(lin, x)
    assert np.array_equal(xh, xh.astype(np.float16).astype(np.float64))
    c, L, R, sk, gs = _operands64(lin)
    assert sk == 0.5 and gs == 4.0
    # x^ counts in units of 1 / sqrt(pc), the inner layer's result in 1 / (2 sqrt(pc)); the output
    # transform's partial sums are bounded by the row's sum of magnitudes in those units, and its
    # scaled result (+ a bias of at most 4) by the same count of units 1 / (2 sqrt(pc) sqrt(pr))
    A = gs * (sk * (np.abs(xh) @ np.abs(c).T) + (np.abs(xh) @ np.abs(R).T) @ np.abs(L).T)
    assert (A.sum(1).max() + 4.0 * np.sqrt(pr)) * 2 * np.sqrt(pc) < 2 ** 24
    y32 = gs * (sk * (xh @ c.T) + (xh @ R.T) @ L.T)
    ref = (HC.hadamard64(y32, pr) / np.sqrt(np.float64(pr)))[:, :m]
    if lin.bias is not None:
        ref = ref + lin.bias.double().cpu().numpy()
    y = lin(torch.from_numpy(x).to(DEV))
    assert y.dtype == torch.float32 and np.array_equal(y.double().cpu().numpy(), ref)


_FRACTIONS = []


@pytest.mark.parametrize("T", [1, 16, 17, 64])
@pytest.mark.parametrize("bits,r", [(2, 8), (4, 8), (2, 0)])
@pytest.mark.parametrize("m,n", [(48, 198), (80, 898)])
def test_random_end_to_end_within_the_bar(m, n, bits, r, T):
    lin = _layer(m, n, r, bits, bias=True)
    x = np.random.default_rng(T + n).standard_normal((T, n)).astype(np.float32)
    Wd = lin.cpu().dense_weight().double().numpy()
    lin.to(DEV)
    ref = x.astype(np.float64) @ Wd.T + lin.bias.double().cpu().numpy()
    y = lin(torch.from_numpy(x).to(DEV)).double().cpu().numpy()
    bar = _bar(lin, x.astype(np.float64))
    frac = (np.abs(y - ref) / bar).max()
    _FRACTIONS.append(frac)
    print(f"m{m} n{n} b{bits} r{r} T{T}: {frac:.4f} of the bar (largest so far {max(_FRACTIONS):.4f})")
    assert np.isfinite(y).all() and frac <= 1.0


# ---------------------------------------------------------------------------- a real run
def _tiny_model(seed=0):
    from test_model_host import TinyLlava
    torch.manual_seed(seed)
    m = TinyLlava(n_layers=19, h=512, i=640)
    for p in m.parameters():
        torch.nn.init.normal_(p, std=0.02)
    return m.to(DEV)


@torch.no_grad()
def test_tiny_model_packed_hadamard_beside_the_dense_write_back(tmp_path):
    from ee274_convexcaldera_llm_quantization_amd import model as M
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardCalderaLinear
    from ee274_convexcaldera_llm_quantization_amd.sharding import load_results, save_results
    qp = M.driver_params(16)
    qp.iters = 2
    dense, packed, fresh = _tiny_model(1), _tiny_model(1), _tiny_model(1)
    rep_d = M.apply_caldera_quantization(dense, None, qp, hadamard=True, hadamard_gate=True)
    rep_p = M.apply_caldera_quantization(packed, None, qp, packed=True, packed_hadamard=True)
    assert [(o.name, o.applied) for o in rep_d.layers] == [(o.name, o.applied) for o in rep_p.layers]
    assert all(o.applied for o in rep_p.layers) and len(rep_p.layers) == 6
    assert {o.shape for o in rep_p.layers} == {(512, 512), (640, 512), (512, 640)}     # two of three are padded
    for attr in ("quantized_param_count", "unquantized_language_param_count", "vision_param_count", "total_bits"):
        assert getattr(rep_d, attr) == getattr(rep_p, attr) and rep_p.quantized_param_count > 0
    for a, b in zip(rep_d.layers, rep_p.layers):
        assert abs(a.rel_error - b.rel_error) < 1e-6
    mods_p, mods_d = dict(packed.named_modules()), dict(dense.named_modules())
    g = torch.Generator().manual_seed(5)
    results, worst = [], 0.0
    for o in rep_p.layers:
        lin = mods_p[o.name]
        assert isinstance(lin, HadamardCalderaLinear) and (lin.out_features, lin.in_features) == o.shape
        x = torch.randn(9, lin.in_features, generator=g)
        y = lin(x.to(DEV)).double().cpu().numpy()
        ref = torch.nn.functional.linear(x.double(), lin.dense_weight().double().cpu(),
                                         None if lin.bias is None else lin.bias.double().cpu()).numpy()
        frac = (np.abs(y - ref) / _bar(lin, x.double().numpy())).max()
        worst = max(worst, frac)
        assert frac <= 1.0, (o.name, frac)
        # the packed layer applies what the dense branch wrote back, up to the factors' fp16 rounding
        Wd = mods_d[o.name].weight.float()
        assert float(torch.linalg.norm(lin.dense_weight() - Wd) / torch.linalg.norm(Wd)) < 2e-3
        results.append(lin.to_result(o.name))
    print(f"tiny model: largest fraction of the bar {worst:.4f}")
    # through a results file into a fresh model: the same layers, the same bits
    path = str(tmp_path / "layers.cqrs")
    save_results(path, results)
    assert M.apply_packed_results(fresh, load_results(path)) == [o.name for o in rep_p.layers]
    mods_f = dict(fresh.named_modules())
    x = torch.randn(3, 512, generator=g).to(DEV)
    for o in rep_p.layers:
        if o.shape[1] == 512:
            assert isinstance(mods_f[o.name], HadamardCalderaLinear)
            assert torch.equal(mods_f[o.name](x), mods_p[o.name](x)), o.name


# ---------------------------------------------------------------------------- the rest
def test_module_survives_dtype_casts_of_the_model():
    lin = _layer(48, 198, 8, 2, bias=True)
    x = torch.randn(5, 198, generator=torch.Generator().manual_seed(0)).half().to(DEV)
    before = {key: v.clone() for key, v in lin.state_dict().items() if torch.is_tensor(v)}
    y16, ybf = lin(x), lin(x.bfloat16())
    for cast in (lambda mod: mod.half(), lambda mod: mod.to(torch.bfloat16)):
        cast(lin)
        for key, v in lin.state_dict().items():
            if torch.is_tensor(v):
                assert v.dtype == before[key].dtype and torch.equal(v, before[key]), key
        assert torch.equal(lin(x), y16) and torch.equal(lin(x.bfloat16()), ybf)
    assert y16.dtype == torch.float16 and ybf.dtype == torch.bfloat16
    # the half outputs are the fp32 forward's value rounded once (x is exact in all three types)
    assert torch.equal(lin(x.float()).half(), y16)


@pytest.mark.parametrize("m,n", [(48, 198), (4000, 4096)])
def test_decode_forward_in_a_captured_graph(m, n):
    """No allocation inside the entries and no synchronisation: a captured T = 1 forward replays
    to the bits of the eager one.  (4000, 4096) is the one forward at a real layer's size (16 chunks
    of 2-bit codes, two per wave), so there the eager result is also held against fp64: the fp32
    forward of the same x under _bar, and the fp16 forward as that result rounded once.  At this
    size _bar is wide (its 2^-11 term sums 4096 x 4096 magnitudes: a build whose waves multiply
    their second chunk with the x of their first measured 0.59 of it), so the inner layer is also
    checked on its own: its result on the fp16 x^ it receives, against fp64 under the bar of
    linear_cases.py, output by output (that build: 102 bars)."""
    lin = _layer(m, n, 8, 2, bias=True)
    x = torch.randn(1, n, generator=torch.Generator().manual_seed(1)).half().to(DEV)
    if n == 4096:
        ref = torch.nn.functional.linear(x.double().cpu(), lin.dense_weight().double().cpu(),
                                         lin.bias.double().cpu()).numpy()
        y32 = lin(x.float())
        frac = (np.abs(y32.double().cpu().numpy() - ref) / _bar(lin, x.double().cpu().numpy())).max()
        print(f"m{m} n{n}: {frac:.4f} of the bar")
        assert torch.isfinite(y32).all() and frac <= 1.0
        assert torch.equal(lin(x), y32.half())
        pr, pc = lin.padded_shape
        xh = torch.empty((1, pc), dtype=torch.float16, device=DEV)
        _K().hadamard_rows(x, xh, n_in=n, n_out=pc, P=pc)
        c, L, R, sk, gs = _operands64(lin)
        xh64 = xh.double().cpu().numpy()
        ref_in = gs * (sk * (xh64 @ c.T) + (xh64 @ R.T) @ L.T)
        A = gs * (sk * (np.abs(xh64) @ np.abs(c).T) + (np.abs(xh64) @ np.abs(R).T) @ np.abs(L).T)
        frac_in = (np.abs(lin.inner(xh.float()).double().cpu().numpy() - ref_in)
                   / ((pc + lin.inner.rank + 32) * u24 * A)).max()
        print(f"m{m} n{n}: the inner layer {frac_in:.4f} of its bar")
        assert frac_in <= 1.0
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
