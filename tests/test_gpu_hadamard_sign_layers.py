"""Signed HadamardCalderaLinear layers on the device, held to the unsigned layer on the same inner layer.
Every flip is exact, so with su, sv the layer's +-1 vectors and U the unsigned layer without a bias

    forward     signed(x)                 ==  su * U(sv * x)                  bit for bit, every dtype
    backward    signed: dx(x, dy)         ==  sv * U: dx(sv * x, su * dy)     bit for bit
                signed: dL, dR(x, dy)     ==  U: dL, dR(sv * x, su * dy)      bit for bit
    materialize signed.materialize()      ==  su[:, None] * U.materialize() * sv[None, :]

and the fp64 comparisons run at the bars of the unsigned layer's tests on those flipped operands (flips change
no magnitude): test_gpu_hadamard_linear.py's forward bar against x dense_weight()^T + bias,
test_gpu_hadamard_backward.py's dx bar and its factor-gradient bars against fp64 autograd through the signed
dense weight, test_gpu_linear_dequant.py's norm bar for materialize().

Shapes: (13, 200) -> padded (16, 256) and (100, 198) -> (128, 256): ragged in and out, one-wave transforms of
4, 32 and 64 lanes per row.  The transforms' other kernel forms are test_gpu_hadamard_signs.py's."""
import numpy as np
import pytest
import torch

import linear_glu_cases as UC
import test_gpu_hadamard_backward as HB
import test_gpu_hadamard_linear as HL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
u24 = 2.0 ** -24
SHAPES = [(13, 200), (100, 198)]
SEEDS = (11, 12)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _pair(m, n, bias=False, seeds=SEEDS, r=8, bits=2, seed=0):
    """(signed, unsigned): two layers on equal inner operands (built twice from one seed: no shared module)."""
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardCalderaLinear
    plain, twin = (HL._layer(m, n, r, bits, "fp16", bias, seed=seed) for _ in range(2))
    signed = HadamardCalderaLinear(twin.inner, n, m, twin.bias, sign_seeds=seeds).to(DEV)
    assert signed.sign_in.is_cuda and signed.sign_in.dtype == torch.int8
    return signed, plain


def _pm(lin):
    return lin.sign_out.float(), lin.sign_in.float()


@pytest.mark.parametrize("T", [1, 17])
@pytest.mark.parametrize("m,n", SHAPES)
@torch.no_grad()
def test_forward_is_the_unsigned_layer_between_two_flips(m, n, T):
    signed, plain = _pair(m, n)
    su, sv = _pm(signed)
    g = torch.Generator().manual_seed(T + n)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        x = torch.randn(2, T, n, generator=g).to(dt).to(DEV)
        y = signed(x)
        want = plain(x * sv.to(dt)) * su.to(dt)
        assert y.dtype == dt and y.shape == (2, T, m) and torch.isfinite(y).all()
        assert torch.equal(_bits(y), _bits(want)), dt
        assert not torch.equal(_bits(y), _bits(plain(x)))


_FRACTIONS = []


@pytest.mark.parametrize("T", [1, 17])
@pytest.mark.parametrize("m,n", SHAPES)
@torch.no_grad()
def test_forward_with_bias_against_fp64_dense_weight(m, n, T):
    signed, _ = _pair(m, n, bias=True)
    _, sv = _pm(signed)
    x = np.random.default_rng(T + n).standard_normal((T, n)).astype(np.float32)
    ref = x.astype(np.float64) @ signed.dense_weight().double().cpu().numpy().T + signed.bias.double().cpu().numpy()
    y = signed(torch.from_numpy(x).to(DEV)).double().cpu().numpy()
    bar = HL._bar(signed, x.astype(np.float64) * sv.double().cpu().numpy()[None, :])      # what the inner layer sees
    frac = float((np.abs(y - ref) / bar).max())
    _FRACTIONS.append(frac)
    print(f"m{m} n{n} T{T}: {frac:.4f} of the bar (largest so far {max(_FRACTIONS):.4f})")
    assert np.isfinite(y).all() and frac <= 1.0


@pytest.mark.parametrize("T", [1, 17])
@pytest.mark.parametrize("m,n", SHAPES)
def test_x_grad_is_the_unsigned_layers_between_two_flips_and_within_its_bar(m, n, T):
    signed, plain = _pair(m, n, bias=True)
    su, sv = _pm(signed)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        x, dy = HB._xy(signed, T, dt)
        xs = x.clone().requires_grad_()
        y = signed(xs)
        with torch.no_grad():
            assert torch.equal(_bits(y.detach()), _bits(signed(x)))            # the graph forward is the inference one
        y.backward(dy)
        xp = (x * sv.to(dt)).requires_grad_()
        plain(xp).backward(dy * su.to(dt))
        assert xs.grad.dtype == dt and torch.equal(_bits(xs.grad), _bits(xp.grad * sv.to(dt))), dt
        if dt == torch.float32:
            ref, bar = HB._dx_ref_and_bar(plain, (dy * su).double().cpu().numpy())
            ref = ref * sv.double().cpu().numpy()[None, :]
            frac = float((np.abs(xs.grad.double().cpu().numpy() - ref) / bar).max())
            print(f"m{m} n{n} T{T}: dx {frac:.4f} of the bar")
            assert frac <= 1.0
    assert not list(signed.parameters())


@pytest.mark.parametrize("m,n", SHAPES)
def test_factor_gradients_stay_in_the_signed_basis(m, n):
    T = 5
    signed, plain = _pair(m, n, bias=True)
    su, sv = _pm(signed)
    pr, pc = signed.padded_shape
    L0, R0 = signed.inner.L.clone(), signed.inner.R.clone()
    ps, pp = signed.enable_factor_training(), plain.enable_factor_training()
    x, dy = HB._xy(signed, T)
    signed(x).backward(dy)
    plain(x * sv).backward(dy * su)
    assert torch.equal(ps[0].grad, pp[0].grad) and torch.equal(ps[1].grad, pp[1].grad)
    # fp64 autograd through su (H1 gs (Q + L R) H2)[:m, :n] sv, test_gpu_hadamard_backward.py's bars
    c, _, _, sk, gs = HB._operands64(plain)
    L, R = L0.double().cpu().requires_grad_(), R0.double().cpu().requires_grad_()
    Wt = float(gs) * (torch.from_numpy(c) * float(sk) + L @ R)
    W = HB._times_h(HB._times_h(Wt, pc).t().contiguous(), pr).t()[:m, :n]
    W = su.double().cpu()[:, None] * W * sv.double().cpu()[None, :]
    x64, dy64 = x.double().cpu(), dy.double().cpu()
    ((x64 @ W.t()) * dy64).sum().backward()
    # |x^| and |dy^| of the signed basis: what the kernels' fp16 x^ and dy^ round
    xh = torch.from_numpy(np.abs(HB._hat64((x64 * sv.double().cpu()).numpy(), n, pc)))
    dyh = torch.from_numpy(np.abs(HB._hat64((dy64 * su.double().cpu()).numpy(), m, pr)))
    aL, aR = L.detach().abs(), R.detach().abs()
    barL = ((T + pc + 64) * u24 + 2.0 ** -9) * float(gs) * (dyh.t() @ (xh @ aR.t()))
    barR = ((T + pr + 64) * u24 + 2.0 ** -9) * float(gs) * ((dyh @ aL).t() @ xh)
    eL = ((ps[0].grad.double().cpu() - L.grad).abs() / barL).max().item()
    eR = ((ps[1].grad.double().cpu() - R.grad).abs() / barR).max().item()
    print(f"m{m} n{n}: dL worst {eL:.4f} bars, dR worst {eR:.4f} bars")
    assert eL <= 1 and eR <= 1
    signed.freeze_factors()
    assert torch.equal(signed.inner.L, L0) and not list(signed.parameters())


@pytest.mark.parametrize("m,n", SHAPES)
@torch.no_grad()
def test_materialize_against_dense_weight(m, n):
    """As test_gpu_linear_dequant.py holds the unsigned layer: both against H1 inner.dense_weight() H2 redone in
    fp64 with the signs, under norm bars (H is orthogonal): dense_weight() within that file's 400 2^-24 ||A||_F,
    materialize() within (2 (r + 8) + log2 pc + log2 pr + 2) 2^-24 ||A||_F -- two weights within (r + 8) 2^-24 A
    of the truth, and two fp32 transforms of log2 P + 1 roundings each -- A = gs (|Q| + |L| |R|)."""
    from ee274_convexcaldera_llm_quantization_amd.model import normalized_hadamard
    signed, plain = _pair(m, n)
    su, sv = _pm(signed)
    pr, pc = signed.padded_shape
    Wm = signed.materialize(torch.float32)
    assert tuple(Wm.shape) == (m, n) and Wm.is_contiguous()
    assert torch.equal(_bits(Wm), _bits(su[:, None] * plain.materialize(torch.float32) * sv[None, :]))
    c, L, R, sk, gs = HL._operands64(signed)
    Anorm = float(np.linalg.norm(gs * (sk * np.abs(c) + np.abs(L) @ np.abs(R))))
    Wt = signed.inner.dense_weight().double()
    W = (normalized_hadamard(pr, DEV, torch.float64) @ Wt @ normalized_hadamard(pc, DEV, torch.float64))[:m, :n]
    W = (su.double()[:, None] * W * sv.double()[None, :]).cpu().numpy()
    assert np.abs(W - signed.dense_weight().double().cpu().numpy()).max() <= 400 * u24 * Anorm
    wbar = (2 * (signed.inner.rank + 8) + np.log2(pc) + np.log2(pr) + 2) * u24 * Anorm
    werr = np.abs(Wm.double().cpu().numpy() - W).max()
    print(f"m{m} n{n}: materialize worst {werr / wbar:.4f} bars")
    assert werr <= wbar
    assert torch.equal(signed.materialize(), Wm.to(torch.float16))
    out = torch.empty((m, n), dtype=torch.bfloat16, device=DEV)
    assert torch.equal(signed.materialize(out=out), Wm.to(torch.bfloat16))


def test_unpack_packed_layers_works_unchanged():
    from ee274_convexcaldera_llm_quantization_amd import model as M
    signed, _ = _pair(13, 200, bias=True)
    net = torch.nn.Sequential(signed)
    W = signed.materialize()
    assert M.unpack_packed_layers(net) == ["0"]
    assert type(net[0]) is torch.nn.Linear and torch.equal(net[0].weight.detach(), W)


@torch.no_grad()
def test_decode_forward_in_a_captured_graph():
    signed, _ = _pair(13, 200, bias=True)
    x = torch.randn(1, 200, generator=torch.Generator().manual_seed(1)).half().to(DEV)
    xs = torch.zeros_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        signed(xs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = signed(xs)
    xs.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ys, signed(x))


# ---------------------------------------------------------------------------- groups and fused blocks
def _signed_layer(m, n, seeds, bias=False, seed=0, r=8):
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardCalderaLinear
    base = HL._layer(m, n, r, 2, "fp16", bias, seed=seed)
    return HadamardCalderaLinear(base.inner, n, m, base.bias, sign_seeds=seeds).to(DEV)


def _blocks():
    """Two toy blocks: q / k / v with GQA's narrower k and v (two padded widths), and a gate / up pair; within a
    block every layer shares seed_in, seed_out is per layer."""
    out = []
    for b in range(2):
        s_in = 40 + b
        qkv = [_signed_layer(m, 198, (10 * b + i, s_in), bias=i == 2, seed=10 * b + i)
               for i, m in enumerate((100, 13, 13))]
        mlp = [_signed_layer(200, 198, (10 * b + 5 + i, s_in), bias=i == 0, seed=10 * b + 5 + i) for i in range(2)]
        out.append((qkv, mlp))
    return out


@pytest.mark.parametrize("T", [1, 17])
@torch.no_grad()
def test_signed_group_and_fused_block_keep_the_members_bits(T):
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardGatedMLP, HadamardLinearGroup
    for b, (qkv, (gate, up)) in enumerate(_blocks()):
        g = torch.Generator().manual_seed(T + b)
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            x = torch.randn(T, 198, generator=g).to(dt).to(DEV)
            alone = [lin(x) for lin in qkv]
            group = HadamardLinearGroup(qkv)
            try:
                assert group._grouped(x)
                for i, (y, want) in enumerate(zip(group(x), alone)):
                    assert torch.isfinite(y).all() and torch.equal(_bits(y), _bits(want)), (b, dt, i)
                assert all(torch.equal(_bits(lin(x)), _bits(want)) for lin, want in zip(qkv, alone))   # transparent
            finally:
                group.dissolve()
        x = torch.randn(T, 198, generator=g).to(DEV)
        vg, vu = gate(x), up(x)                                            # fp32 x: the members' own fp32 outputs
        ident = HadamardGatedMLP(gate, up, torch.nn.Identity(), act="identity")
        assert ident._fused(x) and torch.equal(_bits(ident(x)), _bits(vg * vu))
        silu = HadamardGatedMLP(gate, up, torch.nn.Identity())
        h = silu(x)
        hs, bar32, _ = UC.epilogue_reference(UC.ACT_SILU, vg.cpu().numpy(), vu.cpu().numpy())
        frac = float((np.abs(h.double().cpu().numpy() - hs) / bar32).max())
        print(f"block {b} T{T}: {frac:.4f} of the epilogue bar")
        assert h.dtype == torch.float32 and frac <= 1.0
        for dt in (torch.float16, torch.bfloat16):                         # exact in dt: the same pre-activations
            xd = x.to(dt)
            assert torch.equal(_bits(silu(xd)), _bits(silu(xd.float()).to(dt)))


# ---------------------------------------------------------------------------- end to end
@torch.no_grad()
def test_tiny_model_with_hadamard_signs_through_a_results_file(tmp_path):
    from ee274_convexcaldera_llm_quantization_amd import model as M
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardCalderaLinear
    from ee274_convexcaldera_llm_quantization_amd.sharding import load_results, save_results
    qp = M.driver_params(16)
    qp.iters = 2
    orig, packed, fresh = HL._tiny_model(1), HL._tiny_model(1), HL._tiny_model(1)
    rep = M.apply_caldera_quantization(packed, None, qp, packed=True, packed_hadamard=True, hadamard_signs=3)
    assert all(o.applied for o in rep.layers) and len(rep.layers) == 6
    mods, mods_o = dict(packed.named_modules()), dict(orig.named_modules())
    results = []
    for o in rep.layers:
        lin = mods[o.name]
        assert isinstance(lin, HadamardCalderaLinear)
        assert lin.sign_seeds == M.hadamard_sign_seeds(3, o.name, lin.in_features)
        # the gate judged the weight the layer applies: the recovered error is dense_weight()'s, up to the fp16
        # rounding of the factors (test_gpu_hadamard_linear.py: below 2e-3 of ||W||, so of the error as well)
        W = mods_o[o.name].weight.float()
        err = float(torch.linalg.norm(W - lin.dense_weight()) / torch.linalg.norm(W))
        print(f"{o.name}: gate {o.rel_error:.6f}, dense_weight() {err:.6f}")
        assert abs(err - o.rel_error) < 2e-3 and 0 < o.rel_error < 0.99
        results.append(lin.to_result(o.name))
    path = str(tmp_path / "layers.cqrs")
    save_results(path, results)
    loaded = load_results(path)
    assert all(r.extra["hadamard_signs"] == list(mods[r.name].sign_seeds) for r in loaded)
    assert M.apply_packed_results(fresh, loaded) == [o.name for o in rep.layers]
    mods_f = dict(fresh.named_modules())
    g = torch.Generator().manual_seed(5)
    for o in rep.layers:
        a, b = mods[o.name], mods_f[o.name]
        assert isinstance(b, HadamardCalderaLinear) and b.sign_seeds == a.sign_seeds
        assert torch.equal(a.sign_in, b.sign_in) and torch.equal(a.sign_out, b.sign_out)
        for dt in (torch.float32, torch.float16):
            x = torch.randn(3, a.in_features, generator=g).to(dt).to(DEV)
            assert torch.equal(_bits(a(x)), _bits(b(x))), (o.name, dt)
    # q_proj and up_proj of a block read activations of one width: one seed_in
    for blk in (17, 18):
        base = f"language_model.model.layers.{blk}"
        assert mods[f"{base}.self_attn.q_proj"].sign_seeds[1] == mods[f"{base}.mlp.up_proj"].sign_seeds[1]
