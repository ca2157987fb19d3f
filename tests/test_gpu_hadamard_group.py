"""The grouped and gated Hadamard launches on the device: cq_hadamard_group_rows against cq_hadamard_rows bit
for bit, cq_hadamard_glu_rows against the two cq_hadamard_rows fp32 outputs (identity: bit for bit; silu:
the epilogue bar of linear_glu_cases.py; a narrow h: the fp32 h rounded once), HadamardLinearGroup against
its members alone, HadamardGatedMLP against its members and fp64, graph capture, and a tiny model
quantised with packed_hadamard=True.

Every buffer is NaN-filled including the padding of its row stride; the comparisons are on the whole
buffers' bits, so a read of the padding would poison an output and a write to it would show."""
import numpy as np
import pytest
import torch

import hadamard_group_cases as GC
import linear_glu_cases as UC
from hadamard_group_cases import ACT_IDENTITY, ACT_SILU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
u24 = 2.0 ** -24


def _K():
    from ee274_convexcaldera_llm_quantization_amd import _lib as K
    K.load()
    return K


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _padded(rows, cols, pad, dt, values=None):
    """(buffer (rows, cols + pad) NaN-filled, its [:, :cols] view holding `values`)."""
    buf = torch.full((rows, cols + pad), float("nan"), dtype=dt, device=DEV)
    view = buf[:, :cols]
    if values is not None:
        view.copy_(torch.from_numpy(values).to(dt))
    return buf, view


# ---------------------------------------------------------------------------- the group entry
@pytest.mark.parametrize("case", GC.GROUP, ids=lambda c: c.id)
def test_group_entry_equals_the_single_entry_bit_for_bit(case):
    K = _K()
    d = GC.group_inputs(case)
    grouped, alone, bufs = [], [], []
    for mem, inp in zip(case.members, d):
        _, x = _padded(case.rows, mem.n_in, mem.pad_x, DT[mem.xdt], inp["x"])
        bias = None if inp["bias"] is None else torch.from_numpy(inp["bias"]).to(DEV)
        yg_buf, yg = _padded(case.rows, mem.n_out, mem.pad_y, DT[mem.ydt])
        ya_buf, ya = _padded(case.rows, mem.n_out, mem.pad_y, DT[mem.ydt])
        grouped.append(dict(x=x, y=yg, n_in=mem.n_in, n_out=mem.n_out, P=case.P, bias=bias))
        alone.append(dict(x=x, y=ya, n_in=mem.n_in, n_out=mem.n_out, P=case.P, bias=bias))
        bufs.append((yg_buf, ya_buf, mem))
    K.hadamard_group_rows(grouped)
    for a in alone:
        K.hadamard_rows(a["x"], a["y"], n_in=a["n_in"], n_out=a["n_out"], P=a["P"], bias=a["bias"])
    torch.cuda.synchronize()
    for i, (yg_buf, ya_buf, mem) in enumerate(bufs):
        assert torch.isfinite(ya_buf[:, :mem.n_out]).all(), i
        assert torch.equal(_bits(yg_buf), _bits(ya_buf)), f"member {i}"
        assert torch.isnan(yg_buf[:, mem.n_out:]).all(), f"member {i}: written outside [0, n_out)"


def test_group_entry_skips_a_member_with_nothing_to_write():
    K = _K()
    x = torch.randn(5, 64, device=DEV)
    y0, y2 = (torch.full((5, 64), float("nan"), device=DEV) for _ in range(2))
    empty = torch.empty((5, 0), device=DEV)
    K.hadamard_group_rows([dict(x=x, y=y0, n_in=64, n_out=64, P=64), dict(x=x, y=empty, n_in=64, n_out=0, P=64),
                           dict(x=x[:, :60], y=y2, n_in=60, n_out=64, P=64)])
    w0, w2 = torch.empty_like(y0), torch.empty_like(y2)
    K.hadamard_rows(x, w0, n_in=64, n_out=64, P=64)
    K.hadamard_rows(x[:, :60], w2, n_in=60, n_out=64, P=64)
    assert torch.equal(y0, w0) and torch.equal(y2, w2)
    K.hadamard_group_rows([dict(x=x, y=empty, n_in=64, n_out=0, P=64)])      # nothing to launch
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- the gated entry
_WORST = []


@pytest.mark.parametrize("act", [ACT_IDENTITY, ACT_SILU], ids=["identity", "silu"])
@pytest.mark.parametrize("case", GC.GLU, ids=lambda c: c.id)
def test_glu_entry_against_the_two_single_transforms(case, act):
    K = _K()
    d = GC.glu_inputs(case)
    _, g = _padded(case.rows, case.n_in, case.pad, DT[case.gdt], d["g"])
    _, u = _padded(case.rows, case.n_in, (case.pad * 2) % 7, DT[case.udt], d["u"])
    bg = None if d["bias_g"] is None else torch.from_numpy(d["bias_g"]).to(DEV)
    bu = None if d["bias_u"] is None else torch.from_numpy(d["bias_u"]).to(DEV)
    kw = dict(n_in=case.n_in, n_out=case.n_out, P=case.P)
    vg = torch.empty((case.rows, case.n_out), dtype=torch.float32, device=DEV)
    vu = torch.empty_like(vg)
    K.hadamard_rows(g, vg, bias=bg, **kw)
    K.hadamard_rows(u, vu, bias=bu, **kw)
    h32_buf, h32 = _padded(case.rows, case.n_out, case.pad, torch.float32)
    K.hadamard_glu_rows(g, u, h32, bias_g=bg, bias_u=bu, act=act, **kw)
    h_buf, h = _padded(case.rows, case.n_out, case.pad, DT[case.hdt])
    K.hadamard_glu_rows(g, u, h, bias_g=bg, bias_u=bu, act=act, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(h32_buf[:, case.n_out:]).all() and torch.isnan(h_buf[:, case.n_out:]).all()
    assert torch.isfinite(h32).all()
    if act == ACT_IDENTITY:
        assert torch.equal(_bits(h32), _bits(vg * vu))                   # one fp32 multiply of the same bits
    else:
        hs, bar32, _ = UC.epilogue_reference(act, vg.cpu().numpy(), vu.cpu().numpy())
        frac = float((np.abs(h32.double().cpu().numpy() - hs) / bar32).max())
        _WORST.append(frac)
        print(f"{case.id}: {frac:.4f} of the epilogue bar (largest so far {max(_WORST):.4f})")
        assert frac <= 1.0
    assert torch.equal(_bits(h), _bits(h32.to(DT[case.hdt])))            # a narrow h is the fp32 h rounded once


# ---------------------------------------------------------------------------- the classes
def _pow2(n):
    return 1 << (n - 1).bit_length()


def _layer(m, n, r, bits=2, fmt="uniform", factors="fp16", bias=False, seed=0):
    """A HadamardCalderaLinear of an (m, n) weight from host-seeded operands on the padded grid."""
    from ee274_convexcaldera_llm_quantization_amd.linear import (Q_FORMAT_NF, Q_FORMAT_UNIFORM, CalderaLinear,
                                                                  HadamardCalderaLinear)
    pr, pc = _pow2(m), _pow2(n)
    rng = np.random.default_rng(seed * 7919 + 1000 * m + n + 7 * r + bits)
    k = 2 ** (bits - 1) - 1
    if fmt == "nf":
        c = torch.from_numpy(rng.integers(0, 2 ** bits, (pr, pc)).astype(np.uint8))
    else:
        c = torch.from_numpy(rng.integers(-k, k + 1, (pr, pc)).astype(np.int8))
    L = torch.from_numpy((0.15 * rng.standard_normal((pr, r))).astype(np.float32))
    R = torch.from_numpy((0.15 * rng.standard_normal((r, pc))).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal(m).astype(np.float32)) if bias else None
    kw = {}
    if r == 0:
        L = R = None
    elif factors == "coded4":
        kw = dict(L_codes=(torch.from_numpy(rng.integers(-7, 8, (pr, r)).astype(np.int8)), 0.6, 4),
                  R_codes=(torch.from_numpy(rng.integers(-7, 8, (r, pc)).astype(np.int8)), 0.4, 4))
        L = R = None
    inner = CalderaLinear.from_codes(c, L, R, None, qscale=0.05, gscale=1.7, bits=bits,
                                     q_format=Q_FORMAT_NF if fmt == "nf" else Q_FORMAT_UNIFORM, **kw)
    return HadamardCalderaLinear(inner, n, m, b).to(DEV)


# (shapes (m, n, r) per member, Q bits, Q format, factors)
SETS = {
    "uniform2": (((48, 198, 8), (48, 198, 8), (48, 198, 8)), 2, "uniform", "fp16"),
    "uniform4-pr-differs": (((40, 100, 8), (12, 100, 8), (40, 100, 8)), 4, "uniform", "fp16"),   # pr 64, 16, 64; pc 128
    "nf4-rank0": (((48, 198, 8), (80, 198, 0), (48, 198, 40)), 4, "nf", "fp16"),
    "nf2": (((80, 898, 8), (48, 898, 8)), 2, "nf", "fp16"),
    "coded4": (((48, 198, 8), (80, 198, 0), (200, 198, 16)), 2, "uniform", "coded4"),
    "one": (((48, 198, 8),), 2, "uniform", "fp16"),
}
_LAYERS = {}


def _set(name):
    if name not in _LAYERS:
        shapes, bits, fmt, factors = SETS[name]
        _LAYERS[name] = [_layer(m, n, r, bits, fmt, factors, bias=i % 2 == 1, seed=i)
                         for i, (m, n, r) in enumerate(shapes)]
    return _LAYERS[name]


@pytest.mark.parametrize("T", [1, 5, 16, 17, 64])
@pytest.mark.parametrize("name", list(SETS))
@torch.no_grad()
def test_linear_group_equals_each_member_alone(name, T):
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardLinearGroup
    layers = _set(name)
    n = layers[0].in_features
    g = torch.Generator().manual_seed(T + n)
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        x = torch.randn(2, T, n, generator=g).to(dt).to(DEV)
        alone = [lin(x) for lin in layers]
        group = HadamardLinearGroup(layers)
        try:
            ys = group(x)
            for i, (y, want, lin) in enumerate(zip(ys, alone, layers)):
                assert y.dtype == dt and y.shape == (2, T, lin.out_features)
                assert torch.isfinite(y).all() and torch.equal(_bits(y), _bits(want)), (dt, i)
            # the transparent path: one set of launches serves every member, in any order
            outs = [lin(x) for lin in reversed(layers)]
            assert group._kept == {}
            for y, want in zip(reversed(outs), alone):
                assert torch.equal(_bits(y), _bits(want)), dt
        finally:
            group.dissolve()


def _mlp_layers():
    if "mlp" not in _LAYERS:
        _LAYERS["mlp"] = [_layer(200, 198, 8, 2, bias=True, seed=11), _layer(200, 198, 16, 2, seed=12)]
    return _LAYERS["mlp"]


@pytest.mark.parametrize("T", [1, 16, 17, 64])
@torch.no_grad()
def test_gated_mlp_against_its_members(T):
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardGatedMLP
    gate, up = _mlp_layers()
    x = torch.randn(T, 198, generator=torch.Generator().manual_seed(T)).to(DEV)
    vg, vu = gate(x), up(x)                                            # fp32 x: the members' own fp32 outputs
    ident = HadamardGatedMLP(gate, up, torch.nn.Identity(), act="identity")
    assert ident._fused(x) and torch.equal(_bits(ident(x)), _bits(vg * vu))
    silu = HadamardGatedMLP(gate, up, torch.nn.Identity())
    h = silu(x)
    hs, bar32, _ = UC.epilogue_reference(ACT_SILU, vg.cpu().numpy(), vu.cpu().numpy())
    frac = float((np.abs(h.double().cpu().numpy() - hs) / bar32).max())
    print(f"T{T}: {frac:.4f} of the epilogue bar")
    assert h.dtype == torch.float32 and frac <= 1.0
    for dt in (torch.float16, torch.bfloat16):                         # exact in dt: the same pre-activations
        xd = x.to(dt)
        assert torch.equal(_bits(silu(xd)), _bits(silu(xd.float()).to(dt)))


@pytest.mark.parametrize("T", [1, 17])
@torch.no_grad()
def test_gated_mlp_end_to_end_within_the_members_bars(T):
    """Against fp64 x dense_weight()^T: 1.1 |u64| B_g + |silu(g64)| B_u + B_g B_u + 8 2^-24 |h64| with B the
    members' forward bars of test_gpu_hadamard_linear.py."""
    from test_gpu_hadamard_linear import _bar
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardGatedMLP
    gate, up = _mlp_layers()
    x = np.random.default_rng(T + 3).standard_normal((T, 198)).astype(np.float32)
    refs = []
    for lin in (gate, up):
        Wd = lin.dense_weight().double().cpu().numpy()
        v = x.astype(np.float64) @ Wd.T
        refs.append(v if lin.bias is None else v + lin.bias.double().cpu().numpy())
    g64, u64 = refs
    Bg, Bu = _bar(gate, x.astype(np.float64)), _bar(up, x.astype(np.float64))
    a64 = UC.silu64(g64)
    bar = 1.1 * np.abs(u64) * Bg + np.abs(a64) * Bu + Bg * Bu + 8 * u24 * np.abs(a64 * u64)
    h = HadamardGatedMLP(gate, up, torch.nn.Identity())(torch.from_numpy(x).to(DEV)).double().cpu().numpy()
    frac = float((np.abs(h - a64 * u64) / bar).max())
    print(f"T{T}: {frac:.4f} of the end-to-end bar")
    assert np.isfinite(h).all() and frac <= 1.0


def test_gradients_flow_through_the_fallback():
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardGatedMLP
    gate, up = _mlp_layers()
    mlp = HadamardGatedMLP(gate, up, torch.nn.Identity())
    x = torch.randn(5, 198, generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_()
    assert not mlp._fused(x)
    mlp(x).sum().backward()
    got = x.grad.clone()
    x.grad = None
    (torch.nn.functional.silu(gate(x)) * up(x)).sum().backward()
    assert torch.isfinite(got).all() and float(got.abs().max()) > 0 and torch.equal(got, x.grad)


def _replayed(fn, x):
    """fn(xs) captured at T = 1 on a static input and replayed on x."""
    xs = torch.zeros_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(xs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn(xs)
    xs.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("m,n", [(200, 198), (4000, 4096)], ids=["P256", "P4096"])
@torch.no_grad()
def test_decode_in_a_captured_graph(m, n):
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardGatedMLP, HadamardLinearGroup
    layers = [_layer(m, n, 8, 2, bias=True, seed=21), _layer(m, n, 8, 2, seed=22)]
    assert layers[0].padded_shape[0] == _pow2(m)
    x = torch.randn(1, n, generator=torch.Generator().manual_seed(1)).half().to(DEV)
    want = [lin(x) for lin in layers]
    mlp = HadamardGatedMLP(layers[0], layers[1], torch.nn.Identity())
    h = mlp(x)
    assert torch.equal(_bits(_replayed(mlp, x)), _bits(h)) and torch.isfinite(h).all()
    # the eager h itself: the fp32 h of the same (fp16-exact) x rounded once, and that within the epilogue bar
    h32 = mlp(x.float())
    hs, bar32, _ = UC.epilogue_reference(ACT_SILU, layers[0](x.float()).cpu().numpy(), layers[1](x.float()).cpu().numpy())
    assert torch.equal(_bits(h), _bits(h32.half())) and (np.abs(h32.double().cpu().numpy() - hs) <= bar32).all()
    group = HadamardLinearGroup(layers)
    ys = _replayed(group, x)
    for y, w in zip(ys, want):
        assert torch.equal(_bits(y), _bits(w))


# ---------------------------------------------------------------------------- a real run
class _Attn(torch.nn.Module):
    def __init__(self, h):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj = (torch.nn.Linear(h, h, bias=False) for _ in range(3))

    def forward(self, x):
        return self.q_proj(x) * torch.tanh(self.k_proj(x)) + self.v_proj(x)


class _MLP(torch.nn.Module):
    def __init__(self, h, i):
        super().__init__()
        self.gate_proj, self.up_proj = torch.nn.Linear(h, i, bias=False), torch.nn.Linear(h, i, bias=False)
        self.down_proj, self.act_fn = torch.nn.Linear(i, h, bias=False), torch.nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class _Tiny(torch.nn.Module):
    def __init__(self, h=512, i=640):
        super().__init__()
        self.language_model = torch.nn.Module()
        self.language_model.model = torch.nn.Module()
        block = torch.nn.Module()
        block.self_attn, block.mlp = _Attn(h), _MLP(h, i)
        self.language_model.model.layers = torch.nn.ModuleList([block])
        self.language_model.lm_head = torch.nn.Linear(h, 600, bias=False)

    def forward(self, x):
        block = self.language_model.model.layers[0]
        x = x + block.self_attn(x)
        x = x + block.mlp(x)
        return self.language_model.lm_head(x)


@torch.no_grad()
def test_tiny_model_grouped_keeps_its_bits_and_fused_stays_within_the_bar():
    from ee274_convexcaldera_llm_quantization_amd import model as M
    from ee274_convexcaldera_llm_quantization_amd.linear import (HadamardCalderaLinear, HadamardGatedMLP,
                                                                  HadamardLinearGroup)
    torch.manual_seed(3)
    net = _Tiny()
    for p in net.parameters():
        torch.nn.init.normal_(p, std=0.02)
    net.to(DEV)
    qp = M.driver_params(16)
    qp.iters = 2
    rep = M.apply_caldera_quantization(net, None, qp, packed=True, packed_hadamard=True,
                                       selection=M.LayerSelection(layers=None))
    block = net.language_model.model.layers[0]
    assert all(o.applied for o in rep.layers) and len(rep.layers) == 6
    assert all(isinstance(mod, HadamardCalderaLinear) for mod in (*block.self_attn.children(), block.mlp.gate_proj,
                                                                  block.mlp.up_proj, block.mlp.down_proj))
    x = torch.randn(2, 5, 512, generator=torch.Generator().manual_seed(4)).to(DEV)
    logits = net(x)
    grouped, _ = M.group_shared_input_layers(net, hadamard=True)
    assert len(grouped) == 2 and isinstance(block.self_attn.q_proj.group, HadamardLinearGroup)
    assert torch.equal(_bits(net(x)), _bits(logits))                  # grouped: the ungrouped bits
    # fused: the members' fp32 outputs are the same bits, so h moves by the epilogue's rounding alone
    mlp = block.mlp
    hin = x + block.self_attn(x)
    vg, vu = mlp.gate_proj(hin), mlp.up_proj(hin)
    fused, _ = M.fuse_gated_mlps(net, hadamard=True)
    assert len(fused) == 1 and isinstance(block.mlp, HadamardGatedMLP)
    hs, bar32, _ = UC.epilogue_reference(ACT_SILU, vg.cpu().numpy(), vu.cpu().numpy())
    frac = float((np.abs(block.mlp.glu(hin).double().cpu().numpy() - hs) / bar32).max())
    print(f"tiny model: fused h at {frac:.4f} of the epilogue bar")
    assert frac <= 1.0
    assert torch.isfinite(net(x)).all()
    assert M.unfuse_gated_mlps(net) and M.ungroup_shared_input_layers(net)
    assert torch.equal(_bits(net(x)), _bits(logits))
