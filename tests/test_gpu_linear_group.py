"""The grouped packed forward on the GPU (cq_linear_group_forward, CalderaLinearGroup,
model.group_shared_input_layers): every member's output is bit for bit the output of the member's own
single-layer entry on the same operands and, the groups being exact, of the fp64 reference of
linear_group_cases.py; nothing is written outside a member's (T, m); members in another order; graph
capture; and a toy attention + MLP block with and without groups."""
import copy

import numpy as np
import pytest
import torch

import linear_group_cases as GC

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


def _operands(group):
    """(x in a NaN-filled buffer, [member dicts of device operands]) of a group, uploaded once."""
    if group in _OPS:
        return _OPS[group]
    K = _K()
    d = GC.inputs(group)
    T, n = d["x"].shape
    buf = torch.full((T * n + 24,), NAN, dtype=torch.float16, device=DEV)
    x = buf[8:8 + T * n].view(T, n)
    x.copy_(torch.from_numpy(d["x"]))
    mems = []
    for mem in d["members"]:
        op = dict(codes=_t(GC.packed_codes(group, mem)), qscale=float(mem["s"]), gscale=float(mem["gs"]),
                  bias=_t(mem["bias"]), m=mem["m"], n=n, bits=group.bits, r=mem["r"])
        if mem["r"]:
            for which, key in (("l", "L"), ("rho", "R")):
                f = GC.factor_operand(group, mem, which)
                if f[0] == "fp16":
                    op[key] = _t(f[1])
                else:
                    op[key + "_codes"] = (_t(f[1]), float(f[2]), f[3])
        mems.append(op)
    qf = K.QFMT_NF if group.fmt == "nf" else K.QFMT_UNIFORM
    _OPS[group] = (x, mems, qf)
    return _OPS[group]


def _nan_outputs(mems, T, dtype):
    """Per member: (buffer, view): y as a strided (T, m) view in the middle of a NaN-filled buffer."""
    out = []
    for op in mems:
        buf = torch.full((T + 2, op["m"] + 5), NAN, dtype=dtype, device=DEV)
        out.append((buf, buf[1:T + 1, 2:op["m"] + 2]))
    return out


def _claim(outs):
    """The outputs as host arrays, after checking that nothing around them was written."""
    ys = []
    for buf, view in outs:
        y = view.clone()
        view.fill_(NAN)
        assert torch.isnan(buf).all(), "the entry wrote outside a member's output"
        ys.append(y.cpu())
    return ys


def _grouped(group, dtype, order=None):
    K = _K()
    x, mems, qf = _operands(group)
    mems = mems if order is None else [mems[i] for i in order]
    outs = _nan_outputs(mems, group.T, dtype)
    K.linear_group_forward(x, mems, [v for _, v in outs], qf)
    return _claim(outs)


def _alone(group, dtype, order=None):
    """Each member through the single-layer codebook entry (for uniform codes: the packed entry's bits)."""
    K = _K()
    x, mems, qf = _operands(group)
    mems = mems if order is None else [mems[i] for i in order]
    outs = _nan_outputs(mems, group.T, dtype)
    for op, (_, y) in zip(mems, outs):
        K.linear_codebook_forward(x, op["codes"], op["qscale"], op["gscale"], op.get("L"), op.get("R"), op["bias"], y,
                                  m=op["m"], n=op["n"], bits=op["bits"], q_format=qf, r=op["r"],
                                  L_codes=op.get("L_codes"), R_codes=op.get("R_codes"))
    return _claim(outs)


# ---------------------------------------------------------------------------- the entry
@pytest.mark.parametrize("group", GC.ALL, ids=lambda g: g.id)
def test_every_member_is_its_own_entry_and_the_reference_bit_for_bit(group):
    ref = GC.reference(group)
    y32, a32 = _grouped(group, torch.float32), _alone(group, torch.float32)
    y16, a16 = _grouped(group, torch.float16), _alone(group, torch.float16)
    for i, r in enumerate(ref):
        bad = int((y32[i].numpy().astype(np.float64) != r).sum())
        print(f"{group.id} member {i}: {bad} of {r.size} differ from fp64, "
              f"{int((y32[i] != a32[i]).sum())} from the member alone")
        assert y32[i].dtype == torch.float32 and torch.equal(y32[i], a32[i])
        assert y16[i].dtype == torch.float16 and torch.equal(y16[i], a16[i])
        assert np.array_equal(y32[i].numpy().astype(np.float64), r)
        with np.errstate(over="ignore"):                                # beyond 65504 both are inf
            assert np.array_equal(y16[i].numpy(), r.astype(np.float16))  # the fp32 result rounded once


@pytest.mark.parametrize("group", [g for g in GC.ALL if g.count > 1 and g.T in (1, 5, 17, 130)], ids=lambda g: g.id)
def test_members_in_another_order(group):
    order = group.reversed_order
    ref = GC.reference(group, order=order)
    y = _grouped(group, torch.float32, order)
    alone = _alone(group, torch.float32, order)
    straight = _grouped(group, torch.float32)
    for j, i in enumerate(order):
        assert torch.equal(y[j], alone[j]) and torch.equal(y[j], straight[i])
        assert np.array_equal(y[j].numpy().astype(np.float64), ref[j])


def test_the_entry_refuses_before_any_launch_and_accepts_zero_tokens():
    K = _K()
    group = next(g for g in GC.ALL if g.n == 198 and g.T == 5 and g.fmt == "uniform" and g.lb == 16)
    x, mems, qf = _operands(group)
    outs = _nan_outputs(mems, group.T, torch.float32)
    with pytest.raises(ValueError, match="member 1"):
        K.linear_group_forward(x, [mems[0], dict(mems[1], bits=6 - group.bits), mems[2]], [v for _, v in outs], qf)
    torch.cuda.synchronize()
    assert all(torch.isnan(buf).all() for buf, _ in outs)
    # tokens == 0 (on the structs: an empty tensor has no pointer to pass): CQ_OK, nothing launched
    import ctypes
    g = K.linear_group_args(x, mems, [v for _, v in outs], qf)
    for i in range(g.count):
        g.members[i].tokens = 0
    lib = K.load()
    assert lib.cq_linear_group_workspace(ctypes.byref(g)) == 0
    assert lib.cq_linear_group_forward(ctypes.byref(g), None, 0, None) == 0
    torch.cuda.synchronize()
    assert all(torch.isnan(buf).all() for buf, _ in outs)


@pytest.mark.parametrize("group", [g for g in GC.ALL if g.T == 16 and g.n in (198, 64) and g.lb == 16
                                   and g.bits == 2], ids=lambda g: g.id)
def test_decode_group_in_a_captured_graph(group):
    """The entry neither allocates nor synchronises nor copies: a captured decode call replays to the
    eager bits."""
    K = _K()
    x, mems, qf = _operands(group)
    lib = K.load()
    ys = [torch.empty((group.T, op["m"]), dtype=torch.float32, device=DEV) for op in mems]
    import ctypes
    ws = K.workspace(lib.cq_linear_group_workspace(ctypes.byref(K.linear_group_args(x, mems, ys, qf))), DEV)
    xs = torch.zeros_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.linear_group_forward(xs, mems, ys, qf, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.linear_group_forward(xs, mems, ys, qf, ws=ws)
    xs.copy_(x)
    for y in ys:
        y.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    eager = _grouped(group, torch.float32)
    for y, e in zip(ys, eager):
        assert torch.equal(y.cpu(), e)


# ---------------------------------------------------------------------------- the module
class _Block(torch.nn.Module):
    """Attention-like and MLP-like projections on shared inputs, called as a model's code calls them."""

    def __init__(self, layers):
        super().__init__()
        for name, lin in layers.items():
            setattr(self, name, lin)

    def forward(self, h):
        q, k, v = self.q_proj(h), self.k_proj(h), self.v_proj(h)
        a = self.o_proj(torch.tanh(q) * torch.tanh(k[..., :1]) + v[..., :1])
        return self.down_proj(torch.tanh(self.gate_proj(a)) * self.up_proj(a))


def _layer(rng, m, n, r, bits):
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear
    k = GC.k_of(bits)
    c = torch.from_numpy(rng.integers(-k, k + 1, (m, n)).astype(np.int8))
    L = torch.from_numpy((0.15 * rng.standard_normal((m, r))).astype(np.float16)) if r else None
    R = torch.from_numpy((0.15 * rng.standard_normal((r, n))).astype(np.float16)) if r else None
    return CalderaLinear.from_codes(c, L, R, None, qscale=0.05, gscale=1.7, bits=bits)


def _block():
    rng = np.random.default_rng(11)
    n, ff = 96, 200
    shapes = dict(q_proj=(96, n, 8), k_proj=(40, n, 8), v_proj=(40, n, 0), o_proj=(n, 96, 8),
                  gate_proj=(ff, n, 16), up_proj=(ff, n, 16), down_proj=(n, ff, 8))
    return _Block({name: _layer(rng, *s, 2) for name, s in shapes.items()}).to(DEV)


def _count_launches(monkeypatch):
    from ee274_convexcaldera_llm_quantization_amd import _lib as K
    calls = []
    real = K.linear_group_forward
    monkeypatch.setattr(K, "linear_group_forward", lambda *a, **kw: (calls.append(len(a[1])), real(*a, **kw))[1])
    return calls


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.bfloat16], ids=str)
def test_grouped_block_equals_the_ungrouped_block(dtype, monkeypatch):
    from ee274_convexcaldera_llm_quantization_amd import model as M
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinearGroup
    plain = _block()
    grouped = copy.deepcopy(plain)
    made, skipped = M.group_shared_input_layers(grouped)
    assert made == [("q_proj", "k_proj", "v_proj"), ("gate_proj", "up_proj")] and skipped == []
    calls = _count_launches(monkeypatch)
    g = torch.Generator().manual_seed(3)
    for shape in ((1, 1, 96), (2, 3, 96), (1, 40, 96)):       # decode, decode, prefill
        h = torch.randn(shape, generator=g).to(DEV).to(dtype)
        with torch.no_grad():
            want, got = plain(h), grouped(h)
        assert got.dtype == dtype and torch.equal(got, want)
    assert calls == [3, 2] * 3                                 # one group launch per set and forward
    # the group called directly: the members' outputs in member order
    h = torch.randn((2, 3, 96), generator=g).to(DEV).to(dtype)
    with torch.no_grad():
        ys = grouped.q_proj.group(h)
        for y, name in zip(ys, ("q_proj", "k_proj", "v_proj")):
            alone = getattr(plain, name)(h)
            assert y.dtype == alone.dtype and y.shape == alone.shape and torch.equal(y, alone)
    assert isinstance(grouped.q_proj.group, CalderaLinearGroup)
    assert M.ungroup_shared_input_layers(grouped) == made and grouped.q_proj.group is None
    n0 = len(calls)
    with torch.no_grad():
        assert torch.equal(grouped(h), plain(h))
    assert len(calls) == n0


def test_grouped_block_under_inference_mode(monkeypatch):
    """Inference tensors have no version counter: the members run alone for them (nothing is kept),
    the group called directly still launches grouped, and both give the ungrouped bits."""
    from ee274_convexcaldera_llm_quantization_amd import model as M
    plain = _block()
    grouped = copy.deepcopy(plain)
    M.group_shared_input_layers(grouped)
    calls = _count_launches(monkeypatch)
    h0 = torch.randn((2, 3, 96), generator=torch.Generator().manual_seed(13)).to(DEV)
    with torch.inference_mode():
        h = h0 * 1.0
        assert h.is_inference()
        assert torch.equal(grouped(h), plain(h)) and calls == []
        ys = grouped.q_proj.group(h)
        assert calls == [3]
        for y, name in zip(ys, ("q_proj", "k_proj", "v_proj")):
            assert torch.equal(y, getattr(plain, name)(h))
        # h0 keeps its version counter: q/k/v grouped; gate/up's input is made inside the block, under the mode
        assert torch.equal(grouped(h0), plain(h0)) and calls == [3, 3]


def test_grouped_block_under_graph_capture():
    from ee274_convexcaldera_llm_quantization_amd import model as M
    plain = _block()
    grouped = copy.deepcopy(plain)
    M.group_shared_input_layers(grouped)
    h = torch.randn((1, 4, 96), generator=torch.Generator().manual_seed(5)).half().to(DEV)
    hs = torch.zeros_like(h)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        grouped(hs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        ys = grouped(hs)
    hs.copy_(h)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(ys, plain(h))


def test_gradients_go_through_the_members_own_path(monkeypatch):
    from ee274_convexcaldera_llm_quantization_amd import model as M
    plain = _block()
    grouped = copy.deepcopy(plain)
    M.group_shared_input_layers(grouped)
    calls = _count_launches(monkeypatch)
    h0 = torch.randn((2, 3, 96), generator=torch.Generator().manual_seed(7)).to(DEV)
    grads = []
    for net in (plain, grouped):
        h = h0.clone().requires_grad_()
        net(h).square().sum().backward()
        grads.append(h.grad)
    assert calls == [] and torch.equal(grads[0], grads[1])


def test_dense_prefill_threshold_takes_the_members_dense_path(monkeypatch):
    from ee274_convexcaldera_llm_quantization_amd import model as M
    plain = _block()
    grouped = copy.deepcopy(plain)
    M.group_shared_input_layers(grouped)
    M.set_dense_prefill(plain, 64)
    M.set_dense_prefill(grouped, 64)
    calls = _count_launches(monkeypatch)
    h = torch.randn((1, 64, 96), generator=torch.Generator().manual_seed(9)).half().to(DEV)
    with torch.no_grad():
        assert torch.equal(grouped(h), plain(h))
        assert calls == []
        assert torch.equal(grouped(h[:, :63]), plain(h[:, :63]))
    assert calls == [3, 2]
