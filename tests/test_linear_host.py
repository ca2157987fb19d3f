"""Host-side checks of the packed linear layer: the cases of linear_cases.py can see the faults
they are meant to catch (planted in the reference), the ctypes struct matches the header, and
the CalderaLinear / model.py surface (constructors, state dict, errors, packed=False) on CPU
tensors.  No GPU."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import linear_cases as LC
from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import model as M
from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear, pack_rows, row_bytes, unpack_bytes
from ee274_convexcaldera_llm_quantization_amd.sharding import MatrixResult, load_results, save_results
from ee274_convexcaldera_llm_quantization_amd.src.caldera.utils.dataclasses import CalderaDecomposition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "caldera_hip.h")


# ---------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("case", LC.EXACT + LC.EXACT16, ids=lambda c: c.id)
def test_exact_references_are_exact_in_fp32(case):
    y, _ = LC.reference(case)
    assert np.array_equal(y * 2, np.rint(y * 2))          # multiples of 0.5
    d = LC.inputs(case)
    x, c, L, R = (np.abs(d[key].astype(np.float64)) for key in ("x", "c", "L", "R"))
    worst = 4.0 * (0.5 * (x @ c.T) + (x @ R.T) @ L.T)     # bound on every partial sum
    if d["bias"] is not None:
        worst = worst + np.abs(d["bias"])
    assert worst.max() * 2 < 2 ** 24
    if case.kind == "exact16":
        assert np.abs(y).max() <= 2048 and np.array_equal(y, y.astype(np.float16).astype(np.float64))


def _pairs(cases):
    """(case, fault) for every fault that exists for the case (no L / R without a rank, ...)."""
    return [pytest.param(c, f, id=f"{c.id}-{f}") for c in cases for f in LC.FAULTS if LC.fault_applies(c, f)]


@pytest.mark.parametrize("case,fault", _pairs(LC.EXACT))
def test_planted_fault_changes_every_exact_case(case, fault):
    y, _ = LC.reference(case)
    yf, _ = LC.reference(case, fault)
    assert (y != yf).any()


@pytest.mark.parametrize("case,fault", _pairs([c for c in LC.RANDOM if c.n <= 512]))
def test_planted_fault_exceeds_ten_bars_on_random_cases(case, fault):
    y, bar = LC.reference(case)
    yf, _ = LC.reference(case, fault)
    worst = (np.abs(yf - y) / bar).max()
    print(f"{case.id} {fault}: {worst:.1f} bars")
    assert worst >= 10


def _loop_pairs(cases):
    return [pytest.param(c, f, id=f"{c.id}-{f}") for c in cases for f in LC.LOOP_FAULTS if LC.fault_applies(c, f)]


@pytest.mark.parametrize("case,fault", _loop_pairs([c for c in LC.RANDOM if c.n > 512]))
def test_loop_fault_exceeds_ten_bars_on_long_random_cases(case, fault):
    """A wave's second chunk dropped, or multiplied with the x of its first, on the cases that have one."""
    y, bar = LC.reference(case)
    yf, _ = LC.reference(case, fault)
    worst = (np.abs(yf - y) / bar).max()
    print(f"{case.id} {fault}: {worst:.1f} bars")
    assert worst >= 10


def test_every_loop_fault_meets_exact_and_random_cases():
    for cases in (LC.EXACT, LC.RANDOM):
        assert {f for c in cases for f in LC.LOOP_FAULTS if LC.fault_applies(c, f)} == set(LC.LOOP_FAULTS)


def _decode_split():
    """(kDecodeWaves, kDecodeWavesZ, kDecodeSplitZ) as csrc/cq_linear.hip defines them."""
    txt = open(os.path.join(ROOT, "ee274_convexcaldera_llm_quantization_amd", "csrc", "cq_linear.hip")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", txt).group(1))
                 for name in ("kDecodeWaves", "kDecodeWavesZ", "kDecodeSplitZ"))


def test_decode_cases_reach_the_pipelined_loops():
    """The decode kernels prefetch a wave's next chunk and rotate it in; that does something only
    where a wave owns two chunks or more.  Under the split the kernel source has now, the decode
    cases of both case files give some wave >= 2 chunks in each of the five loops, >= 3 (a chunk
    that is neither first nor last) in the code loops and the fp16 / 4-bit z loop, and an uneven
    split (another wave of the same launch takes fewer) in each of them."""
    import linear_factor_cases as FC
    split = _decode_split()
    assert split == (LC.DECODE_WAVES, LC.DECODE_WAVES_Z, LC.DECODE_SPLIT_Z)
    most, uneven, x_paths = {}, set(), set()
    for case in LC.ALL + FC.ALL:
        for loop, (hi, lo) in LC.decode_chunks(case, *split).items():
            most[loop] = max(most.get(loop, 0), hi)
            if hi >= 2 and lo < hi:
                uneven.add(loop)
            if hi >= 2 and loop.startswith("codes"):
                x_paths.add((loop, case.n % 8 == 0))     # x rows 16-byte aligned (vector loads) or not
    print(most, sorted(uneven))
    assert x_paths == {(loop, al) for loop in ("codes2", "codes4") for al in (False, True)}
    assert set(most) == {"codes2", "codes4", "z128", "z256", "L16"}
    assert all(v >= 2 for v in most.values()), most
    assert all(most[loop] >= 3 for loop in ("codes2", "codes4", "z128")), most
    assert uneven == set(most)
    # the restated split against the table it was written from
    case = next(c for c in LC.EXACT if (c.n, c.bits, c.T) == (8454, 2, 16))
    assert LC.decode_chunks(case, 8, 2, 16) == {"codes2": (5, 4), "z128": (3, 2), "L16": (1, 0)}
    case = next(c for c in LC.EXACT if (c.n, c.bits, c.T) == (2600, 4, 1))
    assert LC.decode_chunks(case, 8, 2, 16) == {"codes4": (3, 2), "z128": (1, 0), "L16": (1, 0)}
    case = next(c for c in LC.EXACT if (c.r, c.bits, c.T) == (264, 2, 5))
    assert LC.decode_chunks(case, 8, 2, 16) == {"codes2": (1, 0), "z128": (1, 0), "L16": (2, 1)}
    assert LC.decode_chunks(next(c for c in LC.EXACT if c.T == 17)) == {}


def test_single_fp16_rounding_of_z_fails_the_bar():
    """z rounded once to fp16 (what the contract forbids) is outside the bar at (33, 64, 8)."""
    for case in LC.RANDOM:
        if (case.m, case.n, case.r) != (33, 64, 8) or case.bias:
            continue
        d = LC.inputs(case)
        x, L, R, c = (d[key].astype(np.float64) for key in ("x", "L", "R", "c"))
        z16 = (x @ R.T).astype(np.float16).astype(np.float64)
        y = np.float64(d["gs"]) * (np.float64(d["s"] / np.float32(case.k)) * (x @ c.T) + z16 @ L.T)
        y64, bar = LC.reference(case)
        assert (np.abs(y - y64) / bar).max() > 1


def test_inference_layout_matches_python_packer():
    rng = np.random.default_rng(5)
    for bits, n in ((2, 898), (4, 198), (2, 64), (4, 33)):
        k = 2 ** (bits - 1) - 1
        c = rng.integers(-k, k + 1, (7, n)).astype(np.int8)
        ref = LC.inference_codes(c, bits)
        got = pack_rows(torch.from_numpy(c), bits)
        assert got.shape == (7, row_bytes(n, bits)) == ref.shape and LC.row_bytes(n, bits) == row_bytes(n, bits)
        assert np.array_equal(got.numpy(), ref)
        assert np.array_equal(unpack_bytes(got, bits)[:, :n].numpy(), c)
        assert (unpack_bytes(got, bits)[:, n:] == 0).all()   # the tail is code 0


# ---------------------------------------------------------------------------- the ABI
def _struct_fields(name):
    txt = open(HEADER).read()
    body = txt[txt.index(f"typedef struct {name}"):txt.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*[;,]", body.split("{", 1)[1])


def test_linear_args_struct_matches_header():
    assert [f for f, _ in K.LinearArgs._fields_] == _struct_fields("cq_linear_args")
    txt = open(HEADER).read()
    assert int(re.search(r"#define CQ_LINEAR_DECODE_MAX_TOKENS (\d+)", txt).group(1)) == K.LINEAR_DECODE_MAX_TOKENS
    assert K.LINEAR_DECODE_MAX_TOKENS == LC.DECODE_MAX_TOKENS
    assert int(re.search(r"#define CQ_LINEAR_MAX_RANK (\d+)", txt).group(1)) == K.LINEAR_MAX_RANK >= 256
    assert {"cq_linear_workspace", "cq_linear_forward"} <= set(K.EXPORTS)


def test_linear_entry_rejects_bad_arguments_without_a_device():
    """Validation runs before any launch: CQ_EINVAL with a message."""
    lib = K.load()
    buf = torch.zeros(4096, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16

    def args(**kw):
        a = K.LinearArgs()
        a.x, a.ldx, a.tokens, a.m, a.n, a.r, a.bits = base, 64, 1, 16, 64, 0, 2
        a.codes, a.code_stride, a.qscale, a.gscale = base + 256, 16, 1.0, 1.0
        a.y, a.y_dtype, a.ldy = base + 1024, K.CQ_F32, 16
        for key, v in kw.items():
            setattr(a, key, v)
        return a

    import ctypes
    for kw, word in ((dict(bits=3), "bits"), (dict(bits=8), "bits"), (dict(r=K.LINEAR_MAX_RANK + 1), "rank"),
                     (dict(codes=base + 260), "aligned"), (dict(code_stride=17), "aligned"),
                     (dict(x=base + 1), "misaligned"), (dict(y=base + 1026), "misaligned"),
                     (dict(code_stride=0), "stride"), (dict(ldx=8), "leading")):
        a = args(**kw)
        assert lib.cq_linear_forward(ctypes.byref(a), None, 0, None) == K.CQ_EINVAL, kw
        assert word in lib.cq_last_error().decode(), (kw, lib.cq_last_error())
    a = args(r=8, L=base + 2048, ldl=8, R=base + 3072, ldr=64)
    assert lib.cq_linear_workspace(ctypes.byref(a)) == 16 * 16 * 32 * 4     # decode: fp32 partial z
    a.tokens = 17
    assert lib.cq_linear_workspace(ctypes.byref(a)) == 2 * 64 * 32 * 2
    assert lib.cq_linear_forward(ctypes.byref(a), base, 16, None) == K.CQ_EWORKSPACE


# ---------------------------------------------------------------------------- CalderaLinear
def _layer(m=12, n=198, r=5, bits=2, seed=0):
    rng = np.random.default_rng(seed)
    k = 2 ** (bits - 1) - 1
    c = rng.integers(-k, k + 1, (m, n)).astype(np.int8)
    L = rng.standard_normal((m, r)).astype(np.float32)
    R = rng.standard_normal((r, n)).astype(np.float32)
    return c, L, R, 0.37, 1.25


def _result(c, L, R, s, gs, bits, name="layer"):
    packed, npad = LC.storage_codes(c, bits)
    extra = {"n_padded": npad} if npad != c.shape[1] else {}
    return MatrixResult(name, c.shape[0], c.shape[1], L.shape[1], bits, torch.from_numpy(packed), s,
                        torch.from_numpy(L), torch.from_numpy(R), gs, {}, extra)


def _decomposition(c, L, R, s, gs, bits):
    k = 2 ** (bits - 1) - 1
    Q = torch.from_numpy(c).float() / k * s
    return CalderaDecomposition(Q=Q, L=torch.from_numpy(L), R=torch.from_numpy(R),
                                Q_idxs=torch.from_numpy(c).reshape(1, -1), Q_scale=torch.tensor([[s]]),
                                global_scale=gs)


@pytest.mark.parametrize("bits,n", [(2, 198), (4, 198), (2, 64), (4, 898)])
def test_constructors_build_the_same_state(bits, n):
    c, L, R, s, gs = _layer(n=n, bits=bits)
    a = CalderaLinear.from_result(_result(c, L, R, s, gs, bits))
    b = CalderaLinear.from_decomposition(_decomposition(c, L, R, s, gs, bits), bits)
    assert (a.in_features, a.out_features, a.rank, a.bits) == (n, 12, 5, bits)
    assert a.get_extra_state() == pytest.approx(b.get_extra_state())
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb) and {"codes", "L", "R"} <= set(sa)
    for key in ("codes", "L", "R"):
        assert sa[key].dtype == sb[key].dtype and torch.equal(sa[key], sb[key]), key
    assert sa["L"].dtype == torch.float16 and sa["codes"].shape == (12, row_bytes(n, bits))
    assert not list(a.parameters())
    assert np.array_equal(a.codes.numpy(), LC.inference_codes(c, bits))
    k = 2 ** (bits - 1) - 1
    dense = gs * (c.astype(np.float64) * (s / k) + a.L.double().numpy() @ a.R.double().numpy())
    np.testing.assert_allclose(a.dense_weight().double().numpy(), dense, rtol=1e-5, atol=1e-5)
    # back to the storage form and in again
    again = CalderaLinear.from_result(a.to_result("layer"))
    assert torch.equal(again.codes, a.codes) and torch.equal(again.L, a.L) and torch.equal(again.R, a.R)


def test_state_dict_round_trips(tmp_path):
    c, L, R, s, gs = _layer()
    bias = torch.arange(12, dtype=torch.float32)
    a = CalderaLinear.from_result(_result(c, L, R, s, gs, 2), bias=bias)
    c2, L2, R2, _, _ = _layer(seed=1)
    b = CalderaLinear.from_result(_result(c2, L2, R2, 9.0, 9.0, 2), bias=torch.zeros(12))
    torch.save(a.state_dict(), tmp_path / "sd.pt")
    b.load_state_dict(torch.load(tmp_path / "sd.pt"))
    for key in ("codes", "L", "R", "bias"):
        assert torch.equal(getattr(a, key), getattr(b, key))
    assert (b.qscale, b.gscale, b.bits, b.rank) == (a.qscale, a.gscale, 2, 5)


def test_documented_errors():
    c, L, R, s, gs = _layer()
    res = _result(c, L, R, s, gs, 2)
    res8 = MatrixResult("l", 12, 198, 5, 8, torch.from_numpy(c).reshape(-1), s, res.L, res.R, gs)
    with pytest.raises(ValueError, match="bits"):
        CalderaLinear.from_result(res8)
    dec = _decomposition(c, L, R, s, gs, 2)
    with pytest.raises(ValueError, match="bits"):
        CalderaLinear.from_decomposition(dec, 3)
    with pytest.raises(ValueError, match="bits"):
        CalderaLinear.from_decomposition(dec, 8)
    noq = copy.copy(dec)
    noq.Q_idxs = None
    with pytest.raises(ValueError, match="no Q"):
        CalderaLinear.from_decomposition(noq, 2)
    nf = copy.copy(dec)          # codebook quantisers hand back uint8 level indices / block scales
    nf.Q_idxs = dec.Q_idxs.to(torch.uint8)
    with pytest.raises(ValueError, match="uniform"):
        CalderaLinear.from_decomposition(nf, 2)
    blk = copy.copy(dec)
    blk.Q_scale = torch.ones(4, 1)
    with pytest.raises(ValueError, match="uniform"):
        CalderaLinear.from_decomposition(blk, 2)
    lin = CalderaLinear.from_result(res)
    with pytest.raises(RuntimeError, match="HIP"):
        lin(torch.zeros(2, 198))
    model = torch.nn.Sequential(torch.nn.Linear(198, 12))
    with pytest.raises(KeyError):
        M.apply_packed_results(model, [res])
    res0 = _result(c, L, R, s, gs, 2, name="0")
    assert M.apply_packed_results(model, [res0]) == ["0"]
    assert isinstance(model[0], CalderaLinear) and model[0].bias is not None
    with pytest.raises(ValueError, match="hadamard"):
        M.apply_caldera_quantization(model, None, object(), hadamard=True, packed=True, decompose=lambda *a: [])
    with pytest.raises(ValueError, match="scale_W"):
        M.apply_caldera_quantization(model, None, object(), scale_W=True, packed=True, decompose=lambda *a: [])
    # the binding refuses operands of the wrong type with a message, not a bare assert
    x16, y32 = torch.zeros(2, 198, dtype=torch.float16), torch.zeros(2, 12)
    for kw, word in ((dict(L=lin.L.float()), "fp16"), (dict(bias=torch.zeros(12, dtype=torch.float16)), "bias"),
                     (dict(x=x16.float()), "x must be fp16"), (dict(y=y32.double()), "y must be")):
        ops = dict(x=x16, codes=lin.codes, L=lin.L, R=lin.R, bias=None, y=y32)
        ops.update(kw)
        with pytest.raises(ValueError, match=word):
            K.linear_args(ops["x"], ops["codes"], 1.0, 1.0, ops["L"], ops["R"], ops["bias"], ops["y"], m=12, n=198,
                          bits=2)


def test_dtype_casts_leave_the_stored_operands_alone():
    """model.half() / .to(bfloat16) after quantising must not turn the fp32 bias or the fp16
    factors into something the kernel cannot take (or lose their bits); moves still apply."""
    c, L, R, s, gs = _layer()
    lin = CalderaLinear.from_result(_result(c, L, R, s, gs, 2), bias=torch.arange(12, dtype=torch.float32) / 3)
    before = {key: v.clone() for key, v in lin.state_dict().items() if torch.is_tensor(v)}
    model = torch.nn.Sequential(lin, torch.nn.Linear(12, 4))
    for cast in (lambda mod: mod.half(), lambda mod: mod.to(torch.bfloat16), lambda mod: mod.double(),
                 lambda mod: mod.to("cpu")):
        cast(model)
        assert (lin.codes.dtype, lin.L.dtype, lin.R.dtype, lin.bias.dtype) == \
            (torch.uint8, torch.float16, torch.float16, torch.float32)
        for key, v in before.items():
            assert torch.equal(getattr(lin, key), v), key
    assert model[1].weight.dtype == torch.float64      # the other modules are cast as usual


def test_results_file_round_trip_into_a_model(tmp_path):
    c, L, R, s, gs = _layer(bits=4)
    path = str(tmp_path / "res.cqrs")
    save_results(path, [_result(c, L, R, s, gs, 4, name="proj")])
    model = torch.nn.Module()
    model.proj = torch.nn.Linear(198, 12, bias=False)
    M.apply_packed_results(model, load_results(path))
    direct = CalderaLinear.from_decomposition(_decomposition(c, L, R, s, gs, 4), 4)
    assert torch.equal(model.proj.codes, direct.codes) and torch.equal(model.proj.L, direct.L)
    assert model.proj.bias is None and (model.proj.qscale, model.proj.gscale) == (s, gs)


# ---------------------------------------------------------------------------- model.py
def _tiny():
    torch.manual_seed(0)
    from test_model_host import TinyLlava
    m = TinyLlava(n_layers=19, h=512, i=640)
    for p in m.parameters():
        torch.nn.init.normal_(p, std=0.02)
    return m


class _Dec:
    def __init__(self, W, scale):
        k = 1
        s = float(W.abs().max()) * scale
        c = torch.clamp(torch.round(W.float() / s), -k, k).to(torch.int8) if s > 0 else torch.zeros_like(W, dtype=torch.int8)
        self.Q = c.float() * s
        self.Q_idxs, self.Q_scale = c.reshape(1, -1), torch.tensor([[s]])
        self.L, self.R = torch.zeros(W.shape[0], 1), torch.zeros(1, W.shape[1])
        self.global_scale = 1.0
        self.errors = {"Q": [0.1]}


def _run(packed, monkeypatch):
    m = _tiny()
    names = [n for n, _, _ in M.select_layers(m, None)[0]]
    bad = names[1]
    mods = dict(m.named_modules())

    def decompose(qp, Ws, H):
        return [_Dec(W, 0.0 if W.data_ptr() == mods[bad].weight.data_ptr() else 0.5) for W in Ws]

    monkeypatch.setattr(M, "_reconstruct", lambda dec, dev: dec.Q + dec.L @ dec.R)
    monkeypatch.setattr(M, "_rel_error",
                        lambda W, out: float(torch.linalg.norm(W.float() - out) / torch.linalg.norm(W.float())))
    qp = M.driver_params()
    kw = {"packed": True} if packed else {}
    rep = M.apply_caldera_quantization(m, None, qp, decompose=decompose, device="cpu", **kw)
    return m, rep, names, bad


def test_packed_false_is_todays_behaviour_and_packed_true_keeps_gate_and_counters(monkeypatch):
    m0, rep0, names, bad = _run(False, monkeypatch)
    m1, rep1, _, _ = _run(True, monkeypatch)
    assert [(o.name, o.shape, o.rel_error, o.applied) for o in rep0.layers] == \
        [(o.name, o.shape, o.rel_error, o.applied) for o in rep1.layers]
    for attr in ("quantized_param_count", "unquantized_language_param_count", "vision_param_count", "total_bits"):
        assert getattr(rep0, attr) == getattr(rep1, attr)
    assert not rep0.layers[1].applied and all(o.applied for i, o in enumerate(rep0.layers) if i != 1)
    mods0, mods1 = dict(m0.named_modules()), dict(m1.named_modules())
    ref = _tiny()
    for n in names:
        assert isinstance(mods0[n], torch.nn.Linear)          # packed=False: dense write-back
        if n == bad:
            assert isinstance(mods1[n], torch.nn.Linear) and torch.equal(mods1[n].weight, mods0[n].weight)
            assert torch.equal(mods0[n].weight, dict(ref.named_modules())[n].weight)
        else:
            assert isinstance(mods1[n], CalderaLinear) and mods1[n].bits == 2
            torch.testing.assert_close(mods1[n].dense_weight(), mods0[n].weight.float(), rtol=1e-6, atol=1e-7)
