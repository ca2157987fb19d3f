"""Host-side checks of the packed linear layer with coded factors: the cases of
linear_factor_cases.py are exact where they claim to be and can see the faults they are meant
to catch, the ctypes struct matches the header, the C entry rejects what the header documents,
and the CalderaLinear / sharding / model.py surface carries factor codes on CPU tensors.  No GPU."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import linear_cases as LC
import linear_factor_cases as FC
from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import model as M
from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear, pack_rows, row_bytes, unpack_bytes
from ee274_convexcaldera_llm_quantization_amd.sharding import (MatrixResult, load_results, pack_results, save_results,
                                                               unpack_results)
from ee274_convexcaldera_llm_quantization_amd.src.caldera.utils.dataclasses import CalderaDecomposition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "caldera_hip.h")


# ---------------------------------------------------------------------------- the cases
def test_case_lists_cover_what_they_should():
    for shp in FC.SHAPES:
        combos = {(c.bits, c.lb, c.rb) for c in FC.EXACT if (c.m, c.n, c.r) == shp}
        assert {(2, 4, 4), (2, 2, 2)} <= combos
    combos = {(c.bits, c.lb, c.rb) for c in FC.EXACT}
    assert {(4, 4, 4), (2, 2, 4), (2, 4, 16), (2, 16, 4)} <= combos
    combos = {(c.bits, c.lb, c.rb) for c in FC.EXACT if (c.n, c.T) == (8454, 16)}      # the long-K decode shape
    assert {(2, 4, 4), (2, 2, 2), (4, 4, 4), (2, 4, 16), (2, 16, 4)} <= combos
    assert {c.T for c in FC.EXACT} == {1, 5, 16, 17, 64, 130}
    assert any(c.bias for c in FC.EXACT) and any(c.bias for c in FC.RANDOM)
    assert len({c.id for c in FC.ALL}) == len(FC.ALL)


@pytest.mark.parametrize("case", FC.EXACT + FC.EXACT16, ids=lambda c: c.id)
def test_exact_references_are_exact_in_fp32(case):
    """On the case data: every term is a multiple of the quantum 0.25, the sum of the absolute
    terms of every output (with |hi| + |lo| <= (1 + 2^-10) |z~| for the split) stays below 2^24
    quanta, the unscaled code sums are integers below 2^24, and z~ is exactly hi + lo."""
    y, _ = FC.reference(case)
    d = FC.inputs(case)
    sk, zscale = (np.float64(v) for v in FC.scales(case, d))
    assert sk == 0.5 and zscale == (0.25 if case.lb != 16 and case.rb != 16 else 0.5)
    x, c, l, rho = (np.abs(d[key].astype(np.float64)) for key in ("x", "c", "l", "rho"))
    zabs = zscale * (x @ rho.T)
    inner = sk * (x @ c.T) + (1 + 2.0 ** -10) * zabs @ l.T       # before gs: quantum 0.25
    assert inner.max() / 0.25 < 2 ** 24
    q = 1.0                                                       # gs = 4 (exact): y in units of 1 ...
    if d["bias"] is not None:                                     # ... or of the bias's 0.5
        q = 0.5
        assert (4.0 * inner + np.abs(d["bias"])).max() / q < 2 ** 24
    assert (x @ c.T).max() < 2 ** 24 and (x @ rho.T).max() < 2 ** 24
    assert np.array_equal(y / q, np.rint(y / q))
    z = zscale * (d["x"].astype(np.float64) @ d["rho"].astype(np.float64).T)
    assert np.abs(z).max() < 65504 and zabs.max() < 65504
    hi = z.astype(np.float16)
    lo = (z - hi.astype(np.float64)).astype(np.float16)
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), z)
    if case.kind == "exact16":
        assert np.abs(y).max() <= 2048 and np.array_equal(y, y.astype(np.float16).astype(np.float64))


def _pairs(cases):
    return [pytest.param(c, f, id=f"{c.id}-{f}") for c in cases for f in FC.FAULTS if FC.fault_applies(c, f)]


def test_every_fault_meets_exact_and_random_cases():
    for cases in (FC.EXACT, FC.RANDOM):
        seen = {f for c in cases for f in FC.FAULTS if FC.fault_applies(c, f)}
        assert seen == set(FC.FAULTS)


@pytest.mark.parametrize("case,fault", _pairs(FC.EXACT))
def test_planted_fault_changes_every_exact_case(case, fault):
    y, _ = FC.reference(case)
    yf, _ = FC.reference(case, fault)
    assert (y != yf).any()


@pytest.mark.parametrize("case,fault", _pairs(FC.RANDOM))
def test_planted_fault_exceeds_ten_bars_on_random_cases(case, fault):
    y, bar = FC.reference(case)
    yf, _ = FC.reference(case, fault)
    worst = (np.abs(yf - y) / bar).max()
    print(f"{case.id} {fault}: {worst:.1f} bars")
    assert worst >= 10


def test_reference_with_fp16_factors_is_the_one_of_linear_cases():
    """l_bits = r_bits = 16 and zscale = 1: the formula is cq_linear_forward's."""
    base = next(c for c in LC.RANDOM if (c.m, c.r, c.bits, c.T) == (48, 40, 2, 16))
    d = LC.inputs(base)
    case = FC.Case("random", base.m, base.n, base.r, base.bits, 16, 16, base.T)
    FC._CACHE[case] = dict(x=d["x"], c=d["c"], l=d["L"], rho=d["R"], s=d["s"], sl=None, sr=None, gs=d["gs"], bias=None)
    try:
        y, bar = FC.reference(case)
    finally:
        del FC._CACHE[case]
    y0, bar0 = LC.reference(base)
    assert np.array_equal(y, y0) and np.array_equal(bar, bar0)


# ---------------------------------------------------------------------------- the ABI
def _struct_fields(name):
    txt = open(HEADER).read()
    body = txt[txt.index(f"typedef struct {name}"):txt.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*[;,]", body.split("{", 1)[1])


def test_packed_args_struct_matches_header():
    fields = [f for f, _ in K.LinearPackedArgs._fields_]
    assert fields == _struct_fields("cq_linear_packed_args")
    base = [f for f, _ in K.LinearArgs._fields_]
    assert fields[:len(base)] == base == _struct_fields("cq_linear_args")      # all fields of cq_linear_args, first
    assert fields[len(base):] == ["l_bits", "r_bits", "L_codes", "l_code_stride", "R_codes", "r_code_stride",
                                  "lscale", "rscale"]
    for f in base:
        assert getattr(K.LinearPackedArgs, f).offset == getattr(K.LinearArgs, f).offset
    assert {"cq_linear_packed_workspace", "cq_linear_packed_forward"} <= set(K.EXPORTS)
    assert K.ABI_VERSION == 5 == K.load().cq_abi_version()


def test_packed_entry_rejects_bad_arguments_without_a_device():
    """Validation runs before any launch: CQ_EINVAL with a message."""
    lib = K.load()
    buf = torch.zeros(8192, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16

    def args(**kw):
        a = K.LinearPackedArgs()
        a.x, a.ldx, a.tokens, a.m, a.n, a.r, a.bits = base, 64, 1, 16, 64, 8, 2
        a.codes, a.code_stride, a.qscale, a.gscale = base + 256, 16, 1.0, 1.0
        a.y, a.y_dtype, a.ldy = base + 1024, K.CQ_F32, 16
        a.l_bits, a.r_bits = 4, 4
        a.L_codes, a.l_code_stride, a.lscale = base + 2048, 16, 1.0
        a.R_codes, a.r_code_stride, a.rscale = base + 3072, 32, 1.0
        for key, v in kw.items():
            setattr(a, key, v)
        return a

    def call(a, ws=None, nbytes=0):
        return lib.cq_linear_packed_forward(ctypes.byref(a), ws, nbytes, None)

    bad = ((dict(l_bits=3), "factor bits"), (dict(r_bits=8), "factor bits"), (dict(l_bits=0), "factor bits"),
           (dict(L_codes=None), "null L codes"), (dict(R_codes=None), "null R codes"),
           (dict(L_codes=base + 2052), "aligned"), (dict(R_codes=base + 3080), "aligned"),
           (dict(l_code_stride=24), "aligned"), (dict(r_code_stride=40), "aligned"),
           (dict(l_code_stride=0), "L code row stride"), (dict(r_code_stride=16), "R code row stride"),
           (dict(lscale=float("nan")), "L scale"), (dict(lscale=float("inf")), "L scale"), (dict(lscale=-1.0), "L scale"),
           (dict(rscale=float("nan")), "R scale"), (dict(rscale=-0.5), "R scale"),
           # what cq_linear_forward rejects is rejected here too
           (dict(bits=3), "bits"), (dict(r=K.LINEAR_MAX_RANK + 1), "rank"), (dict(codes=base + 260), "aligned"),
           (dict(x=base + 1), "misaligned"), (dict(ldx=8), "leading"),
           # an fp16 factor needs its pointer and leading dimension as before
           (dict(l_bits=16), "null L / R"), (dict(r_bits=16, R=base + 4096, ldr=8), "leading"))
    for kw, word in bad:
        assert call(args(**kw)) == K.CQ_EINVAL, kw
        assert word in lib.cq_last_error().decode(), (kw, lib.cq_last_error())
    # a coded factor's fp16 pointer and leading dimension are not looked at; valid arguments get as far as
    # the workspace check (still no device)
    a = args()
    assert lib.cq_linear_packed_workspace(ctypes.byref(a)) == 16 * 16 * 32 * 4
    assert call(a, base, 16) == K.CQ_EWORKSPACE and "cq_linear_packed_forward" in lib.cq_last_error().decode()
    a.tokens = 17
    assert lib.cq_linear_packed_workspace(ctypes.byref(a)) == 2 * 64 * 32 * 2
    a = args(l_bits=16, L=base + 4096, ldl=8)      # mixed: fp16 L, coded R
    assert call(a, base, 16) == K.CQ_EWORKSPACE
    assert call(args(r=0, l_bits=16, r_bits=16, tokens=0)) == 0


# ---------------------------------------------------------------------------- CalderaLinear
def _layer(m=12, n=198, r=5, bits=2, lb=4, rb=4, seed=0):
    rng = np.random.default_rng(seed)
    code = lambda b, shape: rng.integers(-(2 ** (b - 1) - 1), 2 ** (b - 1), shape).astype(np.int8)  # noqa: E731
    return dict(c=code(bits, (m, n)), cl=code(lb, (m, r)), cr=code(rb, (r, n)), s=0.37, sl=0.61, sr=0.23, gs=1.25,
                bits=bits, lb=lb, rb=rb)


def _from_codes(p, bias=None, L=None, R=None):
    t = torch.from_numpy
    return CalderaLinear.from_codes(t(p["c"]), L, R, bias, qscale=p["s"], gscale=p["gs"], bits=p["bits"],
                                    L_codes=None if L is not None else (t(p["cl"]), p["sl"], p["lb"]),
                                    R_codes=None if R is not None else (t(p["cr"]), p["sr"], p["rb"]))


def _decomposition(p):
    k, kl, kr = (2 ** (b - 1) - 1 for b in (p["bits"], p["lb"], p["rb"]))
    t = torch.from_numpy
    m, r = p["cl"].shape
    return CalderaDecomposition(
        Q=t(p["c"]).float() / k * p["s"], L=t(p["cl"]).float() / kl * p["sl"], R=t(p["cr"]).float() / kr * p["sr"],
        Q_idxs=t(p["c"]).reshape(1, -1), Q_scale=torch.tensor([[p["s"]]]),
        L_idxs=t(p["cl"]).t().reshape(1, r * m), L_scale=torch.tensor([[p["sl"]]]),      # L^T order
        R_idxs=t(p["cr"]).reshape(1, -1), R_scale=torch.tensor([[p["sr"]]]), global_scale=p["gs"])


def _tensors(lin):
    return {key: v for key, v in lin.state_dict().items() if torch.is_tensor(v)}


@pytest.mark.parametrize("bits,lb,rb,n", [(2, 4, 4, 198), (4, 2, 2, 198), (2, 2, 4, 64), (2, 4, 2, 898)])
def test_constructors_build_the_same_state(bits, lb, rb, n):
    p = _layer(n=n, bits=bits, lb=lb, rb=rb)
    a = _from_codes(p)
    b = CalderaLinear.from_decomposition(_decomposition(p), bits, L_bits=lb, R_bits=rb)
    c = CalderaLinear.from_result(a.to_result("layer"))
    assert (a.in_features, a.out_features, a.rank, a.bits, a.L_bits, a.R_bits) == (n, 12, 5, bits, lb, rb)
    assert a.L is None and a.R is None                       # a coded factor has no fp16 buffer
    assert "L_bits" in a.extra_repr()
    for other in (b, c):
        assert a.get_extra_state() == pytest.approx(other.get_extra_state())
        sa, so = _tensors(a), _tensors(other)
        assert set(sa) == set(so) == {"codes", "L_codes", "R_codes"}
        for key in sa:
            assert sa[key].dtype == so[key].dtype == torch.uint8 and torch.equal(sa[key], so[key]), key
    assert a.L_codes.shape == (12, row_bytes(5, lb)) and a.R_codes.shape == (5, row_bytes(n, rb))
    assert np.array_equal(a.L_codes.numpy(), LC.inference_codes(p["cl"], lb))
    assert np.array_equal(a.R_codes.numpy(), LC.inference_codes(p["cr"], rb))
    assert np.array_equal(unpack_bytes(a.R_codes, rb)[:, :n].numpy(), p["cr"])
    assert not list(a.parameters())
    k, kl, kr = (2 ** (x - 1) - 1 for x in (bits, lb, rb))
    dense = p["gs"] * (p["c"].astype(np.float64) * (p["s"] / k)
                       + (p["cl"].astype(np.float64) * (p["sl"] / kl)) @ (p["cr"].astype(np.float64) * (p["sr"] / kr)))
    np.testing.assert_allclose(a.dense_weight().double().numpy(), dense, rtol=1e-5, atol=1e-5)


def test_mixed_layers_and_packed_bytes():
    p = _layer()
    t = torch.from_numpy
    L = torch.randn(12, 5)
    R = torch.randn(5, 198)
    both, onlyL, onlyR = _from_codes(p), _from_codes(p, R=R), _from_codes(p, L=L)
    fp16 = CalderaLinear.from_codes(t(p["c"]), L, R, qscale=p["s"], gscale=p["gs"], bits=2)
    assert (onlyL.L_bits, onlyL.R_bits, onlyL.L, onlyL.R.dtype) == (4, 16, None, torch.float16)
    assert (onlyR.L_bits, onlyR.R_bits, onlyR.R, onlyR.L.dtype) == (16, 4, None, torch.float16)
    assert (fp16.L_bits, fp16.R_bits, fp16.L_codes, fp16.R_codes) == (16, 16, None, None)
    assert set(_tensors(fp16)) == {"codes", "L", "R"}            # as before this feature
    q = 12 * row_bytes(198, 2)
    lc, rc = 12 * row_bytes(5, 4), 5 * row_bytes(198, 4)
    assert fp16.packed_bytes() == q + 2 * 12 * 5 + 2 * 5 * 198
    assert both.packed_bytes() == q + lc + rc
    assert onlyL.packed_bytes() == q + lc + 2 * 5 * 198
    assert onlyR.packed_bytes() == q + 2 * 12 * 5 + rc
    biased = _from_codes(p, bias=torch.zeros(12))
    assert biased.packed_bytes() == both.packed_bytes() + 4 * 12
    # moves and casts leave the codes alone
    before = {key: v.clone() for key, v in _tensors(biased).items()}
    for cast in (lambda mod: mod.half(), lambda mod: mod.to(torch.bfloat16), lambda mod: mod.to("cpu")):
        cast(biased)
        assert biased.L_codes.dtype == torch.uint8 and biased.bias.dtype == torch.float32
        for key, v in before.items():
            assert torch.equal(getattr(biased, key), v)


def test_state_dict_round_trips_and_an_old_state_still_loads(tmp_path):
    p, p2 = _layer(), _layer(seed=1)
    a = _from_codes(p, bias=torch.arange(12, dtype=torch.float32))
    p2.update(s=9.0, sl=9.0, sr=9.0, gs=9.0)
    b = _from_codes(p2, bias=torch.zeros(12))
    torch.save(a.state_dict(), tmp_path / "sd.pt")
    b.load_state_dict(torch.load(tmp_path / "sd.pt"))
    for key in ("codes", "L_codes", "R_codes", "bias"):
        assert torch.equal(getattr(a, key), getattr(b, key))
    assert (b.qscale, b.gscale, b.lscale, b.rscale, b.L_bits, b.R_bits, b.rank) == \
        (a.qscale, a.gscale, a.lscale, a.rscale, 4, 4, 5)
    # a state saved before factor codes existed: tensors codes / L / R, extra state without the new keys
    t = torch.from_numpy
    L, R = torch.randn(12, 5), torch.randn(5, 198)
    old = CalderaLinear.from_codes(t(p["c"]), L, R, qscale=0.5, gscale=2.0, bits=2)
    sd = old.state_dict()
    sd["_extra_state"] = {key: v for key, v in sd["_extra_state"].items()
                          if key in ("qscale", "gscale", "bits", "in_features", "out_features", "rank")}
    assert set(sd) == {"codes", "L", "R", "_extra_state"}
    new = CalderaLinear.from_codes(t(p2["c"]), torch.zeros(12, 5), torch.zeros(5, 198), qscale=1.0, gscale=1.0, bits=2)
    new.load_state_dict(sd)
    assert torch.equal(new.L, old.L) and torch.equal(new.codes, old.codes) and (new.qscale, new.gscale) == (0.5, 2.0)
    assert (new.L_bits, new.R_bits, new.lscale, new.rscale) == (16, 16, 1.0, 1.0)
    with pytest.raises(RuntimeError):          # a coded state does not fit an fp16-factor layer
        new.load_state_dict(a.state_dict())


def test_results_file_round_trip_with_both_kinds_of_layer(tmp_path):
    p = _layer(bits=4)
    t = torch.from_numpy
    coded = _from_codes(p)
    L, R = torch.randn(12, 5), torch.randn(5, 198)
    plain = CalderaLinear.from_codes(t(p["c"]), L, R, qscale=p["s"], gscale=p["gs"], bits=4)
    mixed = _from_codes(p, L=L)
    results = [coded.to_result("coded"), plain.to_result("plain"), mixed.to_result("mixed")]
    assert results[0].L.shape == (0, 5) and results[0].R.shape == (0, 198)          # zero rows
    assert results[0].L.dtype == torch.float32 and results[2].L.shape == (12, 5)
    assert (results[1].L_codes, results[1].R_codes, results[1].L_bits, results[1].R_bits) == (None, None, 16, 16)
    path = str(tmp_path / "res.cqrs")
    save_results(path, results)
    loaded = load_results(path)
    for res, lin in zip(loaded, (coded, plain, mixed)):
        again = CalderaLinear.from_result(res)
        sa, sb = _tensors(lin), _tensors(again)
        assert set(sa) == set(sb)
        for key in sa:
            assert torch.equal(sa[key], sb[key]), (res.name, key)
        assert again.get_extra_state() == pytest.approx(lin.get_extra_state())
    assert (loaded[0].L_bits, loaded[0].R_bits, loaded[0].L_scale, loaded[0].R_scale) == (4, 4, p["sl"], p["sr"])
    # the file shrinks: 4-bit codes instead of fp32 factors
    assert pack_results([results[0]]).numel() < pack_results([results[1]]).numel()
    # into a model, with no new argument
    model = torch.nn.Module()
    model.coded, model.plain = torch.nn.Linear(198, 12, bias=False), torch.nn.Linear(198, 12, bias=True)
    assert M.apply_packed_results(model, loaded[:2]) == ["coded", "plain"]
    assert torch.equal(model.coded.L_codes, coded.L_codes) and model.coded.L is None
    assert model.plain.L_codes is None and model.plain.bias is not None


def test_payload_without_the_new_keys_unpacks_as_before():
    """A fp16-factor result writes no new array or meta key, so its payload is the earlier
    format bit for bit, and such a payload reads back with the defaults."""
    import json
    import struct
    p = _layer()
    res = MatrixResult("w", 12, 198, 5, 2, torch.from_numpy(LC.storage_codes(p["c"], 2)[0]), 0.37,
                       torch.randn(12, 5), torch.randn(5, 198), 1.25, {"Q": 0.5}, {"n_padded": 200})
    buf = pack_results([res])
    magic, version, mlen = struct.unpack("<4sIQ", bytes(buf[:16].numpy().tobytes()))
    assert (magic, version) == (b"CQRS", 2)
    meta = json.loads(bytes(buf[16:16 + mlen].numpy().tobytes()).decode())[0]
    assert set(meta) == {"name", "m", "n", "rank", "Q_bits", "Q_scale", "global_scale", "errors", "extra", "arrays"}
    assert set(meta["arrays"]) == {"codes", "L", "R"}
    out = unpack_results(buf)[0]
    assert (out.L_codes, out.R_codes, out.L_scale, out.R_scale, out.L_bits, out.R_bits) == (None, None, 1.0, 1.0, 16, 16)
    assert torch.equal(out.L, res.L) and torch.equal(out.codes, res.codes) and out.extra == {"n_padded": 200}
    assert MatrixResult("w", 1, 1, 0, 2, res.codes, 1.0, res.L, res.R, 1.0).L_bits == 16     # trailing, defaulted


def test_documented_errors():
    p = _layer()
    t = torch.from_numpy
    dec = _decomposition(p)
    for kw in (dict(L_bits=3, R_bits=4), dict(L_bits=4, R_bits=8), dict(L_bits=16, R_bits=4)):
        with pytest.raises(ValueError, match="bits"):
            CalderaLinear.from_decomposition(dec, 2, **kw)
    nf = copy.copy(dec)           # codebook quantisers hand back uint8 level indices / block scales
    nf.L_idxs = dec.L_idxs.to(torch.uint8)
    with pytest.raises(ValueError, match="uniform"):
        CalderaLinear.from_decomposition(nf, 2, L_bits=4, R_bits=4)
    blk = copy.copy(dec)
    blk.R_scale = torch.ones(4, 1)
    with pytest.raises(ValueError, match="uniform"):
        CalderaLinear.from_decomposition(blk, 2, L_bits=4, R_bits=4)
    lst = copy.copy(dec)
    lst.L_scale = [1.0, 2.0]
    with pytest.raises(ValueError, match="uniform"):
        CalderaLinear.from_decomposition(lst, 2, L_bits=4, R_bits=4)
    none = copy.copy(dec)
    none.L_idxs = None
    with pytest.raises(ValueError, match="uniform"):
        CalderaLinear.from_decomposition(none, 2, L_bits=4, R_bits=4)
    assert CalderaLinear.from_decomposition(none, 2, R_bits=4).L.dtype == torch.float16     # L from dec.L
    with pytest.raises(ValueError, match="bits"):
        CalderaLinear.from_codes(t(p["c"]), None, None, qscale=1.0, gscale=1.0, bits=2,
                                 L_codes=(t(p["cl"]), 1.0, 8), R_codes=(t(p["cr"]), 1.0, 4))
    with pytest.raises(ValueError, match="integer matrix"):      # codes beyond [-k, k] of their bits
        CalderaLinear.from_codes(t(p["c"]), None, None, qscale=1.0, gscale=1.0, bits=2,
                                 L_codes=(t(p["cl"]), 1.0, 2), R_codes=(t(p["cr"]), 1.0, 4))
    with pytest.raises(ValueError, match="not both"):
        CalderaLinear.from_codes(t(p["c"]), torch.zeros(12, 5), None, qscale=1.0, gscale=1.0, bits=2,
                                 L_codes=(t(p["cl"]), 1.0, 4), R_codes=(t(p["cr"]), 1.0, 4))
    with pytest.raises(ValueError, match="scale"):
        CalderaLinear.from_codes(t(p["c"]), None, None, qscale=1.0, gscale=1.0, bits=2,
                                 L_codes=(t(p["cl"]), float("nan"), 4), R_codes=(t(p["cr"]), 1.0, 4))
    with pytest.raises(RuntimeError, match="HIP"):
        _from_codes(p)(torch.zeros(2, 198))
    # the binding: a coded factor needs its codes as a uint8 matrix with one row per L / R row
    lin = _from_codes(p)
    x16, y32 = torch.zeros(2, 198, dtype=torch.float16), torch.zeros(2, 12)
    ok = dict(m=12, n=198, bits=2, r=5, L_codes=(lin.L_codes, 1.0, 4), R_codes=(lin.R_codes, 1.0, 4))
    a = K.linear_packed_args(x16, lin.codes, 1.0, 1.0, None, None, None, y32, **ok)
    assert (a.r, a.l_bits, a.r_bits, a.l_code_stride, a.r_code_stride) == (5, 4, 4, 16, row_bytes(198, 4))
    assert not a.L and not a.R and a.L_codes == lin.L_codes.data_ptr()
    for kw, word in ((dict(L_codes=(lin.L_codes[:5], 1.0, 4)), "L_codes"), (dict(R_codes=(lin.R_codes.int(), 1.0, 4)), "R_codes"),
                     (dict(r=None), "r is needed")):
        with pytest.raises(ValueError, match=word):
            K.linear_packed_args(x16, lin.codes, 1.0, 1.0, None, None, None, y32, **{**ok, **kw})
    with pytest.raises(ValueError, match="exactly one"):
        K.linear_packed_args(x16, lin.codes, 1.0, 1.0, torch.zeros(12, 5, dtype=torch.float16), None, None, y32, **ok)


# ---------------------------------------------------------------------------- model.py
class _Dec:
    """A stand-in decomposition with 4-bit uniform L, R codes (rank 3)."""

    def __init__(self, W):
        g = torch.Generator().manual_seed(W.shape[0] * 131 + W.shape[1])
        m, n, r = W.shape[0], W.shape[1], 3
        s = float(W.abs().max()) * 0.5
        c = torch.clamp(torch.round(W.float() / s), -1, 1).to(torch.int8)
        cl = torch.randint(-7, 8, (m, r), generator=g, dtype=torch.int8)
        cr = torch.randint(-7, 8, (r, n), generator=g, dtype=torch.int8)
        self.Q, self.Q_idxs, self.Q_scale = c.float() * s, c.reshape(1, -1), torch.tensor([[s]])
        self.L_scale, self.R_scale = torch.tensor([[0.01]]), torch.tensor([[0.02]])
        self.L, self.R = cl.float() / 7 * 0.01, cr.float() / 7 * 0.02
        self.L_idxs, self.R_idxs = cl.t().reshape(1, -1), cr.reshape(1, -1)
        self.global_scale = 1.0
        self.errors = {"Q": [0.1]}


def _model():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(64, 48), torch.nn.ReLU(), torch.nn.Linear(48, 32, bias=False))
    return m


def _quantise(qp, monkeypatch, **kw):
    model = _model()
    monkeypatch.setattr(M, "_reconstruct", lambda dec, dev: dec.Q + dec.L @ dec.R)
    monkeypatch.setattr(M, "_rel_error", lambda W, out: 0.5)
    sel = M.LayerSelection(scope="", keys=("0", "2"), layers=None, min_dim=8)
    rep = M.apply_caldera_quantization(model, None, qp, selection=sel, device="cpu",
                                       decompose=lambda qp, Ws, H: [_Dec(W) for W in Ws], **kw)
    assert [o.applied for o in rep.layers] == [True, True]
    return model


def _params(L_bits=4, R_bits=4, method="uniform"):
    from ee274_convexcaldera_llm_quantization_amd.src.caldera.utils.quantization import QuantizerFactory
    qp = M.driver_params(3)
    qp.L_bits, qp.R_bits = L_bits, R_bits
    qp.quant_factory_LR = QuantizerFactory(method=method, block_size=64)
    return qp


def test_packed_factors_builds_coded_layers_and_false_keeps_todays_buffers(monkeypatch):
    coded = _quantise(_params(), monkeypatch, packed=True, packed_factors=True)
    plain = _quantise(_params(), monkeypatch, packed=True)
    default = _quantise(_params(), monkeypatch, packed=True, packed_factors=False)
    for idx in (0, 2):
        c, p, d = coded[idx], plain[idx], default[idx]
        assert isinstance(c, CalderaLinear) and isinstance(p, CalderaLinear)
        assert (c.L_bits, c.R_bits, c.L, c.R) == (4, 4, None, None) and c.L_codes.dtype == torch.uint8
        assert (c.lscale, c.rscale) == pytest.approx((0.01, 0.02))
        # packed_factors=False: the module's buffers as today
        for mod in (p, d):
            assert set(_tensors(mod)) - {"bias"} == {"codes", "L", "R"}
            assert mod.L.dtype == mod.R.dtype == torch.float16 and (mod.L_bits, mod.R_bits) == (16, 16)
        assert all(torch.equal(_tensors(p)[key], _tensors(d)[key]) for key in _tensors(p))
        assert torch.equal(c.codes, p.codes)
        # the same weight up to the fp16 rounding of the stored factors
        torch.testing.assert_close(c.dense_weight(), p.dense_weight(), rtol=0, atol=2e-6)
        assert c.packed_bytes() < p.packed_bytes() or c.rank * 2 < 16     # 16-byte rows: tiny ranks do not shrink
    assert coded[0].bias is not None and coded[2].bias is None


def test_packed_factors_value_errors(monkeypatch):
    model = _model()
    none = lambda *a: []  # noqa: E731
    with pytest.raises(ValueError, match="packed=True"):
        M.apply_caldera_quantization(model, None, _params(), packed_factors=True, decompose=none)
    with pytest.raises(ValueError, match="uniform"):
        M.apply_caldera_quantization(model, None, _params(method="normal_float"), packed=True, packed_factors=True,
                                     decompose=none)
    for lb, rb in ((16, 16), (4, 16), (8, 4), (4, 3)):
        with pytest.raises(ValueError, match="L_bits / R_bits"):
            M.apply_caldera_quantization(model, None, _params(lb, rb), packed=True, packed_factors=True, decompose=none)
    assert all(isinstance(mod, torch.nn.Linear) for mod in (model[0], model[2]))     # nothing was replaced
