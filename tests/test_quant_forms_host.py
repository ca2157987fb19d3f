"""The cases of tests/quant_form_cases.py, checked on the host (no GPU):

* every case meets the dispatch predicate of the kernel it names and of each loop form (trait)
  it claims, with the predicates restated from cq_quant.hip's host code, and between them the
  cases name every kernel template of the quantiser, dequantiser, unpacker and RMS sum;
* the inputs hold what the bit-pattern checks of tests/test_gpu_quant_forms.py need: exact .5
  ties at every bit width, negative values whose code is 0 (the sign-of-zero check cannot pass
  vacuously), -0.0, both signs of each block's maximum, scales that differ from block to block;
* the numpy packer is weight_stride_cases.pack_codes and round-trips through unpack_np;
* the oracle's NaN and eps behaviour is what the edge-value cases state;
* DESIGN.md's table of kernel forms is the one the cases module prints."""
import os

import numpy as np
import pytest

import quant_form_cases as C
import weight_stride_cases as WS
from oracle import caldera_oracle as O

f32 = np.float32
QUANT = C.ids("quantize_uniform")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------ dispatch
def test_predicates_at_the_numbers_of_the_host_code():
    assert C.grid_for(1, 1) == 1 and C.grid_for(1024, 1) == 1 and C.grid_for(1025, 1) == 2
    assert C.grid_for(1 << 30, 1) == 2048 and C.grid_for(1 << 30, 2) == 1024
    assert C.grid_for(1 << 30, 32) == 64 and C.grid_for(1 << 30, 1000) == 64     # the floor of the cap
    assert C.grid_for(65552, 32) == 64 and C.grid_for(12300, 2) == 13
    assert C.block_grid(1) == 1 and C.block_grid(5) == 2 and C.block_grid(16384) == 4096 and C.block_grid(16400) == 4096
    assert C.small_blocks(4096, False) and not C.small_blocks(4100, False) and not C.small_blocks(4, True)
    assert C.v16(4096, 1024, 8, False, 0, 0) and C.v16(4096, 1024, 2, True, 0, 1)
    assert not C.v16(4096, 512, 8, False, 0, 0) and not C.v16(4032, 64, 2, False, 0, 0)
    assert not C.v16(4096, 1024, 16, False, 0, 0) and not C.v16(4096, 1024, 8, False, 4, 0)
    assert not C.v16(4096, 1024, 8, False, 0, 1)
    assert C.unpack16(48, 2, 0, 0) and not C.unpack16(20, 2, 0, 0) and not C.unpack16(4096, 4, 1, 0)
    assert C.unpack16(4096, 2, 0, 4) and not C.unpack16(4096, 4, 0, 4) and not C.unpack16(4096, 2, 0, 1)
    assert C.v8(128, 0) and not C.v8(660, 0) and not C.v8(128, 2)


@pytest.mark.parametrize("cid", C.ids())
def test_case_reaches_the_form_it_names(cid):
    c, a = C.case(cid), C.case(cid).a
    if c.entry == "quantize_uniform":
        assert a.numel % a.bs == 0 and c.kernel == C.quantize_kernel(a.bs, a.bits, a.packed, bool(a.err))
        if not C.small_blocks(a.bs, bool(a.err)):
            assert a.numel % 4 == 0 and a.bs % 4 == 0        # the large-block path's float4 groups
        if a.packed:
            assert a.bits <= 4 and a.numel % 4 == 0 and a.bs % 4 == 0
        for t in c.traits:
            assert C.TRAITS[t](a.B, a.numel, a.bs, a.bits, bool(a.err)), (cid, t)
        if a.err in ("shared", "rows"):
            assert a.numel % a.ncols == 0 and c.inp["w"].shape == ((a.ncols,) if a.err == "shared" else (a.B, a.ncols))
    elif c.entry == "quantize_known_max":
        assert a.numel % 4 == 0 and c.kernel == C.known_kernel(a.bits, True, False) and a.factor > 1
        assert (c.inp["mx"] > np.abs(c.inp["x"]).max(axis=1)).all()
    elif c.entry == "dequantize_uniform":
        assert c.kernel == C.dequant_kernel(a.total, a.bs, a.bits, a.fmt, a.out_off, a.codes_off)
        assert c.kernel.startswith("dequant16_kernel") == (c.id.startswith("dq-vector"))
        assert a.out_off % 4 == 0 and a.total % a.bs == 0       # out stays a float pointer
    elif c.entry == "unpack_codes":
        assert a.numel % 4 == 0 and c.kernel == C.unpack_kernel(a.B * a.numel, a.bits, a.out_off, a.packed_off)
    else:
        assert c.kernel == C.rms_kernel(a.dtype, a.numel, a.off * np.dtype(a.dtype).itemsize)


def test_cases_name_every_kernel_template():
    named = {c.kernel for c in C.CASES.values()}
    want = {f"quant_block_kernel<{b}>" for b in (2, 4, 8, 16)}
    want |= {"absmax_atomic_kernel + " + C.known_kernel(b, True, e) for b in (2, 4, 8, 16) for e in (False, True)}
    want |= {C.known_kernel(b, True, False) for b in (2, 4)}
    want |= {f"dequant16_kernel<{b}, 0>" for b in (2, 4, 8)} | {f"dequant16_kernel<{b}, 2>" for b in (2, 4)}
    want |= {f"dequant_kernel<{b}, 0>" for b in (2, 4, 8)} | {f"dequant_kernel<{b}, 2>" for b in (2, 4)}
    want |= {"dequant_kernel<16, 1>"}
    want |= {f"{k}<{b}>" for k in ("unpack16_kernel", "unpack_kernel") for b in (2, 4)}
    want |= {f"{k}<{d}>" for k in ("rms_partial_kernel", "rms_partial8_kernel") for d in ("CQ_F16", "CQ_F32")}
    assert want <= named, sorted(want - named)
    # the packed-without-error and error-without-packing forms of the large path, and every trait
    assert "absmax_atomic_kernel + quant_known_kernel<2, true, true>" in named
    assert "absmax_atomic_kernel + quant_known_kernel<8, false, true>" in named
    claimed = {t for c in C.CASES.values() for t in c.traits}
    assert claimed == set(C.TRAITS), set(C.TRAITS) - claimed


def test_scalar_and_vector_forms_meet_on_equal_values():
    """Each dequantise, unpack and RMS group holds a vector-kernel case and a scalar-kernel case."""
    for entry, vec in (("dequantize_uniform", "dequant16_kernel"), ("unpack_codes", "unpack16_kernel"),
                       ("rms_scale", "rms_partial8_kernel")):
        both = [g for g, m in C.groups(entry).items()
                if len({C.case(i).kernel.startswith(vec) for i in m}) == 2]
        assert len(both) >= 2, (entry, both)
    g = C.groups("unpack_codes")
    assert all(len(g[f"up-1-4096-{b}"]) == 3 for b in (2, 4))
    g = C.groups("dequantize_uniform")
    assert all(len(g[f"dq-4096-1024-{b}"]) == (5 if b <= 4 else 3) for b in (2, 4, 8))


# ------------------------------------------------------------------------------ inputs
def oracle_scaled(x, bits, bs):
    """The oracle's `scaled` array (oracle.quantize_uniform, before rint)."""
    blocks = np.ascontiguousarray(x, dtype=f32).reshape(-1, bs)
    mx = np.maximum(np.abs(blocks).max(axis=1, keepdims=True), f32(1e-8))
    return ((blocks / mx).astype(f32) * f32(O.uniform_k(bits))).astype(f32)


@pytest.mark.parametrize("cid", QUANT)
def test_quantise_inputs_hold_ties_negative_zero_codes_and_both_maxima(cid):
    c, a = C.case(cid), C.case(cid).a
    x = c.inp["x"]
    ok = ~np.isnan(x.reshape(-1, a.bs)).any(axis=1)
    blocks = x.reshape(-1, a.bs)[ok]
    for bits in (2, 4, 8, 16):
        sc = oracle_scaled(blocks, bits, a.bs)
        assert (np.abs(sc - np.trunc(sc)) == 0.5).any(), (cid, bits)
    codes = c.ref["codes"].reshape(-1, a.bs)[ok]
    neg0 = (codes == 0) & (blocks < 0)
    assert neg0.any(), cid
    assert (np.signbit(blocks) & (blocks == 0)).any(), cid
    mx = np.abs(blocks).max(axis=1, keepdims=True)
    assert ((blocks == mx) & (mx > 0)).any() and ((blocks == -mx) & (mx > 0)).any(), cid
    if a.bs >= 8:   # every ordinary block holds all of it
        full = blocks[(mx[:, 0] > 1e-8)]
        fm = np.abs(full).max(axis=1, keepdims=True)
        for v in (fm, -fm, fm / 2, -fm / 2):
            assert (full == v).any(axis=1).all(), cid
        assert ((full < 0) & (np.abs(full) < fm * 2.0 ** -16)).any(axis=1).all(), cid
    # neighbouring blocks differ in scale, so a scale read from the wrong block shows in the codes
    if len(mx) > 1:
        assert (mx[1:] != mx[:-1]).mean() > 0.9, cid
    # the oracle's dequantised zeros are all +0.0: the device must write that bit pattern
    d = c.ref["deq"].reshape(-1, a.bs)[ok]
    assert (bits_of(d[d == 0]) == 0).all(), cid


def test_known_max_inputs():
    for cid in C.ids("quantize_known_max"):
        c = C.case(cid)
        x, r = c.inp["x"], c.ref
        assert ((r["codes"] == 0) & (x < 0)).any() and r["codes"].shape == x.shape
        # the given maximum is the scale: no code reaches k, and 1.5 x keeps some codes off zero
        k = O.uniform_k(c.a.bits)
        assert np.abs(r["codes"]).max() == round(k / 1.5) and (r["scale"][:, 0] == c.inp["mx"]).all()


def test_sign_of_zero_in_the_oracle():
    """quantization.py:96-105 goes through int8, so a negative input with code 0 dequantises to
    +0.0 (bit pattern 0), as does -0.0 itself."""
    x = np.asarray([-0.01, 1, -0.0, 0.3], dtype=f32)
    c, s = O.quantize_uniform(x, 2, 4)
    d = O.dequantize_uniform(c, s, 2, (4,))
    assert c.reshape(-1).tolist() == [0, 1, 0, 0] and bits_of(d).tolist() == [0, bits_of(f32(1)).item(), 0, 0]


# ------------------------------------------------------------------------------ packer
def test_packer_is_the_shared_one_and_round_trips():
    assert C.pack_codes is WS.pack_codes
    assert C.pack_codes(np.array([-1, 0, 1, 0]), 2).tolist() == [0b00011001]      # first code in bits 7..6
    assert C.pack_codes(np.array([-7, 7, 0, 1]), 4).tolist() == [0x0E, 0x78]      # first code in the high nibble
    assert C.unpack_np([0b00011011], 2).tolist() == [-1, 0, 1, 2]
    assert C.unpack_np([0x0E, 0x7F], 4).tolist() == [-7, 7, 0, 8]
    rng = np.random.default_rng(3)
    for bits in (2, 4):
        by = rng.integers(0, 256, 257, dtype=np.uint8)
        by[:256] = np.arange(256)                                                # every byte value
        c = C.unpack_np(by, bits)
        assert c.dtype == np.int8 and c.size == by.size * 8 // bits
        assert np.array_equal(C.pack_codes(c, bits), by) and np.array_equal(C.unpack_np(C.pack_codes(c, bits), bits), c)
    for cid in C.ids("unpack_codes"):
        c = C.case(cid)
        assert np.array_equal(C.pack_codes(c.ref["codes"].reshape(-1), c.a.bits), c.inp["packed"].reshape(-1))


# ------------------------------------------------------------------------------ edge values
@pytest.mark.parametrize("bits", [2, 4, 8, 16])
def test_oracle_on_the_edge_values(bits):
    c = C.case(f"q-edge-values-B2-n256-bs64-b{bits}")
    x = c.inp["x"].reshape(2, 4, 64)
    r = {k: v.reshape(2, 4, -1) for k, v in c.ref.items() if k in ("codes", "deq", "scale")}
    eps = f32(1e-8)
    assert not np.isinf(x).any() and np.isnan(x).sum() == 1
    z = x[C.ZERO_BLOCK]
    assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
    assert r["scale"][C.ZERO_BLOCK][0] == eps and (r["codes"][C.ZERO_BLOCK] == 0).all()
    assert (bits_of(r["deq"][C.ZERO_BLOCK]) == 0).all()
    t = x[C.TINY_BLOCK]
    assert np.abs(t).max() == f32(1e-9) and r["scale"][C.TINY_BLOCK][0] == eps
    if bits > 4:   # 0.1 k is a code of its own from 8 bits up
        assert np.abs(r["codes"][C.TINY_BLOCK]).max() == round(0.1 * O.uniform_k(bits))
    assert np.isnan(r["scale"][C.NAN_BLOCK][0]) and np.isnan(r["deq"][C.NAN_BLOCK]).all()
    assert c.ref["nan_blocks"].sum() == 1 and c.ref["nan_blocks"][C.NAN_BLOCK]
    others = np.ones((2, 4), dtype=bool)
    others[C.NAN_BLOCK] = False
    assert not np.isnan(r["scale"][others]).any() and not np.isnan(r["deq"][others]).any()
    e = C.case(f"q-edge-values-B2-n256-bs64-b{bits}-err_plain")
    assert np.array_equal(bits_of(e.inp["x"]), bits_of(c.inp["x"]))       # both paths on the same input
    assert np.isfinite(e.ref["err"][0]) and np.isnan(e.ref["err"][1])


# ------------------------------------------------------------------------------ RMS, dequantise
def test_rms_groups_hold_equal_values():
    for m in C.groups("rms_scale").values():
        a, b = (C.case(i) for i in m)
        assert np.array_equal(a.inp["W"], b.inp["W"]) and (a.a.off, b.a.off) == (0, 1)
    for cid in C.ids("rms_scale"):
        W = C.case(cid).inp["W"]
        assert W.shape[0] == 2 and C.case(cid).ref["gs"][1] > 10 * C.case(cid).ref["gs"][0]


def test_dequantise_inputs_hold_several_scales_and_every_code():
    for cid in C.ids("dequantize_uniform"):
        c, a = C.case(cid), C.case(cid).a
        s, ic = c.inp["scale"], c.inp["int_codes"]
        assert s.size == a.total // a.bs >= 4 and len(set(s.tolist())) == s.size
        k = O.uniform_k(a.bits)
        assert ic.min() == -k and ic.max() == k and (ic == 0).any()
        if a.fmt == "packed":
            assert np.array_equal(c.inp["codes"], C.pack_codes(ic, a.bits))
    for m in C.groups("dequantize_uniform").values():
        r0 = C.case(m[0]).ref["out"]
        assert all(np.array_equal(bits_of(C.case(i).ref["out"]), bits_of(r0)) for i in m)


# ------------------------------------------------------------------------------ the document
def test_design_table_is_the_generated_one():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        doc = f.read()
    assert C.design_table() in doc, "DESIGN.md: regenerate the table with `python tests/quant_form_cases.py`"
