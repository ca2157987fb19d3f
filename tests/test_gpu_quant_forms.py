"""Every launch form of csrc/cq_quant.hip's uniform quantiser, dequantiser, code unpacker and RMS
scaler against the CPU oracle, on the cases of tests/quant_form_cases.py (which kernel and loop
form each case reaches is asserted on the host, tests/test_quant_forms_host.py).

Outputs are compared through integer views, so the sign of a zero counts: codes, packed codes,
scales and dequantised values equal the oracle's bit for bit; error sums are held to the bar the
project keeps for them (1e-6 relative to weight_stride_cases.werr: the fp32 difference squared in
fp32, summed in fp64).  Each quantise case also closes the loop on the device: dequantising its
codes, and its packed codes, gives the bits of its own `deq`, and unpacking `packed` gives
`codes`.  Where two kernels accept equal values (aligned and misaligned storage of one input),
their outputs are equal bit for bit.

Misaligned storage is a slice of a larger buffer, handed only to the entries whose host code
tests alignment and falls back (cq_dequant_uniform, cq_unpack_codes, cq_rms_scale); outputs
written into such a buffer must leave the elements around the slice alone."""
import numpy as np
import pytest
import torch

import quant_form_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS_BITS = int(np.float32(1e-8).view(np.int32))


@pytest.fixture(scope="module")
def K():
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    K.load()
    return K


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).to(DEV)     # a copy: the cases' arrays are read-only


def bits_of(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view({1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_bits(got, ref, what, keep=None):
    """got and ref have the same bits (where keep); a mismatch reports how many differ and how
    many of those are zeros of the other sign."""
    g, r = bits_of(got).reshape(-1), bits_of(ref).reshape(-1)
    assert g.shape == r.shape and g.dtype == r.dtype, (what, g.shape, r.shape, g.dtype, r.dtype)
    bad = g != r
    if keep is not None:
        bad &= np.asarray(keep).reshape(-1)
    if bad.any():
        sign_only = int((bad & ((g ^ r) == np.iinfo(g.dtype).min)).sum())
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.size} differ in bits ({sign_only} in the sign bit alone); "
                             f"first at {i}: got {g[i]:#x}, want {r[i]:#x}")


def at_offset(x, off):
    """x on the device as a contiguous slice that starts `off` bytes past a 16-byte boundary."""
    x = np.ascontiguousarray(x)
    k, rem = divmod(off, x.dtype.itemsize)
    assert rem == 0
    buf = torch.zeros(x.size + k + 16, dtype=getattr(torch, x.dtype.name), device=DEV)
    v = buf[k:k + x.size]
    v.copy_(dev(x.reshape(-1)))
    v = v.view(x.shape)
    assert v.is_contiguous() and buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == off % 16
    return v


class Guarded:
    """An output slice `off` bytes past a 16-byte boundary inside a buffer of a sentinel value;
    intact() tells whether the elements before and after the slice still hold it."""

    def __init__(self, n, dtype, off, shape=None):
        self.k, rem = divmod(off, torch.empty(0, dtype=dtype).element_size())
        assert rem == 0
        self.n = n
        self.sent = float("nan") if dtype.is_floating_point else 0x55
        self.buf = torch.full((n + self.k + 64,), self.sent, dtype=dtype, device=DEV)
        self.out = self.buf[self.k:self.k + n].view(shape or (n,))
        assert self.out.is_contiguous() and self.buf.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == off % 16

    def intact(self):
        rest = torch.cat([self.buf[:self.k], self.buf[self.k + self.n:]])
        return bool(torch.isnan(rest).all() if self.buf.dtype.is_floating_point else (rest == self.sent).all())


def elementwise(nan_blocks, bs):
    """(B, nb) block mask -> keep-mask (B, numel) of the elements outside those blocks."""
    return ~np.repeat(nan_blocks, bs, axis=1)


def check_quant(K, c, out):
    """The outputs of a quantise call against the oracle, then the round trips on the device."""
    a, ref = c.a, c.ref
    B, numel, bits, bs = a.B, a.numel, a.bits, a.bs
    nanb = ref["nan_blocks"]
    keep = elementwise(nanb, bs)
    failures = []

    def check(fn, *args, **kw):
        try:
            fn(*args, **kw)
        except AssertionError as e:     # report every output of the case, not the first alone
            failures.append(str(e))

    check(assert_bits, out["scale"], ref["scale"], f"{c.id} scale", ~nanb)
    if out.get("codes") is not None:
        check(assert_bits, out["codes"], ref["codes"], f"{c.id} codes", keep)
    if out.get("packed") is not None:
        check(assert_bits, out["packed"], ref["packed"], f"{c.id} packed", keep.reshape(B, -1, 8 // bits).all(axis=2))
    if out.get("deq") is not None:
        check(assert_bits, out["deq"], ref["deq"], f"{c.id} deq", keep)
    if nanb.any():      # a NaN block: its scale and every dequantised value are NaN (codes unspecified)
        assert np.isnan(out["scale"].cpu().numpy()[nanb]).all(), f"{c.id}: NaN block's scale"
        if out.get("deq") is not None:
            assert np.isnan(out["deq"].cpu().numpy()[~keep]).all(), f"{c.id}: NaN block's deq"
    if a.err:
        got, want = out["err"].cpu().numpy(), ref["err"]
        for b in range(B):
            if nanb[b].any():
                continue
            rel = abs(got[b] - want[b]) / want[b]
            print(f"{c.id} matrix {b} err: relative deviation {rel:.2e} (bar 1e-06)")
            if not rel <= 1e-6:
                failures.append(f"{c.id} err[{b}]: {got[b]!r} vs {want[b]!r} ({rel:.2e})")
    # round trips on the device; from the reference's codes where the call did not ask for them
    codes = out["codes"] if out.get("codes") is not None else dev(ref["codes"])
    deq = out["deq"] if out.get("deq") is not None else dev(ref["deq"])
    scale = out["scale"].reshape(-1)
    check(assert_bits, K.dequantize_uniform(codes, scale, bits).view(B, numel), deq, f"{c.id} dequantize(codes) vs deq", keep)
    if out.get("packed") is not None:
        check(assert_bits, K.dequantize_uniform(out["packed"], scale, bits, packed=True, numel=B * numel).view(B, numel),
              deq, f"{c.id} dequantize(packed) vs deq", keep)
        check(assert_bits, K.unpack_codes(out["packed"], numel, bits), codes, f"{c.id} unpack(packed) vs codes", keep)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------ quantise
@pytest.mark.parametrize("cid", C.ids("quantize_uniform"))
def test_quantize_uniform_forms(K, cid):
    """cq_quantize_uniform: quant_block_kernel (a wave per block) and absmax_atomic_kernel +
    quant_known_kernel, each at the block sizes, batch sizes and outputs of its loop forms, and
    the edge values (zero block, block below eps, NaN block) on both paths."""
    c, a = C.case(cid), C.case(cid).a
    x = dev(c.inp["x"])
    assert x.data_ptr() % 16 == 0
    kw = dict(codes="codes" in a.outputs, packed="packed" in a.outputs, deq="deq" in a.outputs)
    if a.err == "plain":
        kw["want_err"] = True
    elif a.err:
        kw.update(err_w=dev(c.inp["w"]), err_ncols=a.ncols)
    out = K.quantize_uniform(x, a.bs, a.bits, **kw)
    assert (out["err"] is not None) == bool(a.err) and (out["packed"] is not None) == a.packed
    check_quant(K, c, out)
    if a.edge:
        s = bits_of(out["scale"]).reshape(2, 4)
        assert s[C.ZERO_BLOCK] == EPS_BITS and s[C.TINY_BLOCK] == EPS_BITS, (cid, s)
        assert (out["codes"].cpu().numpy().reshape(2, 4, 64)[C.ZERO_BLOCK] == 0).all(), cid
        assert (bits_of(out["deq"]).reshape(2, 4, 64)[C.ZERO_BLOCK] == 0).all(), cid


@pytest.mark.parametrize("cid", C.ids("quantize_known_max"))
def test_quantize_known_max_forms(K, cid):
    """cq_quantize_uniform_known_max with a maximum above the data's own: the scale is the given
    one (quant_known_kernel's `single` form without the absmax pass)."""
    c, a = C.case(cid), C.case(cid).a
    x = dev(c.inp["x"])
    o = {"codes": torch.empty(a.B, a.numel, dtype=K.code_dtype(a.bits), device=DEV),
         "packed": torch.empty(a.B, a.numel * a.bits // 8, dtype=torch.uint8, device=DEV),
         "deq": torch.empty(a.B, a.numel, device=DEV), "scale": torch.empty(a.B, 1, device=DEV)}
    K.quantize_known_max(x, dev(c.inp["mx"]).view(torch.int32), a.bits, **o)
    check_quant(K, c, o)


# ------------------------------------------------------------------------------ dequantise
def run_dequant(K, c):
    a = c.a
    codes = at_offset(c.inp["codes"], a.codes_off)
    g = Guarded(a.total, torch.float32, a.out_off)
    out = K.dequantize_uniform(codes, dev(c.inp["scale"]), a.bits, packed=a.fmt == "packed", numel=a.total, out=g.out)
    assert out.data_ptr() == g.out.data_ptr()
    torch.cuda.synchronize()
    assert g.intact(), f"{c.id}: wrote outside out"
    return out.cpu().numpy()


@pytest.mark.parametrize("cid", C.ids("dequantize_uniform"))
def test_dequantize_uniform_forms(K, cid):
    """cq_dequant_uniform: dequant16_kernel on int8 and packed codes with four scales a call, and
    dequant_kernel through each condition that sends the host code there."""
    c = C.case(cid)
    assert_bits(run_dequant(K, c), c.ref["out"], cid)


@pytest.mark.parametrize("group", sorted(C.groups("dequantize_uniform")))
def test_dequantize_forms_agree(K, group):
    """The vector and the scalar kernel, int8 and packed codes, on equal values: equal bits."""
    m = C.groups("dequantize_uniform")[group]
    outs = [run_dequant(K, C.case(i)) for i in m]
    for i, o in zip(m[1:], outs[1:]):
        assert_bits(o, outs[0], f"{i} vs {m[0]}")


# ------------------------------------------------------------------------------ unpack
def run_unpack(K, c):
    a = c.a
    packed = at_offset(c.inp["packed"], a.packed_off)
    g = Guarded(a.B * a.numel, torch.int8, a.out_off, shape=(a.B, a.numel))
    out = K.unpack_codes(packed, a.numel, a.bits, out=g.out)
    assert out.data_ptr() == g.out.data_ptr()
    torch.cuda.synchronize()
    assert g.intact(), f"{c.id}: wrote outside codes"
    return out.cpu().numpy()


@pytest.mark.parametrize("cid", C.ids("unpack_codes"))
def test_unpack_codes_forms(K, cid):
    """cq_unpack_codes: unpack16_kernel and, through each of its failed conditions, unpack_kernel,
    on bytes that hold every field value, against the numpy unpacking."""
    c = C.case(cid)
    assert_bits(run_unpack(K, c), c.ref["codes"], cid)


@pytest.mark.parametrize("group", sorted(C.groups("unpack_codes")))
def test_unpack_forms_agree(K, group):
    m = C.groups("unpack_codes")[group]
    outs = [run_unpack(K, C.case(i)) for i in m]
    for i, o in zip(m[1:], outs[1:]):
        assert_bits(o, outs[0], f"{i} vs {m[0]}")


# ------------------------------------------------------------------------------ RMS scale
def run_rms(K, c, do_scale):
    W = at_offset(c.inp["W"], c.a.off * c.inp["W"].dtype.itemsize)
    gs, Ws = K.rms_scale(W, do_scale)
    return gs.cpu().numpy(), Ws.cpu().numpy()


@pytest.mark.parametrize("cid", C.ids("rms_scale"))
def test_rms_scale_forms(K, cid):
    """cq_rms_scale: rms_partial8_kernel and the scalar rms_partial_kernel (numel % 8 != 0, or W
    off the 16-byte boundary), at test_rms_scale_matches_oracle's bars: fp16 gs and Ws equal to
    the oracle's; fp32 gs within 2e-7 relative, Ws the bits of W / gs at the device's own gs."""
    c = C.case(cid)
    W, ref = c.inp["W"], c.ref
    gs, Ws = run_rms(K, c, True)
    assert gs.dtype == np.float32 and Ws.dtype == W.dtype and Ws.shape == W.shape
    for b in range(2):
        if W.dtype == np.float16:
            assert float(gs[b]) == ref["gs"][b], (cid, b, float(gs[b]), ref["gs"][b])
            assert_bits(Ws[b], ref["Ws"][b], f"{cid} Ws[{b}]")
        else:
            rel = abs(float(gs[b]) - ref["gs"][b]) / ref["gs"][b]
            print(f"{cid} matrix {b} gs: relative deviation {rel:.2e} (bar 2e-07)")
            assert rel <= 2e-7, (cid, b, rel)
            assert_bits(Ws[b], (W[b] / gs[b]).astype(np.float32), f"{cid} Ws[{b}]")
    gs1, Ws1 = run_rms(K, c, False)
    assert (bits_of(gs1) == bits_of(np.float32(1))).all(), cid
    assert_bits(Ws1, (W.astype(np.float32) / np.float32(1)).astype(W.dtype), f"{cid} Ws (do_scale false)")


@pytest.mark.parametrize("group", sorted(g for g in C.groups("rms_scale") if "float16" in g))
def test_rms_sums_agree(K, group):
    """The 8-wide and the scalar sum of equal fp16 data give one gs: the sum of fp16 squares is
    exact in fp64 in any order."""
    m = C.groups("rms_scale")[group]
    assert {C.case(i).kernel.split("<")[0] for i in m} == {"rms_partial8_kernel", "rms_partial_kernel"}
    (g0, w0), (g1, w1) = (run_rms(K, C.case(i), True) for i in m)
    assert_bits(g1, g0, f"{m[1]} vs {m[0]} gs")
    assert_bits(w1, w0, f"{m[1]} vs {m[0]} Ws")
