"""cq_hadamard_rows on the device against the fp64 reference of hadamard_cases.py: exact cases
bit for bit, random cases within the derived bar, x and y inside NaN-filled buffers with a row
stride above the row (the NaNs around y survive, none enters y), half-precision outputs as the
fp32 result rounded once, and rows independent of their batch, index and stride."""
import numpy as np
import pytest
import torch

import hadamard_cases as HC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def _K():
    from ee274_convexcaldera_llm_quantization_amd import _lib as K
    return K


def _pad(n, P):
    """Whole rows keep 16-byte aligned chunks (the vector path); cut rows get an odd stride."""
    return 8 if n == P else 3


def run(case, ydt=None, x=None, xpad=None, ypad=None, xoff=0):
    """The case on the device: x (default the case's) sits at column xoff of a NaN-filled
    (rows, n_in + pad) buffer, y in another.  Returns y as a host tensor in its own dtype."""
    K = _K()
    d = HC.inputs(case)
    xs = torch.from_numpy(d["x"] if x is None else x)
    rows = xs.shape[0]
    xpad = _pad(case.n_in, case.P) if xpad is None else xpad
    ypad = _pad(case.n_out, case.P) if ypad is None else ypad
    xbuf = torch.full((rows, xoff + case.n_in + xpad), float("nan"), dtype=TDT[case.xdt])
    xbuf[:, xoff:xoff + case.n_in] = xs.to(TDT[case.xdt])
    xbuf = xbuf.to(DEV)
    ybuf = torch.full((rows, case.n_out + ypad), float("nan"), dtype=TDT[ydt or case.ydt], device=DEV)
    bias = None if d["bias"] is None else torch.from_numpy(d["bias"]).to(DEV)
    K.hadamard_rows(xbuf[:, xoff:xoff + case.n_in], ybuf[:, :case.n_out], n_in=case.n_in, n_out=case.n_out,
                    P=case.P, bias=bias)
    out = ybuf.cpu()
    assert torch.isnan(out[:, case.n_out:]).all(), "the kernel wrote beyond n_out"
    y = out[:, :case.n_out].contiguous()
    assert not torch.isnan(y).any(), "a NaN from beyond n_in (or from y's buffer) entered y"
    return y


@pytest.mark.parametrize("case", HC.EXACT, ids=lambda c: c.id)
def test_exact_cases_match_bit_for_bit(case):
    y = run(case)
    ref, _ = HC.reference(case)
    assert y.dtype == torch.float32 and np.array_equal(y.numpy().astype(np.float64), ref)


@pytest.mark.parametrize("case", HC.EXACT16, ids=lambda c: c.id)
def test_exact16_cases_are_equal(case):
    y = run(case)
    ref, _ = HC.reference(case)
    assert y.dtype == TDT[case.ydt] and np.array_equal(y.double().numpy(), ref)


@pytest.mark.parametrize("case", HC.RANDOM, ids=lambda c: c.id)
def test_random_cases_within_the_bar(case):
    y = run(case)
    ref, bar = HC.reference(case)
    frac = (np.abs(y.numpy().astype(np.float64) - ref) / bar).max()
    print(f"{case.id}: {frac:.3f} of the bar")
    assert frac <= 1.0


@pytest.mark.parametrize("case", [c for c in HC.RANDOM if c.rows in (3, 70)], ids=lambda c: c.id)
def test_half_outputs_are_the_fp32_result_rounded_once(case):
    y32 = run(case)
    for ydt in ("f16", "bf16"):
        y = run(case, ydt=ydt)
        assert y.dtype == TDT[ydt]
        assert torch.equal(y.view(torch.int16), y32.to(TDT[ydt]).view(torch.int16)), ydt


@pytest.mark.parametrize("P", [4, 64, 512, 2048, 4096, 16384, 32768])
def test_rows_do_not_depend_on_batch_index_or_stride(P):
    n_in, n_out = P, max(P - 5, 1)
    case = HC.Case("random", P, 70, n_in, n_out, "f32", "f32")
    x = HC.inputs(case)["x"]
    y = run(case)
    assert torch.equal(run(case).view(torch.int32), y.view(torch.int32))           # two calls, the same bits
    for t in (0, 5, 69):
        alone = run(case, x=x[t:t + 1], xpad=1, ypad=6, xoff=1)                    # unaligned: the scalar path
        assert torch.equal(alone.view(torch.int32), y[t:t + 1].view(torch.int32)), t
    part = run(case, x=x[3:20], xpad=4, ypad=4)                                    # another batch, another stride
    assert torch.equal(part.view(torch.int32), y[3:20].view(torch.int32))
    for xdt in ("f16", "bf16"):                                                    # the same holds per input dtype
        c16 = HC.Case("random", P, 17, n_in, n_out, xdt, "f32")
        x16 = HC.inputs(c16)["x"]
        full = run(c16)
        alone = run(c16, x=x16[16:17], xpad=1, ypad=2, xoff=1)
        assert torch.equal(alone.view(torch.int32), full[16:17].view(torch.int32)), xdt


def test_round_trip_is_the_identity_within_twice_the_bar():
    """H (H x) = x at P = 8192, through the kernel both ways."""
    K = _K()
    P = 8192
    case = HC.Case("random", P, 17, P, P, "f32", "f32")
    x = torch.from_numpy(HC.inputs(case)["x"]).to(DEV)
    y, back = torch.empty_like(x), torch.empty_like(x)
    K.hadamard_rows(x, y, n_in=P, n_out=P, P=P)
    K.hadamard_rows(y, back, n_in=P, n_out=P, P=P)
    _, bar = HC.reference(case)
    frac = ((back - x).abs().double().cpu().numpy() / (2 * bar)).max()
    print(f"round trip: {frac:.4f} of twice the bar")
    assert frac <= 1.0


def test_rows_zero_and_many_rows():
    K = _K()
    x = torch.zeros((0, 64), device=DEV)
    assert K.hadamard_rows(x, torch.zeros((0, 64), device=DEV), n_in=64, n_out=64, P=64).shape == (0, 64)
    # a one-hot row picks a row of H: y[t] = H[j] / sqrt(P), at a row count above one workgroup's share
    P, rows = 256, 1000
    j = torch.arange(rows) % P
    x = torch.zeros((rows, P))
    x[torch.arange(rows), j] = 1.0
    y = torch.empty((rows, P), device=DEV)
    K.hadamard_rows(x.to(DEV), y, n_in=P, n_out=P, P=P)
    i = torch.arange(P)
    signs = torch.tensor([[(-1.0) ** bin(int(a) & int(b)).count("1") for b in i] for a in range(P)])
    assert torch.equal(y.cpu(), signs[j] / 16.0)
