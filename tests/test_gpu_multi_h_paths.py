"""Per-matrix diagonal Hessians in one engine batch (ABI 5) on the engine paths that
tests/test_gpu_multi_h.py's four 896-square layers do not take: a wide and a tall shape (m > n:
the dense Gram, Y V and the row-weighted code product), 4-bit and NF4 Q (the codebook error
weights), 4-bit factors (the LPLR weights), activation_aware_LR off (err = h, lplr = h^2) and
fp32 W.  B = 3 matrices, each with its own H = diag(h_b); the rows of h differ in scale and in
pattern (tests/weight_stride_cases.weights).  Per case:

* every matrix is bit-identical (Q_idxs, Q_scale, L, R, errors) to the same matrix in a batch
  of three copies of it sharing its H (caldera_batch's promise);
* every matrix agrees with the CPU oracle's caldera(params, W_b, diag(h_b)) at the bars
  tests/test_gpu_methods.py uses for the same kind of configuration."""
import numpy as np
import pytest
import torch

from oracle import caldera_oracle as O
import weight_stride_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = C.B

# name: (m, n, W dtype, params common to CalderaParams and the oracle's Params, Q method, kind)
CASES = {
    "wide-256x512-q2-r64": (256, 512, torch.float16, dict(Q_bits=2, L_bits=16, R_bits=16, rank=64), "uniform", "f16"),
    "tall-512x256-q2-r32": (512, 256, torch.float16, dict(Q_bits=2, L_bits=16, R_bits=16, rank=32), "uniform", "f16"),
    "q4-256x512-r32": (256, 512, torch.float16, dict(Q_bits=4, L_bits=16, R_bits=16, rank=32), "uniform", "f16"),
    "nf4-256x512-r16": (256, 512, torch.float16, dict(Q_bits=4, L_bits=16, R_bits=16, rank=16), "nf4", "codebook"),
    "lr4-256x256-r16": (256, 256, torch.float16, dict(Q_bits=2, L_bits=4, R_bits=4, rank=16, lplr_iters=3), "uniform",
                        "lr4"),
    "not-aware-256x512-r32": (256, 512, torch.float16,
                              dict(Q_bits=2, L_bits=16, R_bits=16, rank=32, activation_aware_LR=False), "uniform", "f16"),
    "fp32-256x512-r32": (256, 512, torch.float32, dict(Q_bits=2, L_bits=16, R_bits=16, rank=32), "uniform", "f16"),
}
COMMON = dict(iters=2, update_order=["Q", "LR"], sigma_reg=1e-8)


def _inputs(name):
    m, n, dt, kw, method, kind = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Ws = [(torch.randn(m, n, generator=g) * 0.02).to(dt) for _ in range(B)]
    h = C.weights(n, 7 + n + len(name))
    return Ws, h


def _params(name):
    from src.caldera.decomposition.alg import CalderaParams, QuantizerFactory
    _, _, _, kw, method, _ = CASES[name]
    extra = {} if method == "uniform" else dict(quant_factory_Q=QuantizerFactory(method, 64))
    return CalderaParams(**kw, **COMMON, **extra), O.Params(**kw, **COMMON, method_Q=method)


_RUNS = {}


def _mixed(name):
    """One caldera_batch call over the three matrices, each with its own H (run once per case)."""
    if name not in _RUNS:
        from ee274_convexcaldera_llm_quantization_amd.api import caldera_batch
        Ws, h = _inputs(name)
        Hs = [torch.diag_embed(torch.from_numpy(h[b])).to(DEV) for b in range(B)]
        decs, eng = caldera_batch(_params(name)[0], [W.to(DEV) for W in Ws], Hs, device=DEV, return_engine=True)
        assert len(eng.parts) == 1   # one lockstep batch
        print(f"{name}: LR steps from the sparse codes {eng.lr_steps_from_codes}")
        _RUNS[name] = decs
    return _RUNS[name]


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return torch.equal(torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu())


@pytest.mark.parametrize("name", list(CASES))
def test_distinct_h_bit_identical_to_shared_h(name):
    from ee274_convexcaldera_llm_quantization_amd.api import caldera_batch
    Ws, h = _inputs(name)
    mixed = _mixed(name)
    for b in range(B):
        H = torch.diag_embed(torch.from_numpy(h[b])).to(DEV)
        ref = caldera_batch(_params(name)[0], [Ws[b].to(DEV)] * B, H, device=DEV)[b]
        d = mixed[b]
        assert _same(d.Q_idxs, ref.Q_idxs) and _same(d.Q_scale, ref.Q_scale), (name, b)
        assert torch.equal(d.L.cpu(), ref.L.cpu()) and torch.equal(d.R.cpu(), ref.R.cpu()), (name, b)
        assert d.errors == ref.errors, (name, b, d.errors, ref.errors)
        assert d.global_scale == ref.global_scale


@pytest.mark.parametrize("b", range(B))
@pytest.mark.parametrize("name", list(CASES))
def test_distinct_h_each_matches_the_oracle(name, b):
    """Bars of tests/test_gpu_methods.py: 16-bit factors with a non-trivial H
    (test_dense_H_activation_aware): first errors 1e-5 / 1e-4, every error 1e-3, Q + L R 1e-4
    relative Frobenius; NF4 Q (test_codebook_Q): 1e-6 / 1e-4 / 1e-3 / 2e-3; 4-bit factors
    (test_dense_H_quantized_factors_and_not_aware): first Q error 1e-5, LR errors 2e-2."""
    kind = CASES[name][5]
    Ws, h = _inputs(name)
    d = _mixed(name)[b]
    ref = O.caldera(_params(name)[1], Ws[b].numpy(), np.diag(h[b]))
    print(f"{name} matrix {b}: errors {d.errors}, oracle {ref.errors}")
    assert d.global_scale == ref.global_scale
    assert abs(d.errors["Q"][0] - ref.errors["Q"][0]) < (1e-6 if kind == "codebook" else 1e-5), (d.errors, ref.errors)
    if kind == "lr4":
        np.testing.assert_allclose(d.errors["LR"], ref.errors["LR"], rtol=0, atol=2e-2)
        return
    assert abs(d.errors["LR"][0] - ref.errors["LR"][0]) < 1e-4, (d.errors, ref.errors)
    for k in ("Q", "LR"):
        np.testing.assert_allclose(d.errors[k], ref.errors[k], rtol=0, atol=1e-3)
    out = (d.Q.double() + d.L.double() @ d.R.double()).cpu().numpy()
    exp = ref.Q.astype(np.float64) + ref.L.astype(np.float64) @ ref.R.astype(np.float64)
    rel = np.linalg.norm(out - exp) / np.linalg.norm(exp)
    print(f"{name} matrix {b}: Q + L R relative Frobenius {rel:.2e}")
    assert rel < (2e-3 if kind == "codebook" else 1e-4), rel
