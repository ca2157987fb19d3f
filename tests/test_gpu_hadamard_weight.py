"""model.hadamard_transform(kernels=True) against fp64.  Each of the p_r + p_c stages has relative error 2^-24, each
of the two scales is one rounding; twice that: ||W^ - W~||_F <= (p_r + p_c + 2) 2^-23 ||W||_F, and twice again
for the inverse of W^ against W (two transforms in the chain)."""
import numpy as np
import pytest
import torch

import test_gpu_hadamard_linear as HL
from hadamard_cases import hadamard64
from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import model as M
from ee274_convexcaldera_llm_quantization_amd.linear import HadamardCalderaLinear, hadamard_sign_vector

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("signed", [False, True], ids=["plain", "signed"])
@pytest.mark.parametrize("shape,dtype", [((48, 198), torch.float16), ((160, 256), torch.float32)])
def test_transform_and_inverse_against_fp64(shape, dtype, signed):
    m, n = shape
    W = (0.05 * torch.randn(m, n, generator=torch.Generator().manual_seed(m))).to(dtype)
    signs = (hadamard_sign_vector(3, m), hadamard_sign_vector(4, n)) if signed else None
    pr, pc = 1 << (m - 1).bit_length(), 1 << (n - 1).bit_length()
    Wp = np.zeros((pr, pc))
    Wp[:m, :n] = W.double().numpy()
    if signed:
        Wp[:m, :n] *= signs[0].double().numpy()[:, None] * signs[1].double().numpy()[None, :]
    ref = hadamard64(np.ascontiguousarray(hadamard64(Wp, pc).T), pr).T / np.sqrt(float(pr * pc))
    bar = (np.log2(pr) + np.log2(pc) + 2) * 2.0 ** -23 * np.linalg.norm(Wp)
    Wt, shp = M.hadamard_transform(W.to(HL.DEV), signs=signs, kernels=True)
    err = np.linalg.norm(Wt.double().cpu().numpy() - ref)
    back = M.hadamard_transform(Wt, inverse=True, original_shape=shp, signs=signs, kernels=True)
    err_back = np.linalg.norm(back.double().cpu().numpy() - W.double().numpy())
    print(f"forward {err / bar:.3f} of the bar, round trip {err_back / (2 * bar):.3f}")
    assert shp == back.shape == (m, n) and Wt.shape == (pr, pc) and err <= bar and err_back <= 2 * bar


@torch.no_grad()
def test_tiny_model_with_the_switch_runs_no_gemm_in_the_transform(monkeypatch):
    gemms, transforms, gemm, transform = [], [], K.gemm, M.hadamard_transform

    def counted_transform(*a, **kw):
        before = len(gemms)
        out = transform(*a, **kw)
        transforms.append((kw.get("kernels"), len(gemms) - before))   # the switch, the GEMMs run inside
        return out

    monkeypatch.setattr(K, "gemm", lambda *a, **kw: (gemms.append(1), gemm(*a, **kw))[1])
    monkeypatch.setattr(M, "hadamard_transform", counted_transform)
    qp = M.driver_params(16)
    qp.iters = 2
    net = HL._tiny_model(1)
    rep = M.apply_caldera_quantization(net, None, qp, packed=True, packed_hadamard=True, hadamard_signs=3,
                                       hadamard_kernels=True)
    assert len(rep.layers) == 6 and all(o.applied and 0 < o.rel_error < 0.99 for o in rep.layers)
    assert all(isinstance(net.get_submodule(o.name), HadamardCalderaLinear) for o in rep.layers)
    assert transforms == [(True, 0)] * 12 and gemms   # the GEMMs counted are _reconstruct's


class _Exact:  # a decomposition that returns the transformed weight itself: Q = W~, L R = 0
    def __init__(self, Wt):
        self.Q, self.errors = Wt.float(), {}
        self.L, self.R = Wt.new_zeros(Wt.shape[0], 1, dtype=torch.float32), Wt.new_zeros(1, Wt.shape[1], dtype=torch.float32)


@torch.no_grad()
def test_dense_write_back_with_the_switch_recovers_the_weight():
    """hadamard=True, unsigned: the inverse writes back W itself within the round-trip bar (640 -> 1024: two passes)."""
    net = HL._tiny_model(2)
    rep = M.apply_caldera_quantization(net, None, M.driver_params(16), hadamard=True, hadamard_kernels=True,
                                       decompose=lambda qp, Ws, H: [_Exact(W) for W in Ws])
    bars = [2 * (sum((d - 1).bit_length() for d in o.shape) + 2) * 2.0 ** -23 for o in rep.layers]
    assert len(bars) == 6 and all(o.rel_error <= b for o, b in zip(rep.layers, bars))
