"""cq_gram_f64 where K is not split (gram_splits == 1: at least 1024 output tiles, or K < 512):
the MFMA kernel writes C itself -- no partial in the workspace, no reduction launch -- and a
symmetric Gram's tiles above the diagonal also write their mirror.  Checked at such shapes, K
not a multiple of the 32-deep slice and ragged tile edges included, and at one split-K shape
that still goes through the reduction: the symmetric call is bitwise symmetric, bitwise equal
to the non-symmetric call on a copy of the operand (which computes every tile), and within the
fp64 tolerance of test_gram_f64_mfma_paths of the fp64 product."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(x):
    return x.contiguous().view(torch.int64)


@pytest.mark.parametrize("tk", [False, True])
@pytest.mark.parametrize("B,Kd,p", [(128, 260, 192), (128, 256, 100), (2, 4096, 192)])
def test_gram_f64_direct(B, Kd, p, tk):
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    g = torch.Generator(device=DEV).manual_seed(B + Kd + p)
    X = torch.randn(B, p, Kd, device=DEV, generator=g) if tk else torch.randn(B, Kd, p, device=DEV, generator=g)
    X[:, 3] = 0.0   # a zero row and a zero column of the operand: a row and a column of exact
    X[:, :, 5] = 0.0   # zeros in the product, whichever way it lies
    C = K.gram_f64(X, X, ta=tk, tb=tk)
    Cf = K.gram_f64(X, X.clone(), ta=tk, tb=tk)
    Xd = X.double()
    ref = Xd @ Xd.transpose(1, 2) if tk else Xd.transpose(1, 2) @ Xd
    assert torch.equal(_bits(C), _bits(C.transpose(1, 2)))
    assert torch.equal(_bits(C), _bits(Cf))
    assert ((C - ref).abs().max() / ref.abs().max()).item() < 1e-13
