"""cq_hadamard_cols against fp64 (hadamard_cases.hadamard64 on the transposed input).  Bar: a butterfly stage is
orthogonal up to sqrt(2) with relative error u = 2^-24 and the scale is one more rounding, so for a column
||y^ - y||_2 <= (p + 1) u ||x_col||_2 + O(u^2), p = log2 P; the tests take twice that for every element.
The table crosses every kernel instantiation (tiles of 2^0 .. 2^8 rows: P <= 16 stays in registers, 32 is the
first LDS exchange, 256 the largest single pass, 512 the first two-pass P) with a column count that ends in a
cut group of column tiles and, where ld is a multiple of four, one that also fills whole groups."""
import numpy as np
import pytest
import torch

from hadamard_cases import hadamard64
from ee274_convexcaldera_llm_quantization_amd import _lib as K

pytestmark = pytest.mark.gpu
DEV, SENTINEL = "cuda:0", 12345.0

# (P, cols, n_in, n_out, ld - cols for x and y, signs: "" | "i" | "o" | "io")
TABLE = [(1, 1, 1, 1, 3, "io"), (1, 516, 1, 1, 0, "i"), (2, 5, 1, 2, 2, "o"), (2, 516, 2, 1, 4, ""),
         (4, 516, 3, 4, 0, "io"), (8, 516, 8, 5, 4, "i"), (8, 33, 5, 8, 2, "o"),
         (16, 33, 11, 16, 2, "i"), (16, 516, 16, 9, 0, "io"), (32, 70, 32, 32, 1, "o"), (32, 260, 17, 1, 4, "io"),
         (64, 132, 33, 64, 0, "i"), (128, 70, 128, 100, 2, "io"), (256, 32, 256, 256, 0, ""), (256, 33, 1, 256, 2, "io"),
         (256, 70, 200, 130, 1, "i"), (512, 5, 257, 512, 1, "io"), (512, 516, 512, 300, 0, "o"),
         (4096, 32, 2752, 4096, 4, "io"), (4096, 516, 4096, 2752, 0, "i"), (32768, 8, 22016, 32768, 0, "io"),
         (32768, 8, 32768, 1, 1, "")]


def _signs(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).choice(np.array([-1, 1, -128, 0, 127], dtype=np.int8), n))


def _run(x, P, n_out, ld_extra, si=None, so=None):
    """x (n_in, cols) -> (y, the whole y buffer): x's pad rows and columns hold NaN, y starts as the sentinel."""
    n_in, cols = x.shape
    xb = torch.full((n_in + 2, cols + ld_extra), float("nan"), device=DEV)
    yb = torch.full((n_out + 2, cols + ld_extra), SENTINEL, device=DEV)
    xb[:n_in, :cols] = x.to(DEV)
    K.hadamard_cols(xb[:n_in, :cols], yb[:n_out, :cols], n_in=n_in, n_out=n_out, P=P,
                    sign_in=None if si is None else si.to(DEV), sign_out=None if so is None else so.to(DEV))
    return yb[:n_out, :cols].cpu(), yb.cpu()


def _ref(x, P, n_out, si=None, so=None):
    X = np.zeros((P, x.shape[1]))
    X[:x.shape[0]] = x.double().numpy() * (1 if si is None else np.where(si.numpy() < 0, -1.0, 1.0)[:, None])
    y = hadamard64(np.ascontiguousarray(X.T), P).T[:n_out] / np.sqrt(P)
    return y * (1 if so is None else np.where(so.numpy() < 0, -1.0, 1.0)[:, None])


@pytest.mark.parametrize("P,cols,n_in,n_out,ld_extra,signs", TABLE, ids=lambda v: str(v) or "none")
def test_against_fp64(P, cols, n_in, n_out, ld_extra, signs):
    x = torch.from_numpy(np.random.default_rng(P + cols).standard_normal((n_in, cols)).astype(np.float32))
    si, so = _signs(n_in, 1) if "i" in signs else None, _signs(n_out, 2) if "o" in signs else None
    y, yb = _run(x, P, n_out, ld_extra, si, so)
    bar = (np.log2(P) + 1) * 2.0 ** -23 * np.linalg.norm(x.double().numpy(), axis=0)
    err = np.abs(y.double().numpy() - _ref(x, P, n_out, si, so))
    print(f"max err / bar = {float((err / bar).max()):.3f}")
    assert np.isfinite(y.numpy()).all() and (err <= bar).all()
    yb[:n_out, :cols] = SENTINEL
    assert bool((yb == SENTINEL).all())  # rows past n_out and columns past cols are not written


@pytest.mark.parametrize("P", [4, 64, 4096])
def test_small_integers_are_exact(P):
    """|x| <= 8 and c a power of two: every partial sum is an integer below 2^24 in any order."""
    x = torch.from_numpy(np.random.default_rng(P).integers(-8, 9, (P, 37)).astype(np.float32))
    si, so = _signs(P, 3), _signs(P, 4)
    assert np.array_equal(_run(x, P, P, 3, si, so)[0].double().numpy(), _ref(x, P, P, si, so))


@pytest.mark.parametrize("P", [16, 256, 4096])
def test_a_columns_bits_do_not_depend_on_where_it_stands(P):
    """Alone, at column 7 of an aligned 516-column matrix (vector loads), at column 69 of one with ld = 71."""
    rng = np.random.default_rng(P)
    col = torch.from_numpy(rng.standard_normal((P - 3, 1)).astype(np.float32))
    outs = [_run(col, P, P, 0)[0][:, 0]]
    for cols, at, ld_extra in ((516, 7, 0), (70, 69, 1)):
        x = torch.from_numpy(rng.standard_normal((P - 3, cols)).astype(np.float32))
        x[:, at] = col[:, 0]
        outs.append(_run(x, P, P, ld_extra)[0][:, at])
    assert all(torch.equal(o.view(torch.int32), outs[0].view(torch.int32)) for o in outs[1:])
