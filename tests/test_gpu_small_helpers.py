"""Library entries the engine calls in its error and solver paths that had no test of their own:
cq_batched_dot (the LPLR error's inner products), cq_scale_rc (the factor scalings, among them
the transposed form that builds R), cq_dequant_nf and cq_ritz_product_error (the solver's
stopping test), each against a plain numpy fp64 reference at a derived bar."""
import numpy as np
import pytest
import torch

from oracle import caldera_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3


@pytest.fixture(scope="module")
def K():
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    K.load()
    return K


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ------------------------------------------------------------------------------ batched_dot
@pytest.mark.parametrize("numel", [1, 1000, 70000])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_batched_dot(K, dt, numel):
    """out[b] = <x[b], y[b]> accumulated in fp64, one block (numel 1, 1000) and many (70000).
    fp32 products are exact in fp64, so only the summation order differs from numpy's:
    |out - ref| <= numel 2^-52 sum |x_i y_i| (fp64 inputs: the products round once, in the
    kernel as in numpy)."""
    rng = np.random.default_rng(numel + (dt == np.float64))
    x = (rng.standard_normal((B, numel)) * 10.0 ** rng.uniform(-2, 2, (B, numel))).astype(dt)
    y = rng.standard_normal((B, numel)).astype(dt)
    out = K.batched_dot(dev(x), dev(y)).cpu().numpy()
    prod = x.astype(np.float64) * y.astype(np.float64)
    ref = np.array([float(np.sum(prod[b])) for b in range(B)])
    bound = numel * 2.0 ** -52 * np.abs(prod).sum(1)
    print(f"batched_dot {np.dtype(dt).name} numel {numel}: |out - ref| / bound {np.abs(out - ref) / bound}")
    assert (np.abs(out - ref) <= bound).all(), (out, ref, bound)


# ------------------------------------------------------------------------------ scale_rc
@pytest.mark.parametrize("per_matrix", [True, False], ids=["per-matrix", "shared"])
@pytest.mark.parametrize("which", ["row", "col", "both"])
@pytest.mark.parametrize("trans", [False, True], ids=["plain", "trans"])
@pytest.mark.parametrize("shape", [(33, 20), (64, 200), (200, 64)])
def test_scale_rc(K, shape, trans, which, per_matrix):
    """Y[b][i][j] = op(X[b])[i][j] rowscale[i] colscale[j]: plain and transposed X, either scale
    or both, (B, len) scales and shared ones.  One scale: the fp32 product, bit-exact; two:
    within 2^-22 relative of the fp64 product (two fp32 roundings)."""
    rng = np.random.default_rng(shape[0] * 7 + shape[1] + 2 * trans)
    X = rng.standard_normal((B,) + shape).astype(np.float32)
    rows, cols = shape[::-1] if trans else shape
    rs = (10.0 ** rng.uniform(-2, 2, (B, rows))).astype(np.float32) if which != "col" else None
    cs = (10.0 ** rng.uniform(-2, 2, (B, cols))).astype(np.float32) if which != "row" else None
    if not per_matrix:
        rs, cs = (None if rs is None else rs[1]), (None if cs is None else cs[1])
    out = K.scale_rc(dev(X), trans=trans, rowscale=None if rs is None else dev(rs), colscale=None if cs is None else dev(cs))
    assert out.shape == (B, rows, cols)
    out = out.cpu().numpy()
    op = X.transpose(0, 2, 1) if trans else X
    r_ = 1.0 if rs is None else (rs[:, :, None] if per_matrix else rs[None, :, None])
    c_ = 1.0 if cs is None else (cs[:, None, :] if per_matrix else cs[None, None, :])
    if which == "both":
        ref = op.astype(np.float64) * r_.astype(np.float64) * c_.astype(np.float64)
        assert (np.abs(out - ref) <= 2.0 ** -22 * np.abs(ref)).all()
    else:
        assert np.array_equal(out, (op * (r_ if cs is None else c_)).astype(np.float32))


@pytest.mark.parametrize("which", ["row", "col"])
def test_scale_rc_in_place(K, which):
    """out= aliasing the input, as the engine scales L and R in place (engine.py: K.scale_rc(R,
    colscale=rinv, out=R), K.scale_rc(R, rowscale=rs, out=R)): the bits of a separate output."""
    rng = np.random.default_rng(3)
    X = dev(rng.standard_normal((B, 64, 200)).astype(np.float32))
    s = dev((10.0 ** rng.uniform(-2, 2, (B, 64 if which == "row" else 200))).astype(np.float32))
    kw = {"rowscale" if which == "row" else "colscale": s}
    sep = K.scale_rc(X, **kw)
    Y = X.clone()
    assert K.scale_rc(Y, out=Y, **kw) is Y
    assert torch.equal(Y, sep) and not torch.equal(Y, X)


# ------------------------------------------------------------------------------ dequantize_nf
@pytest.mark.parametrize("block", [64, "all"])
@pytest.mark.parametrize("bits", [4, 2])
def test_dequantize_nf(K, bits, block):
    """cq_dequant_nf = level[idx] * scale[block]: bit-equal to quantize_nf's own deq output and
    to the oracle's dequantize_nf, blocks of 64 and the whole matrix."""
    m, n = 64, 256
    rng = np.random.default_rng(bits)
    x = (rng.standard_normal((B, m * n)) * 0.02).astype(np.float32)
    x[:, ::97] *= 20.0
    bs = m * n if block == "all" else block
    q = K.quantize_nf(dev(x), bs, bits)
    d = K.dequantize_nf(q["idx"], q["scale"].view(-1), bits)
    assert torch.equal(d.view(B, -1), q["deq"])
    ref = O.dequantize_nf(q["idx"].cpu().numpy().reshape(-1, bs), q["scale"].cpu().numpy().reshape(-1, 1), bits, (B, m * n))
    assert np.array_equal(d.cpu().numpy().reshape(B, -1), ref)
    idx_ref, sf_ref = O.quantize_nf(x, bits, bs)
    assert np.array_equal(q["idx"].cpu().numpy().reshape(-1, bs), idx_ref)


# ------------------------------------------------------------------------------ ritz_product_error
RITZ_K, RITZ_P, RITZ_R = 128, 32, 16
RITZ_SEEDS = (0, 1, 2, 3)
# the largest relative deviation from the fp64 formula measured on an MI355X over RITZ_SEEDS
# (see the test's docstring), and the bar at 8 times that
RITZ_MEASURED = 7.84e-8
RITZ_BAR = 8 * RITZ_MEASURED


def _ritz_inputs(seed):
    """X orthonormal (k x p); theta descending: matrix 0 spans 1e6 (activation-weighted Y),
    matrix 1 is flat (1 - 1e-5 i: every gap below the 1e-3 theta_0 floor), matrix 2 in between;
    Z = theta X + E with E's column i of norm rho_i theta_i, rho_i log-uniform in [1e-3, 1e-1],
    orthogonal to X's span as a Rayleigh-Ritz residual is."""
    rng = np.random.default_rng(seed)
    k, p = RITZ_K, RITZ_P
    i = np.arange(p)
    theta = np.stack([10.0 ** (6.0 * (1.0 - i / (p - 1.0))), 1.0 - 1e-5 * i, 50.0 * 0.8 ** i])
    X = np.stack([np.linalg.qr(rng.standard_normal((k, p)))[0] for _ in range(B)]).astype(np.float32)
    X64 = X.astype(np.float64)
    E = rng.standard_normal((B, k, p))
    E -= X64 @ (X64.transpose(0, 2, 1) @ E)
    rho = 10.0 ** rng.uniform(-3, -1, (B, p))
    E *= (rho * theta / np.linalg.norm(E, axis=1))[:, None, :]
    Z = (theta[:, None, :] * X64 + E).astype(np.float32)
    ysq = (theta.sum(1) * rng.uniform(1.0, 2.0, B))
    return X, Z, theta, ysq


def _ritz_ref(X, Z, theta, ysq, r):
    """The header's formula in fp64: sqrt(sum_{i<r} ||e_i||^2 theta_i / gap_i^2 / ysq)."""
    e = Z.astype(np.float64) - theta[:, None, :] * X.astype(np.float64)
    s = (e * e).sum(1)[:, :r]
    th = np.maximum(theta[:, :r], 0.0)
    raw = th - theta[:, -1:]
    gap = np.maximum(raw, 1e-3 * np.abs(theta[:, :1]))
    return np.sqrt((s * th / gap ** 2).sum(1) / ysq), (raw < 1e-3 * np.abs(theta[:, :1]))


def test_ritz_product_error(K):
    """cq_ritz_product_error against the header's formula in fp64, k = 128, p = 32, r = 16, one
    wide spectrum (theta spanning 1e6), one flat (every column on the max(., 1e-3 theta_0) gap
    floor) and one in between, planted residuals of relative size 1e-3 .. 1e-1.

    The kernel's precision is not documented: it forms e = Z - theta X in fp32 (theta rounded to
    fp32, one product and one difference rounding), sums the squares in fp64 and rounds the
    result to fp32.  Measured on an MI355X over RITZ_SEEDS, the largest relative deviation from
    the fp64 formula is 7.84e-8 (per seed 7.8e-8, 4.0e-8, 3.4e-8, 4.1e-8): the fp32 rounding of
    the output (2^-24 = 6e-8) and little else, far below the 1e-5 of an fp32 sum of 128 terms.
    The bar is 8 times the measurement (rounding varies with the inputs)."""
    worst = 0.0
    for seed in RITZ_SEEDS:
        X, Z, theta, ysq = _ritz_inputs(seed)
        ref, floored = _ritz_ref(X, Z, theta, ysq, RITZ_R)
        assert floored[1].all() and not floored[0].any()       # the gap floor is hit, and not everywhere
        out = K.ritz_product_error(dev(X), dev(Z), dev(theta), RITZ_R, dev(ysq)).cpu().numpy().astype(np.float64)
        dev_ = np.abs(out - ref) / ref
        print(f"ritz_product_error seed {seed}: out {out}, fp64 {ref}, relative deviation {dev_}")
        worst = max(worst, float(dev_.max()))
    print(f"ritz_product_error: largest relative deviation {worst:.3e}")
    assert worst <= RITZ_BAR, (worst, RITZ_BAR)
