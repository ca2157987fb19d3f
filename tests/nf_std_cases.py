"""numpy restatement of the standardised NF4 / NF2 quantiser (csrc/cq_codebook.hip,
cq_quantize_nf_std; the reference's quantization_stable_nf4.py:187-200 and :221-224), shared by
tests/test_nf_std_host.py and tests/test_gpu_nf_std.py.  Per block of bs fp32 elements:

  mean32 = bs <= 256: fp32 sum in torch's CPU order / f32(bs); else: f32(fp64 sum / bs)
  std32  = max(f32(sqrt(sum (x - mean64)^2 / (bs - 1))), eps), fp64 sum about the fp64 mean
  z      = (x - mean32) / std32                     two fp32 operations
  idx    = #{t : z > (l_t + l_{t+1}) / 2}           fp32 thresholds
  deq    = f32(level[idx] * std32) + mean32         two roundings
"""
import os

import numpy as np

from oracle.caldera_oracle import torch_row_sum_f32

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LEVELS = {4: np.array([-1.334, -1.0, -0.784, -0.617, -0.476, -0.347, -0.226, -0.112,
                       0.0, 0.112, 0.226, 0.347, 0.476, 0.617, 0.784, 1.0], dtype=f32),
          2: np.array([-0.8165, -0.3333, 0.3333, 0.8165], dtype=f32)}
METHODS = (("nf4", 4), ("nf2", 2))


def thresholds(bits):
    lv = LEVELS[bits]
    return ((lv[:-1] + lv[1:]) / f32(2)).astype(f32)


def block_stats(blocks, eps=1e-8):
    """(mean32, std32), each (nblk,) fp32, of blocks (nblk, bs) fp32."""
    nblk, bs = blocks.shape
    assert bs >= 2
    b64 = blocks.astype(np.float64)
    mean64 = b64.sum(axis=1) / bs
    if bs <= 256:
        mean32 = np.array([torch_row_sum_f32(r) for r in blocks], dtype=f32) / f32(bs)
    else:
        mean32 = mean64.astype(f32)
    var = ((b64 - mean64[:, None]) ** 2).sum(axis=1) / (bs - 1)
    sd = np.sqrt(var).astype(f32)
    std32 = np.where(np.isnan(sd), sd, np.maximum(sd, f32(eps))).astype(f32)
    return mean32, std32


def standardise(blocks, mean32, std32):
    return ((blocks - mean32[:, None]).astype(f32) / std32[:, None]).astype(f32)


def emit(blocks, mean32, std32, bits):
    """(idx (nblk, bs) uint8, deq (nblk, bs) fp32) for given block parameters."""
    z = standardise(blocks, mean32, std32)
    idx = np.zeros(blocks.shape, dtype=np.uint8)
    for t in thresholds(bits):
        idx += (z > t).astype(np.uint8)
    deq = ((LEVELS[bits][idx] * std32[:, None]).astype(f32) + mean32[:, None]).astype(f32)
    return idx, deq


def quantize(x, bits, bs, eps=1e-8):
    """dict(idx (nblk, bs) uint8, mean / std (nblk, 1) fp32, deq (nblk, bs) fp32) of x (any shape)."""
    blocks = np.ascontiguousarray(x, dtype=f32).reshape(-1, bs)
    mean32, std32 = block_stats(blocks, eps)
    idx, deq = emit(blocks, mean32, std32, bits)
    return dict(idx=idx, mean=mean32[:, None], std=std32[:, None], deq=deq)


def planted(m, n, seed, n_out=40):
    """test_gpu_codebook._planted: small normal values with a few planted outliers."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((m, n)) * 0.02).astype(f32)
    idx = rng.integers(0, m * n, n_out)
    x.reshape(-1)[idx] = (rng.choice([-1.0, 1.0], n_out) * rng.uniform(0.2, 0.5, n_out)).astype(f32)
    return x


def kat_inputs():
    """{name: x} of the quantiser KAT inputs (tests/golden/quant_kat.npz in_*)."""
    kat = np.load(os.path.join(GOLDEN, "quant_kat.npz"), allow_pickle=False)
    return {k[3:]: kat[k] for k in kat.files if k.startswith("in_")}


def fixture():
    return np.load(os.path.join(GOLDEN, "nf_std_kat.npz"), allow_pickle=False)


def kat_cases():
    """(key, name, method, bits, bs) of every quantiser case of nf_std_kat.npz."""
    out = []
    for name, x in kat_inputs().items():
        for method, bits in METHODS:
            for bs in (64, "all"):
                out.append((f"{method}_bs{bs}_{name}", name, method, bits, x.size if bs == "all" else bs))
    return out


def bits_of(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def compare_with_fixture(got, fx, key, x, bits, bs):
    """`got` (dict idx / mean / std / deq in the (nblk, bs) layout) against the reference's outputs of
    case `key` of nf_std_kat.npz: std bit-equal always; idx and deq bit-equal where the mean has the
    reference's bits, else by the near-threshold rule below.  Returns whether the means were equal."""
    exp = {k: fx[f"{key}_{k}"] for k in ("idx", "mean", "std", "deq")}
    assert np.array_equal(bits_of(got["std"]), bits_of(exp["std"])), key
    same_mean = np.array_equal(bits_of(got["mean"]), bits_of(exp["mean"]))
    got_idx, got_deq = np.asarray(got["idx"]).reshape(-1, bs), np.asarray(got["deq"]).reshape(-1, bs)
    exp_idx, exp_deq = exp["idx"].reshape(-1, bs), exp["deq"].reshape(-1, bs)
    assert got_idx.dtype == np.uint8
    if same_mean:
        assert np.array_equal(got_idx, exp_idx), key
        assert np.array_equal(bits_of(got_deq), bits_of(exp_deq)), key
        return True
    # the reference's own fp32 summation error moved the mean: an index may differ only where z is
    # within |dmean| / std (the shift of z) + 4 * 2^-24 max(1, |z|) (the two fp32 roundings of z on
    # either side) of a threshold
    blocks = np.ascontiguousarray(x, dtype=f32).reshape(-1, bs)
    mean, std = np.asarray(got["mean"], f32).reshape(-1), np.asarray(got["std"], f32).reshape(-1)
    z = standardise(blocks, mean, std).astype(np.float64)
    dmean = np.abs(mean.astype(np.float64) - exp["mean"].reshape(-1).astype(np.float64))[:, None]
    dist = np.abs(z[..., None] - thresholds(bits).astype(np.float64)).min(axis=-1)
    near = dist <= dmean / std.astype(np.float64)[:, None] + 4 * 2.0 ** -24 * np.maximum(1.0, np.abs(z))
    differs = got_idx != exp_idx
    assert not (differs & ~near).any(), (key, int((differs & ~near).sum()))
    assert near.mean() <= 1e-4, (key, float(near.mean()))
    agree = ~differs
    tol = dmean + np.spacing(np.abs(exp_deq)).astype(np.float64)   # the shift, then one re-rounding of the final add
    err = np.abs(got_deq.astype(np.float64) - exp_deq.astype(np.float64))
    assert (err[agree] <= np.broadcast_to(tol, err.shape)[agree]).all(), key
    return False
