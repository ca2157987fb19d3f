"""Cases and the fp64 reference of the packed linear layer (include/caldera_hip.h, cq_linear_forward):

    y[t, i] = gs * ((s / k) * sum_j x[t, j] c[i, j] + sum_q z[t, q] L[i, q]) (+ bias[i])
    z[t, q] = sum_j x[t, j] R[q, j]                           k = 2^(bits-1) - 1

Inputs are host-seeded numpy, so the bytes are the same on every machine; the reference is
evaluated in fp64 from the operands as the kernel sees them (fp16 x, L, R; fp32 s, gs, bias;
s / k one fp32 division).

Exact cases: small integers (x in -4..4, codes in -k..k, L, R in -2..2, s = k / 2 so s / k = 0.5,
gs = 4): every partial result in any summation order is a multiple of 0.5 below 2^24 units, so
the kernel must match the reference bit for bit.  "exact16" cases are scaled down (x, L, R in
-1..1, r <= 8, n <= 64) so that y is an even integer of at most 2048 and fp16 output must equal
it too.

Random cases: x ~ N(0, 1), L, R ~ 0.15 N(0, 1) in fp16, s = 0.05, gs = 1.7, with the elementwise
worst-case fp32 bound for any summation order as the bar:

    |y - y64| <= (n + r + 32) 2^-24 A,   A = gs ((s / k) |x| |c|^T + |x| |R|^T |L|^T)

(the + 32 covers the scalings and z held as split fp16 halves).

x[0, 0], x[0, n - 1] and (T > 1) x[1, 0] are set to the largest magnitude of the case's x, so that
the planted single-code faults of test_linear_host.py show at every seed.
"""
from dataclasses import dataclass

import numpy as np

from weight_stride_cases import pack_codes

f16, f32, f64 = np.float16, np.float32, np.float64

DECODE_MAX_TOKENS = 16


@dataclass(frozen=True)
class Case:
    kind: str       # "exact" | "exact16" | "random"
    m: int
    n: int
    r: int
    bits: int
    T: int
    bias: bool = False

    @property
    def id(self):
        return f"{self.kind}-m{self.m}n{self.n}r{self.r}b{self.bits}T{self.T}" + ("-bias" if self.bias else "")

    @property
    def k(self):
        return 2 ** (self.bits - 1) - 1

    @property
    def seed(self):
        return (self.m * 1000003 + self.n * 1009 + self.r * 101 + self.bits * 11 + self.T
                + {"exact": 0, "exact16": 1, "random": 2}[self.kind] * 7919)


_SHAPES = ([(33, 64, 8, b, T) for b in (2, 4) for T in (1, 5)]
           + [(48, 198, 40, b, T) for b in (2, 4) for T in (3, 16)]
           + [(80, 898, 200, b, T) for b in (2, 4) for T in (16, 17, 64)]
           + [(272, 512, 16, 2, 130)]
           + [(48, 198, 0, 2, T) for T in (3, 17)])

EXACT = [Case("exact", *s) for s in _SHAPES] + [Case("exact", 33, 64, 8, 4, 5, bias=True)]
EXACT16 = [Case("exact16", 33, 64, 8, b, T) for b in (2, 4) for T in (1, 5, 17)]
RANDOM = [Case("random", *s) for s in _SHAPES] + [Case("random", 33, 64, 8, 2, 5, bias=True)]
ALL = EXACT + EXACT16 + RANDOM


def row_bytes(n, bits):
    """Bytes per row of the inference layout (rows padded to 16 bytes)."""
    return -(-(n * bits) // 128) * 16


def inference_codes(c, bits):
    """(m, n) codes -> (m, row_bytes) uint8 inference layout, the tail holding code 0."""
    m, n = c.shape
    rb = row_bytes(n, bits)
    full = np.zeros((m, rb * 8 // bits), dtype=np.int8)
    full[:, :n] = c
    return pack_codes(full, bits).reshape(m, rb)


def storage_codes(c, bits):
    """(m, n) codes -> flat storage-layout bytes on the (m, n padded to 4) grid and n_padded."""
    m, n = c.shape
    npad = n + (-n) % 4
    full = np.zeros((m, npad), dtype=np.int8)
    full[:, :n] = c
    return pack_codes(full, bits), npad


_CACHE = {}


def inputs(case: Case):
    """dict(x (T, n) f16, c (m, n) int8, L (m, r) f16, R (r, n) f16, s, gs (f32), bias (m,) f32 | None);
    built once per case and shared (treat as read-only)."""
    if case in _CACHE:
        return _CACHE[case]
    rng = np.random.default_rng(case.seed)
    m, n, r, k, T = case.m, case.n, case.r, case.k, case.T
    c = rng.integers(-k, k + 1, (m, n)).astype(np.int8)
    if case.kind == "random":
        x = rng.standard_normal((T, n)).astype(f16)
        L = (0.15 * rng.standard_normal((m, r))).astype(f16)
        R = (0.15 * rng.standard_normal((r, n))).astype(f16)
        s, gs = f32(0.05), f32(1.7)
        bias = rng.standard_normal(m).astype(f32) if case.bias else None
    else:
        xa, la = (4, 2) if case.kind == "exact" else (1, 1)
        x = rng.integers(-xa, xa + 1, (T, n)).astype(f16)
        L = rng.integers(-la, la + 1, (m, r)).astype(f16)
        R = rng.integers(-la, la + 1, (r, n)).astype(f16)
        s, gs = f32(k / 2), f32(4.0)
        bias = (rng.integers(-8, 9, m) * 0.5).astype(f32) if case.bias else None
    big = np.abs(x.astype(f64)).max()
    for (t, j) in ((0, 0), (0, n - 1)) + (((1, 0),) if T > 1 else ()):
        x[t, j] = f16(big if x[t, j] >= 0 else -big)
    out = dict(x=x, c=c, L=L, R=R, s=s, gs=gs, bias=bias)
    _CACHE[case] = out
    return out


FAULTS = ("flip_last", "flip_first", "swap_L", "drop_R_last", "drop_gs", "s_for_sk", "pad_code")


def fault_applies(case: Case, fault: str) -> bool:
    if fault in ("swap_L", "drop_R_last"):
        return case.r > 0
    if fault == "s_for_sk":
        return case.bits == 4
    if fault == "pad_code":  # a pad column exists and x's buffer holds a finite value there
        return row_bytes(case.n, case.bits) * 8 // case.bits > case.n and case.T > 1
    return True


def _flip(v, k):
    return -v if v != 0 else k


def reference(case: Case, fault: str | None = None):
    """(y64, bar): the fp64 reference (T, m) and the elementwise bar of the random cases.
    fault: one planted error (FAULTS), for checking that the cases can see it.  "pad_code"
    models a nonzero code in row 0's first pad column meeting what a contiguous x holds
    there: the first element of the next row."""
    d = inputs(case)
    x, L, R = d["x"].astype(f64), d["L"].astype(f64), d["R"].astype(f64)
    c = d["c"].astype(f64)
    k = f32(case.k)
    sk = f64(d["s"] / k)        # one fp32 division
    gs = f64(d["gs"])
    if fault == "flip_last":
        c[-1, -1] = _flip(c[-1, -1], case.k)
    elif fault == "flip_first":
        c[0, 0] = _flip(c[0, 0], case.k)
    elif fault == "swap_L":
        L[[0, 1]] = L[[1, 0]]
    elif fault == "drop_R_last":
        R[-1] = 0
    elif fault == "drop_gs":
        gs = f64(1.0)
    elif fault == "s_for_sk":
        sk = f64(d["s"])
    code = x @ c.T
    if fault == "pad_code":
        code[:-1, 0] += x[1:, 0] * case.k
    lr = (x @ R.T) @ L.T
    y = gs * (sk * code + lr)
    if d["bias"] is not None:
        y = y + d["bias"].astype(f64)
    A = f64(d["gs"]) * (f64(d["s"] / k) * (np.abs(x) @ np.abs(d["c"].astype(f64)).T)
                        + (np.abs(x) @ np.abs(d["R"].astype(f64)).T) @ np.abs(d["L"].astype(f64)).T)
    bar = (case.n + case.r + 32) * 2.0 ** -24 * A
    return y, bar
