"""Cases and the fp64 reference of the row-wise Hadamard transform (include/caldera_hip.h,
cq_hadamard_rows):

    y[t, i] = c * sum_{j < n_in} (-1)^popcount(i & j) x[t, j] (+ bias[i])   for i < n_out,  c = 1 / sqrt(P)

Inputs are host-seeded numpy, so the bytes are the same on every machine.  The reference is
built from scipy.linalg.hadamard in fp64; above 256 the Sylvester matrix is applied as its
Kronecker factors H_a (x) H_b (P = a b, b = 256), which is the same matrix without holding P^2
entries.

Exact cases: P a power of 4 (c a power of two), x integers in -4..4: every partial sum in any
stage order is an integer of at most 4 P <= 65536, the scaling is exact, so the fp32 output must
match bit for bit.  With a bias: multiples of 0.5.

Exact16 cases: x in {-1, 0, 1}, P <= 1024: |sum| <= 1024 over sqrt(P) needs at most 11 bits, so an
fp16 output must equal the reference; P <= 64 (at most 7 bits) for a bf16 output.

Random cases: x ~ N(0, 1) held as fp16 / bf16 / fp32, fp32 output, with the bar

    |y - y64| <= 1.01 (log2 P + 2) 2^-24 sum_j |x_j| / sqrt(P)

(log2 P addition levels, the constant, the multiply).

Regimes: rows in {1, 3, 17, 70}; n_in and n_out in {P, P - 5, P / 2 + 1, 1} where P allows.
x[:, 0] and x[0, n_in - 1] hold the case's largest magnitude, so the planted faults of
test_hadamard_host.py show in every case.
"""
from dataclasses import dataclass

import numpy as np
import scipy.linalg

f32, f64 = np.float32, np.float64

XDT = ("f16", "bf16", "f32")


@dataclass(frozen=True)
class Case:
    kind: str       # "exact" | "exact16" | "random"
    P: int
    rows: int
    n_in: int
    n_out: int
    xdt: str        # "f16" | "bf16" | "f32"
    ydt: str
    bias: bool = False

    @property
    def id(self):
        return (f"{self.kind}-P{self.P}r{self.rows}i{self.n_in}o{self.n_out}-{self.xdt}-{self.ydt}"
                + ("-bias" if self.bias else ""))

    @property
    def seed(self):
        return (self.P * 1000003 + self.rows * 10007 + self.n_in * 101 + self.n_out * 13
                + XDT.index(self.xdt) * 5 + XDT.index(self.ydt)
                + {"exact": 0, "exact16": 1, "random": 2}[self.kind] * 7919)


def regimes(P):
    """(rows, n_in, n_out) of one P: every row count and every cut of either side."""
    raw = [(1, P, P), (3, P - 5, P), (17, P, P // 2 + 1), (70, P // 2 + 1, P - 5), (3, 1, P), (17, P - 5, 1),
           (70, P, P)]
    out = []
    for rows, n_in, n_out in raw:
        if 1 <= n_in <= P and 1 <= n_out <= P and (rows, n_in, n_out) not in out:
            out.append((rows, n_in, n_out))
    return out


def _cases(kind, Ps, ydts, bias_every=0):
    out = []
    for P in Ps:
        for i, (rows, n_in, n_out) in enumerate(regimes(P)):
            for ydt in ydts:
                out.append(Case(kind, P, rows, n_in, n_out, XDT[(i + len(out)) % 3] if kind != "exact16" else "f16",
                                ydt, bias=bool(bias_every) and i % bias_every == 1))
    return out


EXACT = _cases("exact", (1, 4, 64, 1024, 4096, 16384), ("f32",), bias_every=2)
EXACT16 = (_cases("exact16", (1, 4, 16, 64, 256, 1024), ("f16",), bias_every=3)
           + _cases("exact16", (1, 4, 16, 64), ("bf16",)))
RANDOM = _cases("random", (2, 32, 128, 512, 2048, 8192, 32768), ("f32",))
ALL = EXACT + EXACT16 + RANDOM


def to_bf16_bits(a):
    """fp32 array -> uint16 bf16 bits, round to nearest even."""
    u = np.ascontiguousarray(a, dtype=f32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bf16_bits(b):
    return (b.astype(np.uint32) << 16).view(f32)


_CACHE = {}


def inputs(case: Case):
    """dict(x (rows, n_in) fp32 holding values exact in case.xdt, bias (n_out,) f32 | None); built
    once per case and shared (treat as read-only)."""
    if case in _CACHE:
        return _CACHE[case]
    rng = np.random.default_rng(case.seed)
    shape = (case.rows, case.n_in)
    if case.kind == "random":
        x = rng.standard_normal(shape).astype(f32)
        x = {"f16": lambda v: v.astype(np.float16).astype(f32), "bf16": lambda v: from_bf16_bits(to_bf16_bits(v)),
             "f32": lambda v: v}[case.xdt](x)
        bias = None
    else:
        a = 4 if case.kind == "exact" else 1
        x = rng.integers(-a, a + 1, shape).astype(f32)
        bias = (rng.integers(-8, 9, case.n_out) * 0.5).astype(f32) if case.bias else None
    big = f32(max(np.abs(x).max(), 1.0))
    x[:, 0] = np.where(x[:, 0] >= 0, big, -big)
    x[0, -1] = big if x[0, -1] >= 0 else -big
    out = dict(x=x, bias=bias)
    _CACHE[case] = out
    return out


def hadamard64(X, P):
    """X (rows, P) fp64 -> X H_P (unnormalised Sylvester matrix, scipy.linalg.hadamard's order)."""
    b = min(P, 256)
    a = P // b
    Ha, Hb = scipy.linalg.hadamard(a).astype(f64), scipy.linalg.hadamard(b).astype(f64)
    Z = X.reshape(-1, a, b) @ Hb           # H symmetric: right-multiplying the low index
    return np.matmul(Ha, Z).reshape(-1, P)


FAULTS = ("flip_sign", "n_in_minus_one")

_REF = {}


def reference(case: Case, fault: str | None = None):
    """(y64 (rows, n_out), bar (rows, 1)): the fp64 reference and the bar of the random cases.
    fault: one planted error (FAULTS), for checking that the cases can see it: the sign of
    H[n_out - 1, 0] flipped, or the last input column dropped."""
    if (case, fault) in _REF:
        return _REF[(case, fault)]
    d = inputs(case)
    P = case.P
    X = np.zeros((case.rows, P), dtype=f64)
    X[:, :case.n_in] = d["x"].astype(f64)
    if fault == "n_in_minus_one":
        X[:, case.n_in - 1] = 0
    c = 1.0 / np.sqrt(f64(P))
    y = hadamard64(X, P)[:, :case.n_out]
    if fault == "flip_sign":       # H[i, 0] = +1 for every i
        y = y.copy()
        y[:, case.n_out - 1] -= 2 * X[:, 0]
    y = y * c
    if d["bias"] is not None:
        y = y + d["bias"].astype(f64)
    bar = 1.01 * (np.log2(P) + 2) * 2.0 ** -24 * np.abs(d["x"].astype(f64)).sum(1, keepdims=True) / np.sqrt(f64(P))
    _REF[(case, fault)] = (y, bar)
    return y, bar
