"""Cases and the fp64 reference of the packed linear layer's input gradient (include/caldera_hip.h,
cq_linear_backward_input):

    dx[t, j] = gs * ((s / k) * sum_i dy[t, i] c[i, j] + sum_q u[t, q] R[q, j])
    u[t, q]  = sum_i dy[t, i] L[i, q]                          k = 2^(bits-1) - 1

Inputs are host-seeded numpy, so the bytes are the same on every machine; the reference is
evaluated in fp64 from the operands as the kernel sees them (fp16 dy, L, R; fp32 s, gs; s / k one
fp32 division).  The contraction runs over the m code rows, in chunks of 32 (CHUNK_ROWS) that the
kernel transposes through a ring of two LDS images.

Shapes (m, n, r), each at bits 2 and 4 and T in {1, 5, 17, 64}, plus (272, 512, 16) and (160, 256, 128) at T = 130:

    (33, 64, 8)      m odd: dy rows 2-byte aligned; one ragged row chunk
    (48, 198, 40)    n, r ragged
    (80, 898, 200)   898: storage / inference strides differ; r not a multiple of 32
    (272, 512, 16)   9 row chunks: the LDS ring wraps
    (600, 198, 40)   19 row chunks
    (2600, 48, 40)   82 row chunks, one column tile
    (198, 48, 0)     codes only
    (160, 256, 128)  also at T = 130: every operand aligned and whole 128-column tiles of L and R, so that
                     each product's mask-free interior loop runs (the u product's at T = 64: 64 whole tokens
                     per workgroup; the code and R products' at T = 130: 128), 5 and 4 chunks long

and one case with a bias on the layer (the bias does not enter dx).

Exact cases: dy in -4..4, codes in -k..k, L, R in -2..2, s = k / 2 (s / k = 0.5), gs = 4: every
partial result in any order is a multiple of 0.5 with sums of absolute terms below 2^24 units
(the largest is 8.6e5 units, at m = 2600), and u <= 20 800 is exact as hi + lo, so dx and u_out
must equal the reference bit for bit in fp32.  "exact16": (33, 64, 8) with dy, L, R in -1..1, so
dx is an even integer of magnitude <= 1518 and fp16 dx must equal it too.

Random cases: dy ~ N(0, 1), L, R ~ 0.15 N(0, 1) in fp16, s = 0.05, gs = 1.7, with the forward's
elementwise worst-case fp32 bar, the contraction lengths swapped:

    |dx - dx64| <= (m + r + 32) 2^-24 A,   A = gs ((s / k) |dy| |c| + |dy| |L| |R|)
    |u - u64|   <= (m + 8) 2^-24 |dy| |L|

dy[0, 0], dy[0, m - 1] and (T > 1) dy[1, 0] are set to the largest magnitude of the case's dy, so
that the planted faults below show at every seed.

Planted faults (`reference(case, fault)`): "flip_first" / "flip_last" one code, moved to the
farthest code (by k at least); "tr_block" the
first 16 x 16 block of the codes transposed (a tile that was not transposed, or twice);
"drop_last_rows" the rows from 32 floor((m - 1) / 32) on contribute nothing (the ragged last
chunk lost); "pad_row" a phantom row m with code k in column 0 meets what a contiguous dy holds
past its row, the next token's dy[., 0] (a pad row that was masked out of the loads but not
zeroed); "drop_gs"; "s_for_sk" (4-bit only; at 2 bits k = 1); "swap_R" rows 0 and 1; "drop_L_last"
the last row of L.

Against the bar of a random case a fault that touches a bounded number of the m rows is small on
a long contraction: its signal is a fixed number of terms while A grows like m (1 + r) terms and
the bar's factor like m.  A numpy run of these formulas gave, at (80, 898, 200) / (600, 198, 40) /
(2600, 48, 40): flip_* >= 12 / 15 / 0.7 bars, pad_row >= 37 / 16 / 0.8, tr_block >= 124 / 49 / 2.8,
drop_last_rows >= 1460 / 230 / 8.0, drop_L_last >= 766 / 129 / 5.5 -- and drop_gs >= 49, swap_R >= 44,
s_for_sk >= 186 at m = 2600.  So the row-local faults are checked on random cases where
m (r + 1) <= 25 000 (ROW_LOCAL_LIMIT) and on the long case by the exact cases alone, where any
difference fails; the three global faults must show on every random case.  swap_R at T = 1 hangs
on one token's u[0] - u[1] and is below ten bars at some seed of a long case about one time in
ten; the seeds' constant was chosen among a few so that every pair checked shows >= 10 bars (the
smallest is 12.7), which test_linear_backward_host.py asserts for the cases as they are.
"""
from dataclasses import dataclass

import numpy as np

from linear_cases import inference_codes, row_bytes  # noqa: F401  (re-exported for the tests)

f16, f32, f64 = np.float16, np.float32, np.float64

CHUNK_ROWS = 32          # code rows per chunk of csrc/cq_linear_bwd.hip (kRows), restated
ROW_LOCAL_LIMIT = 25000  # m (r + 1) up to which a row-local fault is checked against a random bar


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
                + {"exact": 0, "exact16": 1, "random": 2}[self.kind] * 7919 + 108729)


SHAPES = ((33, 64, 8), (48, 198, 40), (80, 898, 200), (272, 512, 16), (600, 198, 40), (2600, 48, 40), (198, 48, 0),
          (160, 256, 128))
TOKENS = (1, 5, 17, 64)
_ALL = [(m, n, r, b, T) for (m, n, r) in SHAPES for b in (2, 4) for T in TOKENS] + \
       [(m, n, r, b, 130) for (m, n, r) in ((272, 512, 16), (160, 256, 128)) for b in (2, 4)]

EXACT = [Case("exact", *s) for s in _ALL] + [Case("exact", 33, 64, 8, 4, 5, bias=True)]
EXACT16 = [Case("exact16", 33, 64, 8, b, T) for b in (2, 4) for T in (1, 5, 17)]
RANDOM = [Case("random", *s) for s in _ALL] + [Case("random", 33, 64, 8, 2, 5, bias=True)]
ALL = EXACT + EXACT16 + RANDOM

_CACHE = {}


def inputs(case: Case):
    """dict(dy (T, m) f16, c (m, n) int8, L (m, r) f16, R (r, n) f16, s, gs (f32), bias (m,) f32 | None);
    built once per case and shared (treat as read-only)."""
    if case in _CACHE:
        return _CACHE[case]
    rng = np.random.default_rng(case.seed)
    m, n, r, k, T = case.m, case.n, case.r, case.k, case.T
    c = rng.integers(-k, k + 1, (m, n)).astype(np.int8)
    if case.kind == "random":
        dy = rng.standard_normal((T, m)).astype(f16)
        L = (0.15 * rng.standard_normal((m, r))).astype(f16)
        R = (0.15 * rng.standard_normal((r, n))).astype(f16)
        s, gs = f32(0.05), f32(1.7)
        bias = rng.standard_normal(m).astype(f32) if case.bias else None
    else:
        da, la = (4, 2) if case.kind == "exact" else (1, 1)
        dy = rng.integers(-da, da + 1, (T, m)).astype(f16)
        L = rng.integers(-la, la + 1, (m, r)).astype(f16)
        R = rng.integers(-la, la + 1, (r, n)).astype(f16)
        s, gs = f32(k / 2), f32(4.0)
        bias = (rng.integers(-8, 9, m) * 0.5).astype(f32) if case.bias else None
    big = np.abs(dy.astype(f64)).max()
    for (t, i) in ((0, 0), (0, m - 1)) + (((1, 0),) if T > 1 else ()):
        dy[t, i] = f16(big if dy[t, i] >= 0 else -big)
    out = dict(dy=dy, c=c, L=L, R=R, s=s, gs=gs, bias=bias)
    _CACHE[case] = out
    return out


GLOBAL_FAULTS = ("drop_gs", "s_for_sk", "swap_R")
ROW_LOCAL_FAULTS = ("flip_first", "flip_last", "tr_block", "drop_last_rows", "pad_row", "drop_L_last")
FAULTS = ROW_LOCAL_FAULTS + GLOBAL_FAULTS


def fault_applies(case: Case, fault: str) -> bool:
    if fault in ROW_LOCAL_FAULTS and case.kind == "random" and case.m * (case.r + 1) > ROW_LOCAL_LIMIT:
        return False   # see the module docstring
    if fault in ("swap_R", "drop_L_last"):
        return case.r > 0
    if fault == "s_for_sk":
        return case.bits == 4
    if fault == "pad_row":  # the last chunk has a pad row and dy's buffer holds a finite value past the row
        return case.m % CHUNK_ROWS != 0 and case.T > 1
    return True


def _flip(v, k):
    """The code farthest from v: the fault moves it by k at least (v -> -v would move a 4-bit +-1 by 2)."""
    return k if v <= 0 else -k


def reference(case: Case, fault: str | None = None):
    """(dx64 (T, n), u64 (T, r), bar, ubar): the fp64 reference and the elementwise bars of the
    random cases.  fault: one planted error (FAULTS), for checking that the cases can see it."""
    d = inputs(case)
    dy, L, R = d["dy"].astype(f64), d["L"].astype(f64), d["R"].astype(f64)
    c = d["c"].astype(f64)
    k = f32(case.k)
    sk = f64(d["s"] / k)        # one fp32 division
    gs = f64(d["gs"])
    dyw = dy                    # dy as the products see it
    if fault == "flip_first":
        c[0, 0] = _flip(c[0, 0], case.k)
    elif fault == "flip_last":
        c[-1, -1] = _flip(c[-1, -1], case.k)
    elif fault == "tr_block":
        b = min(16, case.m, case.n)
        c[:b, :b] = c[:b, :b].T.copy()
    elif fault == "drop_last_rows":
        dyw = dy.copy()
        dyw[:, CHUNK_ROWS * ((case.m - 1) // CHUNK_ROWS):] = 0
    elif fault == "drop_gs":
        gs = f64(1.0)
    elif fault == "s_for_sk":
        sk = f64(d["s"])
    elif fault == "swap_R":
        R[[0, 1]] = R[[1, 0]]
    elif fault == "drop_L_last":
        L[-1] = 0
    code = dyw @ c
    if fault == "pad_row":
        code[:-1, 0] += dy[1:, 0] * case.k
    u = dyw @ L
    dx = gs * (sk * code + u @ R)
    ady, aL = np.abs(dy), np.abs(d["L"].astype(f64))
    A = f64(d["gs"]) * (f64(d["s"] / k) * (ady @ np.abs(d["c"].astype(f64))) + (ady @ aL) @ np.abs(d["R"].astype(f64)))
    bar = (case.m + case.r + 32) * 2.0 ** -24 * A
    ubar = (case.m + 8) * 2.0 ** -24 * (ady @ aL)
    return dx, u, bar, ubar
