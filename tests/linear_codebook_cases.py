"""Cases and the fp64 reference of the packed linear layer with an NF4 / NF2 codebook Q
(include/caldera_hip.h, cq_linear_codebook_forward / cq_linear_codebook_backward_input):

    fwd:  y[t, i]  = gs * ((s / D) * sum_j x[t, j]  I[idx[i, j]] + sum_q z~[t, q] l[i, q]) (+ bias[i])
          z~[t, q] = zscale * sum_j x[t, j] rho[q, j]
    bwd:  dx[t, j] = gs * ((s / D) * sum_i dy[t, i] I[idx[i, j]] + sum_q u~[t, q] rho[q, j])
          u~[t, q] = zscale * sum_i dy[t, i] l[i, q]

I = D level: NF4 D = 1000, NF2 D = 10000 (LEVELS); idx the level index; l / rho the fp16 factors
or their uniform codes, zscale the fp32 product of the coded factors' scale / k (1 for fp16), as in
linear_factor_cases.py.  Same pattern as linear_cases.py and linear_backward_cases.py: host-seeded
numpy, the reference evaluated in fp64 from the operands as the kernel sees them, s / D one fp32
division.  `a` is the activation operand: x (T, n) forward, dy (T, m) backward; K its length (the
contraction: n forward, m backward).

Exact cases: integers, s = D / 2 (s / D = 0.5), gs = 4, fp16 factors in -2..2, coded factors with
scale = k (scale / k = 1, zscale = 1), so every term is a multiple of 0.5 and the kernel must match
bit for bit as long as, per output,

    sum |a| |I| + (LR terms) / 0.5  <  2^24 units of 0.5

(test_linear_codebook_host.py asserts it per case from the data).  |a| is bounded for that: at NF4
a in -4..4 holds to K = 898 (4.8 M + 5.7 M units) and a in -1..1 at n = 2600 (3.5 M + 0.8 M); at
NF2 |I| <= 8165 forces a in -1..1 at K <= 898 (7.3 M + 1.4 M) and at n = 2600 at most 1490 + 3
nonzero x per token (12.2 M + 0.5 M), spread over every 256-column chunk.  "exact16" cases
((33, 64, 8), a, factors in -1..1, gs = 2^-4): the fp32 result is exact and below fp16's range, and
the kernel rounds it once, so the fp16 output must equal f16(reference) bit for bit (sums of NF
levels are not fp16 values themselves, unlike the uniform exact16 cases' even integers).

Random cases: a ~ N(0, 1), fp16 factors ~ 0.15 N(0, 1), coded factors with scale 0.3, gs = 1.7,
s = 0.05 (Q = s level is as large as the uniform cases' (s / k) c), with the bar

    |out - out64| <= (P K + r + 32) 2^-24 A,   A = gs ((s / D) |a| |I| + zscale |a| |rho| |l|)

P = 1 at NF4 and 2 at NF2: the two planes are two products per column.

a[0, 0], a[0, K - 1] and (T > 1) a[1, 0] carry the largest magnitude of the case's a, and at NF4
idx[0, 0] = 0 (the level without a mirror image), so that single-code faults show at every seed.

Planted faults (`reference(case, fault)`):
    offset_binary   the index decoded as the uniform code u - k
    sym_table       NF4: index 0 decoded as -1000, the mirror image of index 15
    nibble_order    the indices of a byte taken LSB-first
    drop_lo         NF2: the lo plane lost (I = 8164 / 3332)
    s_for_sD        s applied where s / D belongs
    tr_block        backward: the first 16 x 16 block of the indices transposed
    drop_last_rows  backward: the rows from 32 floor((m - 1) / 32) on contribute nothing
Against a random case's bar (a numpy run of these formulas; the smallest over the random cases):
s_for_sD changes every term by a factor D, >= 15 000 bars.  offset_binary replaces levels of
magnitude ~D by codes of magnitude <= 2, so the code term all but vanishes: >= 10.3 bars (the
smallest at NF2 and n = 2600, where the factor term carries most of A).  nibble_order changes about
every other term by a level difference, >= 11.8.  drop_last_rows drops up to 32 rows, >= 539, and
tr_block measures >= 40.  All of these must show on every random case they apply to.  sym_table
changes one term per index 0 by 334 (s / D) |a|: like one flipped code it is held to ten bars only
while K r <= 10 000 (linear_cases.py's rule; >= 70 there, 2.6 to 3.5 on the forward cases beyond),
and on the longer random cases it is left to the exact cases, where any difference fails.  drop_lo
is 1 part in 3333 .. 8165 of the code term, below every random bar: the exact cases alone catch it
(every NF2 exact case moves).
"""
from dataclasses import dataclass

import numpy as np

import linear_backward_cases as BC
import linear_cases as LC
from linear_cases import f16, f32, f64, inference_codes, row_bytes  # noqa: F401  (re-exported)

LEVELS = {4: np.array([-1334, -1000, -784, -617, -476, -347, -226, -112, 0, 112, 226, 347, 476, 617, 784, 1000], f64),
          2: np.array([-8165, -3333, 3333, 8165], f64)}
DENOM = {4: 1000.0, 2: 10000.0}
# the NF quantiser's fp32 levels (quantization.py:45-57): what the reference dequantises with
LEVEL32 = {4: np.array([-1.334, -1.0, -0.784, -0.617, -0.476, -0.347, -0.226, -0.112, 0.0, 0.112, 0.226, 0.347,
                        0.476, 0.617, 0.784, 1.0], f32),
           2: np.array([-0.8165, -0.3333, 0.3333, 0.8165], f32)}
TAIL_INDEX = {4: 8, 2: 0}
CHUNK_ROWS = BC.CHUNK_ROWS
NF2_LONG_NONZERO = 1490


@dataclass(frozen=True)
class Case:
    kind: str       # "exact" | "exact16" | "random"
    dirn: str       # "fwd" | "bwd"
    m: int
    n: int
    r: int
    bits: int       # 4: NF4, 2: NF2
    T: int
    lb: int = 16    # L: 2 | 4 | 16
    rb: int = 16    # R
    bias: bool = False

    @property
    def id(self):
        fac = "" if self.lb == self.rb == 16 else f"L{self.lb}R{self.rb}"
        return (f"{self.dirn}-{self.kind}-m{self.m}n{self.n}r{self.r}nf{self.bits}{fac}T{self.T}"
                + ("-bias" if self.bias else ""))

    @property
    def K(self):
        return self.n if self.dirn == "fwd" else self.m

    @property
    def planes(self):
        return 1 if self.bits == 4 else 2

    @property
    def seed(self):
        return (self.m * 1000003 + self.n * 1009 + self.r * 101 + self.bits * 11 + self.lb * 307 + self.rb * 701
                + self.T + {"exact": 0, "exact16": 1, "random": 2}[self.kind] * 7919
                + (0 if self.dirn == "fwd" else 108729) + 424243)


_FWD = ([(33, 64, 8, T) for T in (1, 5)] + [(48, 198, 40, T) for T in (3, 16)]
        + [(80, 898, 200, T) for T in (16, 17, 64)] + [(48, 198, 0, T) for T in (3, 17)]
        + [(48, 2600, 40, T) for T in (1, 16)])      # decode waves own two chunks
_BWD = ([(m, n, r, T) for (m, n, r) in ((33, 64, 8), (80, 898, 200), (272, 512, 16), (198, 48, 0), (160, 256, 128))
         for T in (1, 17, 64)] + [(272, 512, 16, 130), (160, 256, 128, 130)])
# factor formats beside fp16 / fp16: 4-bit / 4-bit and 2-bit / fp16, decode and prefill resp. one T
_FWD_FACTORS = [(48, 198, 40, T, lb, rb) for (lb, rb) in ((4, 4), (2, 16)) for T in (16, 17)]
_BWD_FACTORS = [(160, 256, 128, 17, lb, rb) for (lb, rb) in ((4, 4), (2, 16))]


def _cases(kind):
    out = []
    for b in (4, 2):
        out += [Case(kind, "fwd", m, n, r, b, T) for (m, n, r, T) in _FWD]
        out += [Case(kind, "fwd", m, n, r, b, T, lb, rb) for (m, n, r, T, lb, rb) in _FWD_FACTORS]
        out += [Case(kind, "fwd", 33, 64, 8, b, 5, bias=True)]
        out += [Case(kind, "bwd", m, n, r, b, T) for (m, n, r, T) in _BWD]
        out += [Case(kind, "bwd", m, n, r, b, T, lb, rb) for (m, n, r, T, lb, rb) in _BWD_FACTORS]
    return out


EXACT = _cases("exact")
RANDOM = _cases("random")
EXACT16 = [Case("exact16", d, 33, 64, 8, b, T) for d in ("fwd", "bwd") for b in (4, 2) for T in (1, 5, 17)]
ALL = EXACT + EXACT16 + RANDOM
FORWARD = [c for c in ALL if c.dirn == "fwd"]
BACKWARD = [c for c in ALL if c.dirn == "bwd"]


def _kf(bits):
    return 2 ** (bits - 1) - 1


def amax_exact(case):
    """The largest |a| of an exact case, see the module docstring."""
    if case.kind == "exact16" or case.bits == 2 or case.K > LC.LONG_N:
        return 1
    return 4


_CACHE = {}


def inputs(case: Case):
    """dict(a (T, K) f16, idx (m, n) uint8, l (m, r) int8 codes | f16, rho (r, n) int8 codes | f16,
    s, sl, sr, gs (f32; sl / sr None for an fp16 factor), bias (m,) f32 | None); built once per case
    and shared (treat as read-only)."""
    if case in _CACHE:
        return _CACHE[case]
    rng = np.random.default_rng(case.seed)
    m, n, r, T, K = case.m, case.n, case.r, case.T, case.K
    random = case.kind == "random"
    idx = rng.integers(0, 2 ** case.bits, (m, n)).astype(np.uint8)
    if case.bits == 4:
        idx[0, 0] = 0
    fa = 2 if case.kind == "exact" else 1

    def factor(bits, shape):
        if bits != 16:
            k = _kf(bits)
            return rng.integers(-k, k + 1, shape).astype(np.int8), f32(0.3) if random else f32(k)
        if random:
            return (0.15 * rng.standard_normal(shape)).astype(f16), None
        return rng.integers(-fa, fa + 1, shape).astype(f16), None

    if random:
        a = rng.standard_normal((T, K)).astype(f16)
    else:
        xa = amax_exact(case)
        a = rng.integers(-xa, xa + 1, (T, K)).astype(f16)
        if case.bits == 2 and K > LC.LONG_N:  # bounded number of nonzeros per token
            for t in range(T):
                a[t, rng.permutation(K)[NF2_LONG_NONZERO:]] = 0
    l, sl = factor(case.lb, (m, r))
    rho, sr = factor(case.rb, (r, n))
    big = max(np.abs(a.astype(f64)).max(), 1.0)
    for (t, j) in ((0, 0), (0, K - 1)) + (((1, 0),) if T > 1 else ()):
        a[t, j] = f16(big if a[t, j] >= 0 else -big)
    if random:
        s, gs = f32(0.05), f32(1.7)
        bias = rng.standard_normal(m).astype(f32) if case.bias else None
    else:
        s = f32(DENOM[case.bits] / 2)
        gs = f32(4.0) if case.kind == "exact" else f32(2.0 ** -4)
        bias = (rng.integers(-8, 9, m) * 0.5).astype(f32) if case.bias else None
    out = dict(a=a, idx=idx, l=l, rho=rho, s=s, sl=sl, sr=sr, gs=gs, bias=bias)
    _CACHE[case] = out
    return out


def scales(case: Case, d=None):
    """(s / D, zscale) as the kernel forms them: fp32 divisions, fp32 product."""
    d = inputs(case) if d is None else d
    sd = f32(d["s"] / f32(DENOM[case.bits]))
    z = f32(1.0)
    if case.lb != 16:
        z = f32(d["sl"] / f32(_kf(case.lb)))
    if case.rb != 16:
        skr = f32(d["sr"] / f32(_kf(case.rb)))
        z = f32(z * skr) if case.lb != 16 else skr
    return sd, z


def index_codes(idx, bits, tail=None, stride=None):
    """(m, n) level indices -> (m, stride or row_bytes) uint8 inference layout (MSB-first, the index
    itself), the tail filled with index `tail` (default: TAIL_INDEX)."""
    m, n = idx.shape
    per = 8 // bits
    rb = row_bytes(n, bits) if stride is None else stride
    full = np.full((m, rb * per), TAIL_INDEX[bits] if tail is None else tail, dtype=np.uint8)
    full[:, :n] = idx
    full = full.reshape(m, rb, per)
    out = np.zeros((m, rb), dtype=np.uint8)
    for i in range(per):
        out |= full[:, :, i] << (bits * (per - 1 - i))
    return out


def storage_index_codes(idx, bits):
    """(m, n) level indices -> flat storage-layout bytes on the (m, n padded to 4) grid and n_padded."""
    m, n = idx.shape
    npad = n + (-n) % 4
    per = 8 // bits
    full = np.full((m, npad), TAIL_INDEX[bits], dtype=np.uint8)
    full[:, :n] = idx
    full = full.reshape(-1, per)
    out = np.zeros(full.shape[0], dtype=np.uint8)
    for i in range(per):
        out |= full[:, i] << (bits * (per - 1 - i))
    return out, npad


def factor_operand(case: Case, which: str):
    """("codes", uint8 inference layout, scale, bits) or ("fp16", array) of factor "l" / "rho"."""
    d = inputs(case)
    bits = case.lb if which == "l" else case.rb
    if bits == 16:
        return "fp16", d[which]
    return "codes", inference_codes(d[which], bits), d["sl" if which == "l" else "sr"], bits


FAULTS = ("offset_binary", "sym_table", "nibble_order", "drop_lo", "s_for_sD", "tr_block", "drop_last_rows")
# faults that must move a random case by ten bars where they apply to it (the others: the exact cases)
RANDOM_FAULTS = ("offset_binary", "sym_table", "nibble_order", "s_for_sD", "tr_block", "drop_last_rows")


def fault_applies(case: Case, fault: str) -> bool:
    """Whether a planted fault exists for the case and, from its data's design, must show."""
    if case.kind == "exact16":
        return False
    random = case.kind == "random"
    if fault == "sym_table":
        return case.bits == 4 and not (random and case.K * case.r > 10000)
    if fault == "drop_lo":
        return case.bits == 2 and not random
    if fault in ("tr_block", "drop_last_rows"):
        return case.dirn == "bwd"
    return True


def weight_levels(case: Case, fault: str | None = None):
    """(m, n) fp64 integer levels I[idx] as the (possibly faulty) decode sees them."""
    idx = inputs(case)["idx"].astype(np.int64)
    bits = case.bits
    if fault == "nibble_order":
        per = 8 // bits
        npad = -(-case.n // per) * per
        full = np.full((case.m, npad), TAIL_INDEX[bits], dtype=np.int64)
        full[:, :case.n] = idx
        idx = full.reshape(case.m, -1, per)[:, :, ::-1].reshape(case.m, npad)[:, :case.n]
    if fault == "offset_binary":
        return (idx - _kf(bits)).astype(f64)
    lev = LEVELS[bits].copy()
    if fault == "sym_table":
        lev[0] = -1000.0
    elif fault == "drop_lo":
        lev = lev - np.sign(lev)
    w = lev[idx]
    if fault == "tr_block":
        b = min(16, case.m, case.n)
        w[:b, :b] = w[:b, :b].T.copy()
    return w


def reference(case: Case, fault: str | None = None):
    """(out64, bar): the fp64 reference -- y (T, m) forward, dx (T, n) backward -- and the elementwise
    bar of the random cases.  fault: one planted error (FAULTS), for checking that the cases can see it."""
    d = inputs(case)
    a, l, rho = (d[key].astype(f64) for key in ("a", "l", "rho"))
    sd32, z32 = scales(case, d)
    sd, zscale, gs = f64(sd32), f64(z32), f64(d["gs"])
    if fault == "s_for_sD":
        sd = f64(d["s"])
    w = weight_levels(case, fault)
    aw = a
    if fault == "drop_last_rows":
        aw = a.copy()
        aw[:, CHUNK_ROWS * ((case.m - 1) // CHUNK_ROWS):] = 0
    absw = np.abs(LEVELS[case.bits][d["idx"].astype(np.int64)])
    aa, al, ar = np.abs(a), np.abs(l), np.abs(rho)
    if case.dirn == "fwd":
        out = gs * (sd * (aw @ w.T) + (zscale * (aw @ rho.T)) @ l.T)
        if d["bias"] is not None:
            out = out + d["bias"].astype(f64)
        A = f64(d["gs"]) * (f64(sd32) * (aa @ absw.T) + zscale * ((aa @ ar.T) @ al.T))
    else:
        out = gs * (sd * (aw @ w) + (zscale * (aw @ l)) @ rho)
        A = f64(d["gs"]) * (f64(sd32) * (aa @ absw) + zscale * ((aa @ al) @ ar))
    bar = (case.planes * case.K + case.r + 32) * 2.0 ** -24 * A
    return out, bar


def exact_units(case: Case):
    """The largest per-output sum of absolute terms of an exact case in units of 0.5 gs' (gs' = 1:
    before the global scale): sum |a| |I| + 2 zscale |a| |rho| |l|, and the largest |z~|."""
    d = inputs(case)
    a, l, rho = (np.abs(d[key].astype(f64)) for key in ("a", "l", "rho"))
    absw = np.abs(LEVELS[case.bits][d["idx"].astype(np.int64)])
    zscale = f64(scales(case, d)[1])
    if case.dirn == "fwd":
        z = zscale * (a @ rho.T)
        units = a @ absw.T + 2.0 * (z @ l.T)
    else:
        z = zscale * (a @ l)
        units = a @ absw + 2.0 * (z @ rho)
    return float(units.max()), float(z.max()) if z.size else 0.0
