"""Cases and the fp64 reference of the packed linear layer with coded factors
(include/caldera_hip.h, cq_linear_packed_forward):

    y[t, i]  = gs * ((s / k) * sum_j x[t, j] c[i, j] + sum_q z~[t, q] l[i, q]) (+ bias[i])
    z~[t, q] = zscale * sum_j x[t, j] rho[q, j]

l is the L codes (l_bits 2 | 4) or the fp16 L (16), rho the R codes or the fp16 R; zscale is the
fp32 product of the coded factors' scale / k (each one fp32 division).  Same pattern as
linear_cases.py: host-seeded numpy, the reference evaluated in fp64 from the operands as the
kernel sees them, the fp32 divisions and the fp32 zscale product included.

Exact cases: integers (x in -4..4, codes in -k..k, an fp16 factor in -2..2), s = k / 2,
s_L = k_L / 2, s_R = k_R / 2 (every scale / k is 0.5, zscale 0.25 or 0.5), gs = 4.  Every term is
a multiple of 0.25; test_linear_factors_host.py checks on the case data that for every output
the sum of the absolute terms, the |hi| + |lo| of z~'s split included, stays below 2^24 such
units and that z~ splits exactly into fp16 halves, so any summation order is exact and the
kernel must match bit for bit.  Row 0 of x is xa everywhere but x[0, 0] = xa - 1 and row 0 of
rho is k_R everywhere, so z~[0, 0] = zscale k_R (n xa - 1) is zscale times an odd integer: where
that integer reaches 2048 a single fp16 rounding of z~ (fault "z16") cannot represent it.
"exact16" cases (x in -1..1, (33, 64, 8)) keep |y| <= 2048 so fp16 output equals y.

Random cases: x ~ N(0, 1), random codes, s = 0.05, s_L = s_R = 0.3, gs = 1.7, an fp16 factor
~ 0.15 N(0, 1), with the project's bar

    |y - y64| <= (n + r + 32) 2^-24 A,   A = gs ((s / k) |x| |c|^T + zscale |x| |rho|^T |l|^T)

Rounding count behind the + 32, beyond the n roundings of a K sum and the r of the L product
(the hi and lo products of one q are exact in fp32 and |lo| <= 2^-11 |hi|): s / k on the code sum
1, zscale on z 1 (new here), the split into halves 2^-22 = 4, the sum of the two terms 1, gs 1,
bias 1: 9 <= 32, so the constant stands.

x[0, 0], x[0, n - 1] and (T > 1) x[1, 0] carry the largest magnitude of the case's x (random
cases), as in linear_cases.py.  At (33, 64, 8) row q < min(T, r) of rho follows the signs of x[q] and
row q of l is k_L e_q, so y[q, q]'s factor term is one z~ without cancellation.

Long-K decode cases ((48, 2600, 40) and (33, 8454, 40), see linear_cases.py): the exact ones take x
from -1..1, which keeps |z~| <= 0.5 * 7 * 8454 = 29589 inside fp16 and the absolute sums below 2^24
units; row 0 of x is all ones but x[0, 1] = 0 (z~[0, 0] stays zscale times an odd integer), and
c[0, 8 CK + 1] = k so that "stale_x", which swaps x[0, 1] in there, shows at T = 1.  The random
ones plant y[0, 0] as in linear_cases.py: over wave 0's second chunk row 0 of the layer's codes is
k sign(x[0]) and row 0 of rho is k_R sign(x[0]) (0.3 sign(x[0]) for fp16 R), and row 0 of l is
k_L e_0 (0.45 e_0 for fp16 L).  The loop faults "drop_chunk", "stale_x", "drop_R_chunk" and
"stale_x_R" are those of linear_cases.py, with the z product's chunk 256 columns for 2-bit R.
"""
from dataclasses import dataclass

import numpy as np

import linear_cases as LC
from linear_cases import f16, f32, f64, inference_codes, row_bytes  # noqa: F401  (re-exported)


@dataclass(frozen=True)
class Case:
    kind: str       # "exact" | "exact16" | "random"
    m: int
    n: int
    r: int
    bits: int       # Q
    lb: int         # L: 2 | 4 | 16
    rb: int         # R
    T: int
    bias: bool = False

    @property
    def id(self):
        return (f"{self.kind}-m{self.m}n{self.n}r{self.r}b{self.bits}L{self.lb}R{self.rb}T{self.T}"
                + ("-bias" if self.bias else ""))

    @property
    def k(self):
        return 2 ** (self.bits - 1) - 1

    @property
    def kl(self):
        return 2 ** (self.lb - 1) - 1 if self.lb != 16 else None

    @property
    def kr(self):
        return 2 ** (self.rb - 1) - 1 if self.rb != 16 else None

    @property
    def seed(self):
        return (self.m * 1000003 + self.n * 1009 + self.r * 101 + self.bits * 11 + self.lb * 307 + self.rb * 701
                + self.T + {"exact": 0, "exact16": 1, "random": 2}[self.kind] * 7919)


SHAPES = [(33, 64, 8), (48, 198, 40), (80, 898, 200), (48, 198, 264), (272, 512, 16), (48, 2600, 40), (33, 8454, 40)]
_T = {(33, 64, 8): (1, 5, 17), (48, 198, 40): (5, 16, 64), (80, 898, 200): (1, 16, 17), (48, 198, 264): (5, 16, 64),
      (272, 512, 16): (16, 130), (48, 2600, 40): (1, 16), (33, 8454, 40): (5, 16)}


def _shapes():
    out = []
    for shp in SHAPES:                          # every shape meets (2, 4, 4) and (2, 2, 2)
        for T in _T[shp]:
            out.append((*shp, 2, 4, 4, T))
            out.append((*shp, 2, 2, 2, T))
    for shp in ((48, 198, 40), (80, 898, 200)):  # the other combinations: one decode, one prefill T
        for bits in ((4, 4, 4), (2, 2, 4), (2, 4, 16), (2, 16, 4)):
            for T in (16, 17 if shp[0] == 80 else 64):
                out.append((*shp, *bits, T))
    for bits in ((4, 4, 4), (2, 4, 16), (2, 16, 4)):  # decode K loops past one chunk per wave
        out.append((33, 8454, 40, *bits, 16))
    return out


EXACT = [Case("exact", *s) for s in _shapes()] + [Case("exact", 33, 64, 8, 2, 4, 4, 5, bias=True)]
EXACT16 = [Case("exact16", 33, 64, 8, 2, lb, rb, T) for lb, rb in ((2, 2), (4, 2)) for T in (1, 5, 17)]
RANDOM = [Case("random", *s) for s in _shapes()] + [Case("random", 33, 64, 8, 2, 4, 4, 5, bias=True)]
ALL = EXACT + EXACT16 + RANDOM

_CACHE = {}


def _xa(case):
    """The largest |x| of an exact case."""
    return 4 if case.kind == "exact" and case.n <= LC.LONG_N else 1


def _z_chunk(case):
    """Columns of the second chunk of the z product's first slot, or None."""
    return LC.second_chunk(case, case.rb, LC.DECODE_WAVES_Z * LC.DECODE_SPLIT_Z)


def inputs(case: Case):
    """dict(x (T, n) f16, c (m, n) int8, l (m, r) int8 codes | f16, rho (r, n) int8 codes | f16,
    s, sl, sr, gs (f32; sl / sr None for an fp16 factor), bias (m,) f32 | None); built once per case
    and shared (treat as read-only)."""
    if case in _CACHE:
        return _CACHE[case]
    rng = np.random.default_rng(case.seed)
    m, n, r, T = case.m, case.n, case.r, case.T
    c = rng.integers(-case.k, case.k + 1, (m, n)).astype(np.int8)
    random = case.kind == "random"
    fa = 2 if case.kind == "exact" else 1

    def factor(bits, shape):
        if bits != 16:
            k = 2 ** (bits - 1) - 1
            return rng.integers(-k, k + 1, shape).astype(np.int8), f32(0.3) if random else f32(k / 2)
        if random:
            return (0.15 * rng.standard_normal(shape)).astype(f16), None
        return rng.integers(-fa, fa + 1, shape).astype(f16), None

    if random:
        x = rng.standard_normal((T, n)).astype(f16)
    else:
        xa = _xa(case)
        x = rng.integers(-xa, xa + 1, (T, n)).astype(f16)
    l, sl = factor(case.lb, (m, r))
    rho, sr = factor(case.rb, (r, n))
    if random:
        s, gs = f32(0.05), f32(1.7)
        bias = rng.standard_normal(m).astype(f32) if case.bias else None
        big = np.abs(x.astype(f64)).max()
        for (t, j) in ((0, 0), (0, n - 1)) + (((1, 0),) if T > 1 else ()):
            x[t, j] = f16(big if x[t, j] >= 0 else -big)
        if (m, n, r) == (33, 64, 8) and case.lb != 16 and case.rb != 16:
            # y[q, q] hangs on z~[q, q] alone, and that is its own absolute sum (no cancellation): a
            # single fp16 rounding of it (fault "z16") stands against the bar of that one output
            for q in range(min(T, r)):
                rho[q, :] = np.where(x[q].astype(f64) >= 0, case.kr, -case.kr)
                l[q, :] = 0
                l[q, q] = case.kl
        if n > LC.LONG_N and T <= LC.DECODE_MAX_TOKENS:
            # y[0, 0] hangs on wave 0's second chunk of both products without cancellation
            lo, hi = LC.second_chunk(case, case.bits, LC.DECODE_WAVES)
            c[0, lo:hi] = (case.k * LC._sign(x[0, lo:hi])).astype(np.int8)
            l[0, :] = 0
            l[0, 0] = case.kl if case.lb != 16 else f16(0.45)
            zc = _z_chunk(case)
            if zc:
                sg = LC._sign(x[0, zc[0]:zc[1]])
                rho[0, zc[0]:zc[1]] = ((case.kr * sg).astype(np.int8) if case.rb != 16
                                       else (0.3 * sg).astype(f16))
    else:
        s, gs = f32(case.k / 2), f32(4.0)
        bias = (rng.integers(-8, 9, m) * 0.5).astype(f32) if case.bias else None
        if case.kind == "exact":   # z~[0, 0] = zscale * (an odd multiple of the largest rho), l[0, 0] != 0
            x[0, :] = xa
            x[0, 0 if xa > 1 else 1] = xa - 1         # not x[0, 0] = 0: "flip_R" needs it at T = 1
            rho[0, :] = case.kr if case.rb != 16 else fa
            l[0, 0] = case.kl if case.lb != 16 else fa
            if n > LC.LONG_N and T <= LC.DECODE_MAX_TOKENS:
                c[0, LC.second_chunk(case, case.bits, LC.DECODE_WAVES)[0] + 1] = case.k
    out = dict(x=x, c=c, l=l, rho=rho, s=s, sl=sl, sr=sr, gs=gs, bias=bias)
    _CACHE[case] = out
    return out


def scales(case: Case, d=None):
    """(sk, zscale) as the kernel forms them: fp32 divisions, fp32 product."""
    d = inputs(case) if d is None else d
    sk = f32(d["s"] / f32(case.k))
    z = f32(1.0)
    if case.lb != 16:
        z = f32(d["sl"] / f32(case.kl))
    if case.rb != 16:
        skr = f32(d["sr"] / f32(case.kr))
        z = f32(z * skr) if case.lb != 16 else skr
    return sk, z


LOOP_FAULTS = ("drop_chunk", "stale_x", "drop_R_chunk", "stale_x_R")
FAULTS = ("flip_L", "flip_R", "L_transposed", "sl_for_skl", "drop_zscale", "pad_L", "z16") + LOOP_FAULTS


def fault_applies(case: Case, fault: str) -> bool:
    """Whether a planted fault exists for the case and, from its data's design, must show."""
    random = case.kind == "random"
    if case.kind == "exact16":
        return False
    if fault in ("drop_chunk", "stale_x"):      # a wave of the code product has a second chunk
        return LC.second_chunk(case, case.bits, LC.DECODE_WAVES) is not None
    if fault in ("drop_R_chunk", "stale_x_R"):  # ... of the z product
        return _z_chunk(case) is not None
    if fault in ("flip_L", "L_transposed", "sl_for_skl", "pad_L") and case.lb == 16:
        return False
    if fault == "flip_R" and case.rb == 16:
        return False
    if fault in ("flip_L", "flip_R") and random:
        # one code against the bar: |x| dl |rho| (or |x| |l| drho) over A ~ n r E|x| E|rho| E|l| must
        # reach 10 (n + r + 32) 2^-24; that holds with room up to n r ~ 10^4
        return case.n * case.r <= 10000
    if fault == "sl_for_skl":
        return case.lb == 4                     # k_L = 1 at 2 bits: s_L / k_L is s_L
    if fault == "pad_L":                        # a z pad column exists inside the z buffers' row
        # (one code again: k_L |z~| over A ~ r sqrt(n) E|l| |z~| against the bar; not at n = 898)
        return case.r % 32 != 0 and not (random and case.n > 512)
    if fault == "z16":
        if random:
            # <= 2^-11, typically 2^-13, of one z~ against (n + r + 32) 2^-24 of A: visible only where
            # n + r + 32 is ~100 and one z~ carries the whole output, see inputs()
            return (case.m, case.n, case.r) == (33, 64, 8) and case.lb != 16 and case.rb != 16
        if case.rb == 16:
            return False
        return case.kr * (case.n * _xa(case) - 1) >= 2048   # z~[0, 0] / zscale: an odd integer, see inputs()
    return True


def _flip(v, k):
    return -v if v != 0 else k


def reference(case: Case, fault: str | None = None):
    """(y64, bar): the fp64 reference (T, m) and the elementwise bar of the random cases.
    fault: one planted error (FAULTS), for checking that the cases can see it.  "L_transposed"
    reads the (m, r) codes as if they lay in L^T order; "pad_L" models a nonzero code (k_L) in
    row 0's first pad column meeting a z pad column that holds z~ of the last R row (what a
    row-clamped z product leaves there); "z16" rounds z~ once to fp16.  The loop faults act on
    wave 0's second chunk as in linear_cases.py: row 0 of the layer's codes, all rows of rho."""
    d = inputs(case)
    x, c, l, rho = (d[key].astype(f64) for key in ("x", "c", "l", "rho"))
    sk, zscale = (f64(v) for v in scales(case, d))
    gs = f64(d["gs"])
    m, r = case.m, case.r
    if fault == "flip_L":
        l[0, 0] = _flip(l[0, 0], case.kl)
    elif fault == "flip_R":
        rho[0, 0] = _flip(rho[0, 0], case.kr)
    elif fault == "L_transposed":
        l = l.reshape(-1).reshape(r, m).T.copy()
    elif fault == "sl_for_skl":
        zscale = f64(f32(d["sl"]) * (f32(d["sr"] / f32(case.kr)) if case.rb != 16 else f32(1.0)))
    elif fault == "drop_zscale":
        zscale = f64(1.0)
    z = x @ rho.T
    if fault in ("drop_R_chunk", "stale_x_R"):
        lo, hi = _z_chunk(case)
        z -= x[:, lo:hi] @ rho[:, lo:hi].T
        if fault == "stale_x_R":
            z += x[:, :hi - lo] @ rho[:, lo:hi].T
    z = zscale * z
    if fault == "z16":
        z = z.astype(f16).astype(f64)
    lr = z @ l.T
    if fault == "pad_L":
        lr[:, 0] += z[:, -1] * case.kl
    code = x @ c.T
    if fault in ("drop_chunk", "stale_x"):
        lo, hi = LC.second_chunk(case, case.bits, LC.DECODE_WAVES)
        code[:, 0] -= x[:, lo:hi] @ c[0, lo:hi]
        if fault == "stale_x":
            code[:, 0] += x[:, :hi - lo] @ c[0, lo:hi]
    y = gs * (sk * code + lr)
    if d["bias"] is not None:
        y = y + d["bias"].astype(f64)
    ax = np.abs(d["x"].astype(f64))
    A = f64(d["gs"]) * (f64(scales(case, d)[0]) * (ax @ np.abs(d["c"].astype(f64)).T)
                        + f64(scales(case, d)[1]) * (ax @ np.abs(d["rho"].astype(f64)).T) @ np.abs(d["l"].astype(f64)).T)
    bar = (case.n + case.r + 32) * 2.0 ** -24 * A
    return y, bar


def factor_operand(case: Case, which: str):
    """("codes", uint8 inference layout, scale, bits) or ("fp16", array) of factor "l" / "rho"."""
    d = inputs(case)
    bits = case.lb if which == "l" else case.rb
    if bits == 16:
        return ("fp16", d[which])
    return ("codes", inference_codes(d[which], bits), d["sl" if which == "l" else "sr"], bits)
